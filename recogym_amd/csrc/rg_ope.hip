// rg_ope.hip — off-policy evaluation replay (evaluate_IPS / evaluate_SNIPS, reference evaluate_agent.py:753-810) over a
// sorted device log: every evaluated user's rows are walked in log order, the target policy's `ps-a` entry of the logged
// action is recomputed from the user's rows so far, and r = pi[a] / ps is written for every bandit row.
//
// One wave per user, users assigned statically (wave w takes users w, w + W, ...): the per-wave partial sums — and so the
// reduced sums — are the same on every run.  Rows stream in coalesced 64-row chunks (16-byte rg_event per lane + the row's
// float64 ps).  RandomAgent and the last-view table are decided per lane; the OrganicUserEventCounter walks the chunk's rows
// in order with the user's (product, count) table:
//   - in LDS (1024 slots per wave) for users of at most 512 rows (distinct products <= organic rows <= 512: load <= 1/2);
//   - in a per-wave global table of 2^g_log2 >= 2 x (longest user) slots otherwise — slower, equally exact (nothing is
//     dropped: a dropped view would be a wrong pi).
// Dense forms (epsilon smoothing, reverse_pop, the argmax of the explore flip) take one wave-wide pass over all P products,
// cached until the user's next organic row.  No float atomics: the sums reduce in a second one-block pass in a fixed order
// (k_ope_reduce, here, for every replay unit: rg_ope_common.hpp).
#include "rg_ope_common.hpp"

namespace {

constexpr uint32_t kOpeLdsLog2 = 10;
constexpr uint32_t kOpeLdsSlots = 1u << kOpeLdsLog2;
constexpr uint32_t kOpeLdsRows = kOpeLdsSlots / 2;
constexpr uint32_t kOpeMaxWaves = 5120;         // 256 CUs x 20 waves (LDS: 4 waves x 8 KiB per block)

uint32_t ope_global_log2(const rg_ope_policy* pol, uint32_t max_user_rows) {
    if (pol->kind != RG_POLICY_ORGANIC_USER_COUNT || max_user_rows <= kOpeLdsRows) return 0;
    uint32_t l = kOpeLdsLog2 + 1;
    while ((1ull << l) < 2ull * max_user_rows) ++l;
    return l;
}

// (product + 1, count) open-addressing table; every lane of the wave calls the writer with the same product, so each
// lane reads back its own (identical) writes
__device__ __forceinline__ uint32_t ope_slot(uint32_t p, uint32_t shift) { return (p * 2654435761u) >> shift; }

__device__ __forceinline__ uint32_t ope_count(const uint32_t* key, const uint32_t* cnt, uint32_t mask, uint32_t shift, uint32_t p) {
    uint32_t s = ope_slot(p, shift);
    for (uint32_t i = 0; i <= mask; ++i) {
        const uint32_t k = key[s];
        if (k == p + 1) return cnt[s];
        if (k == 0) return 0;
        s = (s + 1) & mask;
    }
    return 0;
}

__device__ __forceinline__ uint32_t ope_add(uint32_t* key, uint32_t* cnt, uint32_t mask, uint32_t shift, uint32_t p, bool* fresh) {
    uint32_t s = ope_slot(p, shift);
    for (uint32_t i = 0; i <= mask; ++i) {
        const uint32_t k = key[s];
        if (k == p + 1) { const uint32_t c = cnt[s] + 1; cnt[s] = c; *fresh = false; return c; }
        if (k == 0) { key[s] = p + 1; cnt[s] = 1; *fresh = true; return 1; }
        s = (s + 1) & mask;
    }
    *fresh = false;
    return 0;
}

struct OpeDense {
    double S, S2;        // sum(eps + count) over the P products; reverse_pop: sum(1 - (eps + count) / S)
    uint32_t minp;       // first product of the smallest count (the first unseen one while any is unseen)
    uint32_t minc;
};

// one pass over all P products (every lane of the wave, the same table state)
__device__ OpeDense ope_dense(const uint32_t* key, const uint32_t* cnt, uint32_t mask, uint32_t shift, uint32_t P, double eps,
                              bool second, uint32_t lane) {
    double s = 0.0;
    uint32_t minc = 0xFFFFFFFFu, minp = 0;
    for (uint32_t p = lane; p < P; p += 64) {
        const uint32_t c = ope_count(key, cnt, mask, shift, p);
        s += eps + static_cast<double>(c);
        if (c < minc) { minc = c; minp = p; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t oc = __shfl_xor(minc, o), op = __shfl_xor(minp, o);
        if (oc < minc || (oc == minc && op < minp)) { minc = oc; minp = op; }
    }
    OpeDense d;
    d.S = wave_sum(s);
    d.minc = minc;
    d.minp = minp;
    d.S2 = 0.0;
    if (second) {
        double s2 = 0.0;
        for (uint32_t p = lane; p < P; p += 64)
            s2 += 1.0 - (eps + static_cast<double>(ope_count(key, cnt, mask, shift, p))) / d.S;
        d.S2 = wave_sum(s2);
    }
    return d;
}

// The OrganicUserEventCounter pi of every bandit lane of one chunk: the rows in log order, the table updated at each
// organic row (organic_user_count.py:45-96 with with_ps_all = True; the counts persist across sessions until reset())
struct OucState {
    uint32_t total, distinct, maxc, maxp;
    bool dense_ok;
    OpeDense dense;
};

__device__ __forceinline__ double ouc_chunk(const rg_ope_policy& pol, uint32_t* key, uint32_t* cnt, uint32_t mask, uint32_t shift,
                                            OucState& st, uint64_t omask, uint64_t emask, uint32_t n, uint32_t idx, uint32_t lane) {
    const uint32_t P = pol.num_products;
    const double eps = pol.ouc_epsilon;
    const bool ee = pol.ouc_exploit_explore != 0, sr = pol.ouc_select_randomly != 0, rp = pol.ouc_reverse_pop != 0;
    double pi = 0.0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t p = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(idx), static_cast<int>(k)));
        if ((omask >> k) & 1) {
            bool fresh;
            const uint32_t c = ope_add(key, cnt, mask, shift, p, &fresh);
            st.total += 1;
            st.distinct += fresh ? 1u : 0u;
            if (c > st.maxc || (c == st.maxc && p < st.maxp)) { st.maxc = c; st.maxp = p; }   // counts only grow: first maximum
            st.dense_ok = false;
            continue;
        }
        const bool explore = (emask >> k) & 1;
        const uint32_t ca = ope_count(key, cnt, mask, shift, p);
        const bool need_dense = !ee || (explore && !sr);
        if (need_dense && !st.dense_ok) {
            st.dense = ope_dense(key, cnt, mask, shift, P, ee ? 0.0 : eps, !ee && rp && sr, lane);
            st.dense_ok = true;
        }
        double v;
        if (ee && !explore) {
            // p = views / sum(views): one correctly rounded division (the sum of integers is exact in any order)
            v = sr ? static_cast<double>(ca) / static_cast<double>(st.total) : (p == st.maxp ? 1.0 : 0.0);
        } else if (ee) {
            // explore flip: p = [views == 0] / (P - distinct); argmax = the first unseen product (all NaN -> 0)
            if (sr) v = (ca == 0 ? 1.0 : 0.0) / static_cast<double>(P - st.distinct);
            else v = p == (st.dense.minc == 0 ? st.dense.minp : 0u) ? 1.0 : 0.0;
        } else if (!rp) {
            v = sr ? (eps + static_cast<double>(ca)) / st.dense.S : (p == st.maxp ? 1.0 : 0.0);
        } else {
            v = sr ? (1.0 - (eps + static_cast<double>(ca)) / st.dense.S) / st.dense.S2 : (p == st.dense.minp ? 1.0 : 0.0);
        }
        if (lane == k) pi = v;
    }
    return pi;
}

template <bool kLds>
__device__ __forceinline__ void ope_user(const rg_ope_policy& pol, const OpeLog& log, int64_t b, int64_t e, uint32_t* key,
                                         uint32_t* cnt, uint32_t mask, uint32_t shift, uint32_t lane, OpeAcc& acc) {
    const bool ouc = pol.kind == RG_POLICY_ORGANIC_USER_COUNT;
    const bool lvt = pol.kind == RG_POLICY_LAST_VIEW_TABLE;
    const double eps = pol.ouc_epsilon;
    const bool draw_explore = ouc && pol.ouc_exploit_explore && eps != 0.0;
    if (ouc) {
        for (uint32_t i = lane; i <= mask; i += 64) key[i] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");     // the cleared slots are read by every lane of the wave
    }
    OucState st{0u, 0u, 0u, 0u, false, OpeDense{0.0, 0.0, 0u, 0u}};
    uint32_t lpv = 0;
    for (int64_t base = b; base < e; base += 64) {
        const OpeRow r = ope_load(log, base, e, lane);
        double pi = 0.0;
        if (ouc) {
            bool explore = false;
            if (draw_explore && r.isb) {
                const rg_u32x4 w = rg_draw(pol.policy_seed, r.x.x, r.x.y, 0, RG_DRAW_POLICY);
                explore = !(eps / (eps + (1.0 - eps)) <= rg_uniform(w.w[0], w.w[1]));
            }
            const uint64_t omask = __ballot(r.iso), emask = __ballot(explore);
            const uint32_t n = static_cast<uint32_t>(e - base < 64 ? e - base : 64);
            pi = ouc_chunk(pol, key, cnt, mask, shift, st, omask, emask, n, r.idx, lane);
        } else if (lvt) {
            const uint32_t mine = ope_last_view(r, lane, lpv);
            pi = mine < pol.num_products && static_cast<uint32_t>(pol.table[mine]) == r.idx ? 1.0 : 0.0;
        } else {
            pi = 1.0 / static_cast<double>(pol.num_products);
        }
        if (r.isb) acc.emit(log, r, pi);
    }
}

__global__ __launch_bounds__(64 * kOpeWaves) void k_ope_replay(
    rg_ope_policy pol, const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users,
    uint32_t ps_mode, const double* __restrict__ ps64, double ps_const, double* __restrict__ ratio, uint8_t* __restrict__ click,
    double* __restrict__ slots, uint32_t* __restrict__ gtab, uint32_t g_log2, uint32_t n_waves) {
    __shared__ uint32_t s_key[kOpeWaves][kOpeLdsSlots];
    __shared__ uint32_t s_cnt[kOpeWaves][kOpeLdsSlots];
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kOpeWaves + wib;
    const OpeLog log{rows, offsets, n_users, ps_mode, ps64, ps_const, ratio, click, slots, n_waves};
    OpeAcc acc;
    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        if (pol.kind != RG_POLICY_ORGANIC_USER_COUNT || e - b <= static_cast<int64_t>(kOpeLdsRows) || g_log2 == 0) {
            ope_user<true>(pol, log, b, e, s_key[wib], s_cnt[wib], kOpeLdsSlots - 1, 32 - kOpeLdsLog2, lane, acc);
        } else {
            const size_t G = size_t(1) << g_log2;
            uint32_t* key = gtab + static_cast<size_t>(wave) * 2 * G;
            ope_user<false>(pol, log, b, e, key, key + G, static_cast<uint32_t>(G - 1), 32 - g_log2, lane, acc);
        }
    }
    acc.store(log, wave, lane);
}

// the per-wave slots -> (n, sum c r, sum r), one block, fixed order
__global__ __launch_bounds__(256) void k_ope_reduce(const double* __restrict__ slots, uint32_t n_waves, double* __restrict__ out) {
    __shared__ double sh[3][256];
    double a[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = threadIdx.x; i < n_waves; i += 256)
        for (int j = 0; j < 3; ++j) a[j] += slots[3 * static_cast<size_t>(i) + j];
    for (int j = 0; j < 3; ++j) sh[j][threadIdx.x] = a[j];
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s)
            for (int j = 0; j < 3; ++j) sh[j][threadIdx.x] += sh[j][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int j = 0; j < 3; ++j) out[j] = sh[j][0];
}

}  // namespace

int rgk::ope_reduce(const double* slots, uint32_t n_waves, double* d_sums, hipStream_t stream) {
    hipLaunchKernelGGL(k_ope_reduce, dim3(1), dim3(256), 0, stream, slots, n_waves, d_sums);
    HIP_TRY(hipGetLastError());
    return RG_OK;
}

extern "C" size_t rg_ope_workspace_bytes(const rg_ope_policy* pol, uint64_t n_users, uint32_t max_user_rows) {
    if (!pol) { fail(RG_EINVAL, "rg_ope_workspace_bytes: null policy"); return 0; }
    const uint32_t W = ope_waves(n_users, kOpeMaxWaves);
    const uint32_t l = ope_global_log2(pol, max_user_rows);
    return ope_slot_bytes(W) + (l ? static_cast<size_t>(W) * 2 * (size_t(1) << l) * sizeof(uint32_t) : 0);
}

extern "C" int rg_ope_replay(const rg_ope_policy* pol, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                             uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                             uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!pol) return fail(RG_EINVAL, "rg_ope_replay: null policy");
    if (pol->kind != RG_POLICY_RANDOM_AGENT && pol->kind != RG_POLICY_ORGANIC_USER_COUNT && pol->kind != RG_POLICY_LAST_VIEW_TABLE)
        return fail(RG_EINVAL, "rg_ope_replay: policy kind %u has no replay form", pol->kind);
    if (pol->num_products == 0 || pol->num_products > RG_EV_INDEX_MASK) return fail(RG_EINVAL, "rg_ope_replay: bad num_products");
    if (pol->kind == RG_POLICY_LAST_VIEW_TABLE && !pol->table) return fail(RG_EINVAL, "rg_ope_replay: null table");
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    if (int rc = ope_args_ok("rg_ope_replay", c, rg_ope_workspace_bytes(pol, n_users, max_user_rows))) return rc;
    const uint32_t W = ope_waves(n_users, kOpeMaxWaves);
    const uint32_t l = ope_global_log2(pol, max_user_rows);
    double* slots = c.at<double>(0);
    uint32_t* gtab = l ? c.at<uint32_t>(ope_slot_bytes(W)) : nullptr;
    hipLaunchKernelGGL(k_ope_replay, dim3(W / kOpeWaves), dim3(64 * kOpeWaves), 0, c.stream, *pol, c.d_rows, c.d_offsets, c.n_users, c.ps_mode,
                       c.d_ps, c.ps_const, c.d_ratio, c.d_click, slots, gtab, l, W);
    HIP_TRY(hipGetLastError());
    return ope_reduce(slots, W, c.d_sums, c.stream);
}
