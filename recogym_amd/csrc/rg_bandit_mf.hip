// rg_bandit_mf.hip — BanditMFSquare's training from a sorted device log (reference agents/bandit_mf.py:89-126 under the offline
// protocol of bench_agents.py:168-190).
//
// rg_bmf_samples: the log -> the training triples (last product viewed, action, reward), grouped by optimiser step.  The CALLS
// are rg_omf_pairs' (an organic-only user's call sits on its last row, every bandit row of any other user is one); call number
// k = first_call + 1 + (calls in front of it); k % mini_batch == 0 is a TRIGGER: it stores nothing, the samples stored since the
// previous trigger make one step.  A wave per user validates, writes the call bit of every row and forward-fills the last view
// (ballots over 64-row chunks, the last organic view of a chunk carried into the next); one exclusive scan of the call bits numbers
// the calls, a second one of the kept bandit rows compacts the list, and the CSR row of a step is a lower bound in the (ascending)
// step numbers of the kept samples.  Integer work only: the same bytes on every run.
//
// rg_bmf_steps: the chain of RMSprop steps of such a list in ONE launch of ONE workgroup (the steps depend on each other, and
// __syncthreads is the only barrier there is).  Per step of n samples: a thread per sample stages (l_s, a_s) and
// d_s = (sigmoid(<Ep[a_s], Eu[l_s]>) - r_s) / n in LDS (from exp(-|z|), rg_exp64.hpp's table exp, without cancellation); a sample is the
// FIRST of its action (of its last view) when no sample in front of it has the same one, and ballots list the first samples in
// sample order; every thread then owns cells (distinct row, e) and sums its samples in sample order:
// g_Ep[a][e] = sum_{a_s = a} d_s Eu[l_s][e], g_Eu[l][e] = sum_{l_s = l} d_s Ep[a_s][e] — n E n work whatever P is, no floating-point
// atomics; then the dense RMSprop update of all 2 P E parameters (a row the step did not touch has g = 0: its square average
// decays, its value stays), and the owners zero their cells again.  float64 throughout: two runs give the same bits.
// Two instantiations of one body: the embeddings, their square averages and the gradients in LDS (256 threads) while
// bmf_lds_bytes(P, E, kBmfMaxStep, true) fits 64 KiB — P <= 245 at E = 5 — else in global memory (1024 threads, the caller's
// arrays in place, the gradients in the workspace), up to P = 16384 and E = 64.
#include "rg_common.hpp"
#include "rg_bmf_common.hpp"
#include "rg_scan_common.hpp"

namespace {

using namespace rgbmf;
using rgomf::omf_rmsprop;

typedef unsigned long long bmf_u64;

constexpr int kBmfOutWords = 8;

// ---------------------------------------------------------------------------------------------------------------------------
// rg_bmf_samples
// ---------------------------------------------------------------------------------------------------------------------------
// workspace: call[n + 1] | keep[n + 1] | step[n_pending + n] | sums[blocks of n + 1] (uint32 each) | lv[n] (int32: the last view
// at a call's row, -1 at every other row)
struct BmfSamplesWs {
    uint32_t *call, *keep, *step, *sums;
    int32_t* lv;
    size_t bytes;
};

BmfSamplesWs bmf_samples_carve(void* base, uint64_t n, uint64_t n_pending) {
    BmfSamplesWs w;
    static uint32_t none[1];                                      // (base = null: only the size is asked for)
    uint32_t* p = base ? static_cast<uint32_t*>(base) : none;
    const uint64_t nb = (n + 1 + kOmfScanBlock - 1) / kOmfScanBlock;
    w.call = p; p += n + 1;
    w.keep = p; p += n + 1;
    w.step = p; p += n_pending + n;
    w.sums = p; p += nb;
    w.lv = reinterpret_cast<int32_t*>(p);
    w.bytes = 4 * (2 * (n + 1) + n_pending + n + nb + n);
    w.bytes = (w.bytes + 255) / 256 * 256;
    return w;
}

// a wave per user: the validation, the call bit of every row and the last view at every call
__global__ __launch_bounds__(256) void k_bmf_flags(const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users,
                                                   uint64_t n_organic, uint64_t n_rows, uint32_t P, uint32_t* __restrict__ call,
                                                   int32_t* __restrict__ lv, int64_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = blockIdx.x * 4ull + (threadIdx.x >> 6), n_waves = gridDim.x * 4ull;
    bmf_u64 err = 0;
    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        if (b < 0 || e < b || static_cast<uint64_t>(e) > n_rows) { err |= kBmfErrOffsets; continue; }
        const bool organic_only = user < n_organic;
        if (b == e) {
            if (organic_only) err |= kBmfErrEmptyOrganic;      // (its call would have no row to sit on)
            continue;
        }
        if (rows[b].code & RG_EV_BANDIT) err |= kBmfErrFirstBandit;
        int carry = -1;                                         // the last organic view of the chunks in front
        for (int64_t base = b; base < e; base += 64) {          // (uniform over the wave: every lane takes part in the ballot)
            const int64_t row = base + lane;
            const bool in = row < e;
            const uint32_t code = in ? rows[row].code : RG_EV_BANDIT;
            const bool isb = (code & RG_EV_BANDIT) != 0;
            const int idx = static_cast<int>(code & RG_EV_INDEX_MASK);
            const bmf_u64 org = __ballot(in && !isb);
            const bmf_u64 at_or_below = org & (lanes_below(lane) | (1ull << lane));
            const int src = at_or_below ? top_bit(at_or_below) : 0;
            const int got = __shfl(idx, src);
            const int last = at_or_below ? got : carry;
            const int chunk_last = __shfl(idx, org ? top_bit(org) : 0);
            if (org) carry = chunk_last;
            if (in) {
                if (static_cast<uint32_t>(idx) >= P) err |= kBmfErrProduct;
                if (isb && organic_only) err |= kBmfErrOrganicBandit;
                const bool is_call = organic_only ? row == e - 1 : isb;
                call[row] = is_call ? 1u : 0u;
                lv[row] = is_call ? last : -1;                  // (-1 at a call only for a user that opens with a bandit row: refused)
            }
        }
    }
    if (err) (void)__hip_atomic_fetch_or(reinterpret_cast<bmf_u64*>(out), err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// call[r] (scanned: the calls in front of row r) -> the step of the sample at r; keep[r] = the row stores a sample; the last
// call's last view
__global__ __launch_bounds__(256) void k_bmf_keep(const rg_event* __restrict__ rows, uint32_t* __restrict__ call, const int32_t* __restrict__ lv,
                                                  uint32_t* __restrict__ keep, uint64_t n_rows, uint64_t first_call, uint32_t mb,
                                                  uint32_t n_calls, int64_t* __restrict__ out) {
    for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r <= n_rows; r += gridDim.x * 256ull) {
        if (r == n_rows) {                                      // (call[n_rows] = the number of calls: left as it is)
            keep[r] = 0;
            if (n_calls == 0) out[5] = -1;
            continue;
        }
        const uint32_t in_front = call[r];
        const uint64_t k = first_call + 1 + in_front;
        const bool is_call = lv[r] >= 0;
        const bool kept = is_call && (rows[r].code & RG_EV_BANDIT) && (k % mb != 0);
        keep[r] = kept ? 1u : 0u;
        call[r] = static_cast<uint32_t>(k / mb - first_call / mb);
        if (is_call && in_front + 1 == n_calls) out[5] = lv[r];
    }
}

__global__ __launch_bounds__(256) void k_bmf_scatter(const rg_event* __restrict__ rows, const uint32_t* __restrict__ stepno,
                                                     const uint32_t* __restrict__ keep, const int32_t* __restrict__ lv, uint64_t n_rows,
                                                     const int32_t* __restrict__ pending, uint64_t n_pending, int32_t* __restrict__ triples,
                                                     uint32_t* __restrict__ step) {
    for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r < n_rows + n_pending; r += gridDim.x * 256ull) {
        if (r < n_pending) {                                    // the triples carried in belong to the first step
            triples[3 * r] = pending[3 * r];
            triples[3 * r + 1] = pending[3 * r + 1];
            triples[3 * r + 2] = pending[3 * r + 2];
            step[r] = 0;
            continue;
        }
        const uint64_t row = r - n_pending;
        if (keep[row + 1] == keep[row]) continue;
        const uint64_t q = n_pending + keep[row];
        const uint32_t code = rows[row].code;
        triples[3 * q] = lv[row];
        triples[3 * q + 1] = static_cast<int32_t>(code & RG_EV_INDEX_MASK);
        triples[3 * q + 2] = (code & RG_EV_CLICK) ? 1 : 0;
        step[q] = stepno[row];
    }
}

// step_offsets[s] = the first triple whose step is >= s, s = 0 .. n_steps; step_offsets[n_steps + 1] = all triples (the row behind
// the last trigger: the new pending set)
__global__ __launch_bounds__(256) void k_bmf_offsets(const uint32_t* __restrict__ call, const uint32_t* __restrict__ keep,
                                                     const uint32_t* __restrict__ step, uint64_t n_rows, uint64_t n_pending, uint64_t first_call,
                                                     uint32_t mb, int64_t* __restrict__ step_offsets, uint64_t step_capacity,
                                                     int64_t* __restrict__ out) {
    const uint64_t n_calls = call[n_rows], n_triples = n_pending + keep[n_rows];
    const uint64_t n_steps = (first_call + n_calls) / mb - first_call / mb;
    if (n_steps + 2 > step_capacity) {
        if (blockIdx.x == 0 && threadIdx.x == 0) out[0] |= static_cast<int64_t>(kBmfErrCapacity);
        return;
    }
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s < n_steps + 2; s += gridDim.x * 256ull) {
        uint64_t lo = 0, hi = n_triples;
        if (s > n_steps) lo = n_triples;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (step[mid] < s) lo = mid + 1; else hi = mid;
        }
        step_offsets[s] = static_cast<int64_t>(lo);
        if (s == n_steps) {
            out[1] = static_cast<int64_t>(n_calls);
            out[2] = static_cast<int64_t>(n_steps);
            out[3] = static_cast<int64_t>(n_triples);
            out[4] = static_cast<int64_t>(n_triples - lo);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// rg_bmf_steps
// ---------------------------------------------------------------------------------------------------------------------------
template <bool kLds, int kThreads>
__global__ __launch_bounds__(kThreads) void k_bmf_steps(rg_bmf_model m, double* __restrict__ g_grad, double lr, double alpha, double eps,
                                                        const int32_t* __restrict__ triples, uint64_t n_triples,
                                                        const int64_t* __restrict__ step_offsets, uint64_t n_steps, int64_t* __restrict__ out) {
    extern __shared__ double s_bmf[];
    const uint32_t P = m.num_products, E = m.embed_dim, PE = P * E;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr uint32_t kWaves = kThreads / 64;
    static_assert(kWaves <= 16, "the per-wave counts have 16 words each");
    // the layout bmf_lds_bytes counts
    double* sd = s_bmf;
    double* lds_state = sd + kBmfMaxStep;
    uint32_t* tab = reinterpret_cast<uint32_t*>(lds_state + (kLds ? 6 * static_cast<size_t>(PE) : 0));
    int* sl = reinterpret_cast<int*>(tab + 64);
    int* sa = sl + kBmfMaxStep;
    int* list_a = sa + kBmfMaxStep;
    int* list_l = list_a + kBmfMaxStep;
    int* flag = list_l + kBmfMaxStep;                             // [0 .. 3] the verdict, [16 .. 31] / [32 .. 47] first samples per wave
    double *pp, *pu, *qp, *qu, *gp, *gu;
    if constexpr (kLds) {
        pp = lds_state; pu = pp + PE; qp = pu + PE; qu = qp + PE; gp = qu + PE; gu = gp + PE;
    } else {
        pp = m.ep; pu = m.eu; qp = m.sq_ep; qu = m.sq_eu; gp = g_grad; gu = gp + PE;
    }

    // the whole list is validated before anything is touched
    if (tid < 4) flag[tid] = 0;
    __syncthreads();
    {
        bool bad_index = false, bad_reward = false, bad_off = false, bad_len = false;
        for (uint64_t q = tid; q < n_triples; q += kThreads) {
            if (static_cast<uint32_t>(triples[3 * q]) >= P || static_cast<uint32_t>(triples[3 * q + 1]) >= P) bad_index = true;
            if (static_cast<uint32_t>(triples[3 * q + 2]) > 1u) bad_reward = true;
        }
        for (uint64_t s = tid; s < n_steps; s += kThreads) {
            const int64_t lo = step_offsets[s], hi = step_offsets[s + 1];
            if (lo < 0 || hi < lo || static_cast<uint64_t>(hi) > n_triples) bad_off = true;
            else if (hi - lo > static_cast<int64_t>(kBmfMaxStep)) bad_len = true;
        }
        if (bad_index) flag[0] = 1;
        if (bad_off) flag[1] = 1;
        if (bad_reward) flag[2] = 1;
        if (bad_len) flag[3] = 1;
    }
    __syncthreads();
    if (flag[0] || flag[1] || flag[2] || flag[3]) {
        if (tid == 0) {
            out[0] = static_cast<int64_t>((flag[0] ? kBmfErrProduct : 0ull) | (flag[1] ? kBmfErrOffsets : 0ull) |
                                          (flag[2] ? kBmfErrReward : 0ull) | (flag[3] ? kBmfErrStepLength : 0ull));
            out[1] = out[2] = out[3] = 0;
        }
        return;
    }

    if (tid < 32) exp64t_entry(kExp2Tab32[tid], tid, tab);
    if constexpr (kLds) {
        for (uint32_t i = tid; i < PE; i += kThreads) { pp[i] = m.ep[i]; pu[i] = m.eu[i]; qp[i] = m.sq_ep[i]; qu[i] = m.sq_eu[i]; }
    }
    for (uint32_t i = tid; i < 2 * PE; i += kThreads) gp[i] = 0.0;    // (gp, gu are one array)
    __syncthreads();

    uint64_t n_taken = 0, n_empty = 0, n_used = 0;
    for (uint64_t s = 0; s < n_steps; ++s) {
        const uint64_t lo = static_cast<uint64_t>(step_offsets[s]);
        const uint32_t n = static_cast<uint32_t>(static_cast<uint64_t>(step_offsets[s + 1]) - lo);      // <= kBmfMaxStep <= kThreads
        if (n == 0) { ++n_empty; continue; }
        // a thread per sample: the triple and d_s
        if (tid < n) {
            const int32_t* t3 = triples + 3 * (lo + tid);
            const int l = t3[0], a = t3[1];
            const bool click = t3[2] != 0;
            const double *xa = pp + static_cast<uint32_t>(a) * E, *xl = pu + static_cast<uint32_t>(l) * E;
            double z = 0.0;
            for (uint32_t e = 0; e < E; ++e) z = fma(xa[e], xl[e], z);
            // sigmoid(z) - r without the cancellation at a saturated sigmoid: with t = exp(-|z|) in (0, 1] (nothing overflows),
            // sigmoid(|z|) = 1 / (1 + t) and sigmoid(-|z|) = 1 - sigmoid(|z|) = t / (1 + t); r = 1 gives -(1 - sigmoid(z)) = -sigmoid(-z)
            const double t = exp64t(-fabs(z), tab);
            const double mag = (((z >= 0.0) != click) ? 1.0 : t) / (1.0 + t);
            sl[tid] = l;
            sa[tid] = a;
            sd[tid] = (click ? -mag : mag) / static_cast<double>(n);
        }
        __syncthreads();
        // the first sample of every distinct action and of every distinct last view, in sample order
        bool first_a = false, first_l = false;
        if (tid < n) {
            first_a = first_l = true;
            const int a = sa[tid], l = sl[tid];
            for (uint32_t j = 0; j < tid; ++j) {
                if (sa[j] == a) first_a = false;
                if (sl[j] == l) first_l = false;
            }
        }
        const bmf_u64 mask_a = __ballot(first_a), mask_l = __ballot(first_l);
        if (lane == 0) {
            flag[16 + wave] = __popcll(mask_a);
            flag[32 + wave] = __popcll(mask_l);
        }
        __syncthreads();
        uint32_t base_a = 0, base_l = 0, nd_a = 0, nd_l = 0;
        for (uint32_t w = 0; w < kWaves; ++w) {
            const uint32_t ca = static_cast<uint32_t>(flag[16 + w]), cl = static_cast<uint32_t>(flag[32 + w]);
            if (w < wave) { base_a += ca; base_l += cl; }
            nd_a += ca;
            nd_l += cl;
        }
        if (first_a) list_a[base_a + __popcll(mask_a & lanes_below(lane))] = sa[tid];
        if (first_l) list_l[base_l + __popcll(mask_l & lanes_below(lane))] = sl[tid];
        __syncthreads();
        // a thread per cell (distinct row, e), the samples in sample order
        const uint32_t cells_a = nd_a * E, cells = cells_a + nd_l * E;
        for (uint32_t c = tid; c < cells; c += kThreads) {
            const bool act = c < cells_a;
            const uint32_t cc = act ? c : c - cells_a;
            const uint32_t d = cc / E, e = cc - d * E;
            const int row = act ? list_a[d] : list_l[d];
            const int *mine = act ? sa : sl, *other = act ? sl : sa;
            const double* x = act ? pu : pp;
            double g = 0.0;
            for (uint32_t j = 0; j < n; ++j)
                if (mine[j] == row) g = fma(sd[j], x[static_cast<uint32_t>(other[j]) * E + e], g);
            (act ? gp : gu)[static_cast<uint32_t>(row) * E + e] = g;
        }
        __syncthreads();
        // the dense update: a row the step did not touch has g = 0 (its square average decays, its value stays)
        for (uint32_t idx = tid; idx < 2 * PE; idx += kThreads) {       // (pp, pu / qp, qu / gp, gu: one array each in LDS)
            double* p = idx < PE ? pp + idx : pu + (idx - PE);
            double* q = idx < PE ? qp + idx : qu + (idx - PE);
            double pv = *p, qv = *q;
            omf_rmsprop(pv, qv, gp[idx], lr, alpha, eps);
            *p = pv;
            *q = qv;
        }
        __syncthreads();
        for (uint32_t c = tid; c < cells; c += kThreads) {              // the touched gradient rows are zero again
            const bool act = c < cells_a;
            const uint32_t cc = act ? c : c - cells_a;
            const uint32_t d = cc / E, e = cc - d * E;
            (act ? gp : gu)[static_cast<uint32_t>(act ? list_a[d] : list_l[d]) * E + e] = 0.0;
        }
        // (no barrier: the next step writes the lists and the gradients only behind its own barriers)
        ++n_taken;
        n_used += n;
    }

    if constexpr (kLds) {
        __syncthreads();
        for (uint32_t i = tid; i < PE; i += kThreads) { m.ep[i] = pp[i]; m.eu[i] = pu[i]; m.sq_ep[i] = qp[i]; m.sq_eu[i] = qu[i]; }
    }
    if (tid == 0) {
        out[0] = 0;
        out[1] = static_cast<int64_t>(n_taken);
        out[2] = static_cast<int64_t>(n_empty);
        out[3] = static_cast<int64_t>(n_used);
    }
}

}  // namespace

extern "C" size_t rg_bmf_samples_workspace_bytes(uint64_t n_rows, uint64_t n_pending) {
    return bmf_samples_carve(nullptr, n_rows, n_pending).bytes;
}

extern "C" int rg_bmf_samples(const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users, uint64_t n_organic_users, uint64_t n_rows,
                              uint32_t num_products, uint64_t first_call, uint32_t mini_batch, const int32_t* d_pending, uint64_t n_pending,
                              int32_t* d_triples, uint64_t triples_capacity, int64_t* d_step_offsets, uint64_t step_capacity, int64_t* d_out,
                              void* d_workspace, size_t workspace_bytes, void* stream) {
    if (num_products == 0 || num_products > RG_EV_INDEX_MASK) return fail(RG_EINVAL, "rg_bmf_samples: bad num_products %u", num_products);
    if (mini_batch == 0) return fail(RG_EINVAL, "rg_bmf_samples: mini_batch 0");
    if (!d_offsets || (n_rows && !d_rows)) return fail(RG_EINVAL, "rg_bmf_samples: null rows / offsets");
    if (n_organic_users > n_users) return fail(RG_EINVAL, "rg_bmf_samples: more organic-only users than users");
    if (n_rows > 0xFFFFFFF0ull || n_pending > 0xFFFFFFF0ull) return fail(RG_EINVAL, "rg_bmf_samples: more than 2^32 - 16 rows / pending triples");
    if (n_pending && !d_pending) return fail(RG_EINVAL, "rg_bmf_samples: null pending triples");
    if (!d_triples || !d_step_offsets || !d_out || !d_workspace) return fail(RG_EINVAL, "rg_bmf_samples: null output / workspace");
    if (reinterpret_cast<uintptr_t>(d_rows) % 16) return fail(RG_EINVAL, "rg_bmf_samples: rows not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_workspace) % 8) return fail(RG_EINVAL, "rg_bmf_samples: workspace not 8-byte aligned");
    if (triples_capacity < n_pending + n_rows)
        return fail(RG_ENOMEM, "rg_bmf_samples: room for %llu triples < %llu (pending + rows)", static_cast<unsigned long long>(triples_capacity),
                    static_cast<unsigned long long>(n_pending + n_rows));
    const uint64_t need_steps = (first_call % mini_batch + n_rows) / mini_batch + 2;
    if (step_capacity < need_steps)
        return fail(RG_ENOMEM, "rg_bmf_samples: room for %llu step offsets < %llu", static_cast<unsigned long long>(step_capacity),
                    static_cast<unsigned long long>(need_steps));
    const BmfSamplesWs w = bmf_samples_carve(d_workspace, n_rows, n_pending);
    if (workspace_bytes < w.bytes) return fail(RG_ENOMEM, "rg_bmf_samples: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(d_out, 0, kBmfOutWords * sizeof(int64_t), s));
    HIP_TRY(hipMemsetAsync(w.call, 0, (n_rows + 1) * sizeof(uint32_t), s));
    if (n_rows) HIP_TRY(hipMemsetAsync(w.lv, 0xFF, n_rows * sizeof(int32_t), s));
    if (n_users) {
        const uint64_t blocks64 = (n_users + 3) / 4;
        hipLaunchKernelGGL(k_bmf_flags, dim3(static_cast<uint32_t>(blocks64 > 4096 ? 4096 : blocks64)), dim3(256), 0, s, d_rows, d_offsets,
                           n_users, n_organic_users, n_rows, num_products, w.call, w.lv, d_out);
        HIP_TRY(hipGetLastError());
    }
    const uint64_t n1 = n_rows + 1;
    if (int rc = omf_scan(w.call, n1, w.sums, s)) return rc;      // (workspace only; the verdict is read before any output is written)
    int64_t verdict = 0;
    uint32_t n_calls = 0;
    HIP_TRY(hipMemcpyAsync(&verdict, d_out, sizeof(verdict), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&n_calls, w.call + n_rows, sizeof(n_calls), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (verdict & static_cast<int64_t>(kBmfErrOffsets)) return fail(RG_EINVAL, "rg_bmf_samples: offsets descend or leave the %llu rows; nothing was written",
                                                                     static_cast<unsigned long long>(n_rows));
    if (verdict & static_cast<int64_t>(kBmfErrFirstBandit)) return fail(RG_EINVAL, "rg_bmf_samples: a user opens with a bandit row; nothing was written");
    if (verdict & static_cast<int64_t>(kBmfErrEmptyOrganic)) return fail(RG_EINVAL, "rg_bmf_samples: an organic-only user without rows; nothing was written");
    if (verdict & static_cast<int64_t>(kBmfErrOrganicBandit)) return fail(RG_EINVAL, "rg_bmf_samples: an organic-only user has a bandit row; nothing was written");
    if (verdict & static_cast<int64_t>(kBmfErrProduct))
        return fail(RG_EINVAL, "rg_bmf_samples: the log has an index >= num_products %u; nothing was written", num_products);
    const uint64_t g64 = (n1 + n_pending + 255) / 256;
    const uint32_t grid = static_cast<uint32_t>(g64 > 8192 ? 8192 : g64);
    hipLaunchKernelGGL(k_bmf_keep, dim3(grid), dim3(256), 0, s, d_rows, w.call, w.lv, w.keep, n_rows, first_call, mini_batch, n_calls, d_out);
    HIP_TRY(hipGetLastError());
    if (int rc = omf_scan(w.keep, n1, w.sums, s)) return rc;
    hipLaunchKernelGGL(k_bmf_scatter, dim3(grid), dim3(256), 0, s, d_rows, w.call, w.keep, w.lv, n_rows, d_pending, n_pending, d_triples, w.step);
    HIP_TRY(hipGetLastError());
    const uint64_t gs64 = (need_steps + 255) / 256;
    hipLaunchKernelGGL(k_bmf_offsets, dim3(static_cast<uint32_t>(gs64 > 8192 ? 8192 : gs64)), dim3(256), 0, s, w.call, w.keep, w.step, n_rows,
                       n_pending, first_call, mini_batch, d_step_offsets, step_capacity, d_out);
    HIP_TRY(hipGetLastError());
    return RG_OK;
}

extern "C" int rg_bmf_limits(uint32_t embed_dim, uint32_t* lds_max_products, uint32_t* max_products, uint32_t* max_step) {
    if (embed_dim == 0 || embed_dim > kBmfMaxEmbed) return fail(RG_EINVAL, "rg_bmf_limits: embed_dim %u outside 1 .. %u", embed_dim, kBmfMaxEmbed);
    uint32_t p = 0;
    while (p < kBmfMaxProducts && bmf_lds_fits(p + 1, embed_dim)) ++p;
    if (lds_max_products) *lds_max_products = p;
    if (max_products) *max_products = kBmfMaxProducts;
    if (max_step) *max_step = kBmfMaxStep;
    return RG_OK;
}

extern "C" size_t rg_bmf_steps_workspace_bytes(uint32_t num_products, uint32_t embed_dim) {
    return 8 * 2 * static_cast<size_t>(num_products) * embed_dim;
}

extern "C" int rg_bmf_steps(const rg_bmf_model* model, double lr, double alpha, double eps, const int32_t* d_triples, uint64_t n_triples,
                            const int64_t* d_step_offsets, uint64_t n_steps, uint32_t force_global, int64_t* d_out, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
    if (!model) return fail(RG_EINVAL, "rg_bmf_steps: null model");
    const uint32_t P = model->num_products, E = model->embed_dim;
    if (P == 0 || P > kBmfMaxProducts) return fail(RG_EINVAL, "rg_bmf_steps: num_products %u outside 1 .. %u", P, kBmfMaxProducts);
    if (E == 0 || E > kBmfMaxEmbed) return fail(RG_EINVAL, "rg_bmf_steps: embed_dim %u outside 1 .. %u", E, kBmfMaxEmbed);
    if (!model->ep || !model->eu || !model->sq_ep || !model->sq_eu) return fail(RG_EINVAL, "rg_bmf_steps: null model array");
    if (!(lr == lr) || !(alpha >= 0.0 && alpha <= 1.0) || !(eps >= 0.0)) return fail(RG_EINVAL, "rg_bmf_steps: bad lr / alpha / eps");
    if ((n_triples && !d_triples) || !d_step_offsets || !d_out) return fail(RG_EINVAL, "rg_bmf_steps: null triples / step offsets / out");
    const bool lds = !force_global && bmf_lds_fits(P, E);
    if (!lds) {
        if (!d_workspace || workspace_bytes < rg_bmf_steps_workspace_bytes(P, E))
            return fail(RG_ENOMEM, "rg_bmf_steps: workspace %zu < %zu bytes", workspace_bytes, rg_bmf_steps_workspace_bytes(P, E));
        if (reinterpret_cast<uintptr_t>(d_workspace) % 8) return fail(RG_EINVAL, "rg_bmf_steps: workspace not 8-byte aligned");
    }
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t shmem = bmf_lds_bytes(P, E, kBmfMaxStep, lds);
    if (lds)
        hipLaunchKernelGGL((k_bmf_steps<true, 256>), dim3(1), dim3(256), shmem, s, *model, static_cast<double*>(nullptr), lr, alpha, eps,
                           d_triples, n_triples, d_step_offsets, n_steps, d_out);
    else
        hipLaunchKernelGGL((k_bmf_steps<false, 1024>), dim3(1), dim3(1024), shmem, s, *model, static_cast<double*>(d_workspace), lr, alpha, eps,
                           d_triples, n_triples, d_step_offsets, n_steps, d_out);
    HIP_TRY(hipGetLastError());
    return RG_OK;
}
