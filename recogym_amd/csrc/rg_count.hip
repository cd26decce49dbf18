// rg_count.hip — the count agents' training as one reduction of a sorted device log (reference agents/organic_count.py:74-82,
// agents/bandit_count.py:49-62 under the offline protocol of bench_agents.py:90-190) and their frozen argmax policy.
//
// One wave per user, users assigned statically (wave w takes users w, w + W, ...); rows stream in coalesced 64-row chunks as
// in rg_ope.hip.  Every counter is an integer and addition commutes: whatever order the updates arrive in, the tables hold the
// same bits.
//
// OrganicCount: a session (a maximal run of organic rows of a user) is kept as a (product, views) list with ONE ENTRY PER LANE
// of the wave, in registers — up to 64 distinct products; its m^2 cell updates views(i) * views(j) are issued when it closes.
// A session with more distinct products switches to the pairwise form: co_counts[v_i][v_j] += 1 for every pair of its ROWS,
// read back from the log — rows^2 updates, no list, nothing dropped.
//
// BanditCount: a bandit row's ix is the last organic view in front of the PREVIOUS bandit row of the log.  Inside a user that
// is a look-up in the chunk (or two carried registers); for a user's first bandit row it is a look-back from the user's first
// row over the previous users' rows — local: the previous user normally ends in its phantom row, an organic view a few rows
// before it.  No scan over users.
//
// What bounds the kernel is atomics, not streaming: the hot cells (popular product x popular product) take a large part of all
// updates.  Every update therefore goes through a per-block LDS table (cell -> 64-bit sum, open addressing, filled first come
// first served, LDS atomics) that lives as long as the block and is added to global memory once at the end; an update that
// finds no slot within kCntProbes probes goes to global memory directly (a cold cell: uncontended).  All global atomics are
// 64-bit integer adds without return value.
#include "rg_count_common.hpp"

namespace {

// The last organic view in front of the last bandit row below row `pos` (the value BanditCount's last_product_viewed has when
// the row at `pos` opens a user), or `carry` where the log has none.  Wave-uniform.
__device__ uint32_t cnt_lookback(const rg_event* __restrict__ rows, int64_t pos, uint32_t carry, uint32_t lane) {
    bool found = false;
    for (int64_t hi = pos; hi > 0; hi -= 64) {
        const int64_t row = hi - 64 + lane;
        const bool live = row >= 0;
        const uint32_t code = live ? rows[row].code : 0u;
        const u64 bm = __ballot(live && (code & RG_EV_BANDIT));
        u64 om = __ballot(live && !(code & RG_EV_BANDIT));
        if (!found) {
            if (!bm) continue;
            found = true;
            om &= lanes_below(top_bit(bm));
        }
        if (om) return lane_value(code, top_bit(om)) & RG_EV_INDEX_MASK;
    }
    return carry;
}

__global__ void k_count_init(u64* __restrict__ ws, int64_t* __restrict__ carry) {
    if (threadIdx.x < kWsWords) ws[threadIdx.x] = 0;
    if (threadIdx.x == 0) { carry[1] = -1; carry[2] = 0; carry[3] = 0; }
}

// every user opens with an organic row
__global__ __launch_bounds__(256) void k_count_check(const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets,
                                                     uint64_t n_users, u64* __restrict__ ws) {
    bool bad = false;
    for (uint64_t u = blockIdx.x * 256ull + threadIdx.x; u < n_users; u += gridDim.x * 256ull) {
        const int64_t b = offsets[u], e = offsets[u + 1];
        if (e < b || (b < e && (rows[b].code & RG_EV_BANDIT))) bad = true;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0)
        (void)__hip_atomic_fetch_or(&ws[kWsErr], kErrFirstBandit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(64 * kCntWaves) void k_count_train(rg_count_tables t, const rg_event* __restrict__ rows,
                                                                const int64_t* __restrict__ offsets, uint64_t n_users,
                                                                int64_t* __restrict__ carry, u64* __restrict__ ws, uint32_t n_waves) {
    __shared__ u64 s_key[kCntHashSlots];
    __shared__ u64 s_cnt[kCntHashSlots];
    for (uint32_t i = threadIdx.x; i < kCntHashSlots; i += 64 * kCntWaves) { s_key[i] = kCntEmpty; s_cnt[i] = 0; }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kCntWaves + wib;
    const uint32_t P = t.num_products;
    const bool do_co = t.co_counts != nullptr, do_b = t.pulls != nullptr;
    CntCtx c{s_key, s_cnt, reinterpret_cast<u64*>(t.co_counts), reinterpret_cast<u64*>(t.pulls), reinterpret_cast<u64*>(t.clicks), 0u};
    const int64_t carry_in64 = carry[0];
    const uint32_t carry_in = carry_in64 < 0 ? kCntNone : static_cast<uint32_t>(carry_in64);
    u64 n_upd = 0;          // wave-uniform count of the cell updates of this wave (lane 0 reports it)
    u64 err = 0;

    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        if (b >= e) continue;
        // the open session: entry i of its (product, views) list lives in lane i
        uint32_t sp = 0, sc = 0, m = 0;
        bool longs = false;
        int64_t sess_start = b;
        // BanditCount: aprev = last_product_viewed after the user's last bandit row so far (before any: after the previous
        // users), lastv = the user's last organic view so far
        bool have_in = false;
        uint32_t aprev = kCntNone, lastv = 0;

        // closes the open session, whose rows are sess_start .. end-1
        auto close = [&](int64_t end) __attribute__((always_inline)) {
            if (longs) {
                const int64_t L = end - sess_start;
                for (int64_t i = sess_start; i < end; ++i) {
                    const u64 pi = rows[i].code & RG_EV_INDEX_MASK;
                    for (int64_t j = sess_start + lane; j < end; j += 64)
                        cnt_add(c, 0, c.co, pi * P + (rows[j].code & RG_EV_INDEX_MASK), 1);
                }
                n_upd += static_cast<u64>(L) * static_cast<u64>(L);
            } else {
                for (uint32_t i = 0; i < m; ++i) {
                    const u64 pi = lane_value(sp, i), ci = lane_value(sc, i);
                    if (lane < m) cnt_add(c, 0, c.co, pi * P + sp, ci * sc);
                }
                n_upd += static_cast<u64>(m) * m;
            }
            m = 0;
            longs = false;
        };

        for (int64_t base = b; base < e; base += 64) {
            const int64_t row = base + lane;
            const bool in = row < e;
            uint4 x = make_uint4(0u, 0u, 0u, 0u);
            if (in) x = reinterpret_cast<const uint4*>(rows)[row];
            const uint32_t idx = x.z & RG_EV_INDEX_MASK;
            const bool ok = in && idx < P;           // a row whose product is out of range is reported and never counted
            if (__ballot(in && !ok)) err |= kErrProduct;
            const bool isb = ok && (x.z & RG_EV_BANDIT);
            const bool iso = ok && !(x.z & RG_EV_BANDIT);
            const u64 omask = __ballot(iso), bmask = __ballot(isb), imask = __ballot(in);

            if (do_co) {
                u64 rem = imask;
                while (rem) {
                    // nothing open: on to the next organic row (the bandit rows behind it stay in `rem`: they close it)
                    const u64 next = (m == 0 && !longs) ? (rem & omask) : rem;
                    if (!next) break;
                    const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(next));
                    rem &= ~lanes_below(k) & ~(1ull << k);
                    if ((omask >> k) & 1) {
                        if (m == 0 && !longs) sess_start = base + k;
                        if (!longs) {
                            const uint32_t p = lane_value(idx, k);
                            const u64 hit = __ballot(lane < m && sp == p);
                            if (hit) {
                                if (lane == static_cast<uint32_t>(__builtin_ctzll(hit))) sc += 1;
                            } else if (m < 64) {
                                if (lane == m) { sp = p; sc = 1; }
                                m += 1;
                            } else {
                                longs = true;        // more than 64 distinct products: the pairwise form, from the log
                            }
                        }
                    } else {
                        close(base + k);
                    }
                }
            }

            if (do_b && bmask) {
                if (!have_in) {
                    aprev = cnt_lookback(rows, b, carry_in, lane);
                    have_in = true;
                }
                // ix = last_product_viewed after the previous bandit row: the last organic view in front of that row
                const u64 pb = bmask & lanes_below(lane);
                const uint32_t r1 = pb ? top_bit(pb) : 0u;
                const u64 po = pb ? (omask & lanes_below(r1)) : 0ull;
                const uint32_t from = static_cast<uint32_t>(__shfl(static_cast<int>(idx), static_cast<int>(po ? top_bit(po) : 0u)));
                const uint32_t ix = pb ? (po ? from : lastv) : aprev;
                if (isb) {
                    const bool click = (x.z & RG_EV_CLICK) != 0;
                    if (ix == kCntNone) {
                        // NumPy's pulls_a[None, a] += 1: the whole row a — added by k_count_none_row (at most one row of a log)
                        carry[1] = static_cast<int64_t>(idx);
                        carry[2] = click ? 1 : 0;
                    } else if (ix < P) {
                        cnt_add(c, 1, c.pulls, static_cast<u64>(ix) * P + idx, 1);
                        if (click) cnt_add(c, 2, c.clicks, static_cast<u64>(ix) * P + idx, 1);
                    } else {
                        err |= kErrProduct;
                    }
                }
                n_upd += static_cast<u64>(__popcll(bmask)) + static_cast<u64>(__popcll(__ballot(isb && (x.z & RG_EV_CLICK))));
                const uint32_t rl = top_bit(bmask);
                const u64 pl = omask & lanes_below(rl);
                aprev = pl ? lane_value(idx, top_bit(pl)) : lastv;
            }
            if (omask) lastv = lane_value(idx, top_bit(omask));
        }
        if (do_co && (m || longs)) close(e);
    }

    // the block's sums -> global memory, one atomic per occupied slot
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < kCntHashSlots; s += 64 * kCntWaves) {
        const u64 k = s_key[s];
        if (k == kCntEmpty || !s_cnt[s]) continue;
        const uint32_t tab = static_cast<uint32_t>(k >> kCntTabShift);
        const u64 cell = k & ((1ull << kCntTabShift) - 1);
        if (tab == 0) cnt_global(c, c.co, cell, s_cnt[s]);
        else if (tab == 1) cnt_global(c, c.pulls, cell, s_cnt[s]);
        else cnt_global(c, c.clicks, cell, s_cnt[s]);
    }
    u64 g = c.n_glob;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) g += __shfl_xor(g, o);
    const u64 any_err = __ballot(err != 0) ? (__ballot(err & kErrProduct) ? kErrProduct : 0ull) : 0ull;
    if (lane == 0) {
        (void)__hip_atomic_fetch_add(&ws[kWsUpdates], n_upd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(&ws[kWsAtomics], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (any_err) (void)__hip_atomic_fetch_or(&ws[kWsErr], any_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// last_product_viewed after the whole log
__global__ __launch_bounds__(64) void k_count_carry(const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets,
                                                    uint64_t n_users, int64_t* __restrict__ carry) {
    const int64_t c0 = carry[0];
    const uint32_t v = cnt_lookback(rows, offsets[n_users], c0 < 0 ? kCntNone : static_cast<uint32_t>(c0), threadIdx.x);
    if (threadIdx.x == 0) carry[0] = v == kCntNone ? -1 : static_cast<int64_t>(v);
}

// pulls[a][:] += 1, clicks[a][:] += c for the bandit row that met last_product_viewed = None
__global__ __launch_bounds__(256) void k_count_none_row(rg_count_tables t, const int64_t* __restrict__ carry) {
    const int64_t a = carry[1];
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (a < 0 || a >= static_cast<int64_t>(t.num_products) || j >= t.num_products) return;
    t.pulls[static_cast<size_t>(a) * t.num_products + j] += 1;
    t.clicks[static_cast<size_t>(a) * t.num_products + j] += carry[2];
}

// first index of the row's maximum: block per row
__global__ __launch_bounds__(256) void k_count_policy(rg_count_tables t, uint32_t kind, int32_t* __restrict__ action,
                                                      int64_t* __restrict__ win_clicks, int64_t* __restrict__ win_pulls) {
    __shared__ u64 s_n[256], s_d[256];
    __shared__ uint32_t s_j[256];
    const uint32_t P = t.num_products, l = blockIdx.x;
    // a value is the fraction n / d (RG_COUNT_ORGANIC: d = 1); x beats y when x is larger, or equal with the smaller index
    u64 bn = 0, bd = 1;
    uint32_t bj = 0xFFFFFFFFu;
    for (uint32_t j = threadIdx.x; j < P; j += 256) {
        const size_t cell = static_cast<size_t>(l) * P + j;
        u64 n, d;
        if (kind == RG_COUNT_ORGANIC) { n = static_cast<u64>(t.co_counts[cell]); d = 1; }
        else { n = static_cast<u64>(t.clicks[cell]) + 1; d = static_cast<u64>(t.pulls[cell]) + 2; }
        if (bj == 0xFFFFFFFFu || n * bd > bn * d) { bn = n; bd = d; bj = j; }      // (j ascends: ties keep the earlier one)
    }
    s_n[threadIdx.x] = bn; s_d[threadIdx.x] = bd; s_j[threadIdx.x] = bj;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const u64 on = s_n[threadIdx.x + s], od = s_d[threadIdx.x + s];
            const uint32_t oj = s_j[threadIdx.x + s];
            const u64 mn = s_n[threadIdx.x], md = s_d[threadIdx.x];
            const uint32_t mj = s_j[threadIdx.x];
            if (oj != 0xFFFFFFFFu) {
                const u64 lhs = on * md, rhs = mn * od;
                if (mj == 0xFFFFFFFFu || lhs > rhs || (lhs == rhs && oj < mj)) {
                    s_n[threadIdx.x] = on; s_d[threadIdx.x] = od; s_j[threadIdx.x] = oj;
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        action[l] = static_cast<int32_t>(s_j[0]);
        if (kind == RG_COUNT_BANDIT) {
            win_clicks[l] = static_cast<int64_t>(s_n[0] - 1);
            win_pulls[l] = static_cast<int64_t>(s_d[0] - 2);
        }
    }
}

}  // namespace

extern "C" size_t rg_count_workspace_bytes(void) { return kWsWords * sizeof(u64); }

extern "C" int rg_count_train(const rg_count_tables* tables, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                              int64_t* d_carry, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = count_tables_ok(tables, "rg_count_train")) return rc;
    if (!tables->co_counts && !tables->pulls) return fail(RG_EINVAL, "rg_count_train: no table given");
    if (!d_offsets || (n_users && !d_rows)) return fail(RG_EINVAL, "rg_count_train: null rows / offsets");
    if (!d_carry || !d_workspace) return fail(RG_EINVAL, "rg_count_train: null carry / workspace");
    if (workspace_bytes < rg_count_workspace_bytes())
        return fail(RG_ENOMEM, "rg_count_train: workspace %zu < %zu bytes", workspace_bytes, rg_count_workspace_bytes());
    if (reinterpret_cast<uintptr_t>(d_rows) % 16) return fail(RG_EINVAL, "rg_count_train: rows not 16-byte aligned");
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    hipStream_t s = static_cast<hipStream_t>(stream);
    u64* ws = static_cast<u64*>(d_workspace);
    hipLaunchKernelGGL(k_count_init, dim3(1), dim3(64), 0, s, ws, d_carry);
    HIP_TRY(hipGetLastError());
    if (n_users == 0) return RG_OK;
    const uint32_t check_blocks = static_cast<uint32_t>(n_users / 256 + 1 > 2048 ? 2048 : n_users / 256 + 1);
    hipLaunchKernelGGL(k_count_check, dim3(check_blocks), dim3(256), 0, s, d_rows, d_offsets, n_users, ws);
    HIP_TRY(hipGetLastError());
    u64 verdict = 0;
    HIP_TRY(hipMemcpyAsync(&verdict, ws + kWsErr, sizeof(verdict), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (verdict & kErrFirstBandit)
        return fail(RG_EINVAL, "rg_count_train: a user opens with a bandit row (or its offsets descend); no table was touched");
    const uint64_t blocks64 = (n_users + kCntWaves - 1) / kCntWaves;
    const uint32_t blocks = static_cast<uint32_t>(blocks64 > kCntMaxBlocks ? kCntMaxBlocks : blocks64);
    hipLaunchKernelGGL(k_count_train, dim3(blocks), dim3(64 * kCntWaves), 0, s, *tables, d_rows, d_offsets, n_users, d_carry, ws,
                       blocks * kCntWaves);
    HIP_TRY(hipGetLastError());
    if (tables->pulls) {
        hipLaunchKernelGGL(k_count_carry, dim3(1), dim3(64), 0, s, d_rows, d_offsets, n_users, d_carry);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_count_none_row, dim3((tables->num_products + 255) / 256), dim3(256), 0, s, *tables, d_carry);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(&verdict, ws + kWsErr, sizeof(verdict), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (verdict & kErrProduct)
        return fail(RG_EINVAL, "rg_count_train: the log has a product >= num_products %u (such rows were not counted)", tables->num_products);
    return RG_OK;
}

extern "C" int rg_count_policy(const rg_count_tables* tables, uint32_t kind, int32_t* d_action, int64_t* d_win_clicks,
                               int64_t* d_win_pulls, void* stream) {
    if (int rc = count_tables_ok(tables, "rg_count_policy")) return rc;
    if (kind != RG_COUNT_ORGANIC && kind != RG_COUNT_BANDIT) return fail(RG_EINVAL, "rg_count_policy: bad kind %u", kind);
    if (kind == RG_COUNT_ORGANIC && !tables->co_counts) return fail(RG_EINVAL, "rg_count_policy: null co_counts");
    if (kind == RG_COUNT_BANDIT && (!tables->pulls || !d_win_clicks || !d_win_pulls))
        return fail(RG_EINVAL, "rg_count_policy: null pulls / clicks / winners");
    if (!d_action) return fail(RG_EINVAL, "rg_count_policy: null action table");
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    hipLaunchKernelGGL(k_count_policy, dim3(tables->num_products), dim3(256), 0, static_cast<hipStream_t>(stream), *tables, kind,
                       d_action, d_win_clicks, d_win_pulls);
    HIP_TRY(hipGetLastError());
    return RG_OK;
}
