// rg_evolve.hip — one step of the epsilon-greedy evolution study (reference evaluate_agent.py:51-146) over a sorted device log:
//
//   rg_evolution_stats      the step's four counters, the per-action clicks and the `explored` byte of every row: one wave per
//                           user, the rows in coalesced 64-row chunks (the layout of rg_ope_common.hpp), the explore flip recomputed
//                           from the addressed draw (eg_explored, shared with rg_ope_eg.hip).  Integer adds only: per-lane
//                           registers -> one butterfly per wave; the per-action clicks through a per-block LDS histogram (P <=
//                           kEvoHistMax: few addresses, which every click of the log would contend for in global memory) or
//                           straight to global memory (more products: the clicks spread out, and flushing a long histogram
//                           per block would cost more atomics than the clicks themselves).  Everything is staged in the
//                           workspace and added to the caller's arrays by k_evo_commit only when the whole log was valid.
//   rg_count_train_online   the count agents' train calls under a row filter.  A row is COUNTED when it is a
//                           bandit row, not the phantom row, and let through by the mask; its session is the run of organic rows
//                           directly in front of it.  OrganicCount: the session list of rg_count.hip, emitted when a counted row
//                           closes it and DROPPED when another bandit row or the user's end does.  BanditCount: ix of a counted
//                           row = the last view of the last non-empty session among the counted rows in front of it, anywhere
//                           in the log — a "last non-None value" scan: k_online_check leaves every user's own last value,
//                           three small kernels turn that into every user's incoming value, k_online_train finishes it inside
//                           the user with ballots.  Rows that meet None add to two P-long arrays; k_online_none_rows adds them
//                           to whole table rows (NumPy's pulls_a[None, a] += 1).
#include "rg_ope_common.hpp"
#include "rg_count_common.hpp"

namespace {

constexpr uint32_t kEvoMaxBlocks = 1280;             // 256 CUs x 5 blocks of 4 waves
constexpr uint32_t kEvoHistMax = 512;                // x 4 bytes = 2 KiB of LDS per block
constexpr int kEvoWsStage = 8;                       // stats workspace: word 0 error bits, words 8..11 the staged counters,
constexpr int kEvoWsHist = 32;                       //   words 32.. the staged per-action clicks
constexpr u64 kErrCarry = 4;                         // d_carry[0] >= P
constexpr int kOnlWsCarry = 3;                       // online workspace: word 3 = last_product_viewed after the log
constexpr uint32_t kOnlTile = 2048, kOnlPer = 8;     // the user scan: 256 threads x 8 users per tile

__device__ __forceinline__ u64 wave_sum_u64(u64 x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

inline uint32_t evo_blocks(uint64_t n_users) {
    const uint64_t b = (n_users + kCntWaves - 1) / kCntWaves;
    return static_cast<uint32_t>(b < 1 ? 1 : (b > kEvoMaxBlocks ? kEvoMaxBlocks : b));
}

// ---------------------------------------------------------------------------------------------------------------------------
// the statistics
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kCntWaves) void k_evo_stats(rg_ope_eg eg, uint32_t has_eg, const rg_event* __restrict__ rows,
                                                              const int64_t* __restrict__ offsets, uint64_t n_users, uint32_t P,
                                                              uint8_t* __restrict__ explored, u64* __restrict__ ws, uint32_t n_waves) {
    __shared__ uint32_t s_hist[kEvoHistMax];
    const bool lds = P <= kEvoHistMax;
    if (lds) {
        for (uint32_t i = threadIdx.x; i < P; i += 64 * kCntWaves) s_hist[i] = 0;
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * kCntWaves + (threadIdx.x >> 6);
    const double thr = eg_threshold(eg.epsilon);
    u64* hist = ws + kEvoWsHist;
    uint32_t n_s = 0, n_f = 0, n_sg = 0, n_fg = 0;
    u64 err = 0;
    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        if (e < b) err |= kErrFirstBandit;
        for (int64_t base = b; base < e; base += 64) {
            const int64_t row = base + lane;
            const bool in = row < e;
            uint4 x = make_uint4(0u, 0u, 0u, 0u);
            if (in) x = reinterpret_cast<const uint4*>(rows)[row];
            const uint32_t idx = x.z & RG_EV_INDEX_MASK;
            const bool isb = in && (x.z & RG_EV_BANDIT);
            if (isb && row == b) err |= kErrFirstBandit;
            if (in && idx >= P) err |= kErrProduct;
            const bool act = isb && !(x.z & RG_EV_PHANTOM) && idx < P;
            bool expl = false;
            if (act) {
                const bool click = (x.z & RG_EV_CLICK) != 0;
                expl = has_eg && eg_explored(eg.seed, thr, x.x, x.y);
                const bool greedy = has_eg && !expl;
                n_s += click ? 1u : 0u;
                n_f += click ? 0u : 1u;
                n_sg += (click && greedy) ? 1u : 0u;
                n_fg += (!click && greedy) ? 1u : 0u;
                if (click) {
                    if (lds) atomicAdd(&s_hist[idx], 1u);
                    else (void)__hip_atomic_fetch_add(hist + idx, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (explored && in) explored[row] = expl ? 1 : 0;
        }
    }
    const u64 t_s = wave_sum_u64(n_s), t_f = wave_sum_u64(n_f), t_sg = wave_sum_u64(n_sg), t_fg = wave_sum_u64(n_fg);
    const u64 e1 = __ballot(err & kErrFirstBandit) ? kErrFirstBandit : 0ull, e2 = __ballot(err & kErrProduct) ? kErrProduct : 0ull;
    if (lane == 0) {
        if (t_s) (void)__hip_atomic_fetch_add(ws + kEvoWsStage + 0, t_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t_f) (void)__hip_atomic_fetch_add(ws + kEvoWsStage + 1, t_f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t_sg) (void)__hip_atomic_fetch_add(ws + kEvoWsStage + 2, t_sg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t_fg) (void)__hip_atomic_fetch_add(ws + kEvoWsStage + 3, t_fg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (e1 | e2) (void)__hip_atomic_fetch_or(ws + kWsErr, e1 | e2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < P; i += 64 * kCntWaves) {
            const uint32_t v = s_hist[i];
            if (v) (void)__hip_atomic_fetch_add(hist + i, static_cast<u64>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// the staged sums -> the caller's arrays, unless the log was invalid
__global__ __launch_bounds__(256) void k_evo_commit(const u64* __restrict__ ws, uint32_t P, int64_t* __restrict__ counts,
                                                    int64_t* __restrict__ action_clicks) {
    if (ws[kWsErr]) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < 4) counts[i] += static_cast<int64_t>(ws[kEvoWsStage + i]);
    if (i < P) action_clicks[i] += static_cast<int64_t>(ws[kEvoWsHist + i]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the filtered training
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool onl_counted(uint32_t code, bool in, const uint8_t* __restrict__ mask, int64_t row) {
    return in && (code & RG_EV_BANDIT) && !(code & RG_EV_PHANTOM) && (!mask || mask[row] != 0);
}

// validation of the whole log (nothing is written to a table before its verdict is read) and, for BanditCount, every user's own
// last value: the last view of the last non-empty session one of its counted rows closes, or -1
__global__ __launch_bounds__(64 * kCntWaves) void k_online_check(const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets,
                                                                 uint64_t n_users, uint32_t P, const uint8_t* __restrict__ mask,
                                                                 int32_t* __restrict__ last, const int64_t* __restrict__ carry,
                                                                 u64* __restrict__ ws, uint32_t n_waves) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * kCntWaves + (threadIdx.x >> 6);
    u64 err = 0;
    // BanditCount's incoming last_product_viewed indexes a table row (any negative value is None)
    if (carry && wave == 0 && lane == 0 && carry[0] >= static_cast<int64_t>(P))
        (void)__hip_atomic_fetch_or(ws + kWsErr, kErrCarry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        if (e < b) err |= kErrFirstBandit;
        uint32_t prev_code = RG_EV_BANDIT;         // the row in front of the chunk (in front of the user: not an organic row)
        int32_t mine = -1;
        for (int64_t base = b; base < e; base += 64) {
            const int64_t row = base + lane;
            const bool in = row < e;
            const uint32_t code = in ? rows[row].code : 0u;
            if (in && (code & RG_EV_INDEX_MASK) >= P) err |= kErrProduct;
            if (in && row == b && (code & RG_EV_BANDIT)) err |= kErrFirstBandit;
            const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(code), 1));
            const uint32_t pcode = lane ? up : prev_code;
            const u64 svm = __ballot(onl_counted(code, in, mask, row) && !(pcode & RG_EV_BANDIT));
            if (svm) mine = static_cast<int32_t>(lane_value(pcode, top_bit(svm)) & RG_EV_INDEX_MASK);
            prev_code = lane_value(code, 63);
        }
        if (last && lane == 0) last[user] = mine;
    }
    const u64 e1 = __ballot(err & kErrFirstBandit) ? kErrFirstBandit : 0ull, e2 = __ballot(err & kErrProduct) ? kErrProduct : 0ull;
    if (lane == 0 && (e1 | e2)) (void)__hip_atomic_fetch_or(ws + kWsErr, e1 | e2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the scan over users, "the last value that is not -1": (1) every tile's own last value
__global__ __launch_bounds__(256) void k_online_tile_last(const int32_t* __restrict__ last, uint64_t n_users, int32_t* __restrict__ tile) {
    __shared__ u64 s[256];
    const uint64_t first = static_cast<uint64_t>(blockIdx.x) * kOnlTile + threadIdx.x * kOnlPer;
    u64 best = 0;                                   // (position + 1) << 32 | value: the largest position wins
    for (uint32_t k = 0; k < kOnlPer; ++k) {
        const uint64_t i = first + k;
        if (i < n_users && last[i] >= 0) best = (static_cast<u64>(threadIdx.x * kOnlPer + k + 1) << 32) | static_cast<uint32_t>(last[i]);
    }
    s[threadIdx.x] = best;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h && s[threadIdx.x + h] > s[threadIdx.x]) s[threadIdx.x] = s[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) tile[blockIdx.x] = s[0] ? static_cast<int32_t>(s[0] & 0xFFFFFFFFu) : -1;
}

// (2) one wave: every tile's incoming value, seeded with the carry; the value after the last tile is the new carry
__global__ __launch_bounds__(64) void k_online_tile_scan(int32_t* __restrict__ tile, uint32_t n_tiles, const int64_t* __restrict__ carry,
                                                         u64* __restrict__ ws) {
    const uint32_t lane = threadIdx.x;
    const int64_t c0 = carry[0];
    int32_t run = c0 < 0 ? -1 : static_cast<int32_t>(c0);
    for (uint32_t base = 0; base < n_tiles; base += 64) {
        const uint32_t i = base + lane;
        const int32_t v = i < n_tiles ? tile[i] : -1;
        const u64 m = __ballot(v >= 0);
        const u64 prior = m & lanes_below(lane);
        const int32_t from = __shfl(v, static_cast<int>(prior ? top_bit(prior) : 0u));
        if (i < n_tiles) tile[i] = prior ? from : run;
        if (m) run = static_cast<int32_t>(lane_value(static_cast<uint32_t>(v), top_bit(m)));
    }
    if (lane == 0) ws[kOnlWsCarry] = static_cast<u64>(static_cast<int64_t>(run));
}

// (3) every user's incoming value, in place
__global__ __launch_bounds__(256) void k_online_apply(int32_t* __restrict__ last, uint64_t n_users, const int32_t* __restrict__ tile) {
    __shared__ int32_t s[2][256];
    const uint64_t first = static_cast<uint64_t>(blockIdx.x) * kOnlTile + threadIdx.x * kOnlPer;
    int32_t v[kOnlPer];
    int32_t own = -1;
#pragma unroll
    for (uint32_t k = 0; k < kOnlPer; ++k) {
        v[k] = first + k < n_users ? last[first + k] : -1;
        if (v[k] >= 0) own = v[k];
    }
    uint32_t cur = 0;
    s[0][threadIdx.x] = own;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {          // inclusive scan: the later value wins where it is not -1
        const int32_t me = s[cur][threadIdx.x];
        const int32_t other = threadIdx.x >= d ? s[cur][threadIdx.x - d] : -1;
        s[cur ^ 1][threadIdx.x] = me >= 0 ? me : other;
        cur ^= 1;
        __syncthreads();
    }
    int32_t run = threadIdx.x ? s[cur][threadIdx.x - 1] : -1;
    if (run < 0) run = tile[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < kOnlPer; ++k) {
        if (first + k < n_users) last[first + k] = run;
        if (v[k] >= 0) run = v[k];
    }
}

__global__ __launch_bounds__(64 * kCntWaves) void k_online_train(rg_count_tables t, const rg_event* __restrict__ rows,
                                                                 const int64_t* __restrict__ offsets, uint64_t n_users,
                                                                 const uint8_t* __restrict__ mask, const int32_t* __restrict__ incoming,
                                                                 u64* __restrict__ ws, u64* __restrict__ none_n, u64* __restrict__ none_c,
                                                                 uint32_t n_waves) {
    __shared__ u64 s_key[kCntHashSlots];
    __shared__ u64 s_cnt[kCntHashSlots];
    for (uint32_t i = threadIdx.x; i < kCntHashSlots; i += 64 * kCntWaves) { s_key[i] = kCntEmpty; s_cnt[i] = 0; }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kCntWaves + wib;
    const uint32_t P = t.num_products;
    const bool do_co = t.co_counts != nullptr, do_b = t.pulls != nullptr;
    CntCtx c{s_key, s_cnt, reinterpret_cast<u64*>(t.co_counts), reinterpret_cast<u64*>(t.pulls), reinterpret_cast<u64*>(t.clicks), 0u};
    u64 n_upd = 0;          // wave-uniform count of the cell updates of this wave (lane 0 reports it)

    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        if (b >= e) continue;
        // the open session: entry i of its (product, views) list lives in lane i (rg_count.hip)
        uint32_t sp = 0, sc = 0, m = 0;
        bool longs = false;
        int64_t sess_start = b;
        // BanditCount: last_product_viewed in front of the chunk
        uint32_t cur = kCntNone;
        if (do_b) { const int32_t in0 = incoming[user]; cur = in0 < 0 ? kCntNone : static_cast<uint32_t>(in0); }
        uint32_t prev_code = RG_EV_BANDIT;

        // a counted row closes the open session, whose rows are sess_start .. end-1
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
        };

        for (int64_t base = b; base < e; base += 64) {
            const int64_t row = base + lane;
            const bool in = row < e;
            uint4 x = make_uint4(0u, 0u, 0u, 0u);
            if (in) x = reinterpret_cast<const uint4*>(rows)[row];
            const uint32_t idx = x.z & RG_EV_INDEX_MASK;
            const bool ok = in && idx < P;           // (k_online_check has refused a log with a product out of range)
            const bool iso = ok && !(x.z & RG_EV_BANDIT);
            const bool counted = ok && onl_counted(x.z, in, mask, row);
            const u64 omask = __ballot(iso), cmask = __ballot(counted), imask = __ballot(in);

            if (do_co) {
                u64 rem = imask;
                while (rem) {
                    // nothing open: on to the next organic row (the bandit rows behind it stay in `rem`: they end it)
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
                        if ((cmask >> k) & 1) close(base + k);      // any other bandit row drops the session uncounted
                        m = 0;
                        longs = false;
                    }
                }
            }

            if (do_b) {
                const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(x.z), 1));
                const uint32_t pcode = lane ? up : prev_code;
                // counted rows with a non-empty session: last_product_viewed moves to the view directly in front of them
                const u64 svm = __ballot(counted && !(pcode & RG_EV_BANDIT));
                const u64 prior = svm & lanes_below(lane);
                const uint32_t from = static_cast<uint32_t>(__shfl(static_cast<int>(pcode), static_cast<int>(prior ? top_bit(prior) : 0u)));
                const uint32_t ix = prior ? (from & RG_EV_INDEX_MASK) : cur;
                if (counted) {
                    const bool click = (x.z & RG_EV_CLICK) != 0;
                    if (ix == kCntNone) {
                        // NumPy's pulls_a[None, a] += 1: the whole row a — summed per action, added by k_online_none_rows
                        cnt_global(c, none_n, idx, 1);
                        if (click) cnt_global(c, none_c, idx, 1);
                    } else if (ix < P) {
                        cnt_add(c, 1, c.pulls, static_cast<u64>(ix) * P + idx, 1);
                        if (click) cnt_add(c, 2, c.clicks, static_cast<u64>(ix) * P + idx, 1);
                    }
                }
                n_upd += static_cast<u64>(__popcll(cmask)) + static_cast<u64>(__popcll(__ballot(counted && (x.z & RG_EV_CLICK))));
                if (svm) cur = lane_value(pcode, top_bit(svm)) & RG_EV_INDEX_MASK;
                prev_code = lane_value(x.z, 63);
            }
        }
        // (a session still open here ends with the user: never counted)
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
    const u64 g = wave_sum_u64(c.n_glob);
    if (lane == 0) {
        (void)__hip_atomic_fetch_add(&ws[kWsUpdates], n_upd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(&ws[kWsAtomics], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// pulls[a][:] += n_a, clicks[a][:] += c_a for the rows that met last_product_viewed = None (block a), and the new carry
__global__ __launch_bounds__(256) void k_online_none_rows(rg_count_tables t, const u64* __restrict__ none_n, const u64* __restrict__ none_c,
                                                          const u64* __restrict__ ws, int64_t* __restrict__ carry) {
    const uint32_t a = blockIdx.x, P = t.num_products;
    if (a == 0 && threadIdx.x == 0) carry[0] = static_cast<int64_t>(ws[kOnlWsCarry]);
    const int64_t n = static_cast<int64_t>(none_n[a]), c = static_cast<int64_t>(none_c[a]);
    if (n == 0 && c == 0) return;
    for (uint32_t j = threadIdx.x; j < P; j += 256) {
        t.pulls[static_cast<size_t>(a) * P + j] += n;
        t.clicks[static_cast<size_t>(a) * P + j] += c;
    }
}

inline size_t onl_tiles(uint64_t n_users) { return static_cast<size_t>((n_users + kOnlTile - 1) / kOnlTile); }
inline size_t onl_head_bytes(uint32_t P) { return (static_cast<size_t>(kWsWords) + 2 * static_cast<size_t>(P)) * sizeof(u64); }

}  // namespace

extern "C" size_t rg_evolution_workspace_bytes(uint32_t num_products) {
    return (static_cast<size_t>(kEvoWsHist) + num_products) * sizeof(u64);
}

extern "C" int rg_evolution_stats(const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                                  uint32_t num_products, uint8_t* d_explored, int64_t* d_counts, int64_t* d_action_clicks,
                                  void* d_workspace, size_t workspace_bytes, void* stream) {
    if (num_products == 0 || num_products > RG_EV_INDEX_MASK) return fail(RG_EINVAL, "rg_evolution_stats: bad num_products %u", num_products);
    if (eg && !(eg->epsilon >= 0.0 && eg->epsilon <= 1.0)) return fail(RG_EINVAL, "rg_evolution_stats: epsilon %g outside [0, 1]", eg->epsilon);
    if (!d_offsets || (n_users && !d_rows)) return fail(RG_EINVAL, "rg_evolution_stats: null rows / offsets");
    if (!d_counts || !d_action_clicks || !d_workspace) return fail(RG_EINVAL, "rg_evolution_stats: null counts / action clicks / workspace");
    if (workspace_bytes < rg_evolution_workspace_bytes(num_products))
        return fail(RG_ENOMEM, "rg_evolution_stats: workspace %zu < %zu bytes", workspace_bytes, rg_evolution_workspace_bytes(num_products));
    if (reinterpret_cast<uintptr_t>(d_rows) % 16) return fail(RG_EINVAL, "rg_evolution_stats: rows not 16-byte aligned");
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    hipStream_t s = static_cast<hipStream_t>(stream);
    u64* ws = static_cast<u64*>(d_workspace);
    HIP_TRY(hipMemsetAsync(ws, 0, rg_evolution_workspace_bytes(num_products), s));
    if (n_users == 0) return RG_OK;
    rg_ope_eg none{};
    const uint32_t blocks = evo_blocks(n_users);
    hipLaunchKernelGGL(k_evo_stats, dim3(blocks), dim3(64 * kCntWaves), 0, s, eg ? *eg : none, eg ? 1u : 0u, d_rows, d_offsets, n_users,
                       num_products, d_explored, ws, blocks * kCntWaves);
    HIP_TRY(hipGetLastError());
    const uint32_t cells = num_products < 4 ? 4 : num_products;
    hipLaunchKernelGGL(k_evo_commit, dim3((cells + 255) / 256), dim3(256), 0, s, ws, num_products, d_counts, d_action_clicks);
    HIP_TRY(hipGetLastError());
    u64 verdict = 0;
    HIP_TRY(hipMemcpyAsync(&verdict, ws + kWsErr, sizeof(verdict), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (verdict & kErrFirstBandit)
        return fail(RG_EINVAL, "rg_evolution_stats: a user opens with a bandit row (or its offsets descend); nothing was added");
    if (verdict & kErrProduct)
        return fail(RG_EINVAL, "rg_evolution_stats: the log has an index >= num_products %u; nothing was added", num_products);
    return RG_OK;
}

extern "C" size_t rg_count_online_workspace_bytes(uint32_t num_products, uint64_t n_users) {
    return onl_head_bytes(num_products) + ((n_users + onl_tiles(n_users) + 2) * sizeof(int32_t) + 7) / 8 * 8;
}

extern "C" int rg_count_train_online(const rg_count_tables* tables, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                                     const uint8_t* d_mask, int64_t* d_carry, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = count_tables_ok(tables, "rg_count_train_online")) return rc;
    if (!tables->co_counts && !tables->pulls) return fail(RG_EINVAL, "rg_count_train_online: no table given");
    if (!d_offsets || (n_users && !d_rows)) return fail(RG_EINVAL, "rg_count_train_online: null rows / offsets");
    if (!d_carry || !d_workspace) return fail(RG_EINVAL, "rg_count_train_online: null carry / workspace");
    const size_t need = rg_count_online_workspace_bytes(tables->num_products, n_users);
    if (workspace_bytes < need) return fail(RG_ENOMEM, "rg_count_train_online: workspace %zu < %zu bytes", workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(d_rows) % 16) return fail(RG_EINVAL, "rg_count_train_online: rows not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_workspace) % 8) return fail(RG_EINVAL, "rg_count_train_online: workspace not 8-byte aligned");
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t P = tables->num_products;
    u64* ws = static_cast<u64*>(d_workspace);
    u64 *none_n = ws + kWsWords, *none_c = none_n + P;
    int32_t* last = reinterpret_cast<int32_t*>(none_c + P);
    int32_t* tile = last + n_users;
    const bool do_b = tables->pulls != nullptr;
    HIP_TRY(hipMemsetAsync(ws, 0, onl_head_bytes(P), s));
    if (n_users == 0) return RG_OK;
    const uint32_t blocks = evo_blocks(n_users);
    hipLaunchKernelGGL(k_online_check, dim3(blocks), dim3(64 * kCntWaves), 0, s, d_rows, d_offsets, n_users, P, d_mask,
                       do_b ? last : nullptr, do_b ? d_carry : nullptr, ws, blocks * kCntWaves);
    HIP_TRY(hipGetLastError());
    u64 verdict = 0;
    HIP_TRY(hipMemcpyAsync(&verdict, ws + kWsErr, sizeof(verdict), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (verdict & kErrFirstBandit)
        return fail(RG_EINVAL, "rg_count_train_online: a user opens with a bandit row (or its offsets descend); no table was touched");
    if (verdict & kErrProduct)
        return fail(RG_EINVAL, "rg_count_train_online: the log has a product >= num_products %u; no table was touched", P);
    if (verdict & kErrCarry)
        return fail(RG_EINVAL, "rg_count_train_online: d_carry[0] >= num_products %u; no table was touched", P);
    if (do_b) {
        const uint32_t n_tiles = static_cast<uint32_t>(onl_tiles(n_users));
        hipLaunchKernelGGL(k_online_tile_last, dim3(n_tiles), dim3(256), 0, s, last, n_users, tile);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_online_tile_scan, dim3(1), dim3(64), 0, s, tile, n_tiles, d_carry, ws);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_online_apply, dim3(n_tiles), dim3(256), 0, s, last, n_users, tile);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_online_train, dim3(blocks), dim3(64 * kCntWaves), 0, s, *tables, d_rows, d_offsets, n_users, d_mask,
                       do_b ? last : nullptr, ws, none_n, none_c, blocks * kCntWaves);
    HIP_TRY(hipGetLastError());
    if (do_b) {
        hipLaunchKernelGGL(k_online_none_rows, dim3(P), dim3(256), 0, s, *tables, none_n, none_c, ws, d_carry);
        HIP_TRY(hipGetLastError());
    }
    return RG_OK;
}
