// rg_ope_logreg.hip — off-policy evaluation replay of the frozen LogReg policy (LogregFrozenAgent / LogregMulticlassIpsAgent,
// reference agents/logreg_ips.py:60-87) over a sorted device log: pi(a | the user's views so far) / ps for every bandit row.
//
// The skeleton is rg_ope_common.hpp's (one wave per user, 64-row chunks, per-wave sums and the fixed-order reduction).  What is
// this unit's own is the state a user carries and the act.  EpsilonGreedy round the argmax form (rg_ope_replay_logreg_eg) is
// k_ope_logreg<false, true>: the same replay, classes[argmax] as the wrapper's GREEDY action, pi from ope_model_pi's EG form.
//
// History.  The user's views are a (product, count) list in ASCENDING PRODUCT ORDER (the float64 walk adds the terms of a class
// in that order, as scipy's CSR x dense product does).  An organic row inserts or increments:
//   - up to 64 entries: entry i in lane i of two registers; the position is popcount(ballot(entry < p)), the tail moves up one
//     lane through a shuffle;
//   - up to 512 entries: a per-wave list in LDS;
//   - beyond: a per-wave list in global memory of max_user_rows entries (distinct products <= rows).
// Nothing is dropped (a dropped view is a wrong pi); the views persist across the user's sessions (the reference's feature
// provider is reset once per user).
//
// Act.  Computed only at a bandit row whose history changed since the user's previous act; the bandit rows up to the next
// organic row reuse it.
//   argmax form   fp32 scores from the fp32 copy of coef^T (lane = class, four class blocks per pass, history entries
//                 broadcast), accepted when best - second > 2 (nd + 3) 2^-24 (bmax + sum_p views_p wmax[p]) — k_logreg_acts'
//                 certificate; otherwise (near-ties, exact ties, no fp32 copy) the float64 walk in scipy's order, first maximum
//                 = smallest class index among equals (logreg_act_wave's arithmetic).  pi = [classes[argmax] == a].
//   softmax form  float64 scores in scipy's order, exp(s - max), per-lane partial sums over the classes lane, lane + 64, ...,
//                 the xor butterfly, e / sum — k_logreg_sample's arithmetic and decomposition, so a log the step loop wrote
//                 under the same model replays to ratios of exactly 1.  Classes 0 .. P-1, P <= 1024: the scores of a lane's
//                 (at most 16) classes stay in registers.
//   ranking form  recall@k of the sampling model (rg_ope_recall_logreg: k_ope_logreg<true, false, OpeRecall>): the softmax form's
//                 scores and numerators, then per counted row the rank rule on the numerators with a relative margin — HIT, MISS
//                 or, inside the margin at the k-th place, listed for the host.  No ratio, no float sums.
#include "rg_ope_common.hpp"

namespace {

typedef unsigned long long lr_u64;

constexpr uint32_t kLrRegs = 64;                 // entries of the register list
constexpr uint32_t kLrLds = 512;                 // entries of the per-wave LDS list (4 KiB per wave, 16 KiB per block)
constexpr uint32_t kLrMaxWaves = 4096;           // 256 CUs x 16 waves
constexpr uint32_t kLrSoftMax = 1024;            // classes of the softmax form
constexpr int kLrSoftBlocks = kLrSoftMax / 64;
constexpr uint32_t kLrNone = 0xFFFFFFFFu;
constexpr uint32_t kLrFp32MaxTerms = 1u << 16;   // longer histories go to the float64 walk

constexpr lr_u64 kLrErrFirstBandit = 1, kLrErrIndex = 2, kLrErrRows = 4;
constexpr int kLrWsErr = 0, kLrWsActs = 1, kLrWsExact = 2, kLrWsRowsRead = 3, kLrWsWords = 32;
constexpr int kLrWsUnresolved = 4, kLrWsOverflow = 5;      // the ranking form's (rg_ope_recall_logreg)

// recall@k, the ranking form: two softmax numerators e = exp(s - max) are ORDERED only where they differ by more than kRcRho
// relative — the host's p = e' / S' of the two classes then compare the same way (1 ulp per exp on either side,
// half an ulp per quotient: 5 2^-52 < 2^-49) — and not both lie under kRcTiny, beneath which an exp or, with S' <= 1024, a
// quotient may be subnormal and the relative bounds do not hold.
constexpr double kRcRho = 0x1p-48, kRcTiny = 0x1p-1000;
constexpr uint32_t kRcListCap = RG_OPE_RECALL_LIST_CAP, kRcListCapMax = 1u << 20;

// entries of a wave's global list (0: no user can outgrow the LDS list)
uint32_t lr_global_cap(uint32_t max_user_rows) { return max_user_rows > kLrLds ? max_user_rows : 0u; }
size_t lr_head_bytes() { return kLrWsWords * sizeof(lr_u64); }

__device__ __forceinline__ double lr_wave_max(double x) {
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o));
    return x;
}

// entry i of the history, wave-uniform (T = 0: registers, 1: LDS, 2: global)
template <int T>
struct LrHist {
    uint32_t hp, hc;
    const uint32_t* lp;
    const uint32_t* lc;
    __device__ __forceinline__ void get(uint32_t i, uint32_t& p, uint32_t& c) const {
        if (T == 0) { p = lane_value(hp, i); c = lane_value(hc, i); }
        else { p = wave_uniform(lp[i]); c = wave_uniform(lc[i]); }
    }
};

// fp32 scores and k_logreg_acts' margin certificate: true = class index *best_out IS the float64 argmax
template <int T>
__device__ __forceinline__ bool lr_fp32(const rg_ope_logreg& m, const LrHist<T>& h, uint32_t nd, uint32_t lane, uint32_t* best_out) {
    const uint32_t C = m.n_classes;
    float Ahat = m.bmax;
    for (uint32_t i = 0; i < nd; ++i) {
        uint32_t p, c;
        h.get(i, p, c);
        Ahat = fmaf(static_cast<float>(c), m.wmax[p], Ahat);
    }
    float best = -INFINITY, second = -INFINITY;
    uint32_t best_c = 0;
    for (uint32_t c0 = 0; c0 < C; c0 += 256) {
        float sc[4];
        uint32_t cc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cc[q] = min(c0 + 64u * q + lane, C - 1);                  // clamped: masked below
            sc[q] = m.intercept32[cc[q]];
        }
        for (uint32_t i = 0; i < nd; ++i) {
            uint32_t p, c;
            h.get(i, p, c);
            const float cnt = static_cast<float>(c);
            const float* row = m.coef32_t + static_cast<size_t>(p) * C;
#pragma unroll
            for (int q = 0; q < 4; ++q) sc[q] = fmaf(cnt, row[cc[q]], sc[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t c = c0 + 64u * q + lane;
            if (c < C) {
                if (sc[q] > best) { second = best; best = sc[q]; best_c = c; }
                else if (sc[q] > second) second = sc[q];
            }
        }
    }
    // wave top-2 over disjoint class sets (equal best scores leave a margin of 0: not certified)
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o), os = __shfl_xor(second, o);
        const uint32_t oc = __shfl_xor(best_c, o);
        const float ns = fmaxf(fminf(best, ob), fmaxf(second, os));
        if (ob > best) best_c = oc;
        best = fmaxf(best, ob);
        second = ns;
    }
    const float bound = static_cast<float>(nd + 3) * 5.9604644775390625e-08f * Ahat * 1.01f;
    *best_out = best_c;
    return C == 1 || best - second > 2.0f * bound;
}

// the float64 walk: per class the viewed products ascending, multiply then add, intercept last; first maximum
template <int T>
__device__ __forceinline__ uint32_t lr_walk(const rg_ope_logreg& m, const LrHist<T>& h, uint32_t nd, uint32_t lane) {
    const uint32_t C = m.n_classes;
    double best_s = -INFINITY;
    uint32_t best_c = kLrNone;
    for (uint32_t c0 = 0; c0 < C; c0 += 256) {
        double sc[4] = {0.0, 0.0, 0.0, 0.0};
        uint32_t cc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) cc[q] = min(c0 + 64u * q + lane, C - 1);
        for (uint32_t i0 = 0; i0 < nd; i0 += 4) {
            double w[4][4], cnt[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t p, c;
                h.get(min(i0 + e, nd - 1), p, c);
                cnt[e] = static_cast<double>(c);
                const double* row = m.coef_t + static_cast<size_t>(p) * C;
#pragma unroll
                for (int q = 0; q < 4; ++q) w[e][q] = row[cc[q]];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < nd) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) sc[q] = __dadd_rn(sc[q], __dmul_rn(cnt[e], w[e][q]));
                }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t c = c0 + 64u * q + lane;
            if (c < C) {
                const double v = __dadd_rn(sc[q], m.intercept[c]);
                if (best_c == kLrNone || v > best_s) { best_s = v; best_c = c; }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(best_s, o);
        const uint32_t oc = __shfl_xor(best_c, o);
        if (oc != kLrNone && (best_c == kLrNone || os > best_s || (os == best_s && oc < best_c))) { best_s = os; best_c = oc; }
    }
    return best_c;
}

// softmax numerators e[j] = exp(s - max) of the classes 64 j + lane and their sum (k_logreg_sample's arithmetic)
template <int T>
__device__ __forceinline__ void lr_soft(const rg_ope_logreg& m, const LrHist<T>& h, uint32_t nd, uint32_t lane,
                                        double (&ev)[kLrSoftBlocks], double& esum) {
    const uint32_t C = m.n_classes;
    double mx = -INFINITY;
#pragma unroll
    for (int g = 0; g < kLrSoftBlocks / 4; ++g) {
        double sc[4] = {0.0, 0.0, 0.0, 0.0};
        if (256u * g < C) {
            uint32_t cc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) cc[q] = min(256u * g + 64u * q + lane, C - 1);
            for (uint32_t i = 0; i < nd; ++i) {
                uint32_t p, c;
                h.get(i, p, c);
                const double cnt = static_cast<double>(c);
                const double* row = m.coef_t + static_cast<size_t>(p) * C;
#pragma unroll
                for (int q = 0; q < 4; ++q) sc[q] = __dadd_rn(sc[q], __dmul_rn(cnt, row[cc[q]]));
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t c = 256u * g + 64u * q + lane;
            double s = 0.0;
            if (c < C) { s = __dadd_rn(sc[q], m.intercept[c]); mx = fmax(mx, s); }
            ev[4 * g + q] = s;
        }
    }
    mx = lr_wave_max(mx);
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < kLrSoftBlocks; ++j) {
        const uint32_t c = 64u * j + lane;
        if (c < C) { const double e = exp(ev[j] - mx); ev[j] = e; sum += e; }
    }
    esum = wave_sum(sum);
}

__global__ void k_lr_init(lr_u64* __restrict__ ws) {
    if (threadIdx.x < kLrWsWords) ws[threadIdx.x] = 0;
}

// every user opens with an organic row and has at most max_user_rows rows; every product and action is < P
__global__ __launch_bounds__(256) void k_lr_check(const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets,
                                                  uint64_t n_users, uint32_t P, uint32_t max_user_rows, lr_u64* __restrict__ ws) {
    lr_u64 err = 0;
    for (uint64_t u = blockIdx.x * 256ull + threadIdx.x; u < n_users; u += gridDim.x * 256ull) {
        const int64_t b = offsets[u], e = offsets[u + 1];
        if (e < b || e - b > static_cast<int64_t>(max_user_rows)) err |= kLrErrRows;
        else if (b < e && (rows[b].code & RG_EV_BANDIT)) err |= kLrErrFirstBandit;
    }
    const int64_t r0 = offsets[0], r1 = offsets[n_users];
    for (int64_t r = r0 + blockIdx.x * 256ll + threadIdx.x; r < r1; r += gridDim.x * 256ll)
        if ((rows[r].code & RG_EV_INDEX_MASK) >= P) err |= kLrErrIndex;
    if (err) (void)__hip_atomic_fetch_or(&ws[kLrWsErr], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Eg = OpeRecall (softmax form only): no ratio — the rank rule's verdict on the next organic view of every counted row (rg_ope_recall_logreg)
template <bool kSoft, bool EG, typename... Eg>     // EG (argmax form only): pi is the EpsilonGreedy wrapper's round this act (rg_ope_replay_logreg_eg)
__global__ __launch_bounds__(64 * kOpeWaves, kSoft ? 2 : 4) void k_ope_logreg(
    rg_ope_logreg m, const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users, uint32_t ps_mode,
    const double* __restrict__ ps64, double ps_const, double* __restrict__ ratio, uint8_t* __restrict__ click,
    double* __restrict__ slots, uint32_t* __restrict__ gscr, uint32_t g_cap, lr_u64* __restrict__ ws, uint32_t n_waves,
    Eg... ega) {
    constexpr bool kRecall = (std::is_same_v<Eg, OpeRecall> || ... || false);
    static_assert(sizeof...(Eg) == ((EG || kRecall) ? 1 : 0), "the EG instantiation takes an OpeEg, the ranking one an OpeRecall, the plain one nothing");
    static_assert(!(kSoft && EG), "the wrapper's greedy action is the argmax form's");
    static_assert(!kRecall || (kSoft && !EG), "the ranking form is the softmax form's");
    __shared__ uint32_t s_p[kOpeWaves][kLrLds];
    __shared__ uint32_t s_c[kOpeWaves][kLrLds];
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kOpeWaves + wib;
    uint32_t* const lp = s_p[wib];
    uint32_t* const lc = s_c[wib];
    uint32_t* const gp = g_cap ? gscr + static_cast<size_t>(wave) * 2 * g_cap : nullptr;
    uint32_t* const gc = gp + g_cap;
    const uint32_t P = m.num_products;
    const OpeLog log{rows, offsets, n_users, ps_mode, ps64, ps_const, ratio, click, slots, n_waves};
    OpeAcc acc;
    lr_u64 c_acts = 0, c_exact = 0, c_rows = 0, err = 0;
    [[maybe_unused]] lr_u64 rc_counted = 0, rc_hits = 0;                           // (wave-uniform; the ranking form's)

    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        uint32_t hp = kLrNone, hc = 0, n = 0, tier = 0;
        bool dirty = true;
        uint32_t act_class = kLrNone;                 // argmax form: classes[argmax]
        double ev[kLrSoftBlocks], esum = 1.0;         // softmax form
#pragma unroll
        for (int j = 0; j < kLrSoftBlocks; ++j) ev[j] = 0.0;

        for (int64_t base = b; base < e; base += 64) {
            const OpeRow r = ope_load(log, base, e, lane);
            const uint32_t idx = r.idx;
            const bool ok = idx < P;                  // (the validation pass has refused such a log: never index the model)
            const bool isb = ok && r.isb, iso = ok && r.iso;
            const lr_u64 omask = __ballot(iso), bmask = __ballot(isb);
            double pi = 0.0;
            [[maybe_unused]] bool counted = false;
            [[maybe_unused]] uint32_t vnext = 0;
            [[maybe_unused]] uint8_t verdict = kRecallNotCounted;
            if constexpr (kRecall) {
                bool has_next;
                const uint32_t next = ope_next_code(rows, r.row, e, r.x.z, lane, has_next);
                vnext = next & RG_EV_INDEX_MASK;
                counted = isb && vnext < P && ope_recall_counted(r.x.z, next, has_next);
            }
            lr_u64 rem = omask | bmask;
            while (rem) {
                const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(rem));
                if ((omask >> k) & 1) {
                    const uint32_t p = lane_value(idx, k);
                    bool done = false;
                    if (tier == 0) {
                        const lr_u64 hit = __ballot(lane < n && hp == p);
                        if (hit) {
                            if (lane == static_cast<uint32_t>(__builtin_ctzll(hit))) hc += 1;
                            done = true;
                        } else if (n < kLrRegs) {
                            const uint32_t pos = static_cast<uint32_t>(__popcll(__ballot(lane < n && hp < p)));
                            const uint32_t up_p = static_cast<uint32_t>(__shfl_up(static_cast<int>(hp), 1));
                            const uint32_t up_c = static_cast<uint32_t>(__shfl_up(static_cast<int>(hc), 1));
                            if (lane > pos && lane <= n) { hp = up_p; hc = up_c; }
                            if (lane == pos) { hp = p; hc = 1; }
                            n += 1;
                            done = true;
                        } else {
                            lp[lane] = hp; lc[lane] = hc;             // the 65th product: on to the LDS list
                            ope_list_sync<true>();
                            tier = 1;
                        }
                    }
                    if (!done && tier == 1) {
                        if (n < kLrLds || !gp) {
                            done = true;
                            if (!ope_list_add<true>(lp, lc, n, kLrLds, p, lane)) err |= kLrErrRows;
                        } else {
                            for (uint32_t j = lane; j < n; j += 64) { gp[j] = lp[j]; gc[j] = lc[j]; }   // on to the global list
                            ope_list_sync<false>();
                            tier = 2;
                        }
                    }
                    if (!done && !ope_list_add<false>(gp, gc, n, g_cap, p, lane)) err |= kLrErrRows;
                    dirty = true;
                    rem &= rem - 1;
                    continue;
                }
                if (dirty) {
                    auto act = [&](auto hist) __attribute__((always_inline)) {
                        if (kSoft) {
                            lr_soft(m, hist, n, lane, ev, esum);
                            c_exact += 1;
                        } else {
                            uint32_t bc = 0;
                            // (the certificate's rounding-up factor covers (nd + 3) 2^-24 << 1)
                            if (!(m.coef32_t && n <= kLrFp32MaxTerms && lr_fp32(m, hist, n, lane, &bc))) { bc = lr_walk(m, hist, n, lane); c_exact += 1; }
                            act_class = static_cast<uint32_t>(m.classes[bc]);
                        }
                    };
                    if (tier == 0) act(LrHist<0>{hp, hc, nullptr, nullptr});
                    else if (tier == 1) act(LrHist<1>{0u, 0u, lp, lc});
                    else act(LrHist<2>{0u, 0u, gp, gc});
                    c_acts += 1;
                    c_rows += n;
                    dirty = false;
                }
                // the bandit rows up to the next organic row share this act
                const lr_u64 next_o = omask & ~lanes_below(k);
                const uint32_t end = next_o ? static_cast<uint32_t>(__builtin_ctzll(next_o)) : 64u;
                const bool mine = isb && lane >= k && lane < end;
                if constexpr (kRecall) {
                    // at most one row of the group is counted: the one in front of the next organic row
                    const lr_u64 cm = __ballot(mine && counted);
                    if (cm) {
                        const OpeRecall& rc = ope_pack_arg(ega...);
                        const uint32_t at = static_cast<uint32_t>(__builtin_ctzll(cm));
                        const uint32_t v = lane_value(vnext, at);     // v < P <= 1024
                        const uint32_t vq = v >> 6;
                        double ev_v = 0.0;
#pragma unroll
                        for (int j = 0; j < kLrSoftBlocks; ++j) {
                            if (64u * j < P) {
                                const double t = __shfl(ev[j], static_cast<int>(v & 63));
                                if (vq == static_cast<uint32_t>(j)) ev_v = t;
                            }
                        }
                        // not_less: classes that may rank at or above v (v itself among them); greater: those that certainly rank above
                        uint32_t not_less = 0, greater = 0;
#pragma unroll
                        for (int j = 0; j < kLrSoftBlocks; ++j) {
                            if (64u * j < P) {
                                const double x = ev[j];
                                const bool on = 64u * j + lane < P;
                                const bool near = fabs(x - ev_v) <= kRcRho * fmax(x, ev_v) || (x < kRcTiny && ev_v < kRcTiny);
                                not_less += static_cast<uint32_t>(__popcll(__ballot(on && (near || x > ev_v))));
                                greater += static_cast<uint32_t>(__popcll(__ballot(on && !near && x > ev_v)));
                            }
                        }
                        const uint8_t out = not_less <= rc.k ? kRecallHit : greater >= rc.k ? kRecallMiss : kRecallUnresolved;
                        if (lane == at) verdict = out;
                        rc_counted += 1;
                        rc_hits += out == kRecallHit ? 1 : 0;
                        if (out == kRecallUnresolved && lane == 0) {
                            const lr_u64 pos = __hip_atomic_fetch_add(&ws[kLrWsUnresolved], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (pos < rc.list_cap) {
                                uint32_t* q = rc.list + 3 * static_cast<size_t>(pos);
                                q[0] = static_cast<uint32_t>(user); q[1] = static_cast<uint32_t>(base - b) + at; q[2] = v;
                            } else {
                                (void)__hip_atomic_fetch_or(&ws[kLrWsOverflow], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            }
                        }
                    }
                } else if constexpr (kSoft) {
                    const uint32_t al = idx & 63, aq = idx >> 6;      // idx < P <= 1024
                    double v = 0.0;
#pragma unroll
                    for (int j = 0; j < kLrSoftBlocks; ++j) {
                        if (64u * j < P) {
                            const double t = __shfl(ev[j], static_cast<int>(al));
                            if (aq == static_cast<uint32_t>(j)) v = t;
                        }
                    }
                    if (mine) pi = v / esum;
                } else if (mine) {
                    pi = ope_model_pi(r, act_class, idx, ega...);
                }
                rem &= end < 64 ? ~lanes_below(end) : 0ull;
            }
            if constexpr (kRecall) {
                if (r.row < e) ope_pack_arg(ega...).hit[r.row] = verdict;
            } else {
                if (isb) acc.emit(log, r, pi);
            }
        }
    }
    if constexpr (!kRecall) acc.store(log, wave, lane);
    if (lane == 0) {
        if constexpr (kRecall) {
            const OpeRecall& rc = ope_pack_arg(ega...);
            // (integer adds: the sums do not depend on their order)
            if (rc_counted) (void)__hip_atomic_fetch_add(&rc.sums[0], rc_counted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (rc_hits) (void)__hip_atomic_fetch_add(&rc.sums[1], rc_hits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (c_acts) {
            (void)__hip_atomic_fetch_add(&ws[kLrWsActs], c_acts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(&ws[kLrWsRowsRead], c_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c_exact) (void)__hip_atomic_fetch_add(&ws[kLrWsExact], c_exact, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (err) (void)__hip_atomic_fetch_or(&ws[kLrWsErr], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int lr_model_ok(const rg_ope_logreg* m, const char* who) {
    if (!m) return fail(RG_EINVAL, "%s: null model", who);
    if (m->num_products == 0 || m->num_products > RG_EV_INDEX_MASK) return fail(RG_EINVAL, "%s: bad num_products %u", who, m->num_products);
    if (m->n_classes == 0) return fail(RG_EINVAL, "%s: n_classes == 0", who);
    if (!m->coef_t || !m->intercept || !m->classes) return fail(RG_EINVAL, "%s: null coef_t / intercept / classes", who);
    const int n32 = (m->coef32_t != nullptr) + (m->intercept32 != nullptr) + (m->wmax != nullptr);
    if (n32 != 0 && n32 != 3) return fail(RG_EINVAL, "%s: coef32_t, intercept32 and wmax come together", who);
    if (m->select_randomly && (m->n_classes != m->num_products || m->num_products > kLrSoftMax))
        return fail(RG_EINVAL, "%s: select_randomly needs the classes 0 .. P-1 and P <= %u (P = %u, %u classes)", who, kLrSoftMax,
                    m->num_products, m->n_classes);
    return RG_OK;
}

}  // namespace

// the head of a history-keeping unit's workspace zeroed (32 words) and the log validated, before anything is written (rg_ope_common.hpp)
int rgk::ope_check_log(const char* who, const OpeCall& c, uint32_t P, unsigned long long* ws) {
    const hipStream_t s = c.stream;
    hipLaunchKernelGGL(k_lr_init, dim3(1), dim3(64), 0, s, ws);
    HIP_TRY(hipGetLastError());
    if (!c.n_users) return RG_OK;
    const uint32_t check_blocks = static_cast<uint32_t>(c.n_users / 256 + 1 > 2048 ? 2048 : c.n_users / 256 + 1);
    hipLaunchKernelGGL(k_lr_check, dim3(check_blocks), dim3(256), 0, s, c.d_rows, c.d_offsets, c.n_users, P, c.max_user_rows, ws);
    HIP_TRY(hipGetLastError());
    lr_u64 verdict = 0;
    HIP_TRY(hipMemcpyAsync(&verdict, ws + kLrWsErr, sizeof(verdict), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (verdict & kLrErrRows)
        return fail(RG_EINVAL, "%s: a user has more than max_user_rows = %u rows (or its offsets descend); nothing was written", who, c.max_user_rows);
    if (verdict & kLrErrFirstBandit) return fail(RG_EINVAL, "%s: a user opens with a bandit row; nothing was written", who);
    if (verdict & kLrErrIndex)
        return fail(RG_EINVAL, "%s: the log has a product or an action >= num_products %u; nothing was written", who, P);
    return RG_OK;
}

extern "C" size_t rg_ope_logreg_workspace_bytes(const rg_ope_logreg* m, uint64_t n_users, uint32_t max_user_rows) {
    if (!m) { fail(RG_EINVAL, "rg_ope_logreg_workspace_bytes: null model"); return 0; }
    const uint32_t W = ope_waves(n_users, kLrMaxWaves);
    return lr_head_bytes() + ope_slot_bytes(W) + static_cast<size_t>(W) * 2 * lr_global_cap(max_user_rows) * sizeof(uint32_t);
}

namespace {

template <bool EG>       // ega: null iff !EG
int lr_replay(const char* who, const rg_ope_logreg* m, const OpeEg* ega, const OpeCall& c) {
    if (int rc = ope_args_ok(who, c, rg_ope_logreg_workspace_bytes(m, c.n_users, c.max_user_rows))) return rc;
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    const hipStream_t s = c.stream;
    if (m->select_randomly) {
        static_assert(kLrSoftMax <= 1024, "the class check reads them into a stack array");
        int32_t cls[kLrSoftMax];
        HIP_TRY(hipMemcpyAsync(cls, m->classes, m->n_classes * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint32_t k = 0; k < m->n_classes; ++k)
            if (cls[k] != static_cast<int32_t>(k))
                return fail(RG_EINVAL, "%s: select_randomly needs classes[c] == c (classes[%u] = %d)", who, k, cls[k]);
    }
    const uint32_t W = ope_waves(c.n_users, kLrMaxWaves);
    const uint32_t g_cap = lr_global_cap(c.max_user_rows);
    lr_u64* ws = c.at<lr_u64>(0);
    double* slots = c.at<double>(lr_head_bytes());
    uint32_t* gscr = g_cap ? c.at<uint32_t>(lr_head_bytes() + ope_slot_bytes(W)) : nullptr;
    if (int rc = ope_check_log(who, c, m->num_products, ws)) return rc;
    // one spelling of the launch: the kernel, and the EG form's one more argument
    auto launch = [&](auto kernel, auto... eg) {
        hipLaunchKernelGGL(kernel, dim3(W / kOpeWaves), dim3(64 * kOpeWaves), 0, s, *m, c.d_rows, c.d_offsets, c.n_users, c.ps_mode, c.d_ps,
                           c.ps_const, c.d_ratio, c.d_click, slots, gscr, g_cap, ws, W, eg...);
    };
    if constexpr (EG) launch(k_ope_logreg<false, true, OpeEg>, *ega);
    else if (m->select_randomly) launch(k_ope_logreg<true, false>);
    else launch(k_ope_logreg<false, false>);
    HIP_TRY(hipGetLastError());
    return ope_reduce(slots, W, c.d_sums, s);
}

}  // namespace

extern "C" int rg_ope_replay_logreg(const rg_ope_logreg* m, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                                    uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                                    uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = lr_model_ok(m, "rg_ope_replay_logreg")) return rc;
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    return lr_replay<false>("rg_ope_replay_logreg", m, nullptr, c);
}

extern "C" int rg_ope_replay_logreg_eg(const rg_ope_logreg* m, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                                       uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                                       double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                                       void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = lr_model_ok(m, "rg_ope_replay_logreg_eg")) return rc;
    if (m->select_randomly)
        return fail(RG_EINVAL, "rg_ope_replay_logreg_eg: a select_randomly model samples its act: no replay form under EpsilonGreedy");
    if (int rc = ope_eg_ok("rg_ope_replay_logreg_eg", eg, m->num_products)) return rc;
    const OpeEg ega{*eg, d_greedy, d_h0};
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    return lr_replay<true>("rg_ope_replay_logreg_eg", m, &ega, c);
}

// ---- recall@k, the ranking form (the sampling model only): k_ope_logreg<true, false, OpeRecall> ----
namespace {

uint32_t rc_list_cap(uint32_t list_cap) { return list_cap ? list_cap : kRcListCap; }
size_t rc_list_bytes(uint32_t cap) { return (static_cast<size_t>(cap) * 3 * sizeof(uint32_t) + 255) & ~size_t(255); }

}  // namespace

extern "C" size_t rg_ope_recall_logreg_workspace_bytes(const rg_ope_logreg* m, uint64_t n_users, uint32_t max_user_rows, uint32_t list_cap) {
    if (!m) { fail(RG_EINVAL, "rg_ope_recall_logreg_workspace_bytes: null model"); return 0; }
    if (list_cap > kRcListCapMax) { fail(RG_EINVAL, "rg_ope_recall_logreg_workspace_bytes: list_cap %u > %u", list_cap, kRcListCapMax); return 0; }
    const uint32_t W = ope_waves(n_users, kLrMaxWaves);
    return lr_head_bytes() + rc_list_bytes(rc_list_cap(list_cap)) + static_cast<size_t>(W) * 2 * lr_global_cap(max_user_rows) * sizeof(uint32_t);
}

extern "C" int rg_ope_recall_logreg(const rg_ope_logreg* m, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                                    uint32_t max_user_rows, uint32_t k, uint32_t list_cap, uint8_t* d_hit, int64_t* d_sums,
                                    void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* who = "rg_ope_recall_logreg";
    if (int rc = lr_model_ok(m, who)) return rc;
    if (!m->select_randomly) return fail(RG_EINVAL, "%s: the ranking form is the sampling model's (select_randomly != 0)", who);
    if (k == 0 || k > m->num_products) return fail(RG_EINVAL, "%s: k %u outside 1 .. %u", who, k, m->num_products);
    if (list_cap > kRcListCapMax) return fail(RG_EINVAL, "%s: list_cap %u > %u", who, list_cap, kRcListCapMax);
    if (n_users && (!d_rows || !d_offsets || !d_hit)) return fail(RG_EINVAL, "%s: null rows / offsets / hit", who);
    if (!d_sums || !d_workspace) return fail(RG_EINVAL, "%s: null sums / workspace", who);
    const size_t need = rg_ope_recall_logreg_workspace_bytes(m, n_users, max_user_rows, list_cap);
    if (workspace_bytes < need) return fail(RG_ENOMEM, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(d_rows) % 16) return fail(RG_EINVAL, "%s: rows not 16-byte aligned", who);
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t cls[kLrSoftMax];
    HIP_TRY(hipMemcpyAsync(cls, m->classes, m->n_classes * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t c = 0; c < m->n_classes; ++c)
        if (cls[c] != static_cast<int32_t>(c)) return fail(RG_EINVAL, "%s: needs classes[c] == c (classes[%u] = %d)", who, c, cls[c]);
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, RG_OPE_PS_ROW, nullptr, 0.0, nullptr, nullptr, nullptr, d_workspace,
                    workspace_bytes, s};
    const uint32_t W = ope_waves(n_users, kLrMaxWaves);
    const uint32_t g_cap = lr_global_cap(max_user_rows), cap = rc_list_cap(list_cap);
    lr_u64* ws = c.at<lr_u64>(0);
    uint32_t* list = c.at<uint32_t>(lr_head_bytes());
    uint32_t* gscr = g_cap ? c.at<uint32_t>(lr_head_bytes() + rc_list_bytes(cap)) : nullptr;
    if (int rc = ope_check_log(who, c, m->num_products, ws)) return rc;
    HIP_TRY(hipMemsetAsync(d_sums, 0, 2 * sizeof(int64_t), s));
    const OpeRecall out{d_hit, reinterpret_cast<unsigned long long*>(d_sums), list, cap, k};
    hipLaunchKernelGGL((k_ope_logreg<true, false, OpeRecall>), dim3(W / kOpeWaves), dim3(64 * kOpeWaves), 0, s, *m, d_rows, d_offsets, n_users,
                       static_cast<uint32_t>(RG_OPE_PS_ROW), static_cast<const double*>(nullptr), 0.0, static_cast<double*>(nullptr),
                       static_cast<uint8_t*>(nullptr), static_cast<double*>(nullptr), gscr, g_cap, ws, W, out);
    HIP_TRY(hipGetLastError());
    return RG_OK;
}
