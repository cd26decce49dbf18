// rg_logreg_poly.hip — librecogym_hip.so: the act of the likelihood agent (LogregPolyAgent, RG_POLICY_LOGREG_POLY) in the step loop.
// (see rg_common.hpp for the shared types and helpers, DESIGN.md 4f for the contract, the merge rule and its proof)

#include "rg_common.hpp"

namespace rgk {

// ------------------------------------------------------------------------------------------
// The reference's act (agents/logreg_poly.py:143-167) is argmax(predict_proba[:, 1]) of a BINARY model over P feature rows, one
// per action: [view counts | the action's index at column a | kron(counts, ones(P)) laid out in slices of n per action].  With
// w = coef_[0] split into wf = w[:P], wa = w[P:2P], wk = w[2P:].reshape(P, P) the decision of action a over the viewed products
// p_0 < ... < p_(n-1) with counts c_j is, in float64, multiply then add, in this order (rg_sim_set_logreg_poly):
//     s = 0;  for j: s += c_j wf[p_j];   s += a wa[a];   for j: s += c_((a n + j) / P) wk[a][p_j];   z[a] = s + b
// — the count of the cross term is the reference's (a n + j) / P-th, not the product's own: reproduced, not fixed.  expit is
// monotone but not injective on doubles, and the decisions are large (z >= 20 in 6.6 % of the acts of a fitted P = 40 model), so
// the action is NOT argmax z: where two decisions round to one expit value the lower index wins.  The host tabulates the top
// steps of expit (th[k] = the smallest double with expit >= 1 - k 2^-53); the step of a decision is the number of thresholds
// above it, an exact comparison.  z* = max z, a* = its first index:
//   z* >= th[K - 1]   the action is the lowest index on the lowest step: exact (RG_CNT_POLY_TABLE);
//   below             the action is a*; the act is UNRESOLVED when some a < a* has 0 < z* - z[a] <= W(z*) (poly_margin): counted,
//                     listed, and recomputed by the host with scipy's expit.  (z* < -700, where expit leaves the normal doubles:
//                     unresolved whenever a* > 0.)
// k_poly_acts: a wave per listed act (k_logreg_select's list), lanes striding over the actions, float64 throughout.  The sorted
// history is read once into LDS (counts as doubles, products); the prefix sum_j c_j wf[p_j] is taken once per act; a lane walks
// four actions and four history entries at a time (16 independent loads of wk_t in flight, as logreg_act_wave), each action's
// terms still added in history order.  The quirk index (a n + j) / P is one 64-bit divide per (lane, action) and an incremental
// (quotient, remainder) pair along j.  One pass keeps, per lane, the lowest step with its first index, the best decision with
// its first index, and the second best DISTINCT decision; the wave reduction of those decides the table zone and tells
// whether ANY decision lies within W of z*; only then (rare) a second pass recomputes the decisions below a* for the index test.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kPolyHist = 256;       // history entries a wave keeps in LDS (the default history row); beyond: read from the row
constexpr uint32_t kPolyNone = 0xFFFFFFFFu;
constexpr double kPolyFloor = -700.0;     // z* below this: outside the domain of the margin's proof (poly_act_wave)

// number of thresholds above z (th never increases, K of them; equal neighbours are fine): K = below the table
__device__ __forceinline__ uint32_t poly_step(const double* th, uint32_t K, double z) {
    if (!(z >= th[K - 1])) return K;
    uint32_t lo = 0, hi = K - 1;            // th[hi] <= z: the first k with th[k] <= z
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (th[mid] <= z) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// W(z*) = 2^-49 (1 + 2^m), m = ceil(z* log2 e) + 1 >= log2 exp(z*): an upper bound of 8 2^-52 (1 + exp(z*)) made of IEEE
// operations only, so that the host restates it to the bit (agents/logreg_poly.py: poly_margin)
__device__ __forceinline__ double poly_margin(double zs) {
    double m = ceil(__dmul_rn(zs, 1.4426950408889634)) + 1.0;
    m = fmin(fmax(m, -1100.0), 1023.0);
    return __dmul_rn(0x1p-49, __dadd_rn(1.0, ldexp(1.0, static_cast<int>(m))));
}

// f(a, z[a]) for every action a < a_end this lane owns (a = lane, lane + 64, ...: ascending), in the contract's order
template <class F>
__device__ __forceinline__ void poly_scan(const DevSim& d, const hent_t* hr, uint32_t nd, const double* s_cnt, const uint32_t* s_prod,
                                          double prefix, uint32_t a_end, int lane, F&& f) {
    const uint32_t P = d.P;
    for (uint32_t a0 = 0; a0 < a_end; a0 += 256) {
        double sc[4];
        uint32_t aa[4], qq[4], rr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            aa[q] = min(a0 + 64u * q + lane, P - 1);                       // clamped: masked below
            sc[q] = __dadd_rn(prefix, __dmul_rn(static_cast<double>(aa[q]), d.pl_wa[aa[q]]));
            const unsigned long long an = static_cast<unsigned long long>(aa[q]) * nd;
            qq[q] = static_cast<uint32_t>(an / P);                         // (a n + j) / P at j = 0, then kept incrementally
            rr[q] = static_cast<uint32_t>(an - static_cast<unsigned long long>(qq[q]) * P);
        }
        for (uint32_t i0 = 0; i0 < nd; i0 += 4) {
            double w[4][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t ie = min(i0 + e, nd - 1);
                const uint32_t prod = ie < kPolyHist ? s_prod[ie] : h_prod(hr[ie]);
                const double* row = d.pl_wk_t + static_cast<size_t>(prod) * P;
#pragma unroll
                for (int q = 0; q < 4; ++q) w[e][q] = row[aa[q]];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < nd) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double c = qq[q] < kPolyHist ? s_cnt[qq[q]] : static_cast<double>(h_cnt(hr[qq[q]]));   // qq < nd here
                        sc[q] = __dadd_rn(sc[q], __dmul_rn(c, w[e][q]));
                        if (++rr[q] == P) { rr[q] = 0; ++qq[q]; }
                    }
                }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t a = a0 + 64u * q + lane;
            if (a < a_end) f(a, __dadd_rn(sc[q], d.pl_b));
        }
    }
}

// The act of the user in `slot` (wave-uniform), by the whole wave.  s_cnt / s_prod: this wave's LDS rows; s_th: the block's copy
// of the step table.  *flags: bit 0 decided on the table, bit 1 unresolved, bit 2 a lower index than a* won.
__device__ uint32_t poly_act_wave(const DevSim& d, uint32_t slot, int lane, const double* s_th, double* s_cnt, uint32_t* s_prod,
                                  uint32_t* flags) {
    const hent_t* hr = hist_row(d, slot) + 1;             // entries after the header
    const uint32_t nd = h_cnt(hr[-1]);
    for (uint32_t i = lane; i < nd && i < kPolyHist; i += 64) {
        const hent_t x = hr[i];
        s_cnt[i] = static_cast<double>(h_cnt(x));
        s_prod[i] = h_prod(x);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // the common prefix, once per act: the products c_j wf[p_j] a lane each (independent loads), summed in history order
    double prefix = 0.0;
    for (uint32_t i0 = 0; i0 < nd; i0 += 64) {
        const uint32_t i = i0 + lane;
        double term = 0.0;
        if (i < nd) {
            const hent_t x = hr[i];
            term = __dmul_rn(static_cast<double>(h_cnt(x)), d.pl_wf[h_prod(x)]);
        }
        const uint32_t m = min(64u, nd - i0);
        for (uint32_t k = 0; k < m; ++k) prefix = __dadd_rn(prefix, __shfl(term, static_cast<int>(k)));
    }
    const uint32_t K = d.pl_nth;
    double v1 = -INFINITY, v2 = -INFINITY;                // best decision, second best distinct one
    uint32_t a1 = kPolyNone, smin = K + 1, sa = kPolyNone; // first index of v1; lowest step and its first index
    poly_scan(d, hr, nd, s_cnt, s_prod, prefix, d.P, lane, [&](uint32_t a, double z) {
        if (a1 == kPolyNone || z > v1) { if (a1 != kPolyNone) v2 = v1; v1 = z; a1 = a; }
        else if (z < v1 && z > v2) v2 = z;
        const uint32_t st = poly_step(s_th, K, z);
        if (st < smin) { smin = st; sa = a; }
    });
    for (int o = 32; o > 0; o >>= 1) {
        const double ov1 = __shfl_xor(v1, o), ov2 = __shfl_xor(v2, o);
        const uint32_t oa1 = __shfl_xor(a1, o), osm = __shfl_xor(smin, o), osa = __shfl_xor(sa, o);
        const bool take = oa1 != kPolyNone && (a1 == kPolyNone || ov1 > v1 || (ov1 == v1 && oa1 < a1));
        const double n1 = take ? ov1 : v1;
        const double c = v1 < n1 ? v1 : v2, e = ov1 < n1 ? ov1 : ov2;     // each side's best below the joint best
        v2 = fmax(c, e);
        v1 = n1;
        if (take) a1 = oa1;
        if (osm < smin || (osm == smin && osa < sa)) { smin = osm; sa = osa; }
    }
    uint32_t action, fl = 0;
    if (smin < K) {                                       // z* lies on the table: the lowest index on its step, exactly
        action = sa;
        fl = 1u | (sa != a1 ? 4u : 0u);
    } else {
        action = a1;
        const double W = poly_margin(v1);
        // below kPolyFloor expit leaves the normal doubles (subnormal from z = -708, 0 from -745): decisions any distance apart may
        // merge there and W's proof does not hold, so such an act is unresolved whenever a lower index exists
        if (v1 < kPolyFloor) { if (a1 != 0u) fl = 2u; }
        else if (__dsub_rn(v1, v2) <= W) {                     // some decision within W of z*: is one of them at a lower index?
            bool hit = false;
            poly_scan(d, hr, nd, s_cnt, s_prod, prefix, a1, lane, [&](uint32_t, double z) {
                const double g = __dsub_rn(v1, z);
                if (g > 0.0 && g <= W) hit = true;
            });
            if (__ballot(hit)) fl = 2u;
        }
    }
    __builtin_amdgcn_wave_barrier();                      // the LDS rows are the next act's from here
    *flags = fl;
    return action;
}

__global__ void __launch_bounds__(kBlock) k_poly_acts(DevSim d, uint32_t t) {
    __shared__ double s_th[kPolySteps];
    __shared__ double s_cnt[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_prod[kBlock / 64][kPolyHist];
    __shared__ unsigned long long s_sum[4];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < d.pl_nth; i += kBlock) s_th[i] = d.pl_th[i];
    if (threadIdx.x < 4) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t n = d.lr_cnt[t];
    const uint32_t waves_total = gridDim.x * (kBlock / 64);
    unsigned long long c_acts = 0, c_rows = 0, c_table = 0;
    for (uint32_t w = blockIdx.x * (kBlock / 64) + wave; w < n; w += waves_total) {
        const uint32_t slot = d.lr_list[w];
        const uint32_t uidx = d.uid[slot];
        uint32_t fl = 0;
        const uint32_t action = poly_act_wave(d, slot, lane, s_th, s_cnt[wave], s_prod[wave], &fl);
        c_acts += 1; c_rows += h_cnt(hist_row(d, slot)[0]);
        c_table += fl & 1u;
        if (lane == 0) {
            d.lr_action[uidx] = action; d.lr_dirty[uidx] = 0;
            if (fl & 2u) {       // (user id, the event index the act was computed at, the action taken) for the host
                const unsigned long long pos = atomicAdd(&d.counters[RG_CNT_POLY_UNRESOLVED], 1ull);
                if (pos < kPolyListCap) {
                    uint32_t* e = d.pl_list + 3 * static_cast<size_t>(pos);
                    e[0] = static_cast<uint32_t>(d.first_user + uidx); e[1] = d.run_ahead ? d.ev[uidx] : t; e[2] = action;
                }
            }
        }
    }
    // the counters once per block (as k_logreg_decide)
    if (lane == 0 && c_acts) {
        atomicAdd(&s_sum[0], c_acts);
        atomicAdd(&s_sum[1], c_rows);
        if (c_table) atomicAdd(&s_sum[2], c_table);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_sum[0]) {
        atomicAdd(&d.counters[RG_CNT_LR_ACTS], s_sum[0]);
        atomicAdd(&d.counters[RG_CNT_LR_ROWS], s_sum[1]);
        if (s_sum[2]) atomicAdd(&d.counters[RG_CNT_POLY_TABLE], s_sum[2]);
    }
}

// rg_sim_debug_poly_acts: the same act for every user index of the reset range (slot == user index right after the reset)
__global__ void __launch_bounds__(kBlock) k_debug_poly_acts(DevSim d, int32_t* action, uint8_t* flags) {
    __shared__ double s_th[kPolySteps];
    __shared__ double s_cnt[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_prod[kBlock / 64][kPolyHist];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < d.pl_nth; i += kBlock) s_th[i] = d.pl_th[i];
    __syncthreads();
    const uint32_t waves_total = gridDim.x * (kBlock / 64);
    for (uint32_t i = blockIdx.x * (kBlock / 64) + wave; i < d.n_users; i += waves_total) {
        uint32_t fl = 0;
        const uint32_t a = poly_act_wave(d, i, lane, s_th, s_cnt[wave], s_prod[wave], &fl);
        if (lane == 0) { action[i] = static_cast<int32_t>(a); flags[i] = static_cast<uint8_t>(fl); }
    }
}

search_kernel_t poly_acts_kernel() { return k_poly_acts; }
void (*poly_debug_kernel())(DevSim, int32_t*, uint8_t*) { return k_debug_poly_acts; }

}  // namespace rgk
