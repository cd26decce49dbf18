// rg_bayes_common.hpp — the act of BayesianAgentVB (RG_POLICY_BAYES_VB) on one history, by a whole wave: shared by the step loop
// (rg_bayes_vb.hip) and the off-policy replay (rg_ope_bayes.hip, as rg_ope_poly.hip takes poly_act).  DESIGN.md 4h has the contract, the
// margin W term by term and the proof of the saturated zone.
//
// The reference's act (agents/bayesian_poly_vb.py:71-91) is argmax_a mean_s expit(sum_p views[p] Lambda[s][p P + a]) over the S
// posterior samples.  Its matmul adds the non-zero terms in BLAS's order, so its value is not a function of the inputs alone; the
// device computes, in float64, multiply then add, over the viewed products p_0 < ... < p_(n-1) with counts c_j (rg_sim_set_bayes_vb):
//     z[a][s] = 0;  for j: z[a][s] += c_j lam_t[p_j][a][s]          m[a][s] = sum_j |c_j lam_t[p_j][a][s]|, M = max m
//     q[a] = (sum_s 1 / (1 + exp(-z[a][s]))) / S
// and decides by the margin W(n, M, S) (bayes_margin) that bounds |q[a] - the reference's mean of a| in ANY summation order:
//   n = 0           action 0 (every mean is 0.5 on both sides);
//   ez >= 1         (ez = (2 n + 4) 2^-53 M, the reordering bound on z) the first maximum of q, UNRESOLVED;
//   A1 = {a: min_s z[a][s] >= kBayesZsat} not empty: a_c = min A1, SATURATED — the reference's mean of a_c is exactly 1.0, the largest
//                   possible value — and UNRESOLVED when some a < a_c has 1 - q[a] <= W (its reference mean may be 1.0 too);
//   else            a* = the first maximum of q; UNRESOLVED when any other action has q[a*] - q[a] <= 2 W.
// bayes_act: lanes stride over the samples (lam_t's s axis is contiguous: 512 bytes per (p, a) and wave), four actions at a time
// (independent loads in flight), each lane's z in the contract's order; per action a lane keeps a partial sum of expit, the
// running min z and the running max m, reduced by a fixed xor butterfly (the same bits in every lane and in every run); the
// per-action results are wave-uniform registers.  Lanes beyond S in the last stride take no part: their partial sum is the
// identity 0.0 and their minimum +inf; no model value is read for them.
//
// Template parameters as poly_act's:  M  the model, members P, by_S, by_lam_t (BayesModel; the step loop fills one from DevSim);
//                                     H  the history, ascending by product (PolyRowHist, PolyListHist).
#pragma once

#include "rg_poly_common.hpp"

namespace rgk {

constexpr double kBayesZsat = RG_BAYES_ZSAT;      // expit is exactly 1.0 from 36.74 upwards; 40 leaves room for a z error below 1

struct BayesModel {
    uint32_t P, by_S;
    const double* by_lam_t;
};

// W = ez / 4 + (2 S + 44) 2^-53 with ez = (2 n + 4) 2^-53 M, IEEE operations only (agents/bayesian_poly_vb.py: bayes_margin computes
// the same bits).  An upper bound of the five terms of DESIGN.md 4h whenever ez < 1.
__device__ __forceinline__ double bayes_margin(uint32_t n, double M, uint32_t S, double* ez_out) {
    const double ez = __dmul_rn(ldexp(static_cast<double>(2ull * n + 4ull), -53), M);
    *ez_out = ez;
    return __dadd_rn(__dmul_rn(ez, 0.25), ldexp(static_cast<double>(2ull * S + 44ull), -53));
}

__device__ __forceinline__ double bayes_expit(double z) { return __ddiv_rn(1.0, __dadd_rn(1.0, exp(-z))); }

// The act on the history `h` (wave-uniform), by the whole wave.  s_cnt / s_prod: this wave's LDS rows (kPolyHist entries each).
// *flags: RG_BAYES_SATURATED | RG_BAYES_UNRESOLVED.  q_out (or nullptr): P doubles that receive the means.
template <class M, class H>
__device__ __forceinline__ uint32_t bayes_act(const M& d, const H& h, int lane, double* s_cnt, uint32_t* s_prod, uint32_t* flags,
                                              double* q_out) {
    const uint32_t nd = h.size(), P = d.P, S = d.by_S;
    if (nd == 0) {                                        // every z is +0: every mean 0.5 on both sides, the first index wins
        if (q_out) for (uint32_t a = lane; a < P; a += 64) q_out[a] = 0.5;
        *flags = 0;
        return 0;
    }
    for (uint32_t i = lane; i < nd && i < kPolyHist; i += 64) {
        uint32_t p;
        typename H::val_t c;
        h.get(i, p, c);
        s_cnt[i] = static_cast<double>(c);
        s_prod[i] = p;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    double v1 = 0.0, v2 = -INFINITY, qlow = -INFINITY;    // best mean, the best among the others, the best below a_c
    uint32_t a1 = 0, ac = kPolyNone;                       // first index of v1; the lowest saturated action
    double mx = 0.0;                                       // this lane's max m
    for (uint32_t a0 = 0; a0 < P; a0 += 4) {
        size_t off[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) off[q] = static_cast<size_t>(min(a0 + q, P - 1)) * S;      // clamped: masked below
        double sum[4] = {0.0, 0.0, 0.0, 0.0}, zmn[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
        for (uint32_t s = lane; s < S; s += 64) {
            double z[4] = {0.0, 0.0, 0.0, 0.0}, m[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
            for (uint32_t i = 0; i < nd; ++i) {
                const uint32_t prod = i < kPolyHist ? s_prod[i] : h.prod(i);
                const double c = i < kPolyHist ? s_cnt[i] : static_cast<double>(h.cnt(i));
                const double* row = d.by_lam_t + static_cast<size_t>(prod) * P * S + s;
                double w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = row[off[q]];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double t = __dmul_rn(c, w[q]);
                    z[q] = __dadd_rn(z[q], t);
                    m[q] = __dadd_rn(m[q], fabs(t));
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sum[q] = __dadd_rn(sum[q], bayes_expit(z[q]));
                zmn[q] = fmin(zmn[q], z[q]);
                mx = fmax(mx, m[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            for (int o = 32; o > 0; o >>= 1) {
                sum[q] = __dadd_rn(sum[q], __shfl_xor(sum[q], o));
                zmn[q] = fmin(zmn[q], __shfl_xor(zmn[q], o));
            }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t a = a0 + q;
            if (a >= P) break;
            const double qa = __ddiv_rn(sum[q], static_cast<double>(S));
            if (q_out && lane == 0) q_out[a] = qa;
            if (ac == kPolyNone && zmn[q] >= kBayesZsat) { ac = a; qlow = a ? v1 : -INFINITY; }
            if (a == 0) v1 = qa;
            else if (qa > v1) { v2 = v1; v1 = qa; a1 = a; }
            else if (qa > v2) v2 = qa;
        }
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    double ez;
    const double W = bayes_margin(nd, mx, S, &ez);
    uint32_t action = a1, fl = 0;
    if (ez >= 1.0) fl = RG_BAYES_UNRESOLVED;              // the z error may cross the saturation point: nothing is certain
    else if (ac != kPolyNone) {
        action = ac;
        fl = RG_BAYES_SATURATED | (__dsub_rn(1.0, qlow) <= W ? RG_BAYES_UNRESOLVED : 0u);
    } else if (__dsub_rn(v1, v2) <= __dmul_rn(2.0, W)) fl = RG_BAYES_UNRESOLVED;
    __builtin_amdgcn_wave_barrier();                      // the LDS rows are the next act's from here
    *flags = fl;
    return action;
}

}  // namespace rgk
