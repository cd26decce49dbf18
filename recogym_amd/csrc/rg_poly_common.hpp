// rg_poly_common.hpp — the act of the likelihood agent (LogregPolyAgent), shared by the step loop (rg_logreg_poly.hip) and the
// off-policy replay (rg_ope_poly.hip).  DESIGN.md 4f has the contract, the merge rule and its proof.
//
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
// poly_act: one act by a whole wave, lanes striding over the actions, float64 throughout.  The sorted history is read once into
// LDS (counts as doubles, products); the prefix sum_j c_j wf[p_j] is taken once per act; a lane walks four actions and four
// history entries at a time (16 independent loads of wk_t in flight, as logreg_act_wave), each action's terms still added in
// history order.  The quirk index (a n + j) / P is one 64-bit divide per (lane, action) and an incremental (quotient, remainder)
// pair along j.  One pass keeps, per lane, the lowest step with its first index, the best decision with its first index, and the
// second best DISTINCT decision; the wave reduction of those decides the table zone and tells whether ANY decision lies within W
// of z*; only then (rare) a second pass recomputes the decisions below a* for the index test.
//
// Two template parameters keep the function one for both callers:
//   M  the model: members P, pl_nth, pl_wf, pl_wa, pl_wk_t ([viewed product][action]), pl_b — DevSim has them; PolyModel is the
//      replay's;
//   H  the history, ascending by product: size(), prod(i), cnt(i), get(i, p, c) for 0 <= i < size(), val_t the type of a value —
//      PolyRowHist over a step-loop history row, PolyListHist over the replay's (product, count) list (integer counts), WhListHist
//      (rg_wh_common.hpp) over a time-weighted feature list (doubles that hold float32 values).
#pragma once

#include "rg_common.hpp"

namespace rgk {

constexpr uint32_t kPolyNone = 0xFFFFFFFFu;
constexpr double kPolyFloor = -700.0;     // z* below this: outside the domain of the margin's proof (poly_act)

// the model as a replay holds it (the step loop's is DevSim)
struct PolyModel {
    uint32_t P, pl_nth;
    const double* pl_wf; const double* pl_wa; const double* pl_wk_t; const double* pl_th;
    double pl_b;
};

// the model's own argument checks (the replay entry points of rg_ope_poly.hip and rg_ope_poly_w.hip)
inline int pl_model_ok(const rg_ope_poly* m, const char* who) {
    if (!m) return fail(RG_EINVAL, "%s: null model", who);
    if (m->num_products == 0 || m->num_products > RG_EV_INDEX_MASK) return fail(RG_EINVAL, "%s: bad num_products %u", who, m->num_products);
    if (m->n_steps == 0 || m->n_steps > kPolySteps) return fail(RG_EINVAL, "%s: n_steps %u outside 1 .. %u", who, m->n_steps, kPolySteps);
    if (!m->wf || !m->wa || !m->wk_t || !m->th) return fail(RG_EINVAL, "%s: null wf / wa / wk_t / th", who);
    return RG_OK;
}

// the entries of a step-loop history row after its header
struct PolyRowHist {
    typedef uint32_t val_t;
    const hent_t* hr;
    uint32_t nd;
    __device__ __forceinline__ uint32_t size() const { return nd; }
    __device__ __forceinline__ uint32_t prod(uint32_t i) const { return h_prod(hr[i]); }
    __device__ __forceinline__ uint32_t cnt(uint32_t i) const { return h_cnt(hr[i]); }
    __device__ __forceinline__ void get(uint32_t i, uint32_t& p, uint32_t& c) const { const hent_t x = hr[i]; p = h_prod(x); c = h_cnt(x); }
};

// a (product, count) list in two arrays (LDS or global)
struct PolyListHist {
    typedef uint32_t val_t;
    const uint32_t* lp;
    const uint32_t* lc;
    uint32_t nd;
    __device__ __forceinline__ uint32_t size() const { return nd; }
    __device__ __forceinline__ uint32_t prod(uint32_t i) const { return lp[i]; }
    __device__ __forceinline__ uint32_t cnt(uint32_t i) const { return lc[i]; }
    __device__ __forceinline__ void get(uint32_t i, uint32_t& p, uint32_t& c) const { p = lp[i]; c = lc[i]; }
};

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
template <class M, class H, class F>
__device__ __forceinline__ void poly_scan(const M& d, const H& h, const double* s_cnt, const uint32_t* s_prod, double prefix,
                                          uint32_t a_end, int lane, F&& f) {
    const uint32_t P = d.P, nd = h.size();
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
                const uint32_t prod = ie < kPolyHist ? s_prod[ie] : h.prod(ie);
                const double* row = d.pl_wk_t + static_cast<size_t>(prod) * P;
#pragma unroll
                for (int q = 0; q < 4; ++q) w[e][q] = row[aa[q]];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < nd) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double c = qq[q] < kPolyHist ? s_cnt[qq[q]] : static_cast<double>(h.cnt(qq[q]));   // qq < nd here
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

// The act on the history `h` (wave-uniform), by the whole wave.  s_cnt / s_prod: this wave's LDS rows (kPolyHist entries each);
// s_th: the block's copy of the step table.  *flags: bit 0 decided on the table, bit 1 unresolved, bit 2 a lower index than a* won.
template <class M, class H>
__device__ __forceinline__ uint32_t poly_act(const M& d, const H& h, int lane, const double* s_th, double* s_cnt, uint32_t* s_prod,
                                             uint32_t* flags) {
    const uint32_t nd = h.size();
    for (uint32_t i = lane; i < nd && i < kPolyHist; i += 64) {
        uint32_t p;
        typename H::val_t c;
        h.get(i, p, c);
        s_cnt[i] = static_cast<double>(c);
        s_prod[i] = p;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // the common prefix, once per act: the products c_j wf[p_j] a lane each (independent loads), summed in history order
    double prefix = 0.0;
    for (uint32_t i0 = 0; i0 < nd; i0 += 64) {
        const uint32_t i = i0 + lane;
        double term = 0.0;
        if (i < nd) {
            uint32_t p;
            typename H::val_t c;
            h.get(i, p, c);
            term = __dmul_rn(static_cast<double>(c), d.pl_wf[p]);
        }
        const uint32_t m = min(64u, nd - i0);
        for (uint32_t k = 0; k < m; ++k) prefix = __dadd_rn(prefix, __shfl(term, static_cast<int>(k)));
    }
    const uint32_t K = d.pl_nth;
    double v1 = -INFINITY, v2 = -INFINITY;                // best decision, second best distinct one
    uint32_t a1 = kPolyNone, smin = K + 1, sa = kPolyNone; // first index of v1; lowest step and its first index
    poly_scan(d, h, s_cnt, s_prod, prefix, d.P, lane, [&](uint32_t a, double z) {
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
            poly_scan(d, h, s_cnt, s_prod, prefix, a1, lane, [&](uint32_t, double z) {
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

}  // namespace rgk
