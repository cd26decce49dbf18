// rg_mlr_common.hpp — the act of PyTorchMLRAgent (RG_POLICY_MLR) on one history, by a whole wave: used by the step loop and the debug
// entry (rg_mlr.hip) and by the off-policy replay (rg_ope_mlr.hip), with the block's dynamic LDS they share (MlrLds, mlr_lds).
// DESIGN.md 4j has the contract, the margin E and its proof.
//
// The reference's act (agents/pytorch_mlr.py:30-32, 59-84) is a = argmax(x W^T), ps = 1, x the user's view counts as float32 and W
// the P x P float32 weight of its one linear layer: an fp32 dot per action in BLAS's order, not a function of the inputs that a
// kernel could be held to bit for bit.  The device computes the same scores in float64 on the fp32 weights widened, in ONE stated
// order (the distinct viewed products ascending; multiply, then add; nothing fused), so that the host restates scores and flags to
// the bit (agents/pytorch_mlr.py: mlr_forward, mlr_rule), and decides by the margin E = (n + 5) 2^-24 M1 (mlr_margin): an act is
// resolved when the best score leads the second best by more than 2 E.
//
// mlr_act: lanes stride over the actions a = lane, lane + 64, ...; wt is [viewed product][action], so the 64 lanes read one
// contiguous piece of a viewed product's row per term.  Each lane keeps its best score, the first index of it and its runner-up,
// and the largest absolute sum m1[a] it met; the wave folds them by an xor butterfly.  Every fold is a maximum (the best with the
// lowest-index rule on ties, the runner-up, M1): the result does not depend on the lane order.  No score is kept, whatever P.
#pragma once

#include "rg_nn_common.hpp"       // (nn_mul / nn_add / nn_sub: a product, a sum and a difference that the compiler may not contract)

namespace rgk {

// E = (n + 5) 2^-24 M1.  IEEE operations only (agents/pytorch_mlr.py: mlr_margin computes the same bits).
__device__ __forceinline__ double mlr_margin(uint32_t n, double M1) {
    return nn_mul(ldexp(static_cast<double>(n + 5u), -24), M1);
}

// The act on the history `h` (wave-uniform), by the whole wave.  s_cnt / s_prod: this wave's LDS rows (kPolyHist entries each); wt:
// the table (LDS or global).  *flags: RG_MLR_UNRESOLVED; z_out (or nullptr): P doubles that receive the scores.
template <class H>
__device__ __forceinline__ uint32_t mlr_act(const double* wt, uint32_t P, const H& h, int lane, double* s_cnt, uint32_t* s_prod,
                                            uint32_t* flags, double* z_out) {
    const uint32_t nd = h.size();
    bool big = false;                                     // a count that is not an fp32 value: the reference's input differs from the device's
    for (uint32_t i = lane; i < nd; i += 64) {
        uint32_t p;
        typename H::val_t c;
        h.get(i, p, c);
        big = big || c > (1u << 24);
        if (i < kPolyHist) { s_cnt[i] = static_cast<double>(c); s_prod[i] = p; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    double v1 = -INFINITY, v2 = -INFINITY, mx = 0.0;
    uint32_t a1 = kPolyNone;
    for (uint32_t a = lane; a < P; a += 64) {
        double s = 0.0, m = 0.0;
#pragma unroll 4
        for (uint32_t i = 0; i < nd; ++i) {
            const uint32_t prod = i < kPolyHist ? s_prod[i] : h.prod(i);
            const double c = i < kPolyHist ? s_cnt[i] : static_cast<double>(h.cnt(i));
            const double t = nn_mul(c, wt[static_cast<size_t>(prod) * P + a]);
            s = nn_add(s, t);
            m = nn_add(m, fabs(t));
        }
        if (z_out) z_out[a] = s;
        mx = fmax(mx, m);
        if (s > v1) { v2 = v1; v1 = s; a1 = a; }
        else if (s > v2) v2 = s;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov1 = __shfl_xor(v1, o), ov2 = __shfl_xor(v2, o);
        const uint32_t oa1 = __shfl_xor(a1, o);
        const bool take = ov1 > v1 || (ov1 == v1 && oa1 < a1);
        v2 = fmax(fmax(v2, ov2), take ? v1 : ov1);
        if (take) { v1 = ov1; a1 = oa1; }
        mx = fmax(mx, __shfl_xor(mx, o));
    }
    // (M1 < 2^126: no partial sum of the reference's fp32 dot can overflow, which the margin's proof assumes)
    const bool resolved = nd != 0u && nn_sub(v1, v2) > nn_mul(2.0, mlr_margin(nd, mx)) && mx < 0x1p126 && __ballot(big) == 0ull;
    __builtin_amdgcn_wave_barrier();                      // the LDS rows are the next act's from here
    *flags = resolved ? 0u : RG_MLR_UNRESOLVED;
    return a1;
}

// The block's dynamic LDS: the table, copied once per block, where m.staged (mlr_host_model decides and sizes it on the host).
template <int kWaves>
__device__ __forceinline__ const double* mlr_lds(const MlrModel& m, uint32_t P, char* smem) {
    const double* wt = m.wt;
    if (m.staged) {
        double* s_w = reinterpret_cast<double*>(smem);
        const uint32_t n = P * P;
        for (uint32_t i = threadIdx.x; i < n; i += 64 * kWaves) s_w[i] = m.wt[i];
        wt = s_w;
    }
    __syncthreads();
    return wt;
}

}  // namespace rgk
