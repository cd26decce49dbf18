// rg_nn_common.hpp — the act of NnIpsAgent (RG_POLICY_NN_IPS) on one history, by a whole wave: used by the step loop and the debug
// entry (rg_nn_ips.hip) and by the off-policy replay (rg_ope_nn.hip), with the block's dynamic LDS they share (NnLds, nn_lds).
// DESIGN.md 4i has the contract, the margin W term by term and its proof.
//
// The reference's act (agents/nn_ips.py:43-63, 111-137) is a = argmax prob, ps = prob[a] with
//     prob = softmax(W3 sigmoid(W2 sigmoid(W1 x + b1) + b2) + b3)            x the user's view counts,
// computed by torch in fp32, in BLAS's summation order, with vectorised exp / sigmoid: not a function of the inputs that a kernel
// could be held to bit for bit.  The device computes the same net in float64 on the fp32 weights widened, in ONE stated order
// (rg_sim_set_nn_ips; multiply then add, index ascending, bias last) with an exponential made of IEEE operations only (nn_exp), so
// that the host restates logits, ps and flags to the bit (agents/nn_ips.py: nn_forward, nn_rule), and decides by the margin
// W(n, M1, H, A2, A3) (nn_margin): an act is resolved when z[a*] - z[b] > 2 W for every other b.
//
// nn_act: lanes stride over the hidden units in layers 1 and 2 and over the products in layer 3; a layer's vector goes through the
// wave's LDS row to the next layer.  Layer 3 runs twice, in the same order (the same bits): once for the maximum, its first index
// and the runner-up, once for the softmax sum — no logit is kept, whatever P.  The maximum is exact in any order; the sum is taken
// per lane over a = lane, lane + 64, ... and then over the lanes by the xor butterfly of rg_bayes_common.hpp (two runs give the
// same bits).  The matrices are read through generic pointers: the block's LDS copy where it fits, global memory otherwise.
#pragma once

#include "rg_poly_common.hpp"

namespace rgk {

// (nn_mul / nn_add / nn_sub / nn_div, not __dmul_rn and its kin: those are a plain product and sum defined where contraction is
// allowed, so the compiler fuses a multiply with the add that consumes it — one rounding where the contract states two.  These
// carry `contract(off)` on the operation itself.)
__device__ __forceinline__ double nn_mul(double x, double y) {
#pragma clang fp contract(off)
    return x * y;
}
__device__ __forceinline__ double nn_add(double x, double y) {
#pragma clang fp contract(off)
    return x + y;
}
__device__ __forceinline__ double nn_sub(double x, double y) {
#pragma clang fp contract(off)
    return x - y;
}
__device__ __forceinline__ double nn_div(double x, double y) {
#pragma clang fp contract(off)
    return x / y;
}

// exp(x) for x clamped to [-700, 700] (beyond: an absolute error below 1e-304 in a sigmoid or a softmax term), IEEE operations only:
// k = rint(x log2 e), r = x - k ln2 in two pieces (k C1 is exact: C1 has 32 significant bits, |k| <= 1010), the Taylor polynomial
// of degree 13 by Horner (|r| <= 0.3466: a truncation below 4e-18), scaled by 2^k (a normal double: no second rounding).  A few
// units of 2^-53 from exp, which DESIGN.md 4i's allowances cover.  nn_exp(0) is exactly 1.
__device__ __forceinline__ double nn_exp(double x) {
    constexpr double C1 = 6.93147180369123816490e-01, C2 = 1.90821492927058770002e-10;      // fdlibm's ln2HI, ln2LO
    constexpr double c[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0,
                              1.0 / 362880.0, 1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
    x = fmin(fmax(x, -700.0), 700.0);
    const double k = rint(nn_mul(x, 1.4426950408889634));
    double r = nn_sub(x, nn_mul(k, C1));
    r = nn_sub(r, nn_mul(k, C2));
    double p = c[13];
#pragma unroll
    for (int i = 12; i >= 0; --i) p = nn_add(nn_mul(p, r), c[i]);
    return ldexp(p, static_cast<int>(k));
}

__device__ __forceinline__ double nn_sigmoid(double z) {
    return nn_div(1.0, nn_add(1.0, nn_exp(-z)));
}

// W = E3 + 2^-20 with, u = 2^-24:  E1 = (n + 5) u M1,  d1 = E1 / 4 + 2^-21,  E2 = A2 ((H + 5) u + d1),  d2 = E2 / 4 + 2^-21,
// E3 = A3 ((H + 5) u + d2).  IEEE operations only (agents/nn_ips.py: nn_margin computes the same bits).  *e3_out: E3, the bound on
// the logits alone.
__device__ __forceinline__ double nn_margin(uint32_t n, double M1, uint32_t H, double A2, double A3, double* e3_out) {
    const double hu = ldexp(static_cast<double>(H + 5u), -24);
    const double E1 = nn_mul(ldexp(static_cast<double>(n + 5u), -24), M1);
    const double d1 = nn_add(nn_mul(E1, 0.25), 0x1p-21);
    const double E2 = nn_mul(A2, nn_add(hu, d1));
    const double d2 = nn_add(nn_mul(E2, 0.25), 0x1p-21);
    const double E3 = nn_mul(A3, nn_add(hu, d2));
    *e3_out = E3;
    return nn_add(E3, 0x1p-20);
}

// z[a] in the contract's order
__device__ __forceinline__ double nn_logit(const double* w3t, const double* b3, const double* s_h2, uint32_t Hn, uint32_t P, uint32_t a) {
    double s = 0.0;
#pragma unroll 4
    for (uint32_t k = 0; k < Hn; ++k) s = nn_add(s, nn_mul(w3t[static_cast<size_t>(k) * P + a], s_h2[k]));
    return nn_add(s, b3[a]);
}

// The act on the history `h` (wave-uniform), by the whole wave.  s_cnt / s_prod: this wave's LDS rows (kPolyHist entries each);
// s_h1 / s_h2: its layer vectors (H doubles each); w1t / w2t / w3t: the matrices (LDS or global).  *flags: RG_NN_UNRESOLVED;
// *ps_out: the softmax at the action; z_out (or nullptr): P doubles that receive the logits.
template <class H>
__device__ __forceinline__ uint32_t nn_act(const NnModel& m, uint32_t P, const H& h, int lane, double* s_cnt, uint32_t* s_prod,
                                           double* s_h1, double* s_h2, const double* w1t, const double* w2t, const double* w3t,
                                           uint32_t* flags, double* ps_out, double* z_out) {
    const uint32_t nd = h.size(), Hn = m.H;
    bool big = false;                                     // a count that is not an fp32 value: torch's input differs from the device's
    for (uint32_t i = lane; i < nd; i += 64) {
        uint32_t p;
        typename H::val_t c;
        h.get(i, p, c);
        big = big || c > (1u << 24);
        if (i < kPolyHist) { s_cnt[i] = static_cast<double>(c); s_prod[i] = p; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // layer 1: lanes over the hidden units, the viewed products ascending; m1 beside s1 in the same order
    double mx = 0.0;
    for (uint32_t j = lane; j < Hn; j += 64) {
        double s = 0.0, a = 0.0;
#pragma unroll 2
        for (uint32_t i = 0; i < nd; ++i) {
            const uint32_t prod = i < kPolyHist ? s_prod[i] : h.prod(i);
            const double c = i < kPolyHist ? s_cnt[i] : static_cast<double>(h.cnt(i));
            const double t = nn_mul(c, w1t[static_cast<size_t>(prod) * Hn + j]);
            s = nn_add(s, t);
            a = nn_add(a, fabs(t));
        }
        const double b = m.b1[j];
        mx = fmax(mx, nn_add(a, fabs(b)));
        s_h1[j] = nn_sigmoid(nn_add(s, b));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // layer 2: lanes over the hidden units, the inputs ascending
    for (uint32_t k = lane; k < Hn; k += 64) {
        double s = 0.0;
#pragma unroll 4
        for (uint32_t j = 0; j < Hn; ++j) s = nn_add(s, nn_mul(w2t[static_cast<size_t>(j) * Hn + k], s_h1[j]));
        s_h2[k] = nn_sigmoid(nn_add(s, m.b2[k]));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // layer 3, first pass: the maximum, its first index, the best of the others (equal to the maximum when two logits tie)
    double v1 = -INFINITY, v2 = -INFINITY;
    uint32_t a1 = kPolyNone;
    for (uint32_t a = lane; a < P; a += 64) {
        const double z = nn_logit(w3t, m.b3, s_h2, Hn, P, a);
        if (z_out) z_out[a] = z;
        if (z > v1) { v2 = v1; v1 = z; a1 = a; }
        else if (z > v2) v2 = z;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov1 = __shfl_xor(v1, o), ov2 = __shfl_xor(v2, o);
        const uint32_t oa1 = __shfl_xor(a1, o);
        const bool take = ov1 > v1 || (ov1 == v1 && oa1 < a1);
        v2 = fmax(fmax(v2, ov2), take ? v1 : ov1);
        if (take) { v1 = ov1; a1 = oa1; }
        mx = fmax(mx, __shfl_xor(mx, o));
    }
    // second pass: the softmax sum in the stated order (lanes beyond P hold the identity 0.0)
    double sum = 0.0;
    for (uint32_t a = lane; a < P; a += 64) sum = nn_add(sum, nn_exp(nn_sub(nn_logit(w3t, m.b3, s_h2, Hn, P, a), v1)));
    for (int o = 32; o > 0; o >>= 1) sum = nn_add(sum, __shfl_xor(sum, o));
    *ps_out = nn_div(1.0, sum);                        // e[a*] = nn_exp(0) = 1
    double e3;
    const double W = nn_margin(nd, mx, Hn, m.A2, m.A3, &e3);
    const bool resolved = nn_sub(v1, v2) > nn_mul(2.0, W) && __ballot(big) == 0ull;
    __builtin_amdgcn_wave_barrier();                      // the LDS rows are the next act's from here
    *flags = resolved ? 0u : RG_NN_UNRESOLVED;
    return a1;
}

// The block's dynamic LDS (nn_host_model sizes it on the host): two layer vectors of H doubles per wave, then — where m.staged —
// the three matrices, copied once per block.  kWaves: the waves of the block (the step loop's kBlock / 64, the replay's kOpeWaves).
struct NnLds {
    double* rows;
    const double* w1t; const double* w2t; const double* w3t;
};

template <int kWaves>
__device__ __forceinline__ NnLds nn_lds(const NnModel& m, uint32_t P, char* smem) {
    NnLds l;
    l.rows = reinterpret_cast<double*>(smem);
    l.w1t = m.w1t; l.w2t = m.w2t; l.w3t = m.w3t;
    if (m.staged) {
        double* s_w = l.rows + static_cast<size_t>(2) * kWaves * m.H;
        const uint32_t n1 = P * m.H, n2 = m.H * m.H;
        for (uint32_t i = threadIdx.x; i < n1; i += 64 * kWaves) { s_w[i] = m.w1t[i]; s_w[n1 + n2 + i] = m.w3t[i]; }
        for (uint32_t i = threadIdx.x; i < n2; i += 64 * kWaves) s_w[n1 + i] = m.w2t[i];
        l.w1t = s_w; l.w2t = s_w + n1; l.w3t = s_w + n1 + n2;
    }
    __syncthreads();
    return l;
}

}  // namespace rgk
