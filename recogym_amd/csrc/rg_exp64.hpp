// rg_exp64.hpp — the table exp of the float64 batch (k_exact_sums_m, k_exact_sums_h).  No HIP dependency: the device units
// get it through rg_common.hpp, tests/test_exp64_host.py compiles it into a host program and holds it against expl.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RG_EXP64_HD __host__ __device__ __forceinline__
#define RG_EXP64_TABLE static __device__ const
#else
#define RG_EXP64_HD inline
#define RG_EXP64_TABLE static const
#endif

// T[j] = 2^(j/32), correctly rounded.
RG_EXP64_TABLE double kExp2Tab32[32] = {
    0x1.0000000000000p+0, 0x1.059b0d3158574p+0, 0x1.0b5586cf9890fp+0, 0x1.11301d0125b51p+0,
    0x1.172b83c7d517bp+0, 0x1.1d4873168b9aap+0, 0x1.2387a6e756238p+0, 0x1.29e9df51fdee1p+0,
    0x1.306fe0a31b715p+0, 0x1.371a7373aa9cbp+0, 0x1.3dea64c123422p+0, 0x1.44e086061892dp+0,
    0x1.4bfdad5362a27p+0, 0x1.5342b569d4f82p+0, 0x1.5ab07dd485429p+0, 0x1.6247eb03a5585p+0,
    0x1.6a09e667f3bcdp+0, 0x1.71f75e8ec5f74p+0, 0x1.7a11473eb0187p+0, 0x1.82589994cce13p+0,
    0x1.8ace5422aa0dbp+0, 0x1.93737b0cdc5e5p+0, 0x1.9c49182a3f090p+0, 0x1.a5503b23e255dp+0,
    0x1.ae89f995ad3adp+0, 0x1.b7f76f2fb5e47p+0, 0x1.c199bdd85529cp+0, 0x1.cb720dcef9069p+0,
    0x1.d5818dcfba487p+0, 0x1.dfc97337b9b5fp+0, 0x1.ea4afa2a490dap+0, 0x1.f50765b6e4540p+0};

// The table as exp64t_parts reads it, 32 entries of two words (low, high): entry j is T[j] with j << 15 taken off its high word,
// so that adding n << 15 (n = 32 e + j) to the high word puts e into the exponent field with no mask (the j << 15 that rides
// along cancels) and no ldexp.  Kept as words so that the add is a 32-bit one: on the 64-bit value the compiler makes a 64-bit add
// with a zero low word of it.
RG_EXP64_HD void exp64t_entry(double tj, uint32_t j, uint32_t* tab) {
    const uint64_t bits = __builtin_bit_cast(uint64_t, tj) - (static_cast<uint64_t>(j) << 47);
    tab[2 * j] = static_cast<uint32_t>(bits);
    tab[2 * j + 1] = static_cast<uint32_t>(bits >> 32);
}

// exp(x) = scale * poly for x < 709 (NaN is not handled; x <= -708, -inf included, gives e^-708: a normal number, negligible
// beside a sum >= 1 and never 0 * inf).  exp(x) = 2^e * T[j] * exp(r) with n = rint(x * 32/ln 2) = 32 e + j and |r| <= ln 2 / 64,
// so a degree-6 polynomial is enough (remainder r^7/5040 < 4e-18).  The rounding is the magic-number form: the low word of
// x * 32/ln 2 + 1.5 * 2^52 is n, and taking the magic off again gives n as a double (no rndne, no convert).  2^e goes into
// T[j] as an integer add to the exponent field (T[j] in [1, 2) and e >= -1022: the result stays normal).
// `tab`: the 32 entries of exp64t_entry (the kernels' copy in LDS: one bank pair each, conflict-free).  No inline assembly here:
// the compiler does not keep an MFMA result's wait states for an instruction inside an asm string.
// The callers accumulate with one fma(scale, poly, sum).
RG_EXP64_HD void exp64t_parts(double x, const uint32_t* tab, double& scale, double& poly) {
    x = __builtin_fmax(x, -708.0);                                      // a float64 clamp: it also takes -inf
    const double t = __builtin_fma(x, 0x1.71547652b82fep+5, 0x1.8p52);  // 32 / ln 2
    const uint32_t n = static_cast<uint32_t>(__builtin_bit_cast(uint64_t, t));
    const double nf = t - 0x1.8p52;
    double r = __builtin_fma(nf, -0x1.62e42fe000000p-6, x);             // ln 2 / 32, high part (29 bits: nf * hi is exact)
    r = __builtin_fma(nf, -0x1.f473de6af278fp-35, r);                   // low part
    double p = 1.3888888888888889e-03;                                  // 1/6!
    p = __builtin_fma(p, r, 8.3333333333333332e-03);                    // 1/5!
    p = __builtin_fma(p, r, 4.1666666666666664e-02);                    // 1/4!
    p = __builtin_fma(p, r, 1.6666666666666666e-01);                    // 1/3!
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    poly = __builtin_fma(p, r, 1.0);
    const uint32_t* w = tab + ((n & 31u) << 1);
    const uint32_t lo = w[0], hi = w[1] + (n << 15);
    scale = __builtin_bit_cast(double, (static_cast<uint64_t>(hi) << 32) | lo);
}

// sum + exp(x)
RG_EXP64_HD double exp64t_add(double sum, double x, const uint32_t* tab) {
    double scale, poly;
    exp64t_parts(x, tab, scale, poly);
    return __builtin_fma(scale, poly, sum);
}

RG_EXP64_HD double exp64t(double x, const uint32_t* tab) { return exp64t_add(0.0, x, tab); }
