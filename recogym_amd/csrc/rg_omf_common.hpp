// rg_omf_common.hpp — what OrganicMFSquare's device training (rg_organic_mf.hip) shares with a host compiler: the limits, the
// LDS budget that decides between the two instantiations of the step kernel, and the arithmetic of one RMSprop update.  No HIP
// dependency (rg_exp64.hpp has none either).
#pragma once

#include <cstddef>
#include <cstdint>

#include "rg_exp64.hpp"

#if defined(__HIPCC__)
#define RG_OMF_HD __host__ __device__ __forceinline__
#else
#define RG_OMF_HD inline
#endif

namespace rgomf {

constexpr uint32_t kOmfMaxProducts = 2048;      // cap on P of the step kernel (global instantiation)
constexpr uint32_t kOmfMaxEmbed = 64;           // cap on E
constexpr size_t kOmfLdsBudget = 64 * 1024;     // dynamic LDS a launch asks for at most (no function attribute needed below it)

constexpr unsigned long long kOmfErrFirstBandit = 1, kOmfErrProduct = 2, kOmfErrOffsets = 4, kOmfErrEmptyOrganic = 8, kOmfErrCapacity = 16,
                             kOmfErrOrganicBandit = 32;

// The step kernel's dynamic LDS in bytes.  Always: the softmax row (P doubles), 32 doubles of reduction scratch, the exp table
// (64 words), three int rows of P (N[i][.], the input counts, the list of distinct inputs) and 4 words of flags.  `state_in_lds`
// adds the model, its square averages and the gradients: 3 x (2 P E + P) doubles.
RG_OMF_HD size_t omf_lds_bytes(uint32_t P, uint32_t E, bool state_in_lds) {
    const size_t np = 2 * static_cast<size_t>(P) * E + P;
    return 8 * (static_cast<size_t>(P) + 32) + (state_in_lds ? 24 * np : 0) + 4 * (64 + 3 * static_cast<size_t>(P) + 4);
}

RG_OMF_HD bool omf_lds_fits(uint32_t P, uint32_t E) { return omf_lds_bytes(P, E, true) <= kOmfLdsBudget; }

// torch.optim.RMSprop's step without momentum, not centred: sq = alpha sq + (1 - alpha) g g; p -= lr g / (sqrt(sq) + eps).
// g = 0 leaves p as it is and still decays sq.  Written without contraction so that a host compiler gives the same bits.
RG_OMF_HD void omf_rmsprop(double& p, double& sq, double g, double lr, double alpha, double eps) {
#pragma clang fp contract(off)
    const double gg = g * g;
    const double a = alpha * sq;
    const double b = (1.0 - alpha) * gg;
    const double q = a + b;
    sq = q;
    const double d = __builtin_sqrt(q) + eps;
    const double u = g / d;
    p = p - lr * u;
}

}  // namespace rgomf
