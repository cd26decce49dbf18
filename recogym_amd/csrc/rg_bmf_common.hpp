// rg_bmf_common.hpp — what BanditMFSquare's device training (rg_bandit_mf.hip) shares with a host compiler: the limits and the
// LDS budget that decides between the two instantiations of the step kernel.  The arithmetic of one RMSprop update is
// rg_omf_common.hpp's omf_rmsprop.  No HIP dependency.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rg_omf_common.hpp"

namespace rgbmf {

constexpr uint32_t kBmfMaxProducts = 16384;     // cap on P of the step kernel (global instantiation)
constexpr uint32_t kBmfMaxEmbed = 64;           // cap on E
constexpr uint32_t kBmfMaxStep = 256;           // cap on the samples of one step: what the kernel stages in LDS
constexpr size_t kBmfLdsBudget = 64 * 1024;     // dynamic LDS a launch asks for at most

// the first six as rg_omf_pairs gives them
constexpr unsigned long long kBmfErrFirstBandit = 1, kBmfErrProduct = 2, kBmfErrOffsets = 4, kBmfErrEmptyOrganic = 8, kBmfErrCapacity = 16,
                             kBmfErrOrganicBandit = 32, kBmfErrReward = 64, kBmfErrStepLength = 128;

// The step kernel's dynamic LDS in bytes.  Always: d_s of the staged step (mb_cap doubles), the exp table (64 words), four int
// rows of mb_cap (the last views, the actions, the first samples of the distinct actions and of the distinct last views) and 64
// words of flags and per-wave counts.  `state_in_lds` adds the two embeddings, their square averages and their gradients:
// 3 x 2 P E doubles.
RG_OMF_HD size_t bmf_lds_bytes(uint32_t P, uint32_t E, uint32_t mb_cap, bool state_in_lds) {
    const size_t np = 2 * static_cast<size_t>(P) * E;
    return 8 * (static_cast<size_t>(mb_cap) + (state_in_lds ? 3 * np : 0)) + 4 * (64 + 4 * static_cast<size_t>(mb_cap) + 64);
}

RG_OMF_HD bool bmf_lds_fits(uint32_t P, uint32_t E) { return bmf_lds_bytes(P, E, kBmfMaxStep, true) <= kBmfLdsBudget; }

}  // namespace rgbmf
