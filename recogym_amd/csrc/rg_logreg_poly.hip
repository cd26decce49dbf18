// rg_logreg_poly.hip — librecogym_hip.so: the act of the likelihood agent (LogregPolyAgent, RG_POLICY_LOGREG_POLY) in the step loop.
// (see rg_common.hpp for the shared types and helpers, DESIGN.md 4f for the contract, the merge rule and its proof)

#include "rg_act_common.hpp"

namespace rgk {

// the likelihood agent's unit of the act skeleton (rg_act_common.hpp): poly_act on the user's history row, the step table in LDS
struct PolyUnit {
    static constexpr uint32_t kUnresolved = 2u;            // (poly_act's flags: bit 0 decided on the table, bit 1 unresolved)
    static constexpr uint32_t kExtraMask = 1u;
    static constexpr int kExtraCounter = RG_CNT_POLY_TABLE;
    static constexpr bool kPs = false, kRow = false, kIdleReturn = false;
    static constexpr ActStage kStage = kStageOpen;
    static constexpr int kSums = 4;                        // (three are used; four words keep the block's static LDS what it was)
    double* s_th;
    double (*s_cnt)[kPolyHist]; uint32_t (*s_prod)[kPolyHist];      // the block's rows, one per wave

    __device__ __forceinline__ const double* stage(const DevSim& d) const {
        for (uint32_t i = threadIdx.x; i < d.pl_nth; i += kBlock) s_th[i] = d.pl_th[i];
        return s_th;
    }
    __device__ __forceinline__ uint32_t act(const DevSim& d, const double* th, uint32_t slot, int lane, int wave, uint32_t* flags, double*, double*) const {
        const hent_t* hr = hist_row(d, slot) + 1;             // entries after the header
        return poly_act(d, PolyRowHist{hr, h_cnt(hr[-1])}, lane, th, s_cnt[wave], s_prod[wave], flags);
    }
};

__global__ void __launch_bounds__(kBlock) k_poly_acts(DevSim d, uint32_t t) {
    __shared__ double s_th[kPolySteps];
    __shared__ double s_cnt[kActWaves][kPolyHist];
    __shared__ uint32_t s_prod[kActWaves][kPolyHist];
    const PolyUnit u{s_th, s_cnt, s_prod};
    act_list_run(d, t, u);
}

// rg_sim_debug_poly_acts: action and flags per user index
__global__ void __launch_bounds__(kBlock) k_debug_poly_acts(DevSim d, int32_t* action, uint8_t* flags) {
    __shared__ double s_th[kPolySteps];
    __shared__ double s_cnt[kActWaves][kPolyHist];
    __shared__ uint32_t s_prod[kActWaves][kPolyHist];
    const PolyUnit u{s_th, s_cnt, s_prod};
    act_debug_run(d, u, action, flags, nullptr, nullptr);
}

search_kernel_t poly_acts_kernel() { return k_poly_acts; }
void (*poly_debug_kernel())(DevSim, int32_t*, uint8_t*) { return k_debug_poly_acts; }

}  // namespace rgk
