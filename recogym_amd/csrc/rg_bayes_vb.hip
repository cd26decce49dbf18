// rg_bayes_vb.hip — librecogym_hip.so: the posterior-sample act of BayesianAgentVB (RG_POLICY_BAYES_VB) in the step loop.
// (see rg_common.hpp for the shared types and helpers, rg_bayes_common.hpp for the act, DESIGN.md 4h for the contract and the margin)

#include "rg_bayes_common.hpp"
#include "rg_act_common.hpp"

namespace rgk {

// BayesianAgentVB's unit of the act skeleton (rg_act_common.hpp): bayes_act on the user's history row; nothing staged.  row: the
// means q[a].
struct BayesUnit {
    static constexpr uint32_t kUnresolved = RG_BAYES_UNRESOLVED;
    static constexpr uint32_t kExtraMask = RG_BAYES_SATURATED;
    static constexpr int kExtraCounter = RG_CNT_BAYES_SATURATED;
    static constexpr bool kPs = false, kRow = true, kIdleReturn = false;
    static constexpr ActStage kStage = kStageNone;
    static constexpr int kSums = 4;                        // (three are used; four words keep the block's static LDS what it was)
    double (*s_cnt)[kPolyHist]; uint32_t (*s_prod)[kPolyHist];      // the block's rows, one per wave

    __device__ __forceinline__ int stage(const DevSim&) const { return 0; }          // (nothing staged)
    __device__ __forceinline__ uint32_t act(const DevSim& d, int, uint32_t slot, int lane, int wave, uint32_t* flags, double*, double* q_out) const {
        const hent_t* hr = hist_row(d, slot) + 1;             // entries after the header
        const BayesModel m{d.P, d.pl_nth, d.pl_wk_t};         // (the model's two slots in DevSim)
        return bayes_act(m, PolyRowHist{hr, h_cnt(hr[-1])}, lane, s_cnt[wave], s_prod[wave], flags, q_out);
    }
};

__global__ void __launch_bounds__(kBlock) k_bayes_acts(DevSim d, uint32_t t) {
    __shared__ double s_cnt[kActWaves][kPolyHist];
    __shared__ uint32_t s_prod[kActWaves][kPolyHist];
    const BayesUnit u{s_cnt, s_prod};
    act_list_run(d, t, u);
}

// rg_sim_debug_bayes_acts: action, flags and the means q[i][a] per user index
__global__ void __launch_bounds__(kBlock) k_debug_bayes_acts(DevSim d, int32_t* action, uint8_t* flags, double* q) {
    __shared__ double s_cnt[kActWaves][kPolyHist];
    __shared__ uint32_t s_prod[kActWaves][kPolyHist];
    const BayesUnit u{s_cnt, s_prod};
    act_debug_run(d, u, action, flags, q, nullptr);
}

search_kernel_t bayes_acts_kernel() { return k_bayes_acts; }
void (*bayes_debug_kernel())(DevSim, int32_t*, uint8_t*, double*) { return k_debug_bayes_acts; }

}  // namespace rgk
