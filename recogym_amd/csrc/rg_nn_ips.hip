// rg_nn_ips.hip — librecogym_hip.so: the three-layer perceptron act of NnIpsAgent (RG_POLICY_NN_IPS) in the step loop.
// (see rg_common.hpp for the shared types and helpers, rg_nn_common.hpp for the act, DESIGN.md 4i for the contract and the margin)

#include "rg_nn_common.hpp"
#include "rg_act_common.hpp"

namespace rgk {

// NnIpsAgent's unit of the act skeleton (rg_act_common.hpp): nn_act on the user's history row, the net in the block's dynamic LDS
// where it fits (nn_lds); the act's propensity goes to lr_ps.  row: the logits z[a].
struct NnUnit {
    static constexpr uint32_t kUnresolved = RG_NN_UNRESOLVED;
    static constexpr uint32_t kExtraMask = 0u;
    static constexpr int kExtraCounter = 0;
    static constexpr bool kPs = true, kRow = true, kIdleReturn = true;
    static constexpr ActStage kStage = kStageSynced;
    static constexpr int kSums = 2;
    NnModel m;
    char* smem;
    double (*s_cnt)[kPolyHist]; uint32_t (*s_prod)[kPolyHist];      // the block's rows, one per wave

    __device__ __forceinline__ NnLds stage(const DevSim& d) const { return nn_lds<kActWaves>(m, d.P, smem); }
    __device__ __forceinline__ uint32_t act(const DevSim& d, const NnLds& l, uint32_t slot, int lane, int wave, uint32_t* flags, double* ps_out, double* z_out) const {
        double* cnt = s_cnt[wave];
        uint32_t* prod = s_prod[wave];
        const hent_t* hr = hist_row(d, slot) + 1;             // entries after the header
        double* s_h1 = l.rows + static_cast<size_t>(2 * wave) * m.H;
        return nn_act(m, d.P, PolyRowHist{hr, h_cnt(hr[-1])}, lane, cnt, prod, s_h1, s_h1 + m.H, l.w1t, l.w2t, l.w3t, flags, ps_out, z_out);
    }
};

__global__ void __launch_bounds__(kBlock) k_nn_acts(DevSim d, NnModel m, uint32_t t) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ double s_cnt[kActWaves][kPolyHist];
    __shared__ uint32_t s_prod[kActWaves][kPolyHist];
    const NnUnit u{m, smem_raw, s_cnt, s_prod};
    act_list_run(d, t, u);
}

// rg_sim_debug_nn_acts: action, flags, the logits z[i][a] and the propensity ps[i] per user index
__global__ void __launch_bounds__(kBlock) k_debug_nn_acts(DevSim d, NnModel m, int32_t* action, uint8_t* flags, double* z, double* ps) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ double s_cnt[kActWaves][kPolyHist];
    __shared__ uint32_t s_prod[kActWaves][kPolyHist];
    const NnUnit u{m, smem_raw, s_cnt, s_prod};
    act_debug_run(d, u, action, flags, z, ps);
}

void (*nn_acts_kernel())(DevSim, NnModel, uint32_t) { return k_nn_acts; }
void (*nn_debug_kernel())(DevSim, NnModel, int32_t*, uint8_t*, double*, double*) { return k_debug_nn_acts; }

}  // namespace rgk
