// rg_mlr.hip — librecogym_hip.so: the argmax act of PyTorchMLRAgent (RG_POLICY_MLR) in the step loop.
// (see rg_common.hpp for the shared types and helpers, rg_mlr_common.hpp for the act, DESIGN.md 4j for the contract and the margin)

#include "rg_mlr_common.hpp"
#include "rg_act_common.hpp"

namespace rgk {

// PyTorchMLRAgent's unit of the act skeleton (rg_act_common.hpp): mlr_act on the user's history row, the table in the block's
// dynamic LDS where it fits (mlr_lds).  ps = 1: lr_ps is not this policy's (one entry is carved and nothing logs it).  row: the
// scores z[a].
struct MlrUnit {
    static constexpr uint32_t kUnresolved = RG_MLR_UNRESOLVED;
    static constexpr uint32_t kExtraMask = 0u;
    static constexpr int kExtraCounter = 0;
    static constexpr bool kPs = false, kRow = true, kIdleReturn = true;
    static constexpr ActStage kStage = kStageSynced;
    static constexpr int kSums = 2;
    MlrModel m;
    char* smem;
    double (*s_cnt)[kPolyHist]; uint32_t (*s_prod)[kPolyHist];      // the block's rows, one per wave

    __device__ __forceinline__ const double* stage(const DevSim& d) const { return mlr_lds<kActWaves>(m, d.P, smem); }
    __device__ __forceinline__ uint32_t act(const DevSim& d, const double* wt, uint32_t slot, int lane, int wave, uint32_t* flags, double*, double* z_out) const {
        const hent_t* hr = hist_row(d, slot) + 1;             // entries after the header
        return mlr_act(wt, d.P, PolyRowHist{hr, h_cnt(hr[-1])}, lane, s_cnt[wave], s_prod[wave], flags, z_out);
    }
};

__global__ void __launch_bounds__(kBlock) k_mlr_acts(DevSim d, MlrModel m, uint32_t t) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ double s_cnt[kActWaves][kPolyHist];
    __shared__ uint32_t s_prod[kActWaves][kPolyHist];
    const MlrUnit u{m, smem_raw, s_cnt, s_prod};
    act_list_run(d, t, u);
}

// rg_sim_debug_mlr_acts: action, flags and the scores z[i][a] per user index
__global__ void __launch_bounds__(kBlock) k_debug_mlr_acts(DevSim d, MlrModel m, int32_t* action, uint8_t* flags, double* z) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ double s_cnt[kActWaves][kPolyHist];
    __shared__ uint32_t s_prod[kActWaves][kPolyHist];
    const MlrUnit u{m, smem_raw, s_cnt, s_prod};
    act_debug_run(d, u, action, flags, z, nullptr);
}

// flag |= 1 where one of wt[0 .. n) is not finite (mlr_host_model: the replay's check of its table, on the device)
__global__ void __launch_bounds__(kBlock) k_mlr_finite(const double* __restrict__ wt, size_t n, uint32_t* __restrict__ flag) {
    bool bad = false;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * kBlock)
        bad = bad || !__builtin_isfinite(wt[i]);
    if (bad) atomicOr(flag, 1u);
}

void (*mlr_finite_kernel())(const double*, size_t, uint32_t*) { return k_mlr_finite; }
void (*mlr_acts_kernel())(DevSim, MlrModel, uint32_t) { return k_mlr_acts; }
void (*mlr_debug_kernel())(DevSim, MlrModel, int32_t*, uint8_t*, double*) { return k_debug_mlr_acts; }

}  // namespace rgk
