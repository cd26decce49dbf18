// rg_mlr.hip — librecogym_hip.so: the argmax act of PyTorchMLRAgent (RG_POLICY_MLR) in the step loop.
// (see rg_common.hpp for the shared types and helpers, rg_mlr_common.hpp for the act, DESIGN.md 4j for the contract and the margin)

#include "rg_mlr_common.hpp"

namespace rgk {

// The act of the user in `slot` (wave-uniform), by the whole wave: mlr_act on the user's history row.
__device__ uint32_t mlr_act_wave(const DevSim& d, const double* wt, uint32_t slot, int lane, double* s_cnt, uint32_t* s_prod,
                                 uint32_t* flags, double* z_out) {
    const hent_t* hr = hist_row(d, slot) + 1;             // entries after the header
    return mlr_act(wt, d.P, PolyRowHist{hr, h_cnt(hr[-1])}, lane, s_cnt, s_prod, flags, z_out);
}

// a wave per listed act, over the lr_list / lr_action / lr_dirty plumbing of k_nn_acts; ps = 1: lr_ps is not this policy's (one
// entry is carved and nothing logs it); unresolved acts to the same list
__global__ void __launch_bounds__(kBlock) k_mlr_acts(DevSim d, MlrModel m, uint32_t t) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ double s_cnt[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_prod[kBlock / 64][kPolyHist];
    __shared__ unsigned long long s_sum[2];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t n = d.lr_cnt[t];
    if (blockIdx.x * (kBlock / 64) >= n) return;          // (the whole block: no act of the grid-stride loop is its)
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0ull;
    const double* wt = mlr_lds<kBlock / 64>(m, d.P, smem_raw);
    const uint32_t waves_total = gridDim.x * (kBlock / 64);
    unsigned long long c_acts = 0, c_rows = 0;
    for (uint32_t w = blockIdx.x * (kBlock / 64) + wave; w < n; w += waves_total) {
        const uint32_t slot = d.lr_list[w];
        const uint32_t uidx = d.uid[slot];
        uint32_t fl = 0;
        const uint32_t action = mlr_act_wave(d, wt, slot, lane, s_cnt[wave], s_prod[wave], &fl, nullptr);
        c_acts += 1; c_rows += h_cnt(hist_row(d, slot)[0]);
        if (lane == 0) {
            d.lr_action[uidx] = action; d.lr_dirty[uidx] = 0;
            if (fl & RG_MLR_UNRESOLVED) {     // (user id, the event index the act was computed at, the action taken) for the host
                const unsigned long long pos = atomicAdd(&d.counters[RG_CNT_POLY_UNRESOLVED], 1ull);
                if (pos < kPolyListCap) {
                    uint32_t* e = d.pl_list + 3 * static_cast<size_t>(pos);
                    e[0] = static_cast<uint32_t>(d.first_user + uidx); e[1] = d.run_ahead ? d.ev[uidx] : t; e[2] = action;
                }
            }
        }
    }
    // the counters once per block (as k_poly_acts)
    if (lane == 0 && c_acts) {
        atomicAdd(&s_sum[0], c_acts);
        atomicAdd(&s_sum[1], c_rows);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_sum[0]) {
        atomicAdd(&d.counters[RG_CNT_LR_ACTS], s_sum[0]);
        atomicAdd(&d.counters[RG_CNT_LR_ROWS], s_sum[1]);
    }
}

// rg_sim_debug_mlr_acts: the same act for every user index of the reset range (slot == user index right after the reset), with the
// scores z[i][a]
__global__ void __launch_bounds__(kBlock) k_debug_mlr_acts(DevSim d, MlrModel m, int32_t* action, uint8_t* flags, double* z) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ double s_cnt[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_prod[kBlock / 64][kPolyHist];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    if (blockIdx.x * (kBlock / 64) >= d.n_users) return;
    const double* wt = mlr_lds<kBlock / 64>(m, d.P, smem_raw);
    const uint32_t waves_total = gridDim.x * (kBlock / 64);
    for (uint32_t i = blockIdx.x * (kBlock / 64) + wave; i < d.n_users; i += waves_total) {
        uint32_t fl = 0;
        const uint32_t a = mlr_act_wave(d, wt, i, lane, s_cnt[wave], s_prod[wave], &fl, z + static_cast<size_t>(i) * d.P);
        if (lane == 0) { action[i] = static_cast<int32_t>(a); flags[i] = static_cast<uint8_t>(fl); }
    }
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
