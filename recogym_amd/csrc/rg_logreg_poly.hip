// rg_logreg_poly.hip — librecogym_hip.so: the act of the likelihood agent (LogregPolyAgent, RG_POLICY_LOGREG_POLY) in the step loop.
// (see rg_common.hpp for the shared types and helpers, DESIGN.md 4f for the contract, the merge rule and its proof)

#include "rg_poly_common.hpp"

namespace rgk {

// The act of the user in `slot` (wave-uniform), by the whole wave: poly_act (rg_poly_common.hpp) on the user's history row.
__device__ uint32_t poly_act_wave(const DevSim& d, uint32_t slot, int lane, const double* s_th, double* s_cnt, uint32_t* s_prod,
                                  uint32_t* flags) {
    const hent_t* hr = hist_row(d, slot) + 1;             // entries after the header
    return poly_act(d, PolyRowHist{hr, h_cnt(hr[-1])}, lane, s_th, s_cnt, s_prod, flags);
}

__global__ void __launch_bounds__(kBlock) k_poly_acts(DevSim d, uint32_t t) {
    __shared__ double s_th[kPolySteps];
    __shared__ double s_cnt[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_prod[kBlock / 64][kPolyHist];
    __shared__ unsigned long long s_sum[4];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < d.pl_nth; i += kBlock) s_th[i] = d.pl_th[i];
    if (threadIdx.x < 4) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t n = d.lr_cnt[t];
    const uint32_t waves_total = gridDim.x * (kBlock / 64);
    unsigned long long c_acts = 0, c_rows = 0, c_table = 0;
    for (uint32_t w = blockIdx.x * (kBlock / 64) + wave; w < n; w += waves_total) {
        const uint32_t slot = d.lr_list[w];
        const uint32_t uidx = d.uid[slot];
        uint32_t fl = 0;
        const uint32_t action = poly_act_wave(d, slot, lane, s_th, s_cnt[wave], s_prod[wave], &fl);
        c_acts += 1; c_rows += h_cnt(hist_row(d, slot)[0]);
        c_table += fl & 1u;
        if (lane == 0) {
            d.lr_action[uidx] = action; d.lr_dirty[uidx] = 0;
            if (fl & 2u) {       // (user id, the event index the act was computed at, the action taken) for the host
                const unsigned long long pos = atomicAdd(&d.counters[RG_CNT_POLY_UNRESOLVED], 1ull);
                if (pos < kPolyListCap) {
                    uint32_t* e = d.pl_list + 3 * static_cast<size_t>(pos);
                    e[0] = static_cast<uint32_t>(d.first_user + uidx); e[1] = d.run_ahead ? d.ev[uidx] : t; e[2] = action;
                }
            }
        }
    }
    // the counters once per block (as k_logreg_decide)
    if (lane == 0 && c_acts) {
        atomicAdd(&s_sum[0], c_acts);
        atomicAdd(&s_sum[1], c_rows);
        if (c_table) atomicAdd(&s_sum[2], c_table);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_sum[0]) {
        atomicAdd(&d.counters[RG_CNT_LR_ACTS], s_sum[0]);
        atomicAdd(&d.counters[RG_CNT_LR_ROWS], s_sum[1]);
        if (s_sum[2]) atomicAdd(&d.counters[RG_CNT_POLY_TABLE], s_sum[2]);
    }
}

// rg_sim_debug_poly_acts: the same act for every user index of the reset range (slot == user index right after the reset)
__global__ void __launch_bounds__(kBlock) k_debug_poly_acts(DevSim d, int32_t* action, uint8_t* flags) {
    __shared__ double s_th[kPolySteps];
    __shared__ double s_cnt[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_prod[kBlock / 64][kPolyHist];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < d.pl_nth; i += kBlock) s_th[i] = d.pl_th[i];
    __syncthreads();
    const uint32_t waves_total = gridDim.x * (kBlock / 64);
    for (uint32_t i = blockIdx.x * (kBlock / 64) + wave; i < d.n_users; i += waves_total) {
        uint32_t fl = 0;
        const uint32_t a = poly_act_wave(d, i, lane, s_th, s_cnt[wave], s_prod[wave], &fl);
        if (lane == 0) { action[i] = static_cast<int32_t>(a); flags[i] = static_cast<uint8_t>(fl); }
    }
}

search_kernel_t poly_acts_kernel() { return k_poly_acts; }
void (*poly_debug_kernel())(DevSim, int32_t*, uint8_t*) { return k_debug_poly_acts; }

}  // namespace rgk
