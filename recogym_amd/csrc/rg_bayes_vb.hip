// rg_bayes_vb.hip — librecogym_hip.so: the posterior-sample act of BayesianAgentVB (RG_POLICY_BAYES_VB) in the step loop.
// (see rg_common.hpp for the shared types and helpers, rg_bayes_common.hpp for the act, DESIGN.md 4h for the contract and the margin)

#include "rg_bayes_common.hpp"

namespace rgk {

// The act of the user in `slot` (wave-uniform), by the whole wave: bayes_act on the user's history row.
__device__ uint32_t bayes_act_wave(const DevSim& d, uint32_t slot, int lane, double* s_cnt, uint32_t* s_prod, uint32_t* flags, double* q_out) {
    const hent_t* hr = hist_row(d, slot) + 1;             // entries after the header
    const BayesModel m{d.P, d.pl_nth, d.pl_wk_t};         // (the model's two slots in DevSim)
    return bayes_act(m, PolyRowHist{hr, h_cnt(hr[-1])}, lane, s_cnt, s_prod, flags, q_out);
}

// a wave per listed act, over the lr_list / lr_action / lr_dirty plumbing of k_poly_acts; unresolved acts go to the same list
__global__ void __launch_bounds__(kBlock) k_bayes_acts(DevSim d, uint32_t t) {
    __shared__ double s_cnt[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_prod[kBlock / 64][kPolyHist];
    __shared__ unsigned long long s_sum[4];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    if (threadIdx.x < 4) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t n = d.lr_cnt[t];
    const uint32_t waves_total = gridDim.x * (kBlock / 64);
    unsigned long long c_acts = 0, c_rows = 0, c_sat = 0;
    for (uint32_t w = blockIdx.x * (kBlock / 64) + wave; w < n; w += waves_total) {
        const uint32_t slot = d.lr_list[w];
        const uint32_t uidx = d.uid[slot];
        uint32_t fl = 0;
        const uint32_t action = bayes_act_wave(d, slot, lane, s_cnt[wave], s_prod[wave], &fl, nullptr);
        c_acts += 1; c_rows += h_cnt(hist_row(d, slot)[0]);
        c_sat += fl & RG_BAYES_SATURATED;
        if (lane == 0) {
            d.lr_action[uidx] = action; d.lr_dirty[uidx] = 0;
            if (fl & RG_BAYES_UNRESOLVED) {   // (user id, the event index the act was computed at, the action taken) for the host
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
        if (c_sat) atomicAdd(&s_sum[2], c_sat);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_sum[0]) {
        atomicAdd(&d.counters[RG_CNT_LR_ACTS], s_sum[0]);
        atomicAdd(&d.counters[RG_CNT_LR_ROWS], s_sum[1]);
        if (s_sum[2]) atomicAdd(&d.counters[RG_CNT_BAYES_SATURATED], s_sum[2]);
    }
}

// rg_sim_debug_bayes_acts: the same act for every user index of the reset range (slot == user index right after the reset), with
// the means q[i][a]
__global__ void __launch_bounds__(kBlock) k_debug_bayes_acts(DevSim d, int32_t* action, uint8_t* flags, double* q) {
    __shared__ double s_cnt[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_prod[kBlock / 64][kPolyHist];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t waves_total = gridDim.x * (kBlock / 64);
    for (uint32_t i = blockIdx.x * (kBlock / 64) + wave; i < d.n_users; i += waves_total) {
        uint32_t fl = 0;
        const uint32_t a = bayes_act_wave(d, i, lane, s_cnt[wave], s_prod[wave], &fl, q + static_cast<size_t>(i) * d.P);
        if (lane == 0) { action[i] = static_cast<int32_t>(a); flags[i] = static_cast<uint8_t>(fl); }
    }
}

search_kernel_t bayes_acts_kernel() { return k_bayes_acts; }
void (*bayes_debug_kernel())(DevSim, int32_t*, uint8_t*, double*) { return k_debug_bayes_acts; }

}  // namespace rgk
