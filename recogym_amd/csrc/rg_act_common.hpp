// rg_act_common.hpp — the skeleton the model agents' act kernels of the step loop share (rg_logreg_poly.hip, rg_bayes_vb.hip,
// rg_nn_ips.hip, rg_mlr.hip; the list append and the counter reduction also rg_weight_history.hip).  DESIGN.md 4k states the contract.
//
// One wave per listed act, grid-stride over lr_list[0 .. lr_cnt[t]) (k_logreg_select's list of the slots whose view history changed
// since their last act).  The wave's act goes to lr_action[user index] (and lr_ps, where the agent yields a propensity), lr_dirty
// clears, an unresolved act is appended to pl_list for the host's confirmation, and the counters are added once per block.
//
// A unit — a small struct its .hip file defines, built whole by the kernel from its own LDS and its model argument, as the replay
// units' act objects are (rg_ope_list.hpp) — is what differs between the agents:
//   stage(d) -> staged                     what the block stages before its first act, handed to every act
//   kStage                                 kStageNone: stage() does nothing; kStageOpen: it writes LDS and the skeleton's barrier ends it;
//                                          kStageSynced: it ends with a barrier of its own (nn_lds, mlr_lds)
//   act(d, staged, slot, lane, wave, &flags, &ps, row)   the wave's act of the user in `slot` (wave-uniform); row: where the debug kernel
//                                          wants the act's per-action values of that user (null in the step loop)
//   kUnresolved                            the flag bit that lists the act
//   kExtraMask, kExtraCounter              flag bit 0 counted into one more counter (kExtraMask == 0: none)
//   kPs                                    the act yields a propensity: lr_ps is written
//   kRow                                   the act has a per-action debug output (the debug kernel's `row`)
//   kIdleReturn                            a block that owns no act returns before it stages (a unit whose staging costs)
//   kSums                                  words of the block's counter sums
// All of them compile-time: a kernel pays for none it does not use.  The two skeleton functions take the kernel's DevSim and the
// unit BY VALUE and the source keeps the order of the kernels it replaced (where the act count is read, where the sums are zeroed,
// the event index chosen inside the list's cap branch): with that the five step-loop kernels compile to the code they had.
#pragma once

#include "rg_poly_common.hpp"

namespace rgk {

constexpr int kActWaves = kBlock / 64;          // waves per block of every act kernel
enum ActStage { kStageNone, kStageOpen, kStageSynced };

// (user id, the event index the act was computed at, the action taken) of an unresolved act, for the host (rg_sim_poly_list).
// kRounds: the act is the count form's, whose event index in a run-ahead round is the user's own (ev[uidx]), `t` in lock-step;
// without it `t` is the event index as the caller has it (k_poly_acts_w).
template <bool kRounds>
__device__ __forceinline__ void act_list_add(const DevSim& d, uint32_t uidx, uint32_t t, uint32_t action) {
    const unsigned long long pos = atomicAdd(&d.counters[RG_CNT_POLY_UNRESOLVED], 1ull);
    if (pos < kPolyListCap) {
        uint32_t* e = d.pl_list + 3 * static_cast<size_t>(pos);
        e[0] = static_cast<uint32_t>(d.first_user + uidx); e[1] = kRounds && d.run_ahead ? d.ev[uidx] : t; e[2] = action;
    }
}

// The wave's N sums c (c[0]: its acts) into the counters idx, once per block: lane 0 of every wave that acted adds to s_sum
// (zeroed before the block's last barrier), thread 0 adds the block's sums to the counters.  Sums 0 and 1 go together; a sum
// from 2 on is added where it is not zero.  Every thread of the block calls it.
template <int N>
__device__ __forceinline__ void act_count(const DevSim& d, unsigned long long* s_sum, int lane, const unsigned long long (&c)[N],
                                          const int (&idx)[N]) {
    if (lane == 0 && c[0]) {
        atomicAdd(&s_sum[0], c[0]);
        atomicAdd(&s_sum[1], c[1]);
#pragma unroll
        for (int k = 2; k < N; ++k)
            if (c[k]) atomicAdd(&s_sum[k], c[k]);
    }
    __syncthreads();
    const unsigned long long acts = s_sum[0];                   // (read by every thread, ahead of thread 0's branch)
    if (threadIdx.x == 0 && acts) {
        atomicAdd(&d.counters[idx[0]], acts);
        atomicAdd(&d.counters[idx[1]], s_sum[1]);
#pragma unroll
        for (int k = 2; k < N; ++k)
            if (s_sum[k]) atomicAdd(&d.counters[idx[k]], s_sum[k]);
    }
}

// the step loop's act kernel of a unit: the acts of lr_list[0 .. lr_cnt[t])  (d, u by value: see the top of the file)
template <class Unit>
__device__ __forceinline__ void act_list_run(const DevSim d, uint32_t t, const Unit u) {
    constexpr bool kExtra = Unit::kExtraMask != 0u;
    __shared__ unsigned long long s_sum[Unit::kSums];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    // the step's acts: read ahead of the staging where an idle block returns on it, behind the staging's barrier otherwise
    uint32_t n = Unit::kIdleReturn ? d.lr_cnt[t] : 0u;
    if (Unit::kIdleReturn && blockIdx.x * kActWaves >= n) return;   // (the whole block: no act of the grid-stride loop is its)
    // the sums are zeroed ahead of the barrier that ends the staging: the unit's own (kStageSynced), or the one here
    if (Unit::kStage == kStageSynced && threadIdx.x < Unit::kSums) s_sum[threadIdx.x] = 0ull;
    const auto staged = u.stage(d);
    if constexpr (Unit::kStage != kStageSynced) {
        if (threadIdx.x < Unit::kSums) s_sum[threadIdx.x] = 0ull;
        __syncthreads();
    }
    if (!Unit::kIdleReturn) n = d.lr_cnt[t];
    const uint32_t waves_total = gridDim.x * kActWaves;
    unsigned long long c_acts = 0, c_rows = 0, c_extra = 0;         // acts, history entries read, acts with the extra flag
    for (uint32_t w = blockIdx.x * kActWaves + wave; w < n; w += waves_total) {
        const uint32_t slot = d.lr_list[w];
        const uint32_t uidx = d.uid[slot];
        uint32_t fl = 0;
        double ps = 1.0;
        const uint32_t action = u.act(d, staged, slot, lane, wave, &fl, &ps, nullptr);
        c_acts += 1; c_rows += h_cnt(hist_row(d, slot)[0]);
        if constexpr (kExtra) c_extra += fl & Unit::kExtraMask;
        if (lane == 0) {
            d.lr_action[uidx] = action;
            if constexpr (Unit::kPs) d.lr_ps[uidx] = ps;
            d.lr_dirty[uidx] = 0;
            if (fl & Unit::kUnresolved) act_list_add<true>(d, uidx, t, action);
        }
    }
    if constexpr (kExtra) act_count(d, s_sum, lane, {c_acts, c_rows, c_extra}, {RG_CNT_LR_ACTS, RG_CNT_LR_ROWS, Unit::kExtraCounter});
    else act_count(d, s_sum, lane, {c_acts, c_rows}, {RG_CNT_LR_ACTS, RG_CNT_LR_ROWS});
}

// a unit's debug kernel: the same act for every user index of the reset range (slot == user index right after the reset), a
// wave per user -> action[i], flags[i] and, of a unit with kRow, its per-action output row[i][0 .. P), of a unit with kPs, ps[i]
template <class Unit>
__device__ __forceinline__ void act_debug_run(const DevSim d, const Unit u, int32_t* action, uint8_t* flags, double* row, double* ps) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    if (Unit::kIdleReturn && blockIdx.x * kActWaves >= d.n_users) return;
    const auto staged = u.stage(d);
    if constexpr (Unit::kStage == kStageOpen) __syncthreads();
    const uint32_t waves_total = gridDim.x * kActWaves;
    for (uint32_t i = blockIdx.x * kActWaves + wave; i < d.n_users; i += waves_total) {
        uint32_t fl = 0;
        double p = 1.0;
        double* r = nullptr;
        if constexpr (Unit::kRow) r = row + static_cast<size_t>(i) * d.P;
        const uint32_t a = u.act(d, staged, i, lane, wave, &fl, &p, r);
        if (lane == 0) {
            action[i] = static_cast<int32_t>(a); flags[i] = static_cast<uint8_t>(fl);
            if constexpr (Unit::kPs) ps[i] = p;
        }
    }
}

}  // namespace rgk
