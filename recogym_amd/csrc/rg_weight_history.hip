// rg_weight_history.hip — librecogym_hip.so: the likelihood agent's act on a time-weighted view history (weight_history_function)
// in the step loop.  (see rg_wh_common.hpp for the timed row, the feature list and the act; DESIGN.md 4g for the contract)
//
// A run with a weight table is lock-step, and none of the step's other kernels knows of it: the draw kernels log the step's organic
// views as ever, k_advance takes the bandit event's action from lr_action and writes the trailing row of a stopping user.  Three
// launches of this unit stand round them (launch_step):
//   k_wh_insert       after the draws: the step's organic views, read back from their log rows, into the users' TIMED rows (WhRun::rows,
//                     indexed by user index, so a repack does not move them) at the clock value logged on the view's row;
//   k_poly_acts_w 0   before k_advance: a fresh act for every bandit event of the step at the clock value of its row -> lr_action;
//   k_poly_acts_w 1   after k_advance: the trailing row of every user that stopped at this step is acted again at ITS clock value
//                     (phantom_time, or the event index t + 1), on a history that holds the step's view, and patched in place.
// The cached act of the count form (lr_dirty, k_logreg_select, k_poly_acts) is not used: an act is stale as soon as the clock moves.

#include "rg_wh_common.hpp"
#include "rg_act_common.hpp"
#include "rg_ope_common.hpp"

namespace rgk {

__device__ __forceinline__ hent_t* wh_row(const DevSim& d, const WhRun& r, uint32_t uidx) { return r.rows + static_cast<size_t>(uidx) * d.hist_cap; }

// a clock value as the reference's int16 cast gives it inside [0, 32767] (truncation); 0xFFFF outside: no act accepts it
__device__ __forceinline__ uint32_t wh_clock16(double x) { return (x >= 0.0 && x < 32768.0) ? static_cast<uint32_t>(x) : 0xFFFFu; }

__global__ void __launch_bounds__(kBlock) k_wh_insert(DevSim d, WhRun r, uint32_t t) {
    const uint32_t n_o = d.step_cnt[2 * t + RG_STATE_ORGANIC];
    const uint32_t* cur = list_ptr(d, t & 1, RG_STATE_ORGANIC);
    for (uint32_t pos = blockIdx.x * kBlock + threadIdx.x; pos < n_o; pos += gridDim.x * kBlock) {
        const uint32_t uidx = d.uid[cur[pos]];
        const uint64_t row = d.log_base[t] + pos;               // write_organic_row's
        if (!d.log || row >= d.log_cap) continue;               // the view is lost with its row: RG_CNT_LOG_DROPPED says so, and the run is repeated
        const uint32_t v = d.log[row].code & RG_EV_INDEX_MASK;
        const uint32_t t16 = wh_clock16(d.time_mode ? d.utime[uidx] : static_cast<double>(t));
        if (t16 == 0xFFFFu) atomicAdd(&d.counters[RG_CNT_WH_CLOCK_RANGE], 1ull);
        if (v < d.P && wh_insert(wh_row(d, r, uidx), d.hist_cap, v, t16)) atomicAdd(&d.counters[RG_CNT_HIST_OVERFLOW], 1ull);
    }
}

// phase 0: the bandit events of step t; phase 1: the trailing rows k_advance wrote at step t.  A wave per act.
__global__ void __launch_bounds__(kBlock) k_poly_acts_w(DevSim d, WhRun r, uint32_t t, uint32_t phase) {
    __shared__ double s_th[kPolySteps];
    __shared__ double s_val[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_prod[kBlock / 64][kPolyHist];
    __shared__ double s_w[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_ep[kBlock / 64][kPolyHist];
    __shared__ unsigned long long s_sum[4];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < d.pl_nth; i += kBlock) s_th[i] = d.pl_th[i];
    if (threadIdx.x < 4) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t n_o = d.step_cnt[2 * t + RG_STATE_ORGANIC], n_b = d.step_cnt[2 * t + RG_STATE_BANDIT];
    const uint32_t* cur_o = list_ptr(d, t & 1, RG_STATE_ORGANIC);
    const uint32_t* cur_b = list_ptr(d, t & 1, RG_STATE_BANDIT);
    const uint32_t n = phase ? n_o + n_b : n_b;
    const uint32_t waves_total = gridDim.x * (kBlock / 64), gw = blockIdx.x * (kBlock / 64) + wave;
    uint32_t* g_prod = r.spill ? r.spill + static_cast<size_t>(gw) * 2 * r.spill_cap : nullptr;      // this wave's, beyond kPolyHist products
    uint32_t* g_bits = r.spill ? g_prod + r.spill_cap : nullptr;
    unsigned long long c[4] = {};             // acts, list entries, acts decided on the table, acts with a clock value out of range
    for (uint32_t w = gw; w < n; w += waves_total) {
        const uint32_t slot = phase ? (w < n_o ? cur_o[w] : cur_b[w - n_o]) : cur_b[w];
        const uint32_t uidx = d.uid[slot];
        if (phase && !(d.has_phantom[uidx] && d.n_events[uidx] == t + 1)) continue;        // (wave-uniform) did not stop here
        const uint32_t t_act = t + phase;                                                    // the event index of the act's own row
        const uint32_t now = d.time_mode ? wh_clock16(phase ? d.phantom_time[uidx] : d.utime[uidx]) : (t_act < kWhTableLen ? t_act : 0xFFFFu);
        const hent_t* hr = wh_row(d, r, uidx);
        const uint32_t ne = min(h_cnt(hr[0]), d.hist_cap - 1);
        uint32_t fl = 0, ln = 0;
        bool range = false;
        const uint32_t action = wh_act(d, r.wt, hr + 1, ne, now, lane, s_th, s_w[wave], s_ep[wave], s_val[wave], s_prod[wave], g_prod, g_bits,
                                       r.spill_cap, &fl, &ln, &range);
        c[0] += 1; c[1] += ln; c[2] += fl & 1u; c[3] += range ? 1u : 0u;
        if (lane == 0) {
            if (phase) d.phantom[uidx].code = RG_EV_BANDIT | RG_EV_PHANTOM | action;
            else d.lr_action[uidx] = action;
            if (fl & 2u) act_list_add<false>(d, uidx, t_act, action);      // (the event index of the act's own row)
        }
    }
    act_count(d, s_sum, lane, c, {RG_CNT_LR_ACTS, RG_CNT_LR_ROWS, RG_CNT_POLY_TABLE, RG_CNT_WH_CLOCK_RANGE});
}

// rg_sim_debug_set_timed_history: the timed rows of the reset range, a thread per user index.  The views go in one at a time, in
// the order given, through the insert a run uses: a view that finds its row full is dropped and counted.  A product outside [0, P)
// is no view of this catalogue and is skipped.
__global__ void __launch_bounds__(kBlock) k_debug_set_timed_history(DevSim d, WhRun r, const uint32_t* n, const uint32_t* prod, const uint16_t* t16,
                                                                     uint32_t stride) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < d.n_users; i += gridDim.x * kBlock) {
        hent_t* hr = wh_row(d, r, i);
        hr[0] = 0ull;
        unsigned long long dropped = 0;
        const uint32_t nv = min(n[i], stride);
        for (uint32_t j = 0; j < nv; ++j) {
            const uint32_t v = prod[static_cast<size_t>(i) * stride + j];
            if (v < d.P) dropped += wh_insert(hr, d.hist_cap, v, t16[static_cast<size_t>(i) * stride + j]);
        }
        if (dropped) atomicAdd(&d.counters[RG_CNT_HIST_OVERFLOW], dropped);
    }
}

// rg_sim_debug_weighted_acts: wh_act for every user index of the reset range at the clock value now16[i], a wave per user; the
// caller's list arrays (stride entries per user) are the act's source of a list longer than kPolyHist as well
__global__ void __launch_bounds__(kBlock) k_debug_weighted_acts(DevSim d, WhRun r, const uint16_t* now16, int32_t* action, uint8_t* flags,
                                                                 uint32_t* list_n, uint32_t* list_prod, uint32_t* list_bits, uint32_t stride) {
    __shared__ double s_th[kPolySteps];
    __shared__ double s_val[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_prod[kBlock / 64][kPolyHist];
    __shared__ double s_w[kBlock / 64][kPolyHist];
    __shared__ uint32_t s_ep[kBlock / 64][kPolyHist];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < d.pl_nth; i += kBlock) s_th[i] = d.pl_th[i];
    __syncthreads();
    const uint32_t waves_total = gridDim.x * (kBlock / 64);
    for (uint32_t i = blockIdx.x * (kBlock / 64) + wave; i < d.n_users; i += waves_total) {
        const hent_t* hr = wh_row(d, r, i);
        const uint32_t ne = min(h_cnt(hr[0]), d.hist_cap - 1);
        uint32_t fl = 0, ln = 0;
        bool range = false;
        const uint32_t a = wh_act(d, r.wt, hr + 1, ne, now16[i], lane, s_th, s_w[wave], s_ep[wave], s_val[wave], s_prod[wave],
                                  list_prod + static_cast<size_t>(i) * stride, list_bits + static_cast<size_t>(i) * stride, stride, &fl, &ln,
                                  &range);
        if (lane == 0) {
            action[i] = static_cast<int32_t>(a); flags[i] = static_cast<uint8_t>(fl); list_n[i] = ln;
            if (range) atomicAdd(&d.counters[RG_CNT_WH_CLOCK_RANGE], 1ull);
        }
    }
}

// ------------------------------------------------------------------------------------------
// The training feed from a sorted device log (rg_weighted_feed): AbstractFeatureProvider.train_data with a weight function — one
// feature row per bandit row (the trailing row included), the user's views before it weighted at the row's clock value.  One wave
// per user, users assigned statically as in the replay units (rg_ope_common.hpp); the wave carries the user's TIMED row in its
// part of the workspace (max_user_rows + 1 words: nothing is dropped), lane 0 inserts every organic row as a run does, and at
// every bandit row the whole wave runs wh_list at the row's time.  mode 0 leaves the list's length at the row's bandit ordinal
// (brow); mode 1 writes the list at crow[ordinal]: products ascending into col, float32 bit patterns into val.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kFeedMaxWaves = 2048;
constexpr int kFeedWsErr = 0, kFeedWsRange = 1, kFeedWsRows = 2;      // head words: ope_check_log's error bits; rows with a time outside [0, 32767]; bandit rows
constexpr size_t kFeedHeadBytes = 256;

__global__ void __launch_bounds__(64 * kOpeWaves) k_weighted_feed(const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users,
                                                                   uint32_t max_user_rows, const uint16_t* __restrict__ t16, WhTable wt, uint32_t mode,
                                                                   const int64_t* __restrict__ brow, int32_t* len, const int64_t* __restrict__ crow,
                                                                   uint32_t* col, uint32_t* val, unsigned long long* ws, hent_t* timed, uint32_t W) {
    __shared__ double s_val[kOpeWaves][kPolyHist];
    __shared__ uint32_t s_prod[kOpeWaves][kPolyHist];
    __shared__ double s_w[kOpeWaves][kPolyHist];
    __shared__ uint32_t s_ep[kOpeWaves][kPolyHist];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kOpeWaves + wv;
    const uint32_t cap = max_user_rows + 1;
    hent_t* hr = timed + static_cast<size_t>(wave) * cap;
    unsigned long long c_range = 0, c_rows = 0;
    for (uint64_t u = wave; u < n_users; u += W) {
        const int64_t b = offsets[u], e = offsets[u + 1];
        if (lane == 0) hr[0] = 0ull;
        ope_list_sync<false>();
        for (int64_t r = b; r < e; ++r) {                      // (r, and everything read at it, is wave-uniform)
            const uint32_t code = rows[r].code, tr = t16[r];
            if (tr >= kWhTableLen) c_range += 1;
            if (!(code & RG_EV_BANDIT)) {
                if (lane == 0) (void)wh_insert(hr, cap, code & RG_EV_INDEX_MASK, tr);      // (ope_check_log: at most max_user_rows rows)
                ope_list_sync<false>();
                continue;
            }
            c_rows += 1;
            const int64_t k = brow[r];
            const uint32_t ne = min(h_cnt(hr[0]), max_user_rows);
            uint32_t* g_prod = nullptr;
            uint32_t* g_bits = nullptr;
            uint32_t g_cap = 0;
            if (mode) { g_prod = col + crow[k]; g_bits = val + crow[k]; g_cap = static_cast<uint32_t>(crow[k + 1] - crow[k]); }
            bool range = false;
            const uint32_t n = wh_list(wt, hr + 1, ne, tr, lane, s_w[wv], s_ep[wv], s_val[wv], s_prod[wv], g_prod, g_bits, g_cap, &range);
            if (!mode && lane == 0) len[k] = static_cast<int32_t>(n);
        }
    }
    if (lane == 0) {
        if (c_range) (void)__hip_atomic_fetch_add(&ws[kFeedWsRange], c_range, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c_rows) (void)__hip_atomic_fetch_add(&ws[kFeedWsRows], c_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

void (*wh_insert_kernel())(DevSim, WhRun, uint32_t) { return k_wh_insert; }
void (*wh_acts_kernel())(DevSim, WhRun, uint32_t, uint32_t) { return k_poly_acts_w; }
void (*wh_debug_set_kernel())(DevSim, WhRun, const uint32_t*, const uint32_t*, const uint16_t*, uint32_t) { return k_debug_set_timed_history; }
void (*wh_debug_acts_kernel())(DevSim, WhRun, const uint16_t*, int32_t*, uint8_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t) {
    return k_debug_weighted_acts;
}

}  // namespace rgk

extern "C" size_t rg_weighted_feed_workspace_bytes(uint64_t n_users, uint32_t max_user_rows) {
    return kFeedHeadBytes + static_cast<size_t>(ope_waves(n_users, kFeedMaxWaves)) * (static_cast<size_t>(max_user_rows) + 1) * sizeof(hent_t);
}

extern "C" int rg_weighted_feed(const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users, uint32_t max_user_rows, uint32_t num_products,
                                const uint16_t* d_t16, const double* d_table, uint32_t n, uint32_t accumulate_f32, uint32_t mode,
                                const int64_t* d_brow, int32_t* d_len, const int64_t* d_crow, int32_t* d_col, float* d_val, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
    const char* who = "rg_weighted_feed";
    if (num_products == 0 || num_products > RG_EV_INDEX_MASK) return fail(RG_EINVAL, "%s: bad num_products %u", who, num_products);
    if (!d_table || n == 0 || n > kWhTableLen) return fail(RG_EINVAL, "%s: the weight table has %u entries (1 .. 32768)", who, n);
    if (mode > 1u) return fail(RG_EINVAL, "%s: mode %u (0: lengths, 1: col / val)", who, mode);
    if (n_users && (!d_rows || !d_offsets || !d_t16 || !d_brow)) return fail(RG_EINVAL, "%s: null rows / offsets / times / ordinals", who);
    if (n_users && (mode ? (!d_crow || !d_col || !d_val) : !d_len)) return fail(RG_EINVAL, "%s: null output of mode %u", who, mode);
    if (!d_workspace || workspace_bytes < rg_weighted_feed_workspace_bytes(n_users, max_user_rows))
        return fail(RG_ENOMEM, "%s: workspace %zu < %zu bytes", who, workspace_bytes, rg_weighted_feed_workspace_bytes(n_users, max_user_rows));
    if (reinterpret_cast<uintptr_t>(d_rows) % 16) return fail(RG_EINVAL, "%s: rows not 16-byte aligned", who);
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    OpeCall c{};
    c.d_rows = d_rows; c.d_offsets = d_offsets; c.n_users = n_users; c.max_user_rows = max_user_rows;
    c.d_workspace = d_workspace; c.workspace_bytes = workspace_bytes; c.stream = static_cast<hipStream_t>(stream);
    unsigned long long* ws = c.at<unsigned long long>(0);
    if (int rc = ope_check_log(who, c, num_products, ws)) return rc;      // zeroes the head, validates the log before anything is written
    if (!n_users) return RG_OK;
    const uint32_t W = ope_waves(n_users, kFeedMaxWaves);
    hipLaunchKernelGGL(k_weighted_feed, dim3(W / kOpeWaves), dim3(64 * kOpeWaves), 0, c.stream, d_rows, d_offsets, n_users, max_user_rows, d_t16,
                       WhTable{d_table, n, accumulate_f32 ? 1u : 0u}, mode, d_brow, d_len, d_crow, reinterpret_cast<uint32_t*>(d_col),
                       reinterpret_cast<uint32_t*>(d_val), ws, c.at<hent_t>(kFeedHeadBytes), W);
    HIP_TRY(hipGetLastError());
    return RG_OK;
}
