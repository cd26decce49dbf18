// rg_ope_poly_w.hip — off-policy evaluation replay of the likelihood agent on a TIME-WEIGHTED view history (LogregPolyFrozenAgent /
// LogregPolyAgent with a weight_history_function, device_weight_history and with_ps_all = True) over a sorted device log:
// pi = [act(the user's views so far, weighted at the row's clock value) == a], / ps, for every bandit row.  DESIGN.md 4g.
//
// The skeleton is rg_ope_common.hpp's (one wave per user, 64-row chunks, per-wave sums and the fixed-order reduction) and the chunk
// walk is k_ope_poly's; the act is rg_wh_common.hpp's wh_act, the one function the step loop's k_poly_acts_w runs.  What is this
// unit's own:
//
// History.  The user's views are a TIMED list — one word (product << 32 | uint16 time) per view, ascending — in the wave's part of
// the workspace, max_user_rows + 1 words as k_weighted_feed keeps it (rg_weight_history.hip): nothing is dropped.  An organic row
// inserts at the clock value d_t16[row], by lane 0; the list lives in global memory only (the serial act per row bounds this path,
// not the insert).
//
// Act.  At EVERY bandit row, by the whole wave, at that row's clock value: an act is stale as soon as the clock moves, so nothing is
// cached between bandit rows.  d_act, where given, receives the act at every bandit row (recall@k's key).  A feature list longer
// than kPolyHist goes through per-wave g_prod / g_bits scratch of min(P, max_user_rows) entries, so no act of a valid log is short
// of room.
//
// Unresolved acts (flag bit 1) follow rg_ope_poly.hip's protocol — (user, position of the bandit row within the user's rows, action
// taken), kPolyListCap entries and an overflow word — with one entry per unresolved bandit row, for sim.weighted_replay_verify.
// Head word 7 counts the rows whose d_t16 lies outside [0, 32767] and, beside them, the acts at a row inside the range whose list
// wh_list built from a clamped table index (a view outside the range or AFTER the act — a clock that runs backwards inside a user —
// or a difference beyond the table's n entries): not 0, the ratios are not the reference's.
//
// W, the wave cap: 4 096 = 256 CUs x 4 blocks of 4 waves (a block holds 32 KB of LDS: 8 KB step table and 6 KB per wave — s_val,
// s_prod, s_w, s_ep of kPolyHist entries).  W is part of the bits of d_sums (rg_ope_common.hpp).
#include "rg_ope_common.hpp"
#include "rg_wh_common.hpp"

namespace {

typedef unsigned long long pw_u64;

constexpr uint32_t kPwMaxWaves = 4096;           // 256 CUs x 16 waves
constexpr int kPwWsErr = 0, kPwWsActs = 1, kPwWsTable = 2, kPwWsLower = 3, kPwWsUnresolved = 4, kPwWsOverflow = 5, kPwWsRowsRead = 6,
              kPwWsRange = 7, kPwWsWords = 32;

// entries of a wave's g_prod / g_bits scratch: the longest feature list (distinct products <= views <= rows), where kPolyHist is short
uint32_t pw_spill_cap(uint32_t P, uint32_t max_user_rows) {
    const uint32_t longest = P < max_user_rows ? P : max_user_rows;
    return longest > kPolyHist ? longest : 0u;
}
size_t pw_head_bytes() { return kPwWsWords * sizeof(pw_u64); }
size_t pw_list_bytes() { return (static_cast<size_t>(kPolyListCap) * 3 * sizeof(uint32_t) + 255) & ~size_t(255); }
size_t pw_timed_bytes(uint32_t W, uint32_t max_user_rows) {
    return (static_cast<size_t>(W) * (static_cast<size_t>(max_user_rows) + 1) * sizeof(hent_t) + 255) & ~size_t(255);
}

__global__ __launch_bounds__(64 * kOpeWaves, 4) void k_ope_poly_w(
    PolyModel m, WhTable wt, const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users, uint32_t max_user_rows,
    const uint16_t* __restrict__ t16, uint32_t ps_mode, const double* __restrict__ ps64, double ps_const, double* __restrict__ ratio,
    uint8_t* __restrict__ click, double* __restrict__ slots, int32_t* __restrict__ act_out, hent_t* timed, uint32_t* gscr, uint32_t g_cap,
    pw_u64* __restrict__ ws, uint32_t* __restrict__ ulist, uint32_t n_waves) {
    __shared__ double s_th[kPolySteps];
    __shared__ double s_val[kOpeWaves][kPolyHist];
    __shared__ uint32_t s_prod[kOpeWaves][kPolyHist];
    __shared__ double s_w[kOpeWaves][kPolyHist];
    __shared__ uint32_t s_ep[kOpeWaves][kPolyHist];
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kOpeWaves + wib;
    for (uint32_t i = threadIdx.x; i < m.pl_nth; i += 64 * kOpeWaves) s_th[i] = m.pl_th[i];
    __syncthreads();
    const uint32_t cap = max_user_rows + 1;
    hent_t* const hr = timed + static_cast<size_t>(wave) * cap;
    uint32_t* const g_prod = g_cap ? gscr + static_cast<size_t>(wave) * 2 * g_cap : nullptr;
    uint32_t* const g_bits = g_cap ? g_prod + g_cap : nullptr;
    const uint32_t P = m.P;
    const OpeLog log{rows, offsets, n_users, ps_mode, ps64, ps_const, ratio, click, slots, n_waves};
    OpeAcc acc;
    pw_u64 c_acts = 0, c_table = 0, c_lower = 0, c_rows = 0, c_range = 0;

    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        if (lane == 0) hr[0] = 0ull;
        ope_list_sync<false>();

        for (int64_t base = b; base < e; base += 64) {
            const OpeRow r = ope_load(log, base, e, lane);
            const uint32_t idx = r.idx;
            const bool live = r.isb || r.iso;
            const uint32_t tr = live ? t16[r.row] : 0u;
            c_range += static_cast<pw_u64>(__popcll(__ballot(live && tr >= kWhTableLen)));
            const bool ok = idx < P;                  // (the validation pass has refused such a log: never index the model)
            const bool isb = ok && r.isb, iso = ok && r.iso;
            const pw_u64 omask = __ballot(iso), bmask = __ballot(isb);
            double pi = 0.0;
            for (pw_u64 rem = omask | bmask; rem; rem &= rem - 1) {
                const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(rem));
                const uint32_t now = lane_value(tr, k);
                if ((omask >> k) & 1) {
                    const uint32_t p = lane_value(idx, k);
                    if (lane == 0) (void)wh_insert(hr, cap, p, now);      // (ope_check_log: at most max_user_rows rows)
                    ope_list_sync<false>();
                    continue;
                }
                const uint32_t ne = min(h_cnt(hr[0]), max_user_rows);
                uint32_t fl = 0, ln = 0;
                bool range = false;
                const uint32_t action = wave_uniform(wh_act(m, wt, hr + 1, ne, now, static_cast<int>(lane), s_th, s_w[wib], s_ep[wib],
                                                            s_val[wib], s_prod[wib], g_prod, g_bits, g_cap, &fl, &ln, &range));
                fl = wave_uniform(fl);                 // (both are the same in every lane: kept in scalar registers)
                c_acts += 1;
                c_rows += wave_uniform(ln);
                c_table += fl & 1u;
                c_lower += (fl >> 2) & 1u;
                // wh_list read the table at a clamped index (a view outside the range or after `now`, a difference beyond the table):
                // the act does not stand.  An act whose own clock is outside was counted with its row above.
                if (range && now < kWhTableLen) c_range += 1;
                if ((fl & 2u) && lane == 0) {
                    const pw_u64 pos = __hip_atomic_fetch_add(&ws[kPwWsUnresolved], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (pos < kPolyListCap) {
                        uint32_t* q = ulist + 3 * static_cast<size_t>(pos);
                        q[0] = static_cast<uint32_t>(user); q[1] = static_cast<uint32_t>(base - b) + k; q[2] = action;
                    } else {
                        (void)__hip_atomic_fetch_or(&ws[kPwWsOverflow], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                if (lane == k) {
                    pi = ope_model_pi(r, action, idx);
                    if (act_out) act_out[r.row] = static_cast<int32_t>(action);
                }
            }
            if (isb) acc.emit(log, r, pi);
        }
    }
    acc.store(log, wave, lane);
    if (lane == 0) {
        if (c_acts) {
            (void)__hip_atomic_fetch_add(&ws[kPwWsActs], c_acts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(&ws[kPwWsRowsRead], c_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c_table) (void)__hip_atomic_fetch_add(&ws[kPwWsTable], c_table, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c_lower) (void)__hip_atomic_fetch_add(&ws[kPwWsLower], c_lower, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (c_range) (void)__hip_atomic_fetch_add(&ws[kPwWsRange], c_range, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int pw_model_ok(const rg_ope_poly_w* m, const char* who) {
    if (!m) return fail(RG_EINVAL, "%s: null model", who);
    if (int rc = pl_model_ok(&m->model, who)) return rc;
    if (!m->table || m->n == 0 || m->n > kWhTableLen) return fail(RG_EINVAL, "%s: the weight table has %u entries (1 .. 32768)", who, m->n);
    return RG_OK;
}

}  // namespace

extern "C" size_t rg_ope_poly_w_workspace_bytes(const rg_ope_poly_w* m, uint64_t n_users, uint32_t max_user_rows) {
    if (!m) { fail(RG_EINVAL, "rg_ope_poly_w_workspace_bytes: null model"); return 0; }
    const uint32_t W = ope_waves(n_users, kPwMaxWaves);
    return pw_head_bytes() + pw_list_bytes() + ope_slot_bytes(W) + pw_timed_bytes(W, max_user_rows) +
           static_cast<size_t>(W) * 2 * pw_spill_cap(m->model.num_products, max_user_rows) * sizeof(uint32_t);
}

extern "C" int rg_ope_replay_poly_w(const rg_ope_poly_w* m, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                                    uint32_t max_user_rows, const uint16_t* d_t16, uint32_t ps_mode, const double* d_ps, double ps_const,
                                    double* d_ratio, uint8_t* d_click, double* d_sums, int32_t* d_act, void* d_workspace,
                                    size_t workspace_bytes, void* stream) {
    const char* who = "rg_ope_replay_poly_w";
    if (int rc = pw_model_ok(m, who)) return rc;
    if (n_users && !d_t16) return fail(RG_EINVAL, "%s: null times", who);
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    if (int rc = ope_args_ok(who, c, rg_ope_poly_w_workspace_bytes(m, n_users, max_user_rows))) return rc;
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    const uint32_t P = m->model.num_products;
    const uint32_t W = ope_waves(n_users, kPwMaxWaves);
    const uint32_t g_cap = pw_spill_cap(P, max_user_rows);
    pw_u64* ws = c.at<pw_u64>(0);
    uint32_t* ulist = c.at<uint32_t>(pw_head_bytes());
    size_t at = pw_head_bytes() + pw_list_bytes();
    double* slots = c.at<double>(at);
    at += ope_slot_bytes(W);
    hent_t* timed = c.at<hent_t>(at);
    at += pw_timed_bytes(W, max_user_rows);
    uint32_t* gscr = g_cap ? c.at<uint32_t>(at) : nullptr;
    if (int rc = ope_check_log(who, c, P, ws)) return rc;
    const PolyModel pm{P, m->model.n_steps, m->model.wf, m->model.wa, m->model.wk_t, m->model.th, m->model.intercept};
    hipLaunchKernelGGL(k_ope_poly_w, dim3(W / kOpeWaves), dim3(64 * kOpeWaves), 0, c.stream, pm, WhTable{m->table, m->n, m->accumulate_f32 ? 1u : 0u},
                       d_rows, d_offsets, n_users, max_user_rows, d_t16, ps_mode, d_ps, ps_const, d_ratio, d_click, slots, d_act, timed, gscr,
                       g_cap, ws, ulist, W);
    HIP_TRY(hipGetLastError());
    return ope_reduce(slots, W, d_sums, c.stream);
}
