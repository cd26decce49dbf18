// rg_ope_poly.hip — off-policy evaluation replay of the likelihood agent (LogregPolyFrozenAgent / LogregPolyAgent, reference
// agents/logreg_poly.py:143-167 with with_ps_all = True) over a sorted device log: pi = [act(the user's views so far) == a], / ps,
// for every bandit row.
//
// The skeleton is rg_ope_common.hpp's (one wave per user, 64-row chunks, per-wave sums and the fixed-order reduction); the act is
// rg_poly_common.hpp's poly_act, the one function the step loop's k_poly_acts runs (decision order, step table, margin W,
// kPolyFloor, the three flag bits: DESIGN.md 4f).  What is this unit's own is the state a user carries and what it reports.
//
// History.  The user's views are a (product, count) list in ASCENDING PRODUCT ORDER, the order poly_act adds the terms in.  An
// organic row inserts or increments (ope_list_add, shared with rg_ope_logreg.hip):
//   - up to 512 entries: a per-wave list in LDS;
//   - beyond: a per-wave list in global memory of max_user_rows entries (distinct products <= rows).
// Nothing is dropped; the views persist across the user's sessions and are reset per user.  (poly_act itself caches the first
// kPolyHist = 256 entries in its own LDS rows and reads the rest from the list.)
//
// Act.  Computed only at a bandit row whose history changed since the user's previous act; the bandit rows up to the next
// organic row reuse it.  Inside a chunk the acts are taken in row order, each by the whole wave.
//
// Unresolved acts (flag bit 1) are appended to a list in the workspace — (user, position of the bandit row the act was computed
// at within the user's rows, action taken), kPolyListCap entries and an overflow word — for the host's confirmation
// (sim.poly_replay_verify); the ratios are written with the device's action whatever the host decides.  The order of the list
// is not fixed (one atomic counter); ratios and sums do not depend on it.
//
// EpsilonGreedy round the agent (rg_ope_replay_poly_eg): k_ope_poly<true> — the same replay, the act above as the wrapper's GREEDY
// action g, and pi from ope_model_pi's EG form (rg_ope_common.hpp).  The unresolved list holds g; workspace and head words are the same.
//
// W, the wave cap: 4 096 = 256 CUs x 4 blocks of 4 waves (a block holds 36 KB of LDS: 8 KB step table, 3 KB of act rows and 4 KB
// of list per wave).  W is part of the bits of d_sums (rg_ope_common.hpp).
#include "rg_ope_common.hpp"
#include "rg_poly_common.hpp"

namespace {

typedef unsigned long long pl_u64;

constexpr uint32_t kPlLds = 512;                 // entries of the per-wave LDS list (4 KiB per wave, 16 KiB per block)
constexpr uint32_t kPlMaxWaves = 4096;           // 256 CUs x 16 waves
constexpr pl_u64 kPlErrRows = 4;                 // (ope_check_log's bit for a user beyond max_user_rows)
constexpr int kPlWsErr = 0, kPlWsActs = 1, kPlWsTable = 2, kPlWsLower = 3, kPlWsUnresolved = 4, kPlWsOverflow = 5, kPlWsRowsRead = 6,
              kPlWsWords = 32;

uint32_t pl_global_cap(uint32_t max_user_rows) { return max_user_rows > kPlLds ? max_user_rows : 0u; }
size_t pl_head_bytes() { return kPlWsWords * sizeof(pl_u64); }
size_t pl_list_bytes() { return (static_cast<size_t>(kPolyListCap) * 3 * sizeof(uint32_t) + 255) & ~size_t(255); }

template <bool EG, typename... Eg>       // EG: pi is the EpsilonGreedy wrapper's round this act (rg_ope_replay_poly_eg)
__global__ __launch_bounds__(64 * kOpeWaves, 4) void k_ope_poly(
    PolyModel m, const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users, uint32_t ps_mode,
    const double* __restrict__ ps64, double ps_const, double* __restrict__ ratio, uint8_t* __restrict__ click,
    double* __restrict__ slots, uint32_t* __restrict__ gscr, uint32_t g_cap, pl_u64* __restrict__ ws, uint32_t* __restrict__ ulist,
    uint32_t n_waves, Eg... ega) {
    static_assert(sizeof...(Eg) == (EG ? 1 : 0), "the EG instantiation takes an OpeEg, the plain one nothing");
    __shared__ double s_th[kPolySteps];
    __shared__ double s_cnt[kOpeWaves][kPolyHist];
    __shared__ uint32_t s_prod[kOpeWaves][kPolyHist];
    __shared__ uint32_t s_p[kOpeWaves][kPlLds];
    __shared__ uint32_t s_c[kOpeWaves][kPlLds];
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kOpeWaves + wib;
    for (uint32_t i = threadIdx.x; i < m.pl_nth; i += 64 * kOpeWaves) s_th[i] = m.pl_th[i];
    __syncthreads();
    uint32_t* const lp = s_p[wib];
    uint32_t* const lc = s_c[wib];
    uint32_t* const gp = g_cap ? gscr + static_cast<size_t>(wave) * 2 * g_cap : nullptr;
    uint32_t* const gc = gp + g_cap;
    const uint32_t P = m.P;
    const OpeLog log{rows, offsets, n_users, ps_mode, ps64, ps_const, ratio, click, slots, n_waves};
    OpeAcc acc;
    pl_u64 c_acts = 0, c_table = 0, c_lower = 0, c_rows = 0, err = 0;

    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        uint32_t n = 0;
        bool global = false, dirty = true;
        uint32_t action = kPolyNone;

        for (int64_t base = b; base < e; base += 64) {
            const OpeRow r = ope_load(log, base, e, lane);
            const uint32_t idx = r.idx;
            const bool ok = idx < P;                  // (the validation pass has refused such a log: never index the model)
            const bool isb = ok && r.isb, iso = ok && r.iso;
            const pl_u64 omask = __ballot(iso), bmask = __ballot(isb);
            double pi = 0.0;
            pl_u64 rem = omask | bmask;
            while (rem) {
                const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(rem));
                if ((omask >> k) & 1) {
                    const uint32_t p = lane_value(idx, k);
                    bool done = false;
                    if (!global) {
                        if (n < kPlLds || !gp) {
                            done = true;
                            if (!ope_list_add<true>(lp, lc, n, kPlLds, p, lane)) err |= kPlErrRows;
                        } else {
                            for (uint32_t j = lane; j < n; j += 64) { gp[j] = lp[j]; gc[j] = lc[j]; }   // on to the global list
                            ope_list_sync<false>();
                            global = true;
                        }
                    }
                    if (!done && !ope_list_add<false>(gp, gc, n, g_cap, p, lane)) err |= kPlErrRows;
                    dirty = true;
                    rem &= rem - 1;
                    continue;
                }
                if (dirty && n) {                     // (n == 0: a user that opens with a bandit row, refused by the validation)
                    uint32_t fl = 0;
                    const PolyListHist hist{global ? gp : lp, global ? gc : lc, n};
                    action = wave_uniform(poly_act(m, hist, static_cast<int>(lane), s_th, s_cnt[wib], s_prod[wib], &fl));
                    fl = wave_uniform(fl);             // (both are the same in every lane: kept in scalar registers)
                    c_acts += 1;
                    c_rows += n;
                    c_table += fl & 1u;
                    c_lower += (fl >> 2) & 1u;
                    if ((fl & 2u) && lane == 0) {
                        const pl_u64 pos = __hip_atomic_fetch_add(&ws[kPlWsUnresolved], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (pos < kPolyListCap) {
                            uint32_t* q = ulist + 3 * static_cast<size_t>(pos);
                            q[0] = static_cast<uint32_t>(user); q[1] = static_cast<uint32_t>(base - b) + k; q[2] = action;
                        } else {
                            (void)__hip_atomic_fetch_or(&ws[kPlWsOverflow], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                    dirty = false;
                }
                // the bandit rows up to the next organic row share this act
                const pl_u64 next_o = omask & ~lanes_below(k);
                const uint32_t end = next_o ? static_cast<uint32_t>(__builtin_ctzll(next_o)) : 64u;
                if (isb && lane >= k && lane < end) pi = ope_model_pi(r, action, idx, ega...);
                rem &= end < 64 ? ~lanes_below(end) : 0ull;
            }
            if (isb) acc.emit(log, r, pi);
        }
    }
    acc.store(log, wave, lane);
    if (lane == 0) {
        if (c_acts) {
            (void)__hip_atomic_fetch_add(&ws[kPlWsActs], c_acts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(&ws[kPlWsRowsRead], c_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c_table) (void)__hip_atomic_fetch_add(&ws[kPlWsTable], c_table, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c_lower) (void)__hip_atomic_fetch_add(&ws[kPlWsLower], c_lower, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (err) (void)__hip_atomic_fetch_or(&ws[kPlWsErr], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

extern "C" size_t rg_ope_poly_workspace_bytes(const rg_ope_poly* m, uint64_t n_users, uint32_t max_user_rows) {
    if (!m) { fail(RG_EINVAL, "rg_ope_poly_workspace_bytes: null model"); return 0; }
    const uint32_t W = ope_waves(n_users, kPlMaxWaves);
    return pl_head_bytes() + pl_list_bytes() + ope_slot_bytes(W) + static_cast<size_t>(W) * 2 * pl_global_cap(max_user_rows) * sizeof(uint32_t);
}

namespace {

template <bool EG>       // ega: null iff !EG
int pl_replay(const char* who, const rg_ope_poly* m, const OpeEg* ega, const OpeCall& c) {
    if (int rc = ope_args_ok(who, c, rg_ope_poly_workspace_bytes(m, c.n_users, c.max_user_rows))) return rc;
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    const uint32_t W = ope_waves(c.n_users, kPlMaxWaves);
    const uint32_t g_cap = pl_global_cap(c.max_user_rows);
    pl_u64* ws = c.at<pl_u64>(0);
    uint32_t* ulist = c.at<uint32_t>(pl_head_bytes());
    double* slots = c.at<double>(pl_head_bytes() + pl_list_bytes());
    uint32_t* gscr = g_cap ? c.at<uint32_t>(pl_head_bytes() + pl_list_bytes() + ope_slot_bytes(W)) : nullptr;
    if (int rc = ope_check_log(who, c, m->num_products, ws)) return rc;
    const PolyModel pm{m->num_products, m->n_steps, m->wf, m->wa, m->wk_t, m->th, m->intercept};
    // one spelling of the launch: the kernel, and the EG form's one more argument
    auto launch = [&](auto kernel, auto... eg) {
        hipLaunchKernelGGL(kernel, dim3(W / kOpeWaves), dim3(64 * kOpeWaves), 0, c.stream, pm, c.d_rows, c.d_offsets, c.n_users, c.ps_mode,
                           c.d_ps, c.ps_const, c.d_ratio, c.d_click, slots, gscr, g_cap, ws, ulist, W, eg...);
    };
    if constexpr (EG) launch(k_ope_poly<true, OpeEg>, *ega);
    else launch(k_ope_poly<false>);
    HIP_TRY(hipGetLastError());
    return ope_reduce(slots, W, c.d_sums, c.stream);
}

}  // namespace

extern "C" int rg_ope_replay_poly(const rg_ope_poly* m, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                                  uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                                  uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = pl_model_ok(m, "rg_ope_replay_poly")) return rc;
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    return pl_replay<false>("rg_ope_replay_poly", m, nullptr, c);
}

extern "C" int rg_ope_replay_poly_eg(const rg_ope_poly* m, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                                     uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                                     double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                                     void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = pl_model_ok(m, "rg_ope_replay_poly_eg")) return rc;
    if (int rc = ope_eg_ok("rg_ope_replay_poly_eg", eg, m->num_products)) return rc;
    const OpeEg ega{*eg, d_greedy, d_h0};
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    return pl_replay<true>("rg_ope_replay_poly_eg", m, &ega, c);
}
