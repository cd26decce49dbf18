// rg_ope_list.hpp — what the replay units of the two newest argmax agents share (rg_ope_nn.hip, rg_ope_bayes.hip): the
// walk of one user's rows that rg_ope_poly.hip states for the likelihood agent, with the act as a parameter.
//
// The skeleton is rg_ope_common.hpp's (one wave per user, 64-row chunks, OpeAcc, the fixed-order reduction).  ol_replay adds the
// state a user carries and what is reported, exactly as the poly unit does:
//
// History.  The user's views are a (product, count) list in ASCENDING PRODUCT ORDER (ope_list_add), the order both acts add
// their terms in: up to kOlLds = 512 entries in a per-wave LDS list, beyond that a per-wave list in global memory of max_user_rows
// entries (distinct products <= rows).  Nothing is dropped; the views persist across the user's sessions and are reset per user.
//
// Act.  `act(hist, &flags)` — nn_act or bayes_act on a PolyListHist, by the whole wave — is taken only at a bandit row whose history
// changed since the user's previous act; the bandit rows up to the next organic row reuse it.  Inside a chunk the acts are taken in
// row order.
//
// Unresolved acts (`unresolved_bit` of the flags) go to the list behind the head — (user index, position of the bandit row the
// act was computed at within the user's rows, action taken), kPolyListCap entries, one atomic counter and an overflow word — for
// the host's confirmation (sim.replay_verify); the ratios are written with the device's action whatever the host decides.
//
// EG form: with an OpeEg as the trailing argument the act is the wrapper's GREEDY action and pi is ope_model_pi's EG overload,
// which also writes d_greedy / d_h0.
//
// Workspace: OPE_HEAD_BYTES of int64 head words (0 error, 1 acts, the rest the unit's: OlHead), the unresolved list, the W slots,
// the W global lists.
#pragma once

#include "rg_ope_common.hpp"
#include "rg_poly_common.hpp"

namespace rgk {

typedef unsigned long long ol_u64;

constexpr uint32_t kOlLds = 512;                 // entries of the per-wave LDS list (4 KiB per wave, 16 KiB per block)
constexpr ol_u64 kOlErrRows = 4;                 // (ope_check_log's bit for a user beyond max_user_rows)
constexpr int kOlWsErr = 0, kOlWsActs = 1, kOlWsWords = 32;

inline uint32_t ol_global_cap(uint32_t max_user_rows) { return max_user_rows > kOlLds ? max_user_rows : 0u; }
inline size_t ol_head_bytes() { return kOlWsWords * sizeof(ol_u64); }
inline size_t ol_list_bytes() { return (static_cast<size_t>(kPolyListCap) * 3 * sizeof(uint32_t) + 255) & ~size_t(255); }
inline size_t ol_workspace_bytes(uint32_t W, uint32_t max_user_rows) {
    return ol_head_bytes() + ol_list_bytes() + ope_slot_bytes(W) + static_cast<size_t>(W) * 2 * ol_global_cap(max_user_rows) * sizeof(uint32_t);
}

// the head words a unit places itself
struct OlHead {
    int unresolved, overflow, rows_read;
};

// a block's four lists
struct OlLds {
    uint32_t p[kOpeWaves][kOlLds];
    uint32_t c[kOpeWaves][kOlLds];
};

// One wave's share of the replay: users wave, wave + n_waves, ...  Every lane of the wave calls it.  `act`: uint32_t operator()(const
// PolyListHist&, uint32_t* flags), wave-uniform results; count(flags) after every act and report(ws) once, by lane 0, for the head
// words that are the unit's own.
template <class Act, typename... Eg>
__device__ __forceinline__ void ol_replay(Act& act, uint32_t unresolved_bit, OlHead hw, uint32_t P, const OpeLog& log, uint32_t* lp,
                                          uint32_t* lc, uint32_t* __restrict__ gscr, uint32_t g_cap, ol_u64* __restrict__ ws,
                                          uint32_t* __restrict__ ulist, uint32_t wave, uint32_t lane, Eg... ega) {
    uint32_t* const gp = g_cap ? gscr + static_cast<size_t>(wave) * 2 * g_cap : nullptr;
    uint32_t* const gc = gp + g_cap;
    OpeAcc acc;
    ol_u64 c_acts = 0, c_rows = 0, err = 0;

    for (uint64_t user = wave; user < log.n_users; user += log.n_waves) {
        const int64_t b = log.offsets[user], e = log.offsets[user + 1];
        uint32_t n = 0;
        bool global = false, dirty = true;
        uint32_t action = kPolyNone;

        for (int64_t base = b; base < e; base += 64) {
            const OpeRow r = ope_load(log, base, e, lane);
            const uint32_t idx = r.idx;
            const bool ok = idx < P;                  // (the validation pass has refused such a log: never index the model)
            const bool isb = ok && r.isb, iso = ok && r.iso;
            const ol_u64 omask = __ballot(iso), bmask = __ballot(isb);
            double pi = 0.0;
            ol_u64 rem = omask | bmask;
            while (rem) {
                const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(rem));
                if ((omask >> k) & 1) {
                    const uint32_t p = lane_value(idx, k);
                    bool done = false;
                    if (!global) {
                        if (n < kOlLds || !gp) {
                            done = true;
                            if (!ope_list_add<true>(lp, lc, n, kOlLds, p, lane)) err |= kOlErrRows;
                        } else {
                            for (uint32_t j = lane; j < n; j += 64) { gp[j] = lp[j]; gc[j] = lc[j]; }   // on to the global list
                            ope_list_sync<false>();
                            global = true;
                        }
                    }
                    if (!done && !ope_list_add<false>(gp, gc, n, g_cap, p, lane)) err |= kOlErrRows;
                    dirty = true;
                    rem &= rem - 1;
                    continue;
                }
                if (dirty && n) {                     // (n == 0: a user that opens with a bandit row, refused by the validation)
                    uint32_t fl = 0;
                    const PolyListHist hist{global ? gp : lp, global ? gc : lc, n};
                    action = wave_uniform(act(hist, &fl));
                    fl = wave_uniform(fl);             // (both are the same in every lane: kept in scalar registers)
                    c_acts += 1;
                    c_rows += n;
                    act.count(fl);
                    if ((fl & unresolved_bit) && lane == 0) {
                        const ol_u64 pos = __hip_atomic_fetch_add(&ws[hw.unresolved], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (pos < kPolyListCap) {
                            uint32_t* q = ulist + 3 * static_cast<size_t>(pos);
                            q[0] = static_cast<uint32_t>(user); q[1] = static_cast<uint32_t>(base - b) + k; q[2] = action;
                        } else {
                            (void)__hip_atomic_fetch_or(&ws[hw.overflow], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                    dirty = false;
                }
                // the bandit rows up to the next organic row share this act
                const ol_u64 next_o = omask & ~lanes_below(k);
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
            (void)__hip_atomic_fetch_add(&ws[kOlWsActs], c_acts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(&ws[hw.rows_read], c_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            act.report(ws);
        }
        if (err) (void)__hip_atomic_fetch_or(&ws[kOlWsErr], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace rgk
