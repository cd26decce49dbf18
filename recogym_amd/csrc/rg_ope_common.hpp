// rg_ope_common.hpp — the skeleton the off-policy replay units share (rg_ope.hip, rg_ope_logreg.hip, rg_ope_eg.hip).
//
// One wave per user, users assigned statically (wave w takes users w, w + W, ...).  A user's rows stream in coalesced 64-row
// chunks (16-byte rg_event per lane + the row's float64 ps); a unit computes the target policy's pi of every bandit lane, the
// skeleton divides by ps, writes the row's ratio and click and adds to the lane's three float64 accumulators.  At the end the
// wave's xor butterfly leaves (n, sum c r, sum r) in the wave's slot and one block reduces the slots in a fixed order: no float
// atomics, so d_sums holds the same bits on every run — and the same bits from every entry point that walks the same rows
// with the same W.  W is part of those bits: every unit keeps its own cap.
#pragma once

#include "rg_common.hpp"

namespace rgk {

constexpr int kOpeWaves = 4;                    // waves per block

inline uint32_t ope_waves(uint64_t n_users, uint32_t max_waves) {
    const uint64_t w = (n_users + kOpeWaves - 1) / kOpeWaves * kOpeWaves;
    return static_cast<uint32_t>(w < kOpeWaves ? kOpeWaves : (w > max_waves ? max_waves : w));
}

inline size_t ope_slot_bytes(uint32_t n_waves) { return (static_cast<size_t>(n_waves) * 3 * sizeof(double) + 255) & ~size_t(255); }

// the log and the outputs of a replay, as every replay kernel gets them
struct OpeLog {
    const rg_event* __restrict__ rows;
    const int64_t* __restrict__ offsets;
    uint64_t n_users;
    uint32_t ps_mode;
    const double* __restrict__ ps64;
    double ps_const;
    double* __restrict__ ratio;
    uint8_t* __restrict__ click;
    double* __restrict__ slots;
    uint32_t n_waves;
};

// a lane's row of the 64-row chunk at `base` of a user whose rows end at `e` (beyond e: neither bandit nor organic)
struct OpeRow {
    int64_t row;
    uint4 x;
    bool isb, iso;
    uint32_t idx;
};

__device__ __forceinline__ OpeRow ope_load(const OpeLog& log, int64_t base, int64_t e, uint32_t lane) {
    OpeRow r;
    r.row = base + lane;
    const bool live = r.row < e;
    r.x = make_uint4(0u, 0u, 0u, 0u);
    if (live) r.x = reinterpret_cast<const uint4*>(log.rows)[r.row];
    r.isb = live && (r.x.z & RG_EV_BANDIT);
    r.iso = live && !(r.x.z & RG_EV_BANDIT);
    r.idx = r.x.z & RG_EV_INDEX_MASK;
    return r;
}

// the product of the last organic row before this lane's (in the chunk, else `lpv`, carried from the chunks before; `lpv`
// moves on to the chunk's last organic row): BanditMFSquare.update_lpv
__device__ __forceinline__ uint32_t ope_last_view(const OpeRow& r, uint32_t lane, uint32_t& lpv) {
    const uint64_t omask = __ballot(r.iso);
    const uint64_t before = omask & (lane ? (~0ull >> (64 - lane)) : 0ull);
    const int src = before ? 63 - __clzll(static_cast<long long>(before)) : 0;
    const uint32_t from = static_cast<uint32_t>(__shfl(static_cast<int>(r.idx), src));
    const uint32_t mine = before ? from : lpv;
    if (omask) lpv = static_cast<uint32_t>(__shfl(static_cast<int>(r.idx), 63 - __clzll(static_cast<long long>(omask))));
    return mine;
}

// EpsilonGreedy's explore flip of the act at (user u, event t): words 0,1 of the policy block of (the wrapper's seed, u, t) against
// the first entry of NumPy's normalised cdf of p = [eps, 1 - eps] (agents/epsilon_greedy.py: rng.choice([True, False], p)).
// Shared by the off-policy replay (rg_ope_eg.hip) and the evolution statistics (rg_evolve.hip).
__device__ __forceinline__ double eg_threshold(double eps) { return eps / (eps + (1.0 - eps)); }
__device__ __forceinline__ bool eg_explored(uint64_t seed, double thr, uint32_t u, uint32_t t) {
    const rg_u32x4 w = rg_draw(seed, u, t, 0, RG_DRAW_POLICY);
    return !(thr <= rg_uniform(w.w[0], w.w[1]));
}

// a lane's (n, sum c r, sum r) over its bandit rows, in row order
struct OpeAcc {
    double n = 0.0, cr = 0.0, r = 0.0;

    // a bandit row whose target probability is pi
    __device__ __forceinline__ void emit(const OpeLog& log, const OpeRow& row, double pi) {
        const double ps = log.ps_mode == RG_OPE_PS_ARRAY ? log.ps64[row.row]
                          : log.ps_mode == RG_OPE_PS_CONST ? log.ps_const : static_cast<double>(__uint_as_float(row.x.w));
        const double q = pi / ps;
        log.ratio[row.row] = q;
        if (log.click) log.click[row.row] = (row.x.z & RG_EV_CLICK) ? 1 : 0;
        n += 1.0;
        cr += ((row.x.z & RG_EV_CLICK) ? 1.0 : 0.0) * q;
        r += q;
    }

    // the wave's sums into its slot (every lane of the wave calls it)
    __device__ __forceinline__ void store(const OpeLog& log, uint32_t wave, uint32_t lane) const {
        const double sn = wave_sum(n), scr = wave_sum(cr), sr = wave_sum(r);
        if (lane == 0) {
            log.slots[3 * static_cast<size_t>(wave) + 0] = sn;
            log.slots[3 * static_cast<size_t>(wave) + 1] = scr;
            log.slots[3 * static_cast<size_t>(wave) + 2] = sr;
        }
    }
};

// the per-wave slots -> d_sums = (n, sum c r, sum r): k_ope_reduce, one block, fixed order (rg_ope.hip)
int ope_reduce(const double* slots, uint32_t n_waves, double* d_sums, hipStream_t stream);

// the argument checks every replay entry point makes after those of its own policy; `need` = its workspace bytes
inline int ope_args_ok(const char* who, uint32_t ps_mode, const double* d_ps, uint64_t n_users, const rg_event* d_rows,
                       const int64_t* d_offsets, const double* d_ratio, const double* d_sums, const void* d_workspace,
                       size_t workspace_bytes, size_t need) {
    if (ps_mode > RG_OPE_PS_ROW || (ps_mode == RG_OPE_PS_ARRAY && !d_ps && n_users)) return fail(RG_EINVAL, "%s: bad ps source", who);
    if (n_users && (!d_rows || !d_offsets || !d_ratio)) return fail(RG_EINVAL, "%s: null rows / offsets / ratio", who);
    if (!d_sums || !d_workspace) return fail(RG_EINVAL, "%s: null sums / workspace", who);
    if (workspace_bytes < need) return fail(RG_ENOMEM, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(d_rows) % 16) return fail(RG_EINVAL, "%s: rows not 16-byte aligned", who);
    return RG_OK;
}

}  // namespace rgk
