// rg_ope_common.hpp — the skeleton the off-policy replay units share (rg_ope.hip, rg_ope_logreg.hip, rg_ope_eg.hip, rg_ope_poly.hip,
// rg_ope_nn.hip, rg_ope_bayes.hip), and what the units that keep a sorted view history share besides: the list
// insert (ope_list_add) and the validation of the log (ope_check_log).
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

// ---- what the units that keep a sorted (product, count) history per wave share (rg_ope_logreg.hip, rg_ope_poly.hip) ----
constexpr uint32_t kOpeNone = 0xFFFFFFFFu;

// what one lane wrote to a list is read by the others: LDS within the workgroup's scope; the global list through the agent's
// (the wave's own stores complete and its L1 lines are dropped before the next read)
template <bool kLds>
__device__ __forceinline__ void ope_list_sync() {
    if (kLds) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    else __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    __builtin_amdgcn_wave_barrier();
}

// one view of product p into the sorted list (lp, lc)[0 .. n); false = the list is full (nothing written)
template <bool kLds>
__device__ __forceinline__ bool ope_list_add(uint32_t* lp, uint32_t* lc, uint32_t& n, uint32_t cap, uint32_t p, uint32_t lane) {
    uint32_t pos = 0, found = kOpeNone;
    for (uint32_t j0 = 0; j0 < n; j0 += 64) {
        const uint32_t j = j0 + lane;
        const uint32_t v = j < n ? lp[j] : kOpeNone;                   // (p < 2^29: never the filler)
        const unsigned long long hit = __ballot(v == p);
        if (hit) { found = j0 + static_cast<uint32_t>(__builtin_ctzll(hit)); break; }
        const uint32_t less = static_cast<uint32_t>(__popcll(__ballot(v < p)));
        pos += less;
        if (less < 64) break;                                         // ascending: nothing smaller beyond
    }
    if (found != kOpeNone) {
        if (lane == 0) lc[found] += 1;
        ope_list_sync<kLds>();
        return true;
    }
    if (n >= cap) return false;
    // entries pos .. n-1 move up one place, 64 at a time from the top (a chunk is read whole before it is written)
    for (uint32_t hi = n; hi > pos; hi = hi - pos > 64 ? hi - 64 : pos) {
        const bool on = lane < hi - pos;
        const uint32_t j = hi - 1 - lane;
        uint32_t vp = 0, vc = 0;
        if (on) { vp = lp[j]; vc = lc[j]; }
        ope_list_sync<kLds>();
        if (on) { lp[j + 1] = vp; lc[j + 1] = vc; }
        ope_list_sync<kLds>();
    }
    if (lane == 0) { lp[pos] = p; lc[pos] = 1; }
    ope_list_sync<kLds>();
    n += 1;
    return true;
}

// EpsilonGreedy's explore flip of the act at (user u, event t): words 0,1 of the policy block of (the wrapper's seed, u, t) against
// the first entry of NumPy's normalised cdf of p = [eps, 1 - eps] (agents/epsilon_greedy.py: rng.choice([True, False], p)).
// Shared by the off-policy replay (rg_ope_eg.hip) and the evolution statistics (rg_evolve.hip).
__device__ __forceinline__ double eg_threshold(double eps) { return eps / (eps + (1.0 - eps)); }
__device__ __forceinline__ bool eg_explored(uint64_t seed, double thr, uint32_t u, uint32_t t) {
    const rg_u32x4 w = rg_draw(seed, u, t, 0, RG_DRAW_POLICY);
    return !(thr <= rg_uniform(w.w[0], w.w[1]));
}

// The EpsilonGreedy form of a model unit's replay kernel (rg_ope_logreg.hip, rg_ope_poly.hip: templates on EG).  The EG
// instantiation takes one more kernel argument, an OpeEg — the wrapper and the two optional outputs of rg_ope_replay_eg — and the
// plain one takes none: its code and its kernel arguments are what they were.  ope_model_pi: pi of a bandit lane whose action is
// `a` under a model whose act is g (one-hot inner pi); the flip is the row's own, the act is shared by the rows up to the next
// organic row.
struct OpeEg {
    rg_ope_eg eg;
    uint8_t* __restrict__ greedy;
    int32_t* __restrict__ h0;
};

__device__ __forceinline__ double ope_model_pi(const OpeRow&, uint32_t g, uint32_t a) { return g == a ? 1.0 : 0.0; }
__device__ __forceinline__ double ope_model_pi(const OpeRow& r, uint32_t g, uint32_t a, const OpeEg& x) {
    const double eps = x.eg.epsilon;
    const bool explore = eg_explored(x.eg.seed, eg_threshold(eps), r.x.x, r.x.y);
    if (x.greedy) x.greedy[r.row] = explore ? 0 : 1;
    if (x.h0) x.h0[r.row] = static_cast<int32_t>(g);
    return explore ? eps * ((x.eg.pure_new && a == g) ? 0.0 : x.eg.prob_explore) : (1.0 - eps) * (a == g ? 1.0 : 0.0);
}

// ---- recall@k (evaluate_recall_at_k: rg_ope_recall.hip the table form, rg_ope_logreg.hip the ranking form) ----
// d_hit values.  A bandit row is COUNTED when it has no click and its successor INSIDE THE USER'S RANGE is an organic row.
constexpr uint8_t kRecallMiss = RG_RECALL_MISS, kRecallHit = RG_RECALL_HIT, kRecallNotCounted = RG_RECALL_NOT_COUNTED,
                  kRecallUnresolved = RG_RECALL_UNRESOLVED;

// The `code` word of every lane's successor row, or 0 with has_next = false where the lane's row is its user's last (or beyond
// `e`).  Lane i < 63 takes lane i + 1's; lane 63 reads the first row of the next chunk, and only where base + 64 < e: no row at
// or beyond the user's end e <= d_offsets[n_users] is ever addressed.
__device__ __forceinline__ uint32_t ope_next_code(const rg_event* __restrict__ rows, int64_t row, int64_t e, uint32_t code, uint32_t lane,
                                                  bool& has_next) {
    has_next = row + 1 < e;
    uint32_t next = static_cast<uint32_t>(__shfl_down(static_cast<int>(code), 1));
    if (lane == 63 && has_next) next = rows[row + 1].code;
    return has_next ? next : 0u;
}

__device__ __forceinline__ bool ope_recall_counted(uint32_t code, uint32_t next, bool has_next) {
    return (code & RG_EV_BANDIT) && !(code & RG_EV_CLICK) && has_next && !(next & RG_EV_BANDIT);
}

// The ranking form of a model unit's replay kernel (rg_ope_logreg.hip: one more kernel argument, as OpeEg is for the EG form).
// sums = (counted, hits); list = (user, position of the row within the user's rows, next view) of the rows inside the margin.
struct OpeRecall {
    uint8_t* __restrict__ hit;
    unsigned long long* __restrict__ sums;
    uint32_t* __restrict__ list;
    uint32_t list_cap;
    uint32_t k;
};

// the first (only) argument of a kernel's trailing pack
template <typename T>
__device__ __forceinline__ const T& ope_pack_arg(const T& x) { return x; }

// the wrapper's own argument checks (the three EpsilonGreedy entry points')
inline int ope_eg_ok(const char* who, const rg_ope_eg* eg, uint32_t num_products) {
    if (!eg) return fail(RG_EINVAL, "%s: null eg", who);
    if (!(eg->epsilon >= 0.0 && eg->epsilon <= 1.0)) return fail(RG_EINVAL, "%s: epsilon %g outside [0, 1]", who, eg->epsilon);
    if (eg->pure_new && num_products < 2u) return fail(RG_EINVAL, "%s: epsilon_pure_new needs at least 2 products", who);
    return RG_OK;
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

// What every replay entry point receives besides its policy or model — the log, the ps source, the outputs and the workspace — packed
// once by the extern "C" function and handed on whole.  Host side only: a kernel takes the pointers as loose __restrict__ arguments
// (a member of a by-value struct would lose the qualifier).
struct OpeCall {
    const rg_event* d_rows;
    const int64_t* d_offsets;
    uint64_t n_users;
    uint32_t max_user_rows;
    uint32_t ps_mode;
    const double* d_ps;
    double ps_const;
    double* d_ratio;
    uint8_t* d_click;
    double* d_sums;
    void* d_workspace;
    size_t workspace_bytes;
    hipStream_t stream;

    // the workspace from byte `first` on
    template <typename T>
    T* at(size_t first) const { return reinterpret_cast<T*>(static_cast<char*>(d_workspace) + first); }
};

// the argument checks every replay entry point makes after those of its own policy; `need` = its workspace bytes
inline int ope_args_ok(const char* who, const OpeCall& c, size_t need) {
    if (c.ps_mode > RG_OPE_PS_ROW || (c.ps_mode == RG_OPE_PS_ARRAY && !c.d_ps && c.n_users)) return fail(RG_EINVAL, "%s: bad ps source", who);
    if (c.n_users && (!c.d_rows || !c.d_offsets || !c.d_ratio)) return fail(RG_EINVAL, "%s: null rows / offsets / ratio", who);
    if (!c.d_sums || !c.d_workspace) return fail(RG_EINVAL, "%s: null sums / workspace", who);
    if (c.workspace_bytes < need) return fail(RG_ENOMEM, "%s: workspace %zu < %zu bytes", who, c.workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(c.d_rows) % 16) return fail(RG_EINVAL, "%s: rows not 16-byte aligned", who);
    return RG_OK;
}

// a history-keeping unit's validation (rg_ope_logreg.hip): zeroes the 32 int64 head words of `ws` (word 0: error bits), then
// refuses a user that opens with a bandit row or has more than max_user_rows rows and a product or an action >= P, before
// anything is written.  Synchronises the stream once (the verdict).
int ope_check_log(const char* who, const OpeCall& c, uint32_t P, unsigned long long* ws);

}  // namespace rgk
