// rg_ope_mlr.hip — off-policy evaluation replay of PyTorchMLRAgent (PyTorchMLRFrozenAgent, reference agents/pytorch_mlr.py:59-84)
// over a sorted device log: pi = [act(the user's views so far) == a], / ps, for every bandit row.
//
// The walk is rg_ope_list.hpp's (history list, act on a changed history only, unresolved list); the act is rg_mlr_common.hpp's
// mlr_act on a PolyListHist, the one function the step loop's k_mlr_acts runs (the stated order, the margin E, RG_MLR_UNRESOLVED —
// a count above 2^24 and an empty history are unresolved by mlr_act itself: DESIGN.md 4j).  Two instantiations: the plain one, and
// the skeleton's EG form (rg_ope_replay_mlr_eg), which writes the act of every bandit row (d_h0) — recall@k reads it, with
// epsilon = 0, as it does for the other argmax agents.  The entry refuses every other epsilon (RG_EINVAL): the EpsilonGreedy
// wrapper round this agent has no step-loop form and no test of its replay.
//
// The entry point checks the table for values that are not finite on the device (mlr_host_model, k_mlr_finite: 4 bytes come back),
// so a replay call synchronises twice — once for the model, once for the validation's verdict — and moves no table to the host.
//
// Head words: error, acts, unresolved, overflow, rows_read.
//
// LDS per block of kOpeWaves = 4 waves.  Static, 28 KB: the four lists (16 KB) and mlr_act's s_cnt / s_prod rows (12 KB).  Dynamic:
// the P x P table where it stays within kNnStageBytes = 48 KB (P <= 78) — the step loop's rule; otherwise mlr_act reads it from
// global memory through the same pointer.  Static + dynamic passes 64 KiB from 36 KB of dynamic LDS on (P >= 68), and the entry
// point then opts the kernel in (set_max_lds).  The most is 28 + 48 = 76 KB (P = 78: 47.5 KB of table).
//
// W, the wave cap: 2 048 = 256 CUs x 2 blocks of 4 waves.  A CU has 160 KB of LDS; two blocks of at most 76 KB are resident
// whatever is staged.  W is part of the bits of d_sums (rg_ope_common.hpp).
#include "rg_mlr_common.hpp"
#include "rg_ope_list.hpp"

namespace {

constexpr uint32_t kOmMaxWaves = 2048;           // 256 CUs x 2 blocks x 4 waves
constexpr OlHead kOmHead{2, 3, 4};               // error, acts, unresolved, overflow, rows_read
constexpr size_t kOmStaticLds = sizeof(OlLds) + kOpeWaves * kPolyHist * (sizeof(double) + sizeof(uint32_t));
static_assert(kOmStaticLds == 28 * 1024, "the header's LDS budget");
static_assert(kOmStaticLds + kNnStageBytes <= 80 * 1024, "two blocks per CU");

// mlr_act on the wave's list
struct OmAct {
    const double* wt;
    uint32_t P;
    int lane;
    double* s_cnt; uint32_t* s_prod;
    __device__ __forceinline__ uint32_t operator()(const PolyListHist& h, uint32_t* fl) const {
        return mlr_act(wt, P, h, lane, s_cnt, s_prod, fl, nullptr);
    }
    __device__ __forceinline__ void count(uint32_t) {}
    __device__ __forceinline__ void report(ol_u64*) const {}
};

template <bool EG, typename... Eg>       // EG: pi is the EpsilonGreedy wrapper's round this act (rg_ope_replay_mlr_eg)
__global__ __launch_bounds__(64 * kOpeWaves, 2) void k_ope_mlr(
    MlrModel m, uint32_t P, const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users, uint32_t ps_mode,
    const double* __restrict__ ps64, double ps_const, double* __restrict__ ratio, uint8_t* __restrict__ click,
    double* __restrict__ slots, uint32_t* __restrict__ gscr, uint32_t g_cap, ol_u64* __restrict__ ws, uint32_t* __restrict__ ulist,
    uint32_t n_waves, Eg... ega) {
    static_assert(sizeof...(Eg) == (EG ? 1 : 0), "the EG instantiation takes an OpeEg, the plain one nothing");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ double s_cnt[kOpeWaves][kPolyHist];
    __shared__ uint32_t s_prod[kOpeWaves][kPolyHist];
    __shared__ OlLds s_l;
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kOpeWaves + wib;
    const double* wt = mlr_lds<kOpeWaves>(m, P, smem_raw);
    const OpeLog log{rows, offsets, n_users, ps_mode, ps64, ps_const, ratio, click, slots, n_waves};
    OmAct act{wt, P, static_cast<int>(lane), s_cnt[wib], s_prod[wib]};
    ol_replay(act, RG_MLR_UNRESOLVED, kOmHead, P, log, s_l.p[wib], s_l.c[wib], gscr, g_cap, ws, ulist, wave, lane, ega...);
}

int om_model_ok(const rg_ope_mlr* m, const char* who) {
    if (!m) return fail(RG_EINVAL, "%s: null model", who);
    if (m->num_products == 0 || m->num_products > kMlrProducts)
        return fail(RG_EINVAL, "%s: num_products %u outside 1 .. %u", who, m->num_products, kMlrProducts);
    if (!m->wt) return fail(RG_EINVAL, "%s: null wt", who);
    return RG_OK;
}

}  // namespace

extern "C" size_t rg_ope_mlr_workspace_bytes(const rg_ope_mlr* m, uint64_t n_users, uint32_t max_user_rows) {
    if (!m) { fail(RG_EINVAL, "rg_ope_mlr_workspace_bytes: null model"); return 0; }
    return ol_workspace_bytes(ope_waves(n_users, kOmMaxWaves), max_user_rows);
}

namespace {

template <bool EG>       // ega: null iff !EG
int om_replay(const char* who, const rg_ope_mlr* m, const OpeEg* ega, const OpeCall& c) {
    if (int rc = ope_args_ok(who, c, rg_ope_mlr_workspace_bytes(m, c.n_users, c.max_user_rows))) return rc;
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    MlrModel mm;
    size_t smem = 0;
    char prefix[64];
    snprintf(prefix, sizeof(prefix), "%s: ", who);
    const uint32_t W = ope_waves(c.n_users, kOmMaxWaves);
    const uint32_t g_cap = ol_global_cap(c.max_user_rows);
    ol_u64* ws = c.at<ol_u64>(0);
    uint32_t* ulist = c.at<uint32_t>(ol_head_bytes());
    double* slots = c.at<double>(ol_head_bytes() + ol_list_bytes());
    uint32_t* gscr = g_cap ? c.at<uint32_t>(ol_head_bytes() + ol_list_bytes() + ope_slot_bytes(W)) : nullptr;
    // (the slots are scratch until the replay kernel writes them: their first word takes the finiteness verdict)
    if (int rc = mlr_host_model(prefix, m->num_products, m->wt, reinterpret_cast<uint32_t*>(slots), c.stream, &mm, &smem)) return rc;
    if (smem + kOmStaticLds > 64 * 1024) {
        set_max_lds(k_ope_mlr<false>, smem);
        set_max_lds(k_ope_mlr<true, OpeEg>, smem);
    }
    if (int rc = ope_check_log(who, c, m->num_products, ws)) return rc;
    // one spelling of the launch: the kernel, and the EG form's one more argument
    auto launch = [&](auto kernel, auto... eg) {
        hipLaunchKernelGGL(kernel, dim3(W / kOpeWaves), dim3(64 * kOpeWaves), smem, c.stream, mm, m->num_products, c.d_rows, c.d_offsets,
                           c.n_users, c.ps_mode, c.d_ps, c.ps_const, c.d_ratio, c.d_click, slots, gscr, g_cap, ws, ulist, W, eg...);
    };
    if constexpr (EG) launch(k_ope_mlr<true, OpeEg>, *ega);
    else launch(k_ope_mlr<false>);
    HIP_TRY(hipGetLastError());
    return ope_reduce(slots, W, c.d_sums, c.stream);
}

}  // namespace

extern "C" int rg_ope_replay_mlr(const rg_ope_mlr* m, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                                 uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                                 uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = om_model_ok(m, "rg_ope_replay_mlr")) return rc;
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    return om_replay<false>("rg_ope_replay_mlr", m, nullptr, c);
}

extern "C" int rg_ope_replay_mlr_eg(const rg_ope_mlr* m, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                                    uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                                    double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                                    void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = om_model_ok(m, "rg_ope_replay_mlr_eg")) return rc;
    if (int rc = ope_eg_ok("rg_ope_replay_mlr_eg", eg, m->num_products)) return rc;
    // (the wrapper that explores has no step-loop form round this agent and nothing holds its replay to a host loop: refused)
    if (eg->epsilon != 0.0) return fail(RG_EINVAL, "rg_ope_replay_mlr_eg: epsilon %g: only the wrapper that never explores (epsilon = 0) is served", eg->epsilon);
    const OpeEg ega{*eg, d_greedy, d_h0};
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    return om_replay<true>("rg_ope_replay_mlr_eg", m, &ega, c);
}
