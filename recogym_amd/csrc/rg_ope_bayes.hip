// rg_ope_bayes.hip — off-policy evaluation replay of BayesianAgentVB (BayesianVBFrozenAgent, reference agents/bayesian_poly_vb.py:71-91
// with with_ps_all = True) over a sorted device log: pi = [act(the user's views so far) == a], / ps, for every bandit row.
//
// The walk is rg_ope_list.hpp's (history list, act on a changed history only, unresolved list, EG form: the poly unit's, with the
// act as a parameter); the act is rg_bayes_common.hpp's bayes_act on a PolyListHist, the one function the step loop's k_bayes_acts
// runs (the stated order, the margin W, the saturated zone, RG_BAYES_SATURATED | RG_BAYES_UNRESOLVED: DESIGN.md 4h).  The model is
// read from global memory as there: lam_t's sample axis is contiguous, 512 bytes per (viewed product, action) and wave.
//
// Head words: error, acts, saturated, unresolved, overflow, rows_read.  Synchronises the stream once (the validation's verdict).
//
// LDS per block of kOpeWaves = 4 waves, all static, 28 KB: the four lists (16 KB) and bayes_act's s_cnt / s_prod rows (12 KB).
//
// W, the wave cap: 3 072 = 256 CUs x 3 blocks of 4 waves.  The LDS would leave five blocks a CU (5 x 28 KB of 160 KB); the registers
// leave three: bayes_act keeps four actions' decisions, sums and minima in flight, and round it the walk's state — bounded to 4
// waves per SIMD (128 registers) the compiler spills 26 / 36 of them to scratch, at 3 waves per SIMD it needs 157 / 166 and none.
// Three blocks of four waves are those 3 waves on each of the CU's four SIMDs.  W is part of the bits of d_sums (rg_ope_common.hpp).
#include "rg_bayes_common.hpp"
#include "rg_ope_list.hpp"

namespace {

constexpr uint32_t kObMaxWaves = 3072;           // 256 CUs x 3 blocks x 4 waves
constexpr int kObWsSaturated = 2;
constexpr OlHead kObHead{3, 4, 5};               // error, acts, saturated, unresolved, overflow, rows_read

// bayes_act on the wave's list
struct ObAct {
    BayesModel m;
    int lane;
    double* s_cnt; uint32_t* s_prod;
    ol_u64 c_sat;
    __device__ __forceinline__ uint32_t operator()(const PolyListHist& h, uint32_t* fl) const {
        return bayes_act(m, h, lane, s_cnt, s_prod, fl, nullptr);
    }
    __device__ __forceinline__ void count(uint32_t fl) { c_sat += fl & RG_BAYES_SATURATED; }
    __device__ __forceinline__ void report(ol_u64* ws) const {
        if (c_sat) (void)__hip_atomic_fetch_add(&ws[kObWsSaturated], c_sat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
static_assert(RG_BAYES_SATURATED == 1u, "ObAct::count adds the bit itself");

template <bool EG, typename... Eg>       // EG: pi is the EpsilonGreedy wrapper's round this act (rg_ope_replay_bayes_eg)
__global__ __launch_bounds__(64 * kOpeWaves, 3) void k_ope_bayes(
    BayesModel m, const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users, uint32_t ps_mode,
    const double* __restrict__ ps64, double ps_const, double* __restrict__ ratio, uint8_t* __restrict__ click,
    double* __restrict__ slots, uint32_t* __restrict__ gscr, uint32_t g_cap, ol_u64* __restrict__ ws, uint32_t* __restrict__ ulist,
    uint32_t n_waves, Eg... ega) {
    static_assert(sizeof...(Eg) == (EG ? 1 : 0), "the EG instantiation takes an OpeEg, the plain one nothing");
    __shared__ double s_cnt[kOpeWaves][kPolyHist];
    __shared__ uint32_t s_prod[kOpeWaves][kPolyHist];
    __shared__ OlLds s_l;
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kOpeWaves + wib;
    const OpeLog log{rows, offsets, n_users, ps_mode, ps64, ps_const, ratio, click, slots, n_waves};
    ObAct act{m, static_cast<int>(lane), s_cnt[wib], s_prod[wib], 0ull};
    ol_replay(act, RG_BAYES_UNRESOLVED, kObHead, m.P, log, s_l.p[wib], s_l.c[wib], gscr, g_cap, ws, ulist, wave, lane, ega...);
}

int ob_model_ok(const rg_ope_bayes* m, const char* who) {
    if (!m) return fail(RG_EINVAL, "%s: null model", who);
    if (m->num_products == 0 || m->num_products > RG_EV_INDEX_MASK) return fail(RG_EINVAL, "%s: bad num_products %u", who, m->num_products);
    if (m->num_samples == 0) return fail(RG_EINVAL, "%s: num_samples is 0", who);
    const uint64_t P = m->num_products;
    if (P * P > kBayesModelBytes / sizeof(double) || P * P * m->num_samples > kBayesModelBytes / sizeof(double))
        return fail(RG_EINVAL, "%s: the model (%u x %u x %u doubles) exceeds %llu bytes", who, m->num_products, m->num_products, m->num_samples,
                    (unsigned long long)kBayesModelBytes);
    if (!m->lam_t) return fail(RG_EINVAL, "%s: null lam_t", who);
    return RG_OK;
}

}  // namespace

extern "C" size_t rg_ope_bayes_workspace_bytes(const rg_ope_bayes* m, uint64_t n_users, uint32_t max_user_rows) {
    if (!m) { fail(RG_EINVAL, "rg_ope_bayes_workspace_bytes: null model"); return 0; }
    return ol_workspace_bytes(ope_waves(n_users, kObMaxWaves), max_user_rows);
}

namespace {

template <bool EG>       // ega: null iff !EG
int ob_replay(const char* who, const rg_ope_bayes* m, const OpeEg* ega, const OpeCall& c) {
    if (int rc = ope_args_ok(who, c, rg_ope_bayes_workspace_bytes(m, c.n_users, c.max_user_rows))) return rc;
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    const uint32_t W = ope_waves(c.n_users, kObMaxWaves);
    const uint32_t g_cap = ol_global_cap(c.max_user_rows);
    ol_u64* ws = c.at<ol_u64>(0);
    uint32_t* ulist = c.at<uint32_t>(ol_head_bytes());
    double* slots = c.at<double>(ol_head_bytes() + ol_list_bytes());
    uint32_t* gscr = g_cap ? c.at<uint32_t>(ol_head_bytes() + ol_list_bytes() + ope_slot_bytes(W)) : nullptr;
    if (int rc = ope_check_log(who, c, m->num_products, ws)) return rc;
    const BayesModel bm{m->num_products, m->num_samples, m->lam_t};
    // one spelling of the launch: the kernel, and the EG form's one more argument
    auto launch = [&](auto kernel, auto... eg) {
        hipLaunchKernelGGL(kernel, dim3(W / kOpeWaves), dim3(64 * kOpeWaves), 0, c.stream, bm, c.d_rows, c.d_offsets, c.n_users, c.ps_mode,
                           c.d_ps, c.ps_const, c.d_ratio, c.d_click, slots, gscr, g_cap, ws, ulist, W, eg...);
    };
    if constexpr (EG) launch(k_ope_bayes<true, OpeEg>, *ega);
    else launch(k_ope_bayes<false>);
    HIP_TRY(hipGetLastError());
    return ope_reduce(slots, W, c.d_sums, c.stream);
}

}  // namespace

extern "C" int rg_ope_replay_bayes(const rg_ope_bayes* m, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                                   uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                                   uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = ob_model_ok(m, "rg_ope_replay_bayes")) return rc;
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    return ob_replay<false>("rg_ope_replay_bayes", m, nullptr, c);
}

extern "C" int rg_ope_replay_bayes_eg(const rg_ope_bayes* m, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                                      uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                                      double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                                      void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = ob_model_ok(m, "rg_ope_replay_bayes_eg")) return rc;
    if (int rc = ope_eg_ok("rg_ope_replay_bayes_eg", eg, m->num_products)) return rc;
    const OpeEg ega{*eg, d_greedy, d_h0};
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    return ob_replay<true>("rg_ope_replay_bayes_eg", m, &ega, c);
}
