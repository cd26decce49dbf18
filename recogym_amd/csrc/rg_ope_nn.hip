// rg_ope_nn.hip — off-policy evaluation replay of NnIpsAgent's argmax form (NnIpsFrozenAgent, reference agents/nn_ips.py:111-137 with
// with_ps_all = True and select_randomly off) over a sorted device log: pi = [act(the user's views so far) == a], / ps, for every
// bandit row.
//
// The walk is rg_ope_list.hpp's (history list, act on a changed history only, unresolved list, EG form: the poly unit's, with the
// act as a parameter); the act is rg_nn_common.hpp's nn_act on a PolyListHist, the one function the step loop's k_nn_acts runs
// (the stated order, nn_exp, the margin W, RG_NN_UNRESOLVED — a count above 2^24 is unresolved by nn_act itself: DESIGN.md 4i).
// The act's propensity is not used: pi is one-hot.
//
// The margin's A2, A3 are the library's: the entry point downloads the net and computes them (nn_host_model, rg_sim_set_nn_ips's
// helper), so a replay call synchronises once more than the poly unit's — once for the model, once for the validation's verdict.
//
// Head words: error, acts, unresolved, overflow, rows_read.
//
// LDS per block of kOpeWaves = 4 waves.  Static, 28 KB: the four lists (16 KB) and nn_act's s_cnt / s_prod rows (12 KB).  Dynamic:
// 2 H doubles per wave of layer vectors (64 H bytes a block), and behind them the three matrices where both stay within
// kNnStageBytes = 48 KB — the step loop's rule for this kernel's wave count; otherwise nn_act reads them from global memory through
// the same generic pointers.  Static + dynamic passes 64 KiB from 36 KB of dynamic LDS on — a staged net above that, or any net
// from H = 577 — and the entry point then opts both instantiations in (set_max_lds).  The most is 28 + 64 = 92 KB at H = 1024.
//
// W, the wave cap: 2 048 = 256 CUs x 2 blocks of 4 waves.  A CU has 160 KB of LDS; a block of a staged net holds at most
// 28 + 48 = 76 KB, so two are resident whatever is staged (and for every net in global memory up to H = 832: 28 + 52 KB); the
// likelihood unit's 4 096 assumes 36 KB a block, which only the smallest nets meet here.  Beyond H = 832 one block per CU is
// resident and the grid runs in two rounds.  W is part of the bits of d_sums (rg_ope_common.hpp).
#include "rg_nn_common.hpp"
#include "rg_ope_list.hpp"

namespace {

constexpr uint32_t kOnMaxWaves = 2048;           // 256 CUs x 2 blocks x 4 waves
constexpr OlHead kOnHead{2, 3, 4};               // error, acts, unresolved, overflow, rows_read
constexpr size_t kOnStaticLds = sizeof(OlLds) + kOpeWaves * kPolyHist * (sizeof(double) + sizeof(uint32_t));
static_assert(kOnStaticLds == 28 * 1024, "the header's LDS budget");

// nn_act on the wave's list
struct OnAct {
    NnModel m;
    uint32_t P;
    int lane;
    double* s_cnt; uint32_t* s_prod; double* s_h1;
    const double* w1t; const double* w2t; const double* w3t;
    __device__ __forceinline__ uint32_t operator()(const PolyListHist& h, uint32_t* fl) const {
        double ps;
        return nn_act(m, P, h, lane, s_cnt, s_prod, s_h1, s_h1 + m.H, w1t, w2t, w3t, fl, &ps, nullptr);
    }
    __device__ __forceinline__ void count(uint32_t) {}
    __device__ __forceinline__ void report(ol_u64*) const {}
};

template <bool EG, typename... Eg>       // EG: pi is the EpsilonGreedy wrapper's round this act (rg_ope_replay_nn_eg)
__global__ __launch_bounds__(64 * kOpeWaves, 2) void k_ope_nn(
    NnModel m, uint32_t P, const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users, uint32_t ps_mode,
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
    const NnLds l = nn_lds<kOpeWaves>(m, P, smem_raw);
    const OpeLog log{rows, offsets, n_users, ps_mode, ps64, ps_const, ratio, click, slots, n_waves};
    OnAct act{m, P, static_cast<int>(lane), s_cnt[wib], s_prod[wib], l.rows + static_cast<size_t>(2 * wib) * m.H, l.w1t, l.w2t, l.w3t};
    ol_replay(act, RG_NN_UNRESOLVED, kOnHead, P, log, s_l.p[wib], s_l.c[wib], gscr, g_cap, ws, ulist, wave, lane, ega...);
}

int on_model_ok(const rg_ope_nn* m, const char* who) {
    if (!m) return fail(RG_EINVAL, "%s: null model", who);
    if (m->num_products == 0 || m->num_products > kNnProducts)
        return fail(RG_EINVAL, "%s: num_products %u outside 1 .. %u", who, m->num_products, kNnProducts);
    if (m->num_hidden == 0 || m->num_hidden > kNnHidden) return fail(RG_EINVAL, "%s: num_hidden %u outside 1 .. %u", who, m->num_hidden, kNnHidden);
    if (!m->w1t || !m->b1 || !m->w2t || !m->b2 || !m->w3t || !m->b3) return fail(RG_EINVAL, "%s: null w1t / b1 / w2t / b2 / w3t / b3", who);
    return RG_OK;
}

}  // namespace

extern "C" size_t rg_ope_nn_workspace_bytes(const rg_ope_nn* m, uint64_t n_users, uint32_t max_user_rows) {
    if (!m) { fail(RG_EINVAL, "rg_ope_nn_workspace_bytes: null model"); return 0; }
    return ol_workspace_bytes(ope_waves(n_users, kOnMaxWaves), max_user_rows);
}

namespace {

template <bool EG>       // ega: null iff !EG
int on_replay(const char* who, const rg_ope_nn* m, const OpeEg* ega, const OpeCall& c) {
    if (int rc = ope_args_ok(who, c, rg_ope_nn_workspace_bytes(m, c.n_users, c.max_user_rows))) return rc;
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    NnModel nm;
    size_t smem = 0;
    char prefix[64];
    snprintf(prefix, sizeof(prefix), "%s: ", who);
    if (int rc = nn_host_model(prefix, m->num_products, m->num_hidden, m->w1t, m->b1, m->w2t, m->b2, m->w3t, m->b3, kOpeWaves, &nm, &smem)) return rc;
    if (smem + kOnStaticLds > 64 * 1024) {
        set_max_lds(k_ope_nn<false>, smem);
        set_max_lds(k_ope_nn<true, OpeEg>, smem);
    }
    const uint32_t W = ope_waves(c.n_users, kOnMaxWaves);
    const uint32_t g_cap = ol_global_cap(c.max_user_rows);
    ol_u64* ws = c.at<ol_u64>(0);
    uint32_t* ulist = c.at<uint32_t>(ol_head_bytes());
    double* slots = c.at<double>(ol_head_bytes() + ol_list_bytes());
    uint32_t* gscr = g_cap ? c.at<uint32_t>(ol_head_bytes() + ol_list_bytes() + ope_slot_bytes(W)) : nullptr;
    if (int rc = ope_check_log(who, c, m->num_products, ws)) return rc;
    // one spelling of the launch: the kernel, and the EG form's one more argument
    auto launch = [&](auto kernel, auto... eg) {
        hipLaunchKernelGGL(kernel, dim3(W / kOpeWaves), dim3(64 * kOpeWaves), smem, c.stream, nm, m->num_products, c.d_rows, c.d_offsets,
                           c.n_users, c.ps_mode, c.d_ps, c.ps_const, c.d_ratio, c.d_click, slots, gscr, g_cap, ws, ulist, W, eg...);
    };
    if constexpr (EG) launch(k_ope_nn<true, OpeEg>, *ega);
    else launch(k_ope_nn<false>);
    HIP_TRY(hipGetLastError());
    return ope_reduce(slots, W, c.d_sums, c.stream);
}

}  // namespace

extern "C" int rg_ope_replay_nn(const rg_ope_nn* m, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                                uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                                uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = on_model_ok(m, "rg_ope_replay_nn")) return rc;
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    return on_replay<false>("rg_ope_replay_nn", m, nullptr, c);
}

extern "C" int rg_ope_replay_nn_eg(const rg_ope_nn* m, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                                   uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                                   double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                                   void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = on_model_ok(m, "rg_ope_replay_nn_eg")) return rc;
    if (int rc = ope_eg_ok("rg_ope_replay_nn_eg", eg, m->num_products)) return rc;
    const OpeEg ega{*eg, d_greedy, d_h0};
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    return on_replay<true>("rg_ope_replay_nn_eg", m, &ega, c);
}
