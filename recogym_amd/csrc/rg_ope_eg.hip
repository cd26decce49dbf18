// rg_ope_eg.hip — off-policy replay of an EpsilonGreedy target (agents/epsilon_greedy.py:30-71 with with_ps_all = True) over a
// sorted device log: the replay skeleton of rg_ope_common.hpp with the wrapper's act per bandit lane:
//   g   = the inner policy's action: table[last organic product before the row], or the inner RandomAgent's bounded draw of
//         (inner seed, u, t)
//   flip from (eg seed, u, t), words 0 and 1 (the draw contract of recogym_rng.h)
//   pi  = act()['ps-a'][a] on that branch: explored eps * (pure_new && a == g ? 0.0 : prob_explore), greedy
//         (1.0 - eps) * pi_inner[a] (1 / P, or the table's one-hot) — one float64 multiply of the host's constants, as the reference
//   r   = pi / ps
// OrganicUserEventCounter and a sampling frozen LogReg have no replay form: their `h0` is the inner policy's SAMPLED action.  The
// LogReg argmax and the likelihood agent inside are their own units' EG instantiations (rg_ope_replay_logreg_eg, rg_ope_replay_poly_eg).
#include "rg_ope_common.hpp"

namespace {

constexpr uint32_t kEgMaxWaves = 5120;          // 256 CUs x 20 waves

__global__ __launch_bounds__(64 * kOpeWaves) void k_ope_eg_replay(
    rg_ope_policy inner, rg_ope_eg eg, const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users,
    uint32_t ps_mode, const double* __restrict__ ps64, double ps_const, double* __restrict__ ratio, uint8_t* __restrict__ click,
    uint8_t* __restrict__ greedy_out, int32_t* __restrict__ h0_out, double* __restrict__ slots, uint32_t n_waves) {
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kOpeWaves + wib;
    const OpeLog log{rows, offsets, n_users, ps_mode, ps64, ps_const, ratio, click, slots, n_waves};
    const uint32_t P = inner.num_products;
    const bool lvt = inner.kind == RG_POLICY_LAST_VIEW_TABLE;
    const double eps = eg.epsilon;
    const double thr = eg_threshold(eps);
    const double pi_uniform = 1.0 / static_cast<double>(P);
    OpeAcc acc;
    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        uint32_t lpv = 0;
        for (int64_t base = b; base < e; base += 64) {
            const OpeRow r = ope_load(log, base, e, lane);
            uint32_t g = 0;
            double pi_inner;
            if (lvt) {
                const uint32_t mine = ope_last_view(r, lane, lpv);
                g = (r.isb && mine < P) ? static_cast<uint32_t>(inner.table[mine]) : 0u;
                pi_inner = g == r.idx ? 1.0 : 0.0;
            } else {
                if (r.isb) {
                    const rg_u32x4 wi = rg_draw(inner.policy_seed, r.x.x, r.x.y, 0, RG_DRAW_POLICY);
                    g = rg_bounded(wi.w[0], wi.w[1], P);
                }
                pi_inner = pi_uniform;
            }
            if (r.isb) {
                const bool explore = eg_explored(eg.seed, thr, r.x.x, r.x.y);
                const double pi = explore ? eps * ((eg.pure_new && r.idx == g) ? 0.0 : eg.prob_explore) : (1.0 - eps) * pi_inner;
                acc.emit(log, r, pi);
                if (greedy_out) greedy_out[r.row] = explore ? 0 : 1;
                if (h0_out) h0_out[r.row] = static_cast<int32_t>(g);
            }
        }
    }
    acc.store(log, wave, lane);
}

}  // namespace

extern "C" size_t rg_ope_eg_workspace_bytes(const rg_ope_policy* inner, uint64_t n_users, uint32_t max_user_rows) {
    (void)max_user_rows;
    if (!inner) { fail(RG_EINVAL, "rg_ope_eg_workspace_bytes: null policy"); return 0; }
    return ope_slot_bytes(ope_waves(n_users, kEgMaxWaves));
}

extern "C" int rg_ope_replay_eg(const rg_ope_policy* inner, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                                uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                                double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                                void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!inner) return fail(RG_EINVAL, "rg_ope_replay_eg: null policy");
    if (inner->kind != RG_POLICY_RANDOM_AGENT && inner->kind != RG_POLICY_LAST_VIEW_TABLE)
        return fail(RG_EINVAL, "rg_ope_replay_eg: inner policy kind %u has no replay form under EpsilonGreedy", inner->kind);
    if (inner->num_products == 0 || inner->num_products > RG_EV_INDEX_MASK) return fail(RG_EINVAL, "rg_ope_replay_eg: bad num_products");
    if (inner->kind == RG_POLICY_LAST_VIEW_TABLE && !inner->table) return fail(RG_EINVAL, "rg_ope_replay_eg: null table");
    if (int rc = ope_eg_ok("rg_ope_replay_eg", eg, inner->num_products)) return rc;
    const OpeCall c{d_rows, d_offsets, n_users, max_user_rows, ps_mode, d_ps, ps_const, d_ratio, d_click, d_sums, d_workspace, workspace_bytes,
                    static_cast<hipStream_t>(stream)};
    if (int rc = ope_args_ok("rg_ope_replay_eg", c, rg_ope_eg_workspace_bytes(inner, n_users, max_user_rows))) return rc;
    const uint32_t W = ope_waves(n_users, kEgMaxWaves);
    double* slots = c.at<double>(0);
    hipLaunchKernelGGL(k_ope_eg_replay, dim3(W / kOpeWaves), dim3(64 * kOpeWaves), 0, c.stream, *inner, *eg, c.d_rows, c.d_offsets, c.n_users,
                       c.ps_mode, c.d_ps, c.ps_const, c.d_ratio, c.d_click, d_greedy, d_h0, slots, W);
    HIP_TRY(hipGetLastError());
    return ope_reduce(slots, W, c.d_sums, c.stream);
}
