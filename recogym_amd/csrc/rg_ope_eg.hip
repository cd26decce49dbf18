// rg_ope_eg.hip — off-policy replay of an EpsilonGreedy target (agents/epsilon_greedy.py:30-71 with with_ps_all = True) over a
// sorted device log: rg_ope.hip's skeleton — one wave per user, users assigned statically (wave w takes users w, w + W, ...),
// rows in coalesced 64-row chunks, per-wave partial sums reduced by a second one-block pass in a fixed order (the same bits on
// every run) — with the wrapper's act per bandit lane:
//   g   = the inner policy's action: table[last organic product before the row], or the inner RandomAgent's bounded draw of
//         (inner seed, u, t)
//   flip from (eg seed, u, t), words 0 and 1 (the draw contract of recogym_rng.h)
//   pi  = act()['ps-a'][a] on that branch: explored eps * (pure_new && a == g ? 0.0 : prob_explore), greedy
//         (1.0 - eps) * pi_inner[a] (1 / P, or the table's one-hot) — one float64 multiply of the host's constants, as the reference
//   r   = pi / ps
// OrganicUserEventCounter and frozen-LogReg inner policies have no form here: their `h0` is the inner policy's SAMPLED action.
#include "rg_common.hpp"

namespace {

constexpr int kEgWaves = 4;                     // waves per block
constexpr uint32_t kEgMaxWaves = 5120;          // 256 CUs x 20 waves

uint32_t eg_waves(uint64_t n_users) {
    const uint64_t w = (n_users + kEgWaves - 1) / kEgWaves * kEgWaves;
    return static_cast<uint32_t>(w < kEgWaves ? kEgWaves : (w > kEgMaxWaves ? kEgMaxWaves : w));
}

size_t eg_slot_bytes(uint32_t n_waves) { return (static_cast<size_t>(n_waves) * 3 * sizeof(double) + 255) & ~size_t(255); }

__device__ __forceinline__ double eg_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

__global__ __launch_bounds__(64 * kEgWaves) void k_ope_eg_replay(
    rg_ope_policy inner, rg_ope_eg eg, const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users,
    uint32_t ps_mode, const double* __restrict__ ps64, double ps_const, double* __restrict__ ratio, uint8_t* __restrict__ click,
    uint8_t* __restrict__ greedy_out, int32_t* __restrict__ h0_out, double* __restrict__ slots, uint32_t n_waves) {
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kEgWaves + wib;
    const uint32_t P = inner.num_products;
    const bool lvt = inner.kind == RG_POLICY_LAST_VIEW_TABLE;
    const double eps = eg.epsilon;
    const double thr = eps / (eps + (1.0 - eps));
    const double pi_uniform = 1.0 / static_cast<double>(P);
    double acc_n = 0.0, acc_cr = 0.0, acc_r = 0.0;
    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        uint32_t lpv = 0;
        for (int64_t base = b; base < e; base += 64) {
            const int64_t row = base + lane;
            const bool live = row < e;
            uint4 x = make_uint4(0u, 0u, 0u, 0u);
            if (live) x = reinterpret_cast<const uint4*>(rows)[row];
            const bool isb = live && (x.z & RG_EV_BANDIT);
            const bool iso = live && !(x.z & RG_EV_BANDIT);
            const uint32_t idx = x.z & RG_EV_INDEX_MASK;
            uint32_t g = 0;
            double pi_inner;
            if (lvt) {
                // the last organic row before this one (in the chunk, else carried), as rg_ope.hip
                const uint64_t omask = __ballot(iso);
                const uint64_t before = omask & (lane ? (~0ull >> (64 - lane)) : 0ull);
                const int src = before ? 63 - __clzll(static_cast<long long>(before)) : 0;
                const uint32_t from = static_cast<uint32_t>(__shfl(static_cast<int>(idx), src));
                const uint32_t mine = before ? from : lpv;
                g = (isb && mine < P) ? static_cast<uint32_t>(inner.table[mine]) : 0u;
                pi_inner = g == idx ? 1.0 : 0.0;
                if (omask) lpv = static_cast<uint32_t>(__shfl(static_cast<int>(idx), 63 - __clzll(static_cast<long long>(omask))));
            } else {
                if (isb) {
                    const rg_u32x4 wi = rg_draw(inner.policy_seed, x.x, x.y, 0, RG_DRAW_POLICY);
                    g = rg_bounded(wi.w[0], wi.w[1], P);
                }
                pi_inner = pi_uniform;
            }
            if (isb) {
                const rg_u32x4 w = rg_draw(eg.seed, x.x, x.y, 0, RG_DRAW_POLICY);
                const bool explore = !(thr <= rg_uniform(w.w[0], w.w[1]));
                const double pi = explore ? eps * ((eg.pure_new && idx == g) ? 0.0 : eg.prob_explore) : (1.0 - eps) * pi_inner;
                const double ps = ps_mode == RG_OPE_PS_ARRAY ? ps64[row]
                                  : ps_mode == RG_OPE_PS_CONST ? ps_const : static_cast<double>(__uint_as_float(x.w));
                const double r = pi / ps;
                ratio[row] = r;
                if (click) click[row] = (x.z & RG_EV_CLICK) ? 1 : 0;
                if (greedy_out) greedy_out[row] = explore ? 0 : 1;
                if (h0_out) h0_out[row] = static_cast<int32_t>(g);
                acc_n += 1.0;
                acc_cr += ((x.z & RG_EV_CLICK) ? 1.0 : 0.0) * r;
                acc_r += r;
            }
        }
    }
    acc_n = eg_wave_sum(acc_n);
    acc_cr = eg_wave_sum(acc_cr);
    acc_r = eg_wave_sum(acc_r);
    if (lane == 0) {
        slots[3 * static_cast<size_t>(wave) + 0] = acc_n;
        slots[3 * static_cast<size_t>(wave) + 1] = acc_cr;
        slots[3 * static_cast<size_t>(wave) + 2] = acc_r;
    }
}

// the per-wave slots -> (n, sum c r, sum r), one block, fixed order (k_ope_reduce's arithmetic)
__global__ __launch_bounds__(256) void k_ope_eg_reduce(const double* __restrict__ slots, uint32_t n_waves, double* __restrict__ out) {
    __shared__ double sh[3][256];
    double a[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = threadIdx.x; i < n_waves; i += 256)
        for (int j = 0; j < 3; ++j) a[j] += slots[3 * static_cast<size_t>(i) + j];
    for (int j = 0; j < 3; ++j) sh[j][threadIdx.x] = a[j];
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s)
            for (int j = 0; j < 3; ++j) sh[j][threadIdx.x] += sh[j][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int j = 0; j < 3; ++j) out[j] = sh[j][0];
}

}  // namespace

extern "C" size_t rg_ope_eg_workspace_bytes(const rg_ope_policy* inner, uint64_t n_users, uint32_t max_user_rows) {
    (void)max_user_rows;
    if (!inner) { fail(RG_EINVAL, "rg_ope_eg_workspace_bytes: null policy"); return 0; }
    return eg_slot_bytes(eg_waves(n_users));
}

extern "C" int rg_ope_replay_eg(const rg_ope_policy* inner, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                                uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                                double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                                void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!inner || !eg) return fail(RG_EINVAL, "rg_ope_replay_eg: null policy");
    if (inner->kind != RG_POLICY_RANDOM_AGENT && inner->kind != RG_POLICY_LAST_VIEW_TABLE)
        return fail(RG_EINVAL, "rg_ope_replay_eg: inner policy kind %u has no replay form under EpsilonGreedy", inner->kind);
    if (inner->num_products == 0 || inner->num_products > RG_EV_INDEX_MASK) return fail(RG_EINVAL, "rg_ope_replay_eg: bad num_products");
    if (inner->kind == RG_POLICY_LAST_VIEW_TABLE && !inner->table) return fail(RG_EINVAL, "rg_ope_replay_eg: null table");
    if (!(eg->epsilon >= 0.0 && eg->epsilon <= 1.0)) return fail(RG_EINVAL, "rg_ope_replay_eg: epsilon %g outside [0, 1]", eg->epsilon);
    if (eg->pure_new && inner->num_products < 2u) return fail(RG_EINVAL, "rg_ope_replay_eg: epsilon_pure_new needs at least 2 products");
    if (ps_mode > RG_OPE_PS_ROW || (ps_mode == RG_OPE_PS_ARRAY && !d_ps && n_users))
        return fail(RG_EINVAL, "rg_ope_replay_eg: bad ps source");
    if (n_users && (!d_rows || !d_offsets || !d_ratio)) return fail(RG_EINVAL, "rg_ope_replay_eg: null rows / offsets / ratio");
    if (!d_sums || !d_workspace) return fail(RG_EINVAL, "rg_ope_replay_eg: null sums / workspace");
    const size_t need = rg_ope_eg_workspace_bytes(inner, n_users, max_user_rows);
    if (workspace_bytes < need) return fail(RG_ENOMEM, "rg_ope_replay_eg: workspace %zu < %zu bytes", workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(d_rows) % 16) return fail(RG_EINVAL, "rg_ope_replay_eg: rows not 16-byte aligned");
    const uint32_t W = eg_waves(n_users);
    double* slots = static_cast<double*>(d_workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_ope_eg_replay, dim3(W / kEgWaves), dim3(64 * kEgWaves), 0, s, *inner, *eg, d_rows, d_offsets, n_users, ps_mode,
                       d_ps, ps_const, d_ratio, d_click, d_greedy, d_h0, slots, W);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ope_eg_reduce, dim3(1), dim3(256), 0, s, slots, W, d_sums);
    HIP_TRY(hipGetLastError());
    return RG_OK;
}
