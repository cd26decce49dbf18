// rg_organic_mf.hip — OrganicMFSquare's training from a sorted device log (reference agents/organic_mf.py:80-116 under the
// offline protocol of bench_agents.py:168-190).
//
// rg_omf_pairs: the log -> the training pairs (view i directly followed by view j inside a session), grouped by optimiser step.
// A CALL is an organic-only user (its call bit sits on its last row) or a bandit row of any other user; call number
// k = first_call + 1 + (calls in front of it); k % mini_batch == 0 is a TRIGGER: its own session is dropped, the sessions stored
// since the previous trigger make one step.  Log order is step order, so nothing is sorted: a wave per user writes the call bit
// and the pair bit of every row, one exclusive scan of the call bits numbers the calls, a second one of the kept pair bits
// compacts the list, and the CSR row of a step is a lower bound in the (ascending) step numbers of the kept pairs.  Integer
// work only: the same bytes on every run.
//
// rg_omf_steps: the chain of RMSprop steps of such a list in ONE launch of ONE workgroup (the steps depend on each other, and
// __syncthreads is the only barrier there is).  Per step: count the pairs per input product, list the distinct inputs in
// ascending order, and for one input i after the other: N[i][.] by integer LDS adds, the logits W emb[i] + b, a max-shifted
// softmax with the table exp of rg_exp64.hpp, G = n_i softmax - N[i][.], then g_b += G, g_w += G^T emb[i] (every thread owns its
// cells: inputs are added in ascending order) and g_emb[i] = G W (a wave per column, a fixed shuffle tree).  Then the dense
// RMSprop update of all 2 P E + P parameters.  float64 throughout, no floating-point atomics: two runs give the same bits.
// Two instantiations of one body: the model, its square averages and the gradients in LDS (256 threads) while
// omf_lds_bytes(P, E, true) fits 64 KiB — P <= 228 at E = 5 — else in global memory, L2-resident (1024 threads, the caller's
// arrays in place, the gradients in the workspace), up to P = 2048 and E = 64.
#include "rg_common.hpp"
#include "rg_omf_common.hpp"
#include "rg_scan_common.hpp"

namespace {

using namespace rgomf;

typedef unsigned long long omf_u64;

constexpr int kOmfOutWords = 8;

// ---------------------------------------------------------------------------------------------------------------------------
// rg_omf_pairs
// ---------------------------------------------------------------------------------------------------------------------------
// workspace: call[n + 1] | keep[n + 1] | step[n_pending + n] | sums[blocks of n + 1] (uint32 each) | pair[n] (uint8)
struct OmfPairsWs {
    uint32_t *call, *keep, *step, *sums;
    uint8_t* pair;
    size_t bytes;
};

OmfPairsWs omf_pairs_carve(void* base, uint64_t n, uint64_t n_pending) {
    OmfPairsWs w;
    static uint32_t none[1];                                      // (base = null: only the size is asked for)
    uint32_t* p = base ? static_cast<uint32_t*>(base) : none;
    const uint64_t nb = (n + 1 + kOmfScanBlock - 1) / kOmfScanBlock;
    w.call = p; p += n + 1;
    w.keep = p; p += n + 1;
    w.step = p; p += n_pending + n;
    w.sums = p; p += nb;
    w.pair = reinterpret_cast<uint8_t*>(p);
    w.bytes = 4 * (2 * (n + 1) + n_pending + n + nb) + n;
    w.bytes = (w.bytes + 255) / 256 * 256;
    return w;
}

// a wave per user: the call bit and the pair bit of every row, and the validation
__global__ __launch_bounds__(256) void k_omf_flags(const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users,
                                                   uint64_t n_organic, uint64_t n_rows, uint32_t P, uint32_t* __restrict__ call,
                                                   uint8_t* __restrict__ pair, int64_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = blockIdx.x * 4ull + (threadIdx.x >> 6), n_waves = gridDim.x * 4ull;
    omf_u64 err = 0;
    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        if (b < 0 || e < b || static_cast<uint64_t>(e) > n_rows) { err |= kOmfErrOffsets; continue; }
        const bool organic_only = user < n_organic;
        if (b == e) {
            if (organic_only) err |= kOmfErrEmptyOrganic;      // (its call would have no row to sit on)
            continue;
        }
        if (rows[b].code & RG_EV_BANDIT) err |= kOmfErrFirstBandit;
        int64_t last_b = -1;                                    // the user's last bandit row: the views behind it belong to no call
        if (!organic_only) {
            for (int64_t base = b; base < e; base += 64) {
                const int64_t row = base + lane;
                const omf_u64 m = __ballot(row < e && (rows[row].code & RG_EV_BANDIT));
                if (m) last_b = base + top_bit(m);
            }
        }
        for (int64_t base = b; base < e; base += 64) {
            const int64_t row = base + lane;
            if (row >= e) continue;
            const uint32_t code = rows[row].code;
            if ((code & RG_EV_INDEX_MASK) >= P) err |= kOmfErrProduct;
            const bool isb = (code & RG_EV_BANDIT) != 0;
            if (isb && organic_only) err |= kOmfErrOrganicBandit;
            const uint32_t next = row + 1 < e ? rows[row + 1].code : RG_EV_BANDIT;
            pair[row] = (!isb && !(next & RG_EV_BANDIT) && (organic_only || row < last_b)) ? 1 : 0;
            call[row] = organic_only ? (row == e - 1 ? 1u : 0u) : (isb ? 1u : 0u);
        }
    }
    if (err) (void)__hip_atomic_fetch_or(reinterpret_cast<omf_u64*>(out), err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// call[r] (scanned: the number of the call that closes row r's session) -> the step of the pair at r; keep[r] = the pair counts
__global__ __launch_bounds__(256) void k_omf_keep(uint32_t* __restrict__ call, const uint8_t* __restrict__ pair, uint32_t* __restrict__ keep,
                                                  uint64_t n_rows, uint64_t first_call, uint32_t mb) {
    for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r <= n_rows; r += gridDim.x * 256ull) {
        if (r == n_rows) { keep[r] = 0; continue; }             // (call[n_rows] = the number of calls: left as it is)
        const uint64_t k = first_call + 1 + call[r];
        const bool kept = pair[r] && (k % mb != 0);
        keep[r] = kept ? 1u : 0u;
        call[r] = static_cast<uint32_t>(k / mb - first_call / mb);
    }
}

__global__ __launch_bounds__(256) void k_omf_scatter(const rg_event* __restrict__ rows, const uint32_t* __restrict__ stepno,
                                                     const uint32_t* __restrict__ keep, uint64_t n_rows, const int32_t* __restrict__ pending,
                                                     uint64_t n_pending, int32_t* __restrict__ pairs, uint32_t* __restrict__ step) {
    for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r < n_rows + n_pending; r += gridDim.x * 256ull) {
        if (r < n_pending) {                                    // the pairs carried in belong to the first step
            pairs[2 * r] = pending[2 * r];
            pairs[2 * r + 1] = pending[2 * r + 1];
            step[r] = 0;
            continue;
        }
        const uint64_t row = r - n_pending;
        if (keep[row + 1] == keep[row]) continue;
        const uint64_t q = n_pending + keep[row];
        pairs[2 * q] = static_cast<int32_t>(rows[row].code & RG_EV_INDEX_MASK);
        pairs[2 * q + 1] = static_cast<int32_t>(rows[row + 1].code & RG_EV_INDEX_MASK);
        step[q] = stepno[row];
    }
}

// step_offsets[s] = the first pair whose step is >= s, s = 0 .. n_steps; step_offsets[n_steps + 1] = all pairs (the row behind
// the last trigger: the new pending set)
__global__ __launch_bounds__(256) void k_omf_offsets(const uint32_t* __restrict__ call, const uint32_t* __restrict__ keep,
                                                     const uint32_t* __restrict__ step, uint64_t n_rows, uint64_t n_pending, uint64_t first_call,
                                                     uint32_t mb, int64_t* __restrict__ step_offsets, uint64_t step_capacity,
                                                     int64_t* __restrict__ out) {
    const uint64_t n_calls = call[n_rows], n_pairs = n_pending + keep[n_rows];
    const uint64_t n_steps = (first_call + n_calls) / mb - first_call / mb;
    if (n_steps + 2 > step_capacity) {
        if (blockIdx.x == 0 && threadIdx.x == 0) out[0] |= static_cast<int64_t>(kOmfErrCapacity);
        return;
    }
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s < n_steps + 2; s += gridDim.x * 256ull) {
        uint64_t lo = 0, hi = n_pairs;
        if (s > n_steps) lo = n_pairs;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (step[mid] < s) lo = mid + 1; else hi = mid;
        }
        step_offsets[s] = static_cast<int64_t>(lo);
        if (s == n_steps) {
            out[1] = static_cast<int64_t>(n_calls);
            out[2] = static_cast<int64_t>(n_steps);
            out[3] = static_cast<int64_t>(n_pairs);
            out[4] = static_cast<int64_t>(n_pairs - lo);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// rg_omf_steps
// ---------------------------------------------------------------------------------------------------------------------------
// every thread gets the block's value; red: one double per wave.  The tree and the order of the waves are fixed.
template <bool kMax>
__device__ __forceinline__ double omf_block_reduce(double v, double* red) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double x = __shfl_xor(v, o);
        v = kMax ? fmax(v, x) : v + x;
    }
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double r = red[0];
    for (uint32_t w = 1; w < nw; ++w) r = kMax ? fmax(r, red[w]) : r + red[w];
    __syncthreads();
    return r;
}

template <bool kLds, int kThreads>
__global__ __launch_bounds__(kThreads) void k_omf_steps(rg_omf_model m, double* __restrict__ g_grad, double lr, double alpha, double eps,
                                                        const int32_t* __restrict__ pairs, uint64_t n_pairs,
                                                        const int64_t* __restrict__ step_offsets, uint64_t n_steps, int64_t* __restrict__ out) {
    extern __shared__ double s_omf[];
    const uint32_t P = m.num_products, E = m.embed_dim, PE = P * E, NP = 2 * PE + P;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr uint32_t kWaves = kThreads / 64;
    // the layout omf_lds_bytes counts
    double* zrow = s_omf;
    double* red = zrow + P;
    double* lds_state = red + 32;
    uint32_t* tab = reinterpret_cast<uint32_t*>(lds_state + (kLds ? 3 * static_cast<size_t>(NP) : 0));
    int* nrow = reinterpret_cast<int*>(tab + 64);
    int* cnt = nrow + P;
    int* list = cnt + P;
    int* flag = list + P;
    double *pe, *pw, *pb, *qe, *qw, *qb, *ge, *gw, *gb;
    if constexpr (kLds) {
        pe = lds_state; pw = pe + PE; pb = pw + PE;
        qe = pb + P; qw = qe + PE; qb = qw + PE;
        ge = qb + P; gw = ge + PE; gb = gw + PE;
    } else {
        pe = m.emb; pw = m.w; pb = m.bias;
        qe = m.sq_emb; qw = m.sq_w; qb = m.sq_bias;
        ge = g_grad; gw = ge + PE; gb = gw + PE;
    }

    // the whole list is validated before anything is touched
    if (tid < 4) flag[tid] = 0;
    __syncthreads();
    {
        bool bad_pair = false, bad_off = false;
        for (uint64_t q = tid; q < n_pairs; q += kThreads)
            if (static_cast<uint32_t>(pairs[2 * q]) >= P || static_cast<uint32_t>(pairs[2 * q + 1]) >= P) bad_pair = true;
        for (uint64_t s = tid; s < n_steps; s += kThreads) {
            const int64_t lo = step_offsets[s], hi = step_offsets[s + 1];
            if (lo < 0 || hi < lo || static_cast<uint64_t>(hi) > n_pairs) bad_off = true;
        }
        if (bad_pair) flag[0] = 1;
        if (bad_off) flag[1] = 1;
    }
    __syncthreads();
    if (flag[0] || flag[1]) {
        if (tid == 0) {
            out[0] = static_cast<int64_t>((flag[0] ? kOmfErrProduct : 0ull) | (flag[1] ? kOmfErrOffsets : 0ull));
            out[1] = out[2] = out[3] = 0;
        }
        return;
    }

    if (tid < 32) exp64t_entry(kExp2Tab32[tid], tid, tab);
    for (uint32_t a = tid; a < P; a += kThreads) { nrow[a] = 0; cnt[a] = 0; }
    if constexpr (kLds) {
        for (uint32_t i = tid; i < PE; i += kThreads) { pe[i] = m.emb[i]; pw[i] = m.w[i]; qe[i] = m.sq_emb[i]; qw[i] = m.sq_w[i]; }
        for (uint32_t i = tid; i < P; i += kThreads) { pb[i] = m.bias[i]; qb[i] = m.sq_bias[i]; }
    }
    for (uint32_t i = tid; i < NP; i += kThreads) ge[i] = 0.0;      // (ge, gw, gb are one array)
    __syncthreads();

    uint64_t n_taken = 0, n_empty = 0, n_used = 0;
    for (uint64_t s = 0; s < n_steps; ++s) {
        const uint64_t lo = static_cast<uint64_t>(step_offsets[s]), hi = static_cast<uint64_t>(step_offsets[s + 1]);
        if (lo == hi) { ++n_empty; continue; }
        // the pairs per input product, then the distinct inputs in ascending order (wave 0: ballots keep the order)
        for (uint64_t q = lo + tid; q < hi; q += kThreads) (void)atomicAdd(&cnt[pairs[2 * q]], 1);
        __syncthreads();
        if (wave == 0) {
            uint32_t n = 0;
            for (uint32_t base = 0; base < P; base += 64) {
                const uint32_t a = base + lane;
                const bool has = a < P && cnt[a] > 0;
                const omf_u64 mask = __ballot(has);
                if (has) list[n + __popcll(mask & lanes_below(lane))] = static_cast<int>(a);
                n += static_cast<uint32_t>(__popcll(mask));
            }
            if (lane == 0) flag[2] = static_cast<int>(n);
        }
        __syncthreads();
        const uint32_t nd = static_cast<uint32_t>(flag[2]);
        for (uint32_t d = 0; d < nd; ++d) {
            const uint32_t i = static_cast<uint32_t>(list[d]);
            const double ni = static_cast<double>(cnt[i]);
            for (uint64_t q = lo + tid; q < hi; q += kThreads)
                if (static_cast<uint32_t>(pairs[2 * q]) == i) (void)atomicAdd(&nrow[pairs[2 * q + 1]], 1);
            double lmax = -1.0e300;
            for (uint32_t a = tid; a < P; a += kThreads) {
                double z = pb[a];
                for (uint32_t e = 0; e < E; ++e) z = fma(pw[a * E + e], pe[i * E + e], z);
                zrow[a] = z;
                lmax = fmax(lmax, z);
            }
            const double mx = omf_block_reduce<true>(lmax, red);
            double lsum = 0.0;
            for (uint32_t a = tid; a < P; a += kThreads) {
                const double x = exp64t(zrow[a] - mx, tab);
                zrow[a] = x;
                lsum += x;
            }
            const double scale = ni / omf_block_reduce<false>(lsum, red);
            for (uint32_t a = tid; a < P; a += kThreads) {
                const double g = scale * zrow[a] - static_cast<double>(nrow[a]);
                zrow[a] = g;
                nrow[a] = 0;
                gb[a] += g;
            }
            __syncthreads();
            for (uint32_t idx = tid; idx < PE; idx += kThreads) {
                const uint32_t a = idx / E, e = idx - a * E;
                gw[idx] += zrow[a] * pe[i * E + e];
            }
            for (uint32_t e = wave; e < E; e += kWaves) {
                double acc = 0.0;
                for (uint32_t a = lane; a < P; a += 64) acc += zrow[a] * pw[a * E + e];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
                if (lane == 0) ge[i * E + e] = acc;
            }
            __syncthreads();
        }
        // the dense update: a row of emb the step did not see has g = 0 (its square average decays, its value stays)
        for (uint32_t idx = tid; idx < PE; idx += kThreads) {
            double p = pe[idx], q = qe[idx];
            omf_rmsprop(p, q, ge[idx], lr, alpha, eps);
            pe[idx] = p; qe[idx] = q; ge[idx] = 0.0;
            p = pw[idx]; q = qw[idx];
            omf_rmsprop(p, q, gw[idx], lr, alpha, eps);
            pw[idx] = p; qw[idx] = q; gw[idx] = 0.0;
        }
        for (uint32_t a = tid; a < P; a += kThreads) {
            double p = pb[a], q = qb[a];
            omf_rmsprop(p, q, gb[a], lr, alpha, eps);
            pb[a] = p; qb[a] = q; gb[a] = 0.0;
            cnt[a] = 0;
        }
        __syncthreads();
        ++n_taken;
        n_used += hi - lo;
    }

    if constexpr (kLds) {
        for (uint32_t i = tid; i < PE; i += kThreads) { m.emb[i] = pe[i]; m.w[i] = pw[i]; m.sq_emb[i] = qe[i]; m.sq_w[i] = qw[i]; }
        for (uint32_t i = tid; i < P; i += kThreads) { m.bias[i] = pb[i]; m.sq_bias[i] = qb[i]; }
    }
    if (tid == 0) {
        out[0] = 0;
        out[1] = static_cast<int64_t>(n_taken);
        out[2] = static_cast<int64_t>(n_empty);
        out[3] = static_cast<int64_t>(n_used);
    }
}

}  // namespace

extern "C" size_t rg_omf_pairs_workspace_bytes(uint64_t n_rows, uint64_t n_pending) {
    return omf_pairs_carve(nullptr, n_rows, n_pending).bytes;
}

extern "C" int rg_omf_pairs(const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users, uint64_t n_organic_users, uint64_t n_rows,
                            uint32_t num_products, uint64_t first_call, uint32_t mini_batch, const int32_t* d_pending, uint64_t n_pending,
                            int32_t* d_pairs, uint64_t pairs_capacity, int64_t* d_step_offsets, uint64_t step_capacity, int64_t* d_out,
                            void* d_workspace, size_t workspace_bytes, void* stream) {
    if (num_products == 0 || num_products > RG_EV_INDEX_MASK) return fail(RG_EINVAL, "rg_omf_pairs: bad num_products %u", num_products);
    if (mini_batch == 0) return fail(RG_EINVAL, "rg_omf_pairs: mini_batch 0");
    if (!d_offsets || (n_rows && !d_rows)) return fail(RG_EINVAL, "rg_omf_pairs: null rows / offsets");
    if (n_organic_users > n_users) return fail(RG_EINVAL, "rg_omf_pairs: more organic-only users than users");
    if (n_rows > 0xFFFFFFF0ull || n_pending > 0xFFFFFFF0ull) return fail(RG_EINVAL, "rg_omf_pairs: more than 2^32 - 16 rows / pending pairs");
    if (n_pending && !d_pending) return fail(RG_EINVAL, "rg_omf_pairs: null pending pairs");
    if (!d_pairs || !d_step_offsets || !d_out || !d_workspace) return fail(RG_EINVAL, "rg_omf_pairs: null output / workspace");
    if (reinterpret_cast<uintptr_t>(d_rows) % 16) return fail(RG_EINVAL, "rg_omf_pairs: rows not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_workspace) % 8) return fail(RG_EINVAL, "rg_omf_pairs: workspace not 8-byte aligned");
    if (pairs_capacity < n_pending + n_rows)
        return fail(RG_ENOMEM, "rg_omf_pairs: room for %llu pairs < %llu (pending + rows)", static_cast<unsigned long long>(pairs_capacity),
                    static_cast<unsigned long long>(n_pending + n_rows));
    const uint64_t need_steps = (first_call % mini_batch + n_rows) / mini_batch + 2;
    if (step_capacity < need_steps)
        return fail(RG_ENOMEM, "rg_omf_pairs: room for %llu step offsets < %llu", static_cast<unsigned long long>(step_capacity),
                    static_cast<unsigned long long>(need_steps));
    const OmfPairsWs w = omf_pairs_carve(d_workspace, n_rows, n_pending);
    if (workspace_bytes < w.bytes) return fail(RG_ENOMEM, "rg_omf_pairs: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(d_out, 0, kOmfOutWords * sizeof(int64_t), s));
    HIP_TRY(hipMemsetAsync(w.call, 0, (n_rows + 1) * sizeof(uint32_t), s));
    if (n_rows) HIP_TRY(hipMemsetAsync(w.pair, 0, n_rows, s));
    if (n_users) {
        const uint64_t blocks64 = (n_users + 3) / 4;
        hipLaunchKernelGGL(k_omf_flags, dim3(static_cast<uint32_t>(blocks64 > 4096 ? 4096 : blocks64)), dim3(256), 0, s, d_rows, d_offsets,
                           n_users, n_organic_users, n_rows, num_products, w.call, w.pair, d_out);
        HIP_TRY(hipGetLastError());
    }
    int64_t verdict = 0;
    HIP_TRY(hipMemcpyAsync(&verdict, d_out, sizeof(verdict), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (verdict & static_cast<int64_t>(kOmfErrOffsets)) return fail(RG_EINVAL, "rg_omf_pairs: offsets descend or leave the %llu rows; nothing was written",
                                                                     static_cast<unsigned long long>(n_rows));
    if (verdict & static_cast<int64_t>(kOmfErrFirstBandit)) return fail(RG_EINVAL, "rg_omf_pairs: a user opens with a bandit row; nothing was written");
    if (verdict & static_cast<int64_t>(kOmfErrEmptyOrganic)) return fail(RG_EINVAL, "rg_omf_pairs: an organic-only user without rows; nothing was written");
    if (verdict & static_cast<int64_t>(kOmfErrOrganicBandit)) return fail(RG_EINVAL, "rg_omf_pairs: an organic-only user has a bandit row; nothing was written");
    if (verdict & static_cast<int64_t>(kOmfErrProduct))
        return fail(RG_EINVAL, "rg_omf_pairs: the log has a product >= num_products %u; nothing was written", num_products);
    const uint64_t n1 = n_rows + 1;
    const uint64_t g64 = (n1 + n_pending + 255) / 256;
    const uint32_t grid = static_cast<uint32_t>(g64 > 8192 ? 8192 : g64);
    if (int rc = omf_scan(w.call, n1, w.sums, s)) return rc;
    hipLaunchKernelGGL(k_omf_keep, dim3(grid), dim3(256), 0, s, w.call, w.pair, w.keep, n_rows, first_call, mini_batch);
    HIP_TRY(hipGetLastError());
    if (int rc = omf_scan(w.keep, n1, w.sums, s)) return rc;
    hipLaunchKernelGGL(k_omf_scatter, dim3(grid), dim3(256), 0, s, d_rows, w.call, w.keep, n_rows, d_pending, n_pending, d_pairs, w.step);
    HIP_TRY(hipGetLastError());
    const uint64_t gs64 = (need_steps + 255) / 256;
    hipLaunchKernelGGL(k_omf_offsets, dim3(static_cast<uint32_t>(gs64 > 8192 ? 8192 : gs64)), dim3(256), 0, s, w.call, w.keep, w.step, n_rows,
                       n_pending, first_call, mini_batch, d_step_offsets, step_capacity, d_out);
    HIP_TRY(hipGetLastError());
    return RG_OK;
}

extern "C" int rg_omf_limits(uint32_t embed_dim, uint32_t* lds_max_products, uint32_t* max_products) {
    if (embed_dim == 0 || embed_dim > kOmfMaxEmbed) return fail(RG_EINVAL, "rg_omf_limits: embed_dim %u outside 1 .. %u", embed_dim, kOmfMaxEmbed);
    uint32_t p = 0;
    while (p < kOmfMaxProducts && omf_lds_fits(p + 1, embed_dim)) ++p;
    if (lds_max_products) *lds_max_products = p;
    if (max_products) *max_products = kOmfMaxProducts;
    return RG_OK;
}

extern "C" size_t rg_omf_steps_workspace_bytes(uint32_t num_products, uint32_t embed_dim) {
    return 8 * (2 * static_cast<size_t>(num_products) * embed_dim + num_products);
}

extern "C" int rg_omf_steps(const rg_omf_model* model, double lr, double alpha, double eps, const int32_t* d_pairs, uint64_t n_pairs,
                            const int64_t* d_step_offsets, uint64_t n_steps, uint32_t force_global, int64_t* d_out, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
    if (!model) return fail(RG_EINVAL, "rg_omf_steps: null model");
    const uint32_t P = model->num_products, E = model->embed_dim;
    if (P == 0 || P > kOmfMaxProducts) return fail(RG_EINVAL, "rg_omf_steps: num_products %u outside 1 .. %u", P, kOmfMaxProducts);
    if (E == 0 || E > kOmfMaxEmbed) return fail(RG_EINVAL, "rg_omf_steps: embed_dim %u outside 1 .. %u", E, kOmfMaxEmbed);
    if (!model->emb || !model->w || !model->bias || !model->sq_emb || !model->sq_w || !model->sq_bias)
        return fail(RG_EINVAL, "rg_omf_steps: null model array");
    if (!(lr == lr) || !(alpha >= 0.0 && alpha <= 1.0) || !(eps >= 0.0)) return fail(RG_EINVAL, "rg_omf_steps: bad lr / alpha / eps");
    if ((n_pairs && !d_pairs) || !d_step_offsets || !d_out) return fail(RG_EINVAL, "rg_omf_steps: null pairs / step offsets / out");
    const bool lds = !force_global && omf_lds_fits(P, E);
    if (!lds) {
        if (!d_workspace || workspace_bytes < rg_omf_steps_workspace_bytes(P, E))
            return fail(RG_ENOMEM, "rg_omf_steps: workspace %zu < %zu bytes", workspace_bytes, rg_omf_steps_workspace_bytes(P, E));
        if (reinterpret_cast<uintptr_t>(d_workspace) % 8) return fail(RG_EINVAL, "rg_omf_steps: workspace not 8-byte aligned");
    }
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t shmem = omf_lds_bytes(P, E, lds);
    if (lds)
        hipLaunchKernelGGL((k_omf_steps<true, 256>), dim3(1), dim3(256), shmem, s, *model, static_cast<double*>(nullptr), lr, alpha, eps,
                           d_pairs, n_pairs, d_step_offsets, n_steps, d_out);
    else
        hipLaunchKernelGGL((k_omf_steps<false, 1024>), dim3(1), dim3(1024), shmem, s, *model, static_cast<double*>(d_workspace), lr, alpha, eps,
                           d_pairs, n_pairs, d_step_offsets, n_steps, d_out);
    HIP_TRY(hipGetLastError());
    return RG_OK;
}
