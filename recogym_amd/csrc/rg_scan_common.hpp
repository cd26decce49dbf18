// rg_scan_common.hpp — the in-place exclusive scan of a uint32 device array that the log reductions share (rg_omf_pairs of
// rg_organic_mf.hip, rg_bmf_samples of rg_bandit_mf.hip).  Included after rg_common.hpp; everything sits in the anonymous namespace,
// so every unit of the per-unit build gets its own copy and the one-unit build exactly one.
#pragma once

#include "rg_common.hpp"

namespace {

constexpr int kOmfScanThreads = 256, kOmfScanPer = 8, kOmfScanBlock = kOmfScanThreads * kOmfScanPer;

// ---------------------------------------------------------------------------------------------------------------------------
// the in-place exclusive scan of a uint32 array (three launches: block sums, their scan, the blocks again)
// ---------------------------------------------------------------------------------------------------------------------------
// exclusive scan of one value per thread over the block; `total` = the block's sum.  s_w: one word per wave.
__device__ __forceinline__ uint32_t omf_block_excl(uint32_t v, uint32_t* s_w, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(inc), o));
        if (lane >= static_cast<uint32_t>(o)) inc += up;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < nw; ++w) {
        const uint32_t x = s_w[w];
        if (w < wave) before += x;
        all += x;
    }
    __syncthreads();
    total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kOmfScanThreads) void k_omf_scan_sums(const uint32_t* __restrict__ a, uint64_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_w[kOmfScanThreads / 64];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kOmfScanBlock + threadIdx.x * kOmfScanPer;
    uint32_t t = 0;
#pragma unroll
    for (int k = 0; k < kOmfScanPer; ++k)
        if (base + k < n) t += a[base + k];
    uint32_t total;
    (void)omf_block_excl(t, s_w, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void k_omf_scan_top(uint32_t* __restrict__ sums, uint64_t nb) {
    __shared__ uint32_t s_w[16];
    uint32_t carry = 0;
    for (uint64_t base = 0; base < nb; base += 1024) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? sums[i] : 0u;
        uint32_t total;
        const uint32_t ex = omf_block_excl(v, s_w, total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(kOmfScanThreads) void k_omf_scan_apply(uint32_t* __restrict__ a, uint64_t n, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_w[kOmfScanThreads / 64];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kOmfScanBlock + threadIdx.x * kOmfScanPer;
    uint32_t v[kOmfScanPer];
    uint32_t t = 0;
#pragma unroll
    for (int k = 0; k < kOmfScanPer; ++k) {
        v[k] = base + k < n ? a[base + k] : 0u;
        t += v[k];
    }
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + omf_block_excl(t, s_w, total);
#pragma unroll
    for (int k = 0; k < kOmfScanPer; ++k) {
        if (base + k < n) a[base + k] = run;
        run += v[k];
    }
}

int omf_scan(uint32_t* a, uint64_t n, uint32_t* sums, hipStream_t s) {
    const uint64_t nb = (n + kOmfScanBlock - 1) / kOmfScanBlock;
    hipLaunchKernelGGL(k_omf_scan_sums, dim3(static_cast<uint32_t>(nb)), dim3(kOmfScanThreads), 0, s, a, n, sums);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_omf_scan_top, dim3(1), dim3(1024), 0, s, sums, nb);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_omf_scan_apply, dim3(static_cast<uint32_t>(nb)), dim3(kOmfScanThreads), 0, s, a, n, sums);
    HIP_TRY(hipGetLastError());
    return RG_OK;
}

}  // namespace
