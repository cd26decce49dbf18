// rg_count_common.hpp — what the count agents' reductions share (rg_count.hip: the offline protocol over a whole log;
// rg_evolve.hip: the filtered, online protocol of the evolution study): the per-block LDS table of 64-bit sums in front of the
// global tables and the argument check of an rg_count_tables (the wave helpers of the session list: rg_common.hpp).
#pragma once

#include "rg_common.hpp"

namespace rgk {

constexpr int kCntWaves = 4;                         // waves per block
constexpr uint32_t kCntHashLog2 = 11;
constexpr uint32_t kCntHashSlots = 1u << kCntHashLog2;   // x 16 bytes = 32 KiB of LDS per block: 5 blocks (20 waves) per CU
constexpr uint32_t kCntProbes = 8;
constexpr uint32_t kCntMaxBlocks = 1280;             // 256 CUs x 5 blocks
constexpr unsigned long long kCntEmpty = ~0ull;
constexpr uint32_t kCntTabShift = 60;                // cell index < 2^58 (P < 2^29); the table's number above it
constexpr uint32_t kCntNone = 0xFFFFFFFFu;           // last_product_viewed = None

constexpr unsigned long long kErrFirstBandit = 1, kErrProduct = 2;
constexpr int kWsErr = 0, kWsUpdates = 1, kWsAtomics = 2, kWsWords = 32;

typedef unsigned long long u64;

struct CntCtx {
    u64* key;
    u64* cnt;
    u64 *co, *pulls, *clicks;   // tables 0, 1, 2
    uint32_t n_glob;      // global atomics this lane issued
};

__device__ __forceinline__ void cnt_global(CntCtx& c, u64* base, u64 cell, u64 val) {
    (void)__hip_atomic_fetch_add(base + cell, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c.n_glob += 1;
}

// base[cell] += val (base = table number `tab`) through the block's LDS table
__device__ __forceinline__ void cnt_add(CntCtx& c, uint32_t tab, u64* base, u64 cell, u64 val) {
    const u64 k = (static_cast<u64>(tab) << kCntTabShift) | cell;
    uint32_t s = static_cast<uint32_t>((k * 0x9E3779B97F4A7C15ull) >> (64 - kCntHashLog2));
    for (uint32_t i = 0; i < kCntProbes; ++i) {
        u64 cur = __hip_atomic_load(&c.key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == kCntEmpty) {
            cur = atomicCAS(&c.key[s], kCntEmpty, k);
            if (cur == kCntEmpty) cur = k;
        }
        if (cur == k) {
            (void)__hip_atomic_fetch_add(&c.cnt[s], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return;
        }
        s = (s + 1) & (kCntHashSlots - 1);
    }
    cnt_global(c, base, cell, val);
}

inline int count_tables_ok(const rg_count_tables* t, const char* who) {
    if (!t) return fail(RG_EINVAL, "%s: null tables", who);
    if (t->num_products == 0 || t->num_products > RG_EV_INDEX_MASK) return fail(RG_EINVAL, "%s: bad num_products %u", who, t->num_products);
    if ((t->pulls == nullptr) != (t->clicks == nullptr)) return fail(RG_EINVAL, "%s: pulls and clicks come together", who);
    return RG_OK;
}

}  // namespace rgk
