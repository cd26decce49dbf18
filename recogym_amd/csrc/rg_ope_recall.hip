// rg_ope_recall.hip — recall@k over a sorted device log (evaluate_recall_at_k, reference evaluate_agent.py:832-870), the table
// form: for every COUNTED bandit row (no click, the successor inside the user's range, the successor organic) whether the
// successor's product is in the top-k set of the target's `ps-a` at that row.
//
// The set is not ranked here.  For the targets this form serves `ps-a` is a function of a small key — the model's act (a one-hot
// vector), under EpsilonGreedy the act and the explore flip, for RandomAgent nothing at all — and np.argpartition on a vector full
// of ties returns a set that only NumPy's own introselect knows.  So the host builds one ascending k-entry set per key that occurs
// with np.argpartition itself (evaluate_agent.recall_sets), and the device tests membership: a binary search per counted row.
//
// The skeleton is rg_ope_common.hpp's: one wave per user, coalesced 64-row chunks.  The successor of the lane at chunk position 63
// is the first row of the next chunk, read only where that row is still the user's (ope_next_code): a user's last row has no
// successor, so nothing at or beyond d_offsets[n_users] is addressed.  The sums are integer adds (the same on every run).
// The ranking form (the sampling LogReg, whose `ps-a` is a softmax) is an instantiation of rg_ope_logreg.hip's kernel.
#include "rg_ope_common.hpp"

namespace {

constexpr uint32_t kRcMaxWaves = 5120;          // 256 CUs x 20 waves

__global__ __launch_bounds__(64 * kOpeWaves) void k_ope_recall_hits(
    const rg_event* __restrict__ rows, const int64_t* __restrict__ offsets, uint64_t n_users, const int32_t* __restrict__ key,
    uint32_t n_keys, const int32_t* __restrict__ sets, uint32_t k, uint8_t* __restrict__ hit, unsigned long long* __restrict__ sums,
    uint32_t n_waves) {
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * kOpeWaves + wib;
    unsigned long long n_counted = 0, n_hits = 0;                 // (wave-uniform)
    for (uint64_t user = wave; user < n_users; user += n_waves) {
        const int64_t b = offsets[user], e = offsets[user + 1];
        for (int64_t base = b; base < e; base += 64) {
            const int64_t row = base + lane;
            const bool live = row < e;
            const uint32_t code = live ? rows[row].code : 0u;
            bool has_next;
            const uint32_t next = ope_next_code(rows, row, e, code, lane, has_next);
            bool counted = live && ope_recall_counted(code, next, has_next);
            uint32_t kk = 0;
            if (counted) {
                kk = static_cast<uint32_t>(key[row]);
                counted = kk < n_keys;                            // (never index the table with a key it does not have)
            }
            bool found = false;
            if (counted) {
                const int32_t* set = sets + static_cast<size_t>(kk) * k;
                const int32_t v = static_cast<int32_t>(next & RG_EV_INDEX_MASK);
                uint32_t lo = 0, hi = k;                          // the first entry >= v in set[0 .. k)
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    if (set[mid] < v) lo = mid + 1; else hi = mid;
                }
                found = lo < k && set[lo] == v;
            }
            if (live) hit[row] = counted ? (found ? kRecallHit : kRecallMiss) : kRecallNotCounted;
            n_counted += static_cast<unsigned long long>(__popcll(__ballot(counted)));
            n_hits += static_cast<unsigned long long>(__popcll(__ballot(found)));
        }
    }
    if (lane == 0) {
        if (n_counted) (void)__hip_atomic_fetch_add(&sums[0], n_counted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_hits) (void)__hip_atomic_fetch_add(&sums[1], n_hits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

extern "C" int rg_ope_recall_hits(const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users, const int32_t* d_key,
                                  uint32_t n_keys, const int32_t* d_sets, uint32_t k, uint8_t* d_hit, int64_t* d_sums, void* stream) {
    const char* who = "rg_ope_recall_hits";
    if (k == 0 || n_keys == 0) return fail(RG_EINVAL, "%s: k = %u, n_keys = %u (both at least 1)", who, k, n_keys);
    if (n_users && (!d_rows || !d_offsets || !d_key || !d_hit)) return fail(RG_EINVAL, "%s: null rows / offsets / key / hit", who);
    if (!d_sets || !d_sums) return fail(RG_EINVAL, "%s: null sets / sums", who);
    if (reinterpret_cast<uintptr_t>(d_rows) % 16) return fail(RG_EINVAL, "%s: rows not 16-byte aligned", who);
    if (rg_device_count() <= 0) return fail(RG_ENODEV, "no HIP device");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(d_sums, 0, 2 * sizeof(int64_t), s));
    if (!n_users) return RG_OK;
    const uint32_t W = ope_waves(n_users, kRcMaxWaves);
    hipLaunchKernelGGL(k_ope_recall_hits, dim3(W / kOpeWaves), dim3(64 * kOpeWaves), 0, s, d_rows, d_offsets, n_users, d_key, n_keys, d_sets,
                       k, d_hit, reinterpret_cast<unsigned long long*>(d_sums), W);
    HIP_TRY(hipGetLastError());
    return RG_OK;
}
