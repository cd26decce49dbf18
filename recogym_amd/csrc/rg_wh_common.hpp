// rg_wh_common.hpp — the time-weighted view history of the likelihood agent (weight_history_function): the timed history row, the
// feature list of one act, and the act on it.  DESIGN.md 4g has the contract; agents/views_history.py (weight_table,
// weighted_list) restates it in NumPy.
//
// The reference casts every clock value to int16 before the weight function sees it, so inside the clock range [0, 32767] the
// function is a TABLE over the differences 0 .. 32767 (the host evaluates it once; a float32 table arrives widened to double).  A
// product's feature at time `now` is the sequential sum, in view order and in the table's dtype, of table[now - t] over its views,
// rounded once to float32; products whose feature is exactly 0 leave the list (which changes n, and with it the cross-term index of
// poly_act).  The float32 arithmetic here never holds a float32 subnormal in a float register: values are doubles that hold float32
// values, rounded by wh_round_f32, so the result does not depend on the float32 denormal mode the unit is compiled with —
// exp(-t) is subnormal for 88 <= t <= 103, and those views decide whether a product stays in the list.
//
// The timed row has the size and the capacity rule of the count row (hist_cap words, keep = hist_cap - 1, RG_CNT_HIST_OVERFLOW per
// dropped view) but holds VIEWS, not distinct products:
//   word 0        header: (views kept << 32) | entries
//   words 1..     (product << 32) | uint16 time, ascending as 64-bit words: product ascending, then view order (the clock never
//                 runs backwards; equal words have equal weights, so their order does not matter)
#pragma once

#include "rg_poly_common.hpp"

namespace rgk {

constexpr uint32_t kWhTableLen = 32768;       // differences of two clock values in [0, 32767]

__device__ __forceinline__ uint32_t wt_prod(hent_t e) { return static_cast<uint32_t>(e >> 32); }
__device__ __forceinline__ uint32_t wt_time(hent_t e) { return static_cast<uint32_t>(e) & 0xFFFFu; }

// s rounded to the nearest float32 value (ties to even, subnormals kept, overflow to infinity), held in a double.  Below 2^-126 the
// float32 grid is the multiples of 2^-149: adding and subtracting 1.5 2^-97 (whose ulp is 2^-149) rounds to it in double
// arithmetic; from 2^-126 up the conversion's result is a normal float32 whatever the denormal mode.
__device__ __forceinline__ double wh_round_f32(double s) {
    if (fabs(s) < 0x1p-126) return __dsub_rn(__dadd_rn(s, 0x1.8p-97), 0x1.8p-97);
    return static_cast<double>(__double2float_rn(s));
}

// the float32 bit pattern of such a value, and back
__device__ __forceinline__ uint32_t wh_f32_bits(double r) {
    if (fabs(r) < 0x1p-126) return (signbit(r) ? 0x80000000u : 0u) | static_cast<uint32_t>(__dmul_rn(fabs(r), 0x1p149));
    return __float_as_uint(__double2float_rn(r));
}
__device__ __forceinline__ double wh_f32_value(uint32_t b) {
    if ((b & 0x7F800000u) == 0u) {
        const double m = __dmul_rn(static_cast<double>(b & 0x007FFFFFu), 0x1p-149);
        return (b >> 31) ? -m : m;
    }
    return static_cast<double>(__uint_as_float(b));
}

// One view into a timed row, by one thread: a sorted insert that never merges.  Returns 1 when the row is full (the view is
// dropped; row and header stay as they are), else 0.
__device__ __forceinline__ uint32_t wh_insert(hent_t* hr, uint32_t hist_cap, uint32_t v, uint32_t t16) {
    const hent_t h0 = hr[0];
    const uint32_t ne = h_cnt(h0);
    if (ne + 1 >= hist_cap) return 1u;
    const hent_t key = (static_cast<hent_t>(v) << 32) | (t16 & 0xFFFFu);
    uint32_t j = ne + 1;                       // entries above the key move up by one, highest first
    while (j > 1 && hr[j - 1] > key) { hr[j] = hr[j - 1]; --j; }
    hr[j] = key;
    hr[0] = h0 + (1ull << 32) + 1ull;
    return 0u;
}

// The feature list of the act at clock value `now` on the `ne` entries `ent` of a timed row, by the whole wave (all arguments
// wave-uniform).  s_w / s_ep: LDS rows of kPolyHist entries that stage the weights and products of the first kPolyHist ENTRIES;
// the list goes to s_val / s_prod (its first kPolyHist products) and, whole, to g_prod / g_bits (global, g_cap entries, float32
// bit patterns) when those are given — the source of a list longer than kPolyHist.  Returns the list's length; *out_of_range is
// set when `now` or a view's time lies outside [0, 32767], a view lies after `now` or a difference is beyond the table: the weight
// is then the table's at the clamped index and the caller discards the result.
__device__ __forceinline__ uint32_t wh_list(const WhTable& wt, const hent_t* ent, uint32_t ne, uint32_t now, int lane, double* s_w,
                                            uint32_t* s_ep, double* s_val, uint32_t* s_prod, uint32_t* g_prod, uint32_t* g_bits,
                                            uint32_t g_cap, bool* out_of_range) {
    bool bad = now >= kWhTableLen;
    const auto weight = [&](hent_t e) {
        const uint32_t tv = wt_time(e);
        const int32_t dt = static_cast<int32_t>(now) - static_cast<int32_t>(tv);
        if (tv >= kWhTableLen || dt < 0 || static_cast<uint32_t>(dt) >= wt.n) bad = true;
        return wt.tab[static_cast<uint32_t>(min(max(dt, 0), static_cast<int32_t>(wt.n) - 1))];
    };
    for (uint32_t i = lane; i < ne && i < kPolyHist; i += 64) {
        const hent_t e = ent[i];
        s_w[i] = weight(e);
        s_ep[i] = wt_prod(e);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const auto prod_at = [&](uint32_t j) { return j < kPolyHist ? s_ep[j] : wt_prod(ent[j]); };
    uint32_t n_out = 0;
    for (uint32_t base = 0; base < ne; base += 64) {
        const uint32_t i = base + lane;
        uint32_t p = 0;
        bool head = false;                      // this lane's entry opens its product's run
        if (i < ne) {
            p = prod_at(i);
            head = i == 0 || prod_at(i - 1) != p;
        }
        double acc = 0.0;
        if (head) {
            for (uint32_t j = i; j < ne && prod_at(j) == p; ++j) {
                const double w = j < kPolyHist ? s_w[j] : weight(ent[j]);
                acc = __dadd_rn(acc, w);
                if (wt.f32) acc = wh_round_f32(acc);
            }
            if (!wt.f32) acc = wh_round_f32(acc);
        }
        const bool keep = head && acc != 0.0;
        const unsigned long long m = __ballot(keep);
        const uint32_t k = n_out + prefix_in_mask(m);
        if (keep) {
            if (k < kPolyHist) { s_val[k] = acc; s_prod[k] = p; }
            if (g_prod && k < g_cap) { g_prod[k] = p; g_bits[k] = wh_f32_bits(acc); }
        }
        n_out += static_cast<uint32_t>(__popcll(m));
    }
    if (__ballot(bad)) *out_of_range = true;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");     // the list is read by other lanes than those that wrote it
    __builtin_amdgcn_wave_barrier();
    return n_out;
}

// the feature list wh_list left, as poly_act reads a history (rg_poly_common.hpp: H)
struct WhListHist {
    typedef double val_t;
    const double* s_val;
    const uint32_t* s_prod;
    const uint32_t* g_prod;
    const uint32_t* g_bits;
    uint32_t nd;
    __device__ __forceinline__ uint32_t size() const { return nd; }
    __device__ __forceinline__ uint32_t prod(uint32_t i) const { return i < kPolyHist ? s_prod[i] : g_prod[i]; }
    __device__ __forceinline__ double cnt(uint32_t i) const { return i < kPolyHist ? s_val[i] : wh_f32_value(g_bits[i]); }
    __device__ __forceinline__ void get(uint32_t i, uint32_t& p, double& c) const { p = prod(i); c = cnt(i); }
};

// The weighted act: the feature list, then poly_act on it, unchanged in rule.  s_val / s_prod are the LDS rows poly_act stages a
// history in: it finds the first kPolyHist entries there already and writes them back as they are.  A list longer than kPolyHist
// needs g_prod / g_bits with g_cap >= min(P, ne); without them (or beyond g_cap) the act is reported unresolved (flag bit 1).
template <class M>
__device__ __forceinline__ uint32_t wh_act(const M& d, const WhTable& wt, const hent_t* ent, uint32_t ne, uint32_t now, int lane,
                                           const double* s_th, double* s_w, uint32_t* s_ep, double* s_val, uint32_t* s_prod,
                                           uint32_t* g_prod, uint32_t* g_bits, uint32_t g_cap, uint32_t* flags, uint32_t* list_n,
                                           bool* out_of_range) {
    const uint32_t n = wh_list(wt, ent, ne, now, lane, s_w, s_ep, s_val, s_prod, g_prod, g_bits, g_cap, out_of_range);
    *list_n = n;
    const bool short_of_room = n > kPolyHist && (!g_prod || n > g_cap);
    const uint32_t a = poly_act(d, WhListHist{s_val, s_prod, g_prod, g_bits, short_of_room ? kPolyHist : n}, lane, s_th, s_val, s_prod, flags);
    if (short_of_room) *flags |= 2u;
    return a;
}

}  // namespace rgk
