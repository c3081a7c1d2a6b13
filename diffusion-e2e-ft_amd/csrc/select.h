// select.h — exact order statistics on the device, defined once: an MSB-first radix select over an order-preserving unsigned image of the values
// (32-bit keys: 11 / 11 / 10 bit digits, 64-bit keys: 11 x 5 + 9), for many independent selections in the same launches.
// Per digit p: the caller's own load loop feeds a DigitHist (2048 LDS bins per selection; only keys that match the prefix found so far count) and
// flushes it into the selection's global histogram with integer atomics (any order gives the same counts); select_scan_kernel, one block per
// selection, scans the 2048 counts, fixes the digit that holds the rank, extends the prefix and clears the bins for the next pass.  After the last
// digit the prefix is the key a of rank k with its multiplicity; the key b of rank k + 1 is a again inside a's run, else the next non-empty bin of the
// last histogram, else unknown: then one SuccMin pass finds the smallest key above a, and select_successor reduces its per-block partials.
// The rank comes from a caller's rule applied to the first digit's total (the number of valid elements).  Nothing is read back to the host.
#pragma once
#include "reduce.h"

namespace e2eft {

constexpr int SEL_BINS = 2048, SEL_DIGIT_BITS = 11;

// ---- keys: unsigned order == numeric order (-0.0 below +0.0; NaNs beyond the infinities, by sign) -------------------------------------------
template <typename K> __device__ __forceinline__ K order_bits(K u) {
    constexpr K SIGN = K(1) << (8 * sizeof(K) - 1);
    return (u & SIGN) ? ~u : (u | SIGN);
}
template <typename K> __device__ __forceinline__ K order_bits_inv(K k) {
    constexpr K SIGN = K(1) << (8 * sizeof(K) - 1);
    return (k & SIGN) ? (k & ~SIGN) : ~k;
}
__device__ __forceinline__ uint32_t order_key(float v) { return order_bits<uint32_t>(__float_as_uint(v)); }
__device__ __forceinline__ uint64_t order_key(double v) { return order_bits<uint64_t>((uint64_t)__double_as_longlong(v)); }
__device__ __forceinline__ float order_value(uint32_t k) { return __uint_as_float(order_bits_inv(k)); }
__device__ __forceinline__ double order_value(uint64_t k) { return __longlong_as_double((long long)order_bits_inv(k)); }

// ---- digit plan: every digit is SEL_DIGIT_BITS wide from the top, the last one takes the rest ----------------------------------------------
struct SelDigit { int shift, width; };
constexpr __host__ __device__ int select_digits(int key_bits) { return (key_bits + SEL_DIGIT_BITS - 1) / SEL_DIGIT_BITS; }
constexpr __host__ __device__ SelDigit select_digit(int key_bits, int p) {
    const int top = key_bits - SEL_DIGIT_BITS * p;                       // the bits below the digits already fixed
    const int shift = top > SEL_DIGIT_BITS ? top - SEL_DIGIT_BITS : 0;
    return SelDigit{shift, top - shift};
}
static_assert(select_digits(32) == 3 && select_digits(64) == 6, "digit count");
static_assert(select_digit(32, 0).shift == 21 && select_digit(32, 1).shift == 10 && select_digit(32, 2).shift == 0, "32-bit plan");
static_assert(select_digit(32, 0).width == 11 && select_digit(32, 1).width == 11 && select_digit(32, 2).width == 10, "32-bit plan: 11 / 11 / 10");
static_assert(select_digit(64, 0).shift == 53 && select_digit(64, 1).shift == 42 && select_digit(64, 2).shift == 31 && select_digit(64, 3).shift == 20 &&
                  select_digit(64, 4).shift == 9 && select_digit(64, 5).shift == 0, "64-bit plan");
static_assert(select_digit(64, 0).width == 11 && select_digit(64, 4).width == 11 && select_digit(64, 5).width == 9, "64-bit plan: 11 x 5 + 9");

// ---- per-selection state (8-byte words), device memory only -------------------------------------------------------------------------------
struct SelState {
    int64_t n;              // 0: nothing to select.  select_init: active or not; after the first scan: the number of valid elements
    int64_t rank;           // rank of a inside the keys that share the prefix
    uint64_t prefix;        // key bits fixed so far; after the last digit: a
    uint64_t succ;          // b, the key of rank k + 1 (a itself when the rule does not ask for it), valid when succ_unknown == 0
    int64_t succ_unknown;   // b lies outside a's last histogram: the SuccMin pass finds it
    int64_t succ_needed;    // the rank rule asked for b
    double weight;          // the rank rule's interpolation weight, for the caller's finishing kernel
};
__device__ __forceinline__ void select_init(SelState* st, bool active) { *st = SelState{active ? 1 : 0, 0, 0, 0, 0, 0, 0.0}; }

// what a rank rule returns: struct Rule { __device__ SelRank operator()(int64_t n, int selection) const; }, n >= 1 valid elements
struct SelRank {
    int64_t rank;           // k, 0 <= k < n
    bool need_succ;         // the caller will read rank k + 1 too (k + 1 < n)
    double weight;
};

// ---- the digit pass: LDS histograms of digit p for the NSEL selections of one data stream (they share its valid elements, so they are active
// together).  Used by every thread of the block: construct, leave if (!any), zero(), add(key) in the caller's load loop, flush(global bins).
template <typename K, int NSEL> struct DigitHist {
    uint32_t* h;
    K prefix[NSEL], himask;   // himask: the bits above the digit; 0 on the first digit (every key counts)
    int shift;
    uint32_t mask;
    bool any;
    __device__ __forceinline__ DigitHist(int p, const SelState* st) {
        __shared__ uint32_t bins[NSEL * SEL_BINS];
        h = bins;
        const SelDigit d = select_digit(8 * sizeof(K), p);
        shift = d.shift;
        mask = (1u << d.width) - 1;
        himask = p ? ~K(0) << (d.shift + d.width) : K(0);
        any = st[0].n != 0;
#pragma unroll
        for (int j = 0; j < NSEL; ++j) prefix[j] = p ? (K)st[j].prefix : K(0);
    }
    __device__ __forceinline__ void zero() {
        for (int i = threadIdx.x; i < NSEL * SEL_BINS; i += blockDim.x) h[i] = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void add(K key) {
#pragma unroll
        for (int j = 0; j < NSEL; ++j)
            if (((key ^ prefix[j]) & himask) == 0) atomicAdd(&h[j * SEL_BINS + ((uint32_t)(key >> shift) & mask)], 1u);
    }
    __device__ __forceinline__ void flush(uint32_t* __restrict__ g /* [NSEL][SEL_BINS], this stream's */) {
        __syncthreads();
        for (int i = threadIdx.x; i < NSEL * SEL_BINS; i += blockDim.x)
            if (h[i]) atomicAdd(&g[i], h[i]);
    }
};

// ---- the scan: block s (1024 threads, two bins each) resolves digit p of selection s.  Counts fit 32 bits (the hosts check the element counts).
template <typename K, typename Rule>
__global__ __launch_bounds__(SEL_BINS / 2) void select_scan_kernel(int p, uint32_t* __restrict__ hist, SelState* __restrict__ state, Rule rule) {
    __shared__ uint32_t wsum[16];
    __shared__ int64_t pick[3];
    __shared__ int next;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const SelDigit d = select_digit(8 * sizeof(K), p);
    uint32_t* hh = hist + (int64_t)blockIdx.x * SEL_BINS;
    SelState* st = state + blockIdx.x;
    if (st->n == 0) return;                                            // (the digit passes left its histogram alone: still clear)
    int64_t k = st->rank;
    bool need = st->succ_needed != 0;
    double weight = st->weight;
    const K before_prefix = p ? (K)st->prefix : K(0);
    const uint32_t c0 = hh[2 * t], c1 = hh[2 * t + 1];
    hh[2 * t] = 0;
    hh[2 * t + 1] = 0;
    if (t == 0) {
        pick[0] = pick[1] = pick[2] = 0;                               // (stay so only if the counts are inconsistent)
        next = SEL_BINS;
    }
    uint32_t incl = c0 + c1;                                           // inclusive scan over the threads' bin pairs
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();                                                   // (every read of *st above precedes thread 0's writes below)
    uint32_t before = 0, total = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    const uint32_t excl = before + incl - (c0 + c1);
    if (p == 0) {
        if (total == 0) {
            if (t == 0) st->n = 0;
            return;
        }
        const SelRank r = rule((int64_t)total, (int)blockIdx.x);
        k = r.rank;
        need = r.need_succ;
        weight = r.weight;
    }
    if (k >= (int64_t)excl && k < (int64_t)excl + c0 + c1) {
        const bool lo = k < (int64_t)excl + c0;
        pick[0] = 2 * t + (lo ? 0 : 1);
        pick[1] = k - excl - (lo ? 0 : c0);
        pick[2] = lo ? c0 : c1;
    }
    __syncthreads();
    const int dig = (int)pick[0];
    const K prefix = before_prefix | ((K)dig << d.shift);
    const bool last = d.shift == 0;
    if (last && need) {                                                // the first non-empty bin above a's
        if (c0 && 2 * t > dig) atomicMin(&next, 2 * t);
        else if (c1 && 2 * t + 1 > dig) atomicMin(&next, 2 * t + 1);
        __syncthreads();
    }
    if (t != 0) return;
    if (p == 0) {
        st->n = total;
        st->succ_needed = need;
        st->weight = weight;
    }
    st->rank = pick[1];
    st->prefix = prefix;
    if (last) {
        const bool in_run = !need || pick[1] + 1 < pick[2];
        st->succ = in_run ? prefix : ((prefix & ~(K)((1u << d.width) - 1)) | (K)next);
        st->succ_unknown = !in_run && next >= SEL_BINS;
    }
}

// ---- the successor pass: the smallest key above a, per block, for the selections whose b is still unknown.  Every thread of the block: construct,
// leave if (!any()), take(key) in the caller's load loop, store(partial of this block, stride between the selections' partials).
template <typename K, int NSEL> struct SuccMin {
    K a[NSEL], mn[NSEL];
    bool need[NSEL];
    __device__ __forceinline__ SuccMin(const SelState* st) {
#pragma unroll
        for (int j = 0; j < NSEL; ++j) {
            need[j] = st[j].n != 0 && st[j].succ_unknown != 0;
            a[j] = need[j] ? (K)st[j].prefix : ~K(0);
            mn[j] = ~K(0);
        }
    }
    __device__ __forceinline__ bool any() const {
        bool r = false;
#pragma unroll
        for (int j = 0; j < NSEL; ++j) r |= need[j];
        return r;
    }
    __device__ __forceinline__ void take(K key) {
#pragma unroll
        for (int j = 0; j < NSEL; ++j)
            if (key > a[j] && key < mn[j]) mn[j] = key;
    }
    __device__ __forceinline__ void store(K* __restrict__ partial, int64_t stride) {
        __shared__ K red[NSEL][16];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
#pragma unroll
        for (int j = 0; j < NSEL; ++j) {
            mn[j] = wave_min(mn[j]);
            if (lane == 0) red[j][wave] = mn[j];
        }
        __syncthreads();
        if (threadIdx.x != 0) return;
#pragma unroll
        for (int j = 0; j < NSEL; ++j)
            if (need[j]) {
                K m = red[j][0];
                for (int w = 1; w < waves; ++w) m = red[j][w] < m ? red[j][w] : m;
                partial[j * stride] = m;
            }
    }
};

// b's key for the finishing kernels, called by one whole wave: the recorded successor, or the minimum over the nblk partials of the SuccMin pass
template <typename K> __device__ __forceinline__ K select_successor(const SelState& st, const K* __restrict__ partial, int nblk) {
    K mn = ~K(0);
    if (st.succ_unknown)
        for (int j = threadIdx.x & 63; j < nblk; j += 64) mn = partial[j] < mn ? partial[j] : mn;
    mn = wave_min(mn);
    return st.succ_unknown ? mn : (K)st.succ;
}

// torch.lerp's and numpy's _lerp two-branch formula
template <typename F> __device__ __forceinline__ F quantile_lerp(F a, F b, F w) { return w < F(0.5) ? a + w * (b - a) : b - (b - a) * (F(1) - w); }

}  // namespace e2eft
