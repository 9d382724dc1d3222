// rsx_search_kernels.hpp -- the kernel behind rsx_search_sorted_device (rsx.hip; launched by rsx_search.hip): the lower
// and upper bounds of m needles in a haystack of N keys that is sorted by mapped key (complemented for descending order):
//     lower[i] = #{ j < N : M(sorted[j]) <  M(needle[i]) }      upper[i] = #{ j < N : M(sorted[j]) <= M(needle[i]) }
// One kernel, rsx_search_kernel<KB, POS, IB>; one workgroup of SEARCH_WG threads per tile of search_tile(KB) consecutive
// needles, thread t holding needles tile * search_tile + j * SEARCH_WG + t (every load and store of a wave one contiguous
// range).  POS false: the needles as given, mapped in registers.  POS true: sorted joined (mapped key, u32 position)
// elements of the presort route (the join of rsx_argsort_device), the result stored at out[position].
//   a. kmin, kmax: the smallest and largest mapped key among the tile's VALID needles (wave shuffles, then LDS).
//   b. the window [lo, hi): lo = lower(kmin), hi = upper(kmax) in the whole haystack; every answer of the tile lies in
//      [lo, hi] whatever the order of the needles, which decides only how narrow the window is.  Wave 0 finds lo and wave
//      1 finds hi at the same time, each by a 64-ary search: a round probes up to 64 evenly spaced positions, one per
//      lane, and a ballot shrinks the range 64-fold -- five dependent rounds at 2^28 keys instead of 28.
//   c. hi - lo <= search_window(KB): the mapped keys of sorted[lo .. hi) go to LDS with coalesced loads and every needle
//      does its binary searches there; otherwise every needle searches [lo, hi) in global memory.  Either way lower first
//      and upper from lower on (rsx_bounds_kernel's order), the four needles of a thread in step: a turn issues their
//      probes together, so four loads are in flight per thread where one dependent chain would leave one.
//   d. the stores: out_lower / out_upper (either may be null) as IB-byte indices.
// No workgroup waits for another one and there are no atomics.  N = n or min(n, *sorted_num), read on the device.  What
// the kernel promises for a haystack that is NOT sorted: the counts of the probes and the fixed-length searches keep every
// position it reads below N and every output in [lo, hi], a sub-range of [0, N] because hi is raised to lo when the two
// searches disagree.  It reads the N keys, the m needles (elements) and sorted_num[0]; it writes out_lower[m] and
// out_upper[m] only (POS: a position of m or more is not stored).
// Known weak spot: a run of equal haystack keys longer than the window sends its tiles to the global route even when the
// needles are ordered.
#pragma once

#include "rsx_device.hpp"
#include "rsx_pairs_kernels.hpp"

namespace rsx {

constexpr uint32_t SEARCH_WG = 256;
// Bytes of mapped keys in LDS: 16 KiB, eight workgroups per CU of 160 KiB (the 16-byte keys 32 KiB and four: two tiles of
// them).  Measured against 32 KiB at 2^28 u32 / 2^26 i64 ordered needles, m = n: 1.64 / 0.51 ms against 2.35 / 0.74 ms.
constexpr uint32_t search_window_bytes(uint32_t kb) { return kb == 16 ? 32768u : 16384u; }
constexpr uint32_t search_window(uint32_t kb) { return search_window_bytes(kb) / kb; }
// Needles per thread.  Measured against 8 and 16 (tiles of 2048 and 4096): a larger tile pays the tile's chain of dependent
// latencies -- needles, five probe rounds, window -- less often, but at m = 2^16 it leaves 32 or 16 workgroups for 256 CUs
// (0.08 and 0.15 ms against 0.05 ms) and at m = n it gains nothing once the window is 16 KiB.
constexpr uint32_t search_ipt(uint32_t) { return 4u; }
constexpr uint32_t search_tile(uint32_t kb) { return SEARCH_WG * search_ipt(kb); }
// the needle element: the key alone, or the joined (mapped key, u32 position)
constexpr uint32_t search_elem(uint32_t kb, bool pos) { return pos ? pairs_elem(kb, 4u) : kb; }

// UP false: a < key (lower bound); UP true: a <= key (upper bound)
template <typename K, bool UP>
__device__ __forceinline__ bool search_before(const K& a, const K& key) {
    return UP ? !(key < a) : a < key;
}

template <typename K>
__device__ __forceinline__ K search_key_max() {
    return (K)~(K)0;
}
template <>
__device__ __forceinline__ PairsU128 search_key_max<PairsU128>() {
    return PairsU128{~0ull, ~0ull};
}

// the mapped key of sorted[j]
template <int KB>
__device__ __forceinline__ typename PairsKey<KB>::type search_hay(const uint8_t* __restrict__ sorted, uint64_t j, uint32_t kind, uint32_t desc) {
    using K = typename PairsKey<KB>::type;
    unsigned char r[KB];
    pairs_load<KB>(r, sorted + j * KB);
    K k;
    __builtin_memcpy(&k, r, KB);
    return pairs_map<K>(k, kind, desc);
}

// One wave, all 64 lanes: the number of j in [0, N) for which before(j) holds, when before is true on a prefix of [0, N) and
// false behind it; for any predicate a value in [0, N] from calls below N.  [a, b] always holds the answer; a round counts
// the probes that are before (a ballot) and keeps the gap behind the last of them.
template <typename F>
__device__ __forceinline__ uint64_t search_wave_count(uint64_t N, F&& before_at) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    uint64_t a = 0, b = N;
    while (a < b) {
        const uint64_t s = b - a;
        const uint64_t step = (s + WAVE - 1) / WAVE;   // s <= 64: every element is probed and the round is the last
        const uint64_t p = a + (uint64_t)(lane + 1) * step - 1;  // (no overflow: p < a + s + 64 * 1)
        bool before = false;
        if (p < b) before = before_at(p);
        const uint64_t c = (uint64_t)__popcll(__ballot(before));
        const uint64_t na = a + c * step;             // c probes lie below b: na <= b
        const uint64_t nb = na + step - 1;            // the probe behind them is not before the key (or lies at b or beyond)
        a = na;
        b = nb < b ? nb : b;
    }
    return a;
}
// ... the number of j in [0, N) with sorted[j] before `key`, for a sorted haystack; for any haystack a value in [0, N]
// from reads below N.
template <int KB, bool UP>
__device__ __forceinline__ uint64_t search_wave_bound(const uint8_t* __restrict__ sorted, uint64_t N, const typename PairsKey<KB>::type& key,
                                                       uint32_t kind, uint32_t desc) {
    using K = typename PairsKey<KB>::type;
    return search_wave_count(N, [&](uint64_t p) { return search_before<K, UP>(search_hay<KB>(sorted, p, kind, desc), key); });
}

// G searches in step, one thread, in positions [0, cnt), cnt >= 1: needle g looks in [base[g], base[g] + len[g]) for the
// first position whose key is not before key[g] and leaves it in base[g] (base[g] + len[g] when there is none).
// span >= every len[g]: both follow x -> x - x / 2, so when span has come down to 1 every len has.  A turn issues the G
// probes before it looks at any of them, and issues them UNCONDITIONALLY -- a needle whose range is used up re-reads a
// clamped position -- so that G loads are in flight instead of one per branch.  Reads only positions below cnt.
template <typename K, bool UP, int G, typename P, typename F>
__device__ __forceinline__ void search_in_step(F&& at, P (&base)[G], P (&len)[G], P span, P cnt, const K* key) {
    const P last = cnt - 1;
    for (; span > 1; span -= span >> 1) {
        K probe[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const P half = len[g] >> 1;
            const P i = base[g] + half - (half != 0 ? 1 : 0);
            probe[g] = at(i < last ? i : last);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const P half = len[g] >> 1;
            if (half != 0 && search_before<K, UP>(probe[g], key[g])) base[g] += half;
            len[g] -= half;
        }
    }
    K probe[G];
#pragma unroll
    for (int g = 0; g < G; ++g) probe[g] = at(base[g] < last ? base[g] : last);
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (len[g] == 1 && search_before<K, UP>(probe[g], key[g])) ++base[g];
}

// ... and when every needle looks in the whole of [0, cnt), cnt >= 1: the length is one scalar, a turn costs a needle its
// probe, a compare and an add.
template <typename K, bool UP, int G, typename P, typename F>
__device__ __forceinline__ void search_in_step_whole(F&& at, P (&base)[G], P cnt, const K* key) {
    P len = cnt;
    for (; len > 1; len -= len >> 1) {
        const P half = len >> 1;
        K probe[G];
#pragma unroll
        for (int g = 0; g < G; ++g) probe[g] = at(base[g] + half - 1);
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (search_before<K, UP>(probe[g], key[g])) base[g] += half;
    }
    K probe[G];  // len == 1: base[g] <= cnt - 1
#pragma unroll
    for (int g = 0; g < G; ++g) probe[g] = at(base[g]);
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (search_before<K, UP>(probe[g], key[g])) ++base[g];
}

// The bounds of G needles in [0, cnt) (positions of type P, read through `at`) -> stored as out[o[g]] = origin + position.
// lower first, upper from lower on; a null output's search is not run; valid[g] false: no store (the needle, a zero key,
// is searched like the others).  cnt == 0: every bound is the origin.
template <typename K, int G, typename I, typename P, typename F>
__device__ __forceinline__ void search_group(F&& at, P cnt, uint64_t origin, const K* key, const uint64_t* o, const bool* valid,
                                             uint8_t* __restrict__ out_lower, uint8_t* __restrict__ out_upper) {
    P base[G];
#pragma unroll
    for (int g = 0; g < G; ++g) base[g] = 0;
    if (out_lower) {
        if (cnt != 0) search_in_step_whole<K, false, G, P>(at, base, cnt, key);
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (valid[g]) reinterpret_cast<I*>(out_lower)[o[g]] = (I)(origin + base[g]);
    }
    if (out_upper) {
        if (out_lower && cnt != 0) {
            P len[G];
#pragma unroll
            for (int g = 0; g < G; ++g) len[g] = cnt - base[g];
            search_in_step<K, true, G, P>(at, base, len, cnt, cnt, key);
        } else if (cnt != 0) {
            search_in_step_whole<K, true, G, P>(at, base, cnt, key);
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (valid[g]) reinterpret_cast<I*>(out_upper)[o[g]] = (I)(origin + base[g]);
    }
}

// needles: m keys (POS false) or m sorted joined elements (POS true).  out_lower / out_upper: either may be null.
template <int KB, bool POS, int IB>
__global__ __launch_bounds__(SEARCH_WG) void rsx_search_kernel(const uint8_t* __restrict__ sorted, uint64_t n, const uint64_t* __restrict__ sorted_num,
                                                               const uint8_t* __restrict__ needles, uint64_t m, uint8_t* __restrict__ out_lower,
                                                               uint8_t* __restrict__ out_upper, uint32_t kind, uint32_t desc) {
    using K = typename PairsKey<KB>::type;
    using I = typename std::conditional<IB == 4, uint32_t, uint64_t>::type;
    constexpr int E = (int)search_elem(KB, POS), VOFF = (int)pairs_voff(KB, 4), IPT = (int)search_ipt(KB), NW = (int)(SEARCH_WG / WAVE);
    constexpr int G = IPT;  // searches in step
    constexpr uint32_t WINDOW = search_window(KB);
    __shared__ K s_win[WINDOW];
    __shared__ K s_min[NW], s_max[NW];
    __shared__ uint64_t s_bound[2];

    uint64_t N = n;
    if (sorted_num) {
        const uint64_t have = sorted_num[0];
        N = have < n ? have : n;
    }
    // a. the needles of this thread, mapped, and the tile's key range
    const uint64_t i0 = (uint64_t)blockIdx.x * search_tile(KB) + threadIdx.x;
    K key[IPT];
    uint64_t o[IPT];  // where the needle's results go
    bool valid[IPT];
    K kmin = search_key_max<K>(), kmax{};
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const uint64_t i = i0 + (uint64_t)j * SEARCH_WG;
        key[j] = K{};
        o[j] = i;
        valid[j] = i < m;
        if (valid[j]) {
            unsigned char er[E];
            pairs_load<E>(er, needles + i * E);
            __builtin_memcpy(&key[j], er, KB);
            if constexpr (POS) {
                uint32_t where;
                __builtin_memcpy(&where, er + VOFF, 4);
                o[j] = where;
            } else {
                key[j] = pairs_map<K>(key[j], kind, desc);
            }
            if (key[j] < kmin) kmin = key[j];
            if (kmax < key[j]) kmax = key[j];
        }
    }
    // (a lane without a valid needle holds kmin = all ones, kmax = 0: it changes neither; every tile has a valid needle)
#pragma unroll
    for (int w = WAVE / 2; w > 0; w >>= 1) {
        const K a = pairs_shfl_xor<K>(kmin, w), b = pairs_shfl_xor<K>(kmax, w);
        if (a < kmin) kmin = a;
        if (kmax < b) kmax = b;
    }
    const uint32_t wave = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        s_min[wave] = kmin;
        s_max[wave] = kmax;
    }
    __syncthreads();
    // b. the window: wave 0 the lower bound of kmin, wave 1 the upper bound of kmax
    if (wave < 2) {
        K k = wave == 0 ? s_min[0] : s_max[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            if (wave == 0) {
                if (s_min[w] < k) k = s_min[w];
            } else {
                if (k < s_max[w]) k = s_max[w];
            }
        }
        const uint64_t r = wave == 0 ? search_wave_bound<KB, false>(sorted, N, k, kind, desc) : search_wave_bound<KB, true>(sorted, N, k, kind, desc);
        if ((threadIdx.x & (WAVE - 1)) == 0) s_bound[wave] = r;
    }
    __syncthreads();
    const uint64_t lo = s_bound[0];
    const uint64_t hi = s_bound[1] < lo ? lo : s_bound[1];  // an unsorted haystack: the end is clamped, not trusted
    const uint64_t cnt = hi - lo;
    if constexpr (POS) {
#pragma unroll
        for (int j = 0; j < IPT; ++j) valid[j] = valid[j] && o[j] < m;  // (a position from outside the call is not stored)
    }
    // c, d. the searches and the stores, G needles in step
    if (cnt <= (uint64_t)WINDOW) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)cnt; i += SEARCH_WG) s_win[i] = search_hay<KB>(sorted, lo + i, kind, desc);
        __syncthreads();
        const auto at = [&](uint32_t i) -> K { return s_win[i]; };
#pragma unroll
        for (int g0 = 0; g0 < IPT; g0 += G) search_group<K, G, I, uint32_t>(at, (uint32_t)cnt, lo, key + g0, o + g0, valid + g0, out_lower, out_upper);
    } else {
        const auto at = [&](uint64_t i) -> K { return search_hay<KB>(sorted, lo + i, kind, desc); };
#pragma unroll
        for (int g0 = 0; g0 < IPT; g0 += G) search_group<K, G, I, uint64_t>(at, cnt, lo, key + g0, o + g0, valid + g0, out_lower, out_upper);
    }
}

}  // namespace rsx
