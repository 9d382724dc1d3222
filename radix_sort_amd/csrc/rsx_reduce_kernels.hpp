// rsx_reduce_kernels.hpp -- the run kernels behind rsx_reduce_by_key_device (rsx.hip; launched by rsx_reduce.hip): what
// follows the sort of the joined (mapped key, value) elements (rsx_pairs_kernels.hpp) when the caller wants ONE value per
// group of equal keys: the sum, minimum or maximum of the group's values.  Heads are those of rsx_unique_kernels.hpp
// (element i is a HEAD when i == 0 or its mapped key differs from that of element i - 1), found and written out by the
// helpers the two sets of run kernels share (rsx_runs.hpp).  Three launches, tiled alike
// (reduce_tile elements per workgroup of 256 threads, every thread reduce_ipt CONSECUTIVE elements: one run of 64
// bytes, or 48 for the 12- and 24-byte elements, loaded in 16-byte words):
//   rsx_reduce_count_kernel  tile t -> tile_heads[t], the heads among its elements, and tile_tail[t], the (+) of its
//                            elements from its last head to its end (of the whole tile when it holds no head)
//   rsx_reduce_scan_kernel   ONE workgroup: tile_base[t] = heads in front of tile t, tile_carry[t] = the (+) of the open
//                            run's elements in front of tile t -- an exclusive SEGMENTED scan of the tails, a tile with a
//                            head cuts the chain (REDUCE_SCAN_SPAN tiles per sweep of its loop, the head count and the
//                            open run's value carried from sweep to sweep); writes out_num[0] = m and out_offsets[m] = n
//   rsx_reduce_write_kernel  the flags again and an inclusive segmented scan of the values in position order (in the
//                            thread, then per wave, then the waves' totals through LDS): a head of rank r at i writes
//                            out_keys[r] (mapping undone) and out_offsets[r] = i; the LAST element of a run (its
//                            successor is a head, or it is element n - 1) writes out_values[rank of its run]: its
//                            inclusive value, with tile_carry[t] on its left when the run began in front of the tile.
// The value of a run is therefore ((carry (+) in front of the thread) (+) in the thread): an association fixed by the
// tiling, that is by (n, key width, value width, the run's start and length) alone -- no atomics, the same bytes on
// every call.  No identity element is ever combined (a group of -0.0 sums to -0.0): a scan item carries a VALID bit
// instead.  The operator is a uniform run-time argument.  No workgroup waits for another one: the three launches are the
// only ordering.  The partial last tile goes element by element.  No kernel reads outside the n elements or writes
// outside tile_heads / tile_base / tile_tail / tile_carry [tiles], out_keys [m], out_values [m], out_offsets [m + 1] and
// out_num [1].
#pragma once

#include "rsx_runs.hpp"

namespace rsx {

constexpr uint32_t REDUCE_WG = 256;
constexpr uint32_t REDUCE_SCAN_WG = 512;
constexpr uint32_t REDUCE_SCAN_SPAN = REDUCE_SCAN_WG;  // tiles per sweep of the scan kernel: one per thread
enum : uint32_t { REDUCE_SUM = 0, REDUCE_MIN = 1, REDUCE_MAX = 2 };  // RSX_REDUCE_*
// the joined element: (mapped key, value of 4 or 8 bytes)
constexpr uint32_t reduce_elem(uint32_t kb, uint32_t vb) { return pairs_elem(kb, vb); }
// elements per thread: whole 16-byte words -- 64 bytes of elements, 48 where the element is 12 or 24 bytes
constexpr uint32_t reduce_ipt(uint32_t e) { return e == 12 ? 4u : e == 24 ? 2u : e <= 4 ? 16u : 64u / e; }
constexpr uint32_t reduce_tile(uint32_t e) { return REDUCE_WG * reduce_ipt(e); }

// A value type: VB bytes of kind VK (0 unsigned, PAIRS_SIGNED, PAIRS_FLOAT), held as its bit pattern.
template <int VB, int VK>
struct ReduceVal {
    using U = typename std::conditional<VB == 4, uint32_t, uint64_t>::type;
    using F = typename std::conditional<VB == 4, float, double>::type;
    static constexpr U MIN = (U)((U)1 << (8 * VB - 1));
    // the order-preserving map to unsigned: sign flip, float total order on bit patterns
    static __device__ __forceinline__ U ord(U x) {
        if constexpr (VK == (int)PAIRS_SIGNED) return (U)(x ^ MIN);
        else if constexpr (VK == (int)PAIRS_FLOAT) return (U)(x ^ ((x & MIN) ? (U) ~(U)0 : MIN));
        else return x;
    }
    // a (+) b, a on the left
    static __device__ __forceinline__ U combine(U a, U b, uint32_t op) {
        if (op == REDUCE_SUM) {
            if constexpr (VK == (int)PAIRS_FLOAT) {
                F fa, fb;
                __builtin_memcpy(&fa, &a, VB);
                __builtin_memcpy(&fb, &b, VB);
                const F fs = fa + fb;
                U s;
                __builtin_memcpy(&s, &fs, VB);
                return s;
            } else {
                return (U)(a + b);  // wraps
            }
        }
        const bool a_less = ord(a) < ord(b);
        return (op == REDUCE_MIN) == a_less ? a : b;
    }
};

// One item of a segmented scan: the (+) of a stretch of elements from its last head on (of all of it when it holds no
// head).  f: bit 0 the stretch holds a head, bit 1 the item is valid (an invalid item is the identity).
constexpr uint32_t REDUCE_HEAD = 1, REDUCE_VALID = 2;
template <typename U>
struct ReduceItem {
    U v;
    uint32_t f;
};
// l in front of r
template <typename RV, typename U>
__device__ __forceinline__ ReduceItem<U> reduce_join(const ReduceItem<U>& l, const ReduceItem<U>& r, uint32_t op) {
    if (!(r.f & REDUCE_VALID)) return l;
    if (!(l.f & REDUCE_VALID)) return r;
    ReduceItem<U> o;
    o.v = (r.f & REDUCE_HEAD) ? r.v : RV::combine(l.v, r.v, op);
    o.f = l.f | r.f;
    return o;
}
// inclusive segmented scan over the 64 lanes of a wave
template <typename RV, typename U>
__device__ __forceinline__ ReduceItem<U> reduce_wave_scan(ReduceItem<U> x, uint32_t op) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
#pragma unroll
    for (int o = 1; o < (int)WAVE; o <<= 1) {
        ReduceItem<U> y;
        y.v = pairs_shfl_up<U>(x.v, o);
        y.f = __shfl_up(x.f, o);
        if (lane >= (uint32_t)o) x = reduce_join<RV, U>(y, x, op);
    }
    return x;
}

// The values of one thread's elements and their inclusive segmented scan inside the thread: s[j] = the (+) of the
// elements from the last head at or in front of j (from the thread's first element when there is none) to j.  Returns the
// thread's item.
template <typename RV, int E, int IPT, int VOFF, typename U>
__device__ __forceinline__ ReduceItem<U> reduce_thread_scan(const unsigned char* er, uint32_t flags, uint32_t cnt, uint32_t op, U* s) {
    ReduceItem<U> it;
    it.v = 0;
    it.f = cnt != 0 ? (REDUCE_VALID | (flags != 0 ? REDUCE_HEAD : 0u)) : 0u;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        U v;
        __builtin_memcpy(&v, er + j * E + VOFF, sizeof(U));
        if (j == 0) s[0] = v;
        else s[j] = (flags >> j & 1u) ? v : RV::combine(s[j - 1], v, op);
        if ((uint32_t)j < cnt) it.v = s[j];
    }
    return it;
}

template <int KB, int VB, int VK>
__global__ __launch_bounds__(REDUCE_WG) void rsx_reduce_count_kernel(const uint8_t* __restrict__ elems, uint64_t n, uint32_t op,
                                                                     uint32_t* __restrict__ tile_heads, uint64_t* __restrict__ tile_tail) {
    constexpr int E = (int)reduce_elem(KB, VB), IPT = (int)reduce_ipt(E), VOFF = (int)pairs_voff(KB, VB);
    constexpr int NW = (int)(REDUCE_WG / WAVE);
    using RV = ReduceVal<VB, VK>;
    using U = typename RV::U;
    __shared__ uint32_t s_wave[NW];
    __shared__ U s_v[NW];
    __shared__ uint32_t s_f[NW];
    uint64_t e0;
    const uint32_t cnt = runs_share<REDUCE_WG, IPT>(n, &e0);
    unsigned char er[E * IPT];
    const uint32_t flags = runs_flags<KB, E, IPT>(elems, e0, cnt, er);
    U s[IPT];
    const ReduceItem<U> mine = reduce_thread_scan<RV, E, IPT, VOFF, U>(er, flags, cnt, op, s);
    const uint32_t incl = wave_incl_scan<false>((uint32_t)__popc(flags));
    const ReduceItem<U> wi = reduce_wave_scan<RV, U>(mine, op);
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) {
        s_wave[threadIdx.x / WAVE] = incl;
        s_v[threadIdx.x / WAVE] = wi.v;
        s_f[threadIdx.x / WAVE] = wi.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        ReduceItem<U> acc{0, 0};
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            total += s_wave[w];
            acc = reduce_join<RV, U>(acc, ReduceItem<U>{s_v[w], s_f[w]}, op);
        }
        tile_heads[blockIdx.x] = total;
        tile_tail[blockIdx.x] = (uint64_t)acc.v;  // (the tile holds an element: valid)
    }
}

// out_offsets may be null
template <int VB, int VK>
__global__ __launch_bounds__(REDUCE_SCAN_WG) void rsx_reduce_scan_kernel(const uint32_t* __restrict__ tile_heads, const uint64_t* __restrict__ tile_tail,
                                                                         uint64_t* __restrict__ tile_base, uint64_t* __restrict__ tile_carry,
                                                                         uint64_t tiles, uint64_t n, uint32_t op, uint64_t* __restrict__ out_num,
                                                                         uint64_t* __restrict__ out_offsets) {
    constexpr int NW = (int)(REDUCE_SCAN_WG / WAVE);
    using RV = ReduceVal<VB, VK>;
    using U = typename RV::U;
    __shared__ uint32_t s_wave[NW];
    __shared__ U s_v[NW];
    __shared__ uint32_t s_f[NW];
    const uint32_t wave = threadIdx.x / WAVE;
    uint64_t carry = 0;          // heads in front of this sweep
    ReduceItem<U> open{0, 0};    // the open run in front of this sweep
    for (uint64_t t0 = 0; t0 < tiles; t0 += REDUCE_SCAN_SPAN) {
        const uint64_t t = t0 + threadIdx.x;
        const uint32_t c = t < tiles ? tile_heads[t] : 0u;
        ReduceItem<U> mine{0, 0};
        if (t < tiles) {
            mine.v = (U)tile_tail[t];
            mine.f = REDUCE_VALID | (c != 0 ? REDUCE_HEAD : 0u);
        }
        const uint32_t incl = wave_incl_scan<false>(c);  // (a sweep's sum is below 2^32: 512 tiles of at most 4096 heads)
        const ReduceItem<U> wi = reduce_wave_scan<RV, U>(mine, op);
        if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) {
            s_wave[wave] = incl;
            s_v[wave] = wi.v;
            s_f[wave] = wi.f;
        }
        __syncthreads();
        uint32_t below = 0, total = 0;
        ReduceItem<U> front = open, all = open;  // in front of this wave; up to the end of the sweep
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const uint32_t v = s_wave[w];
            const ReduceItem<U> wv{s_v[w], s_f[w]};
            below += (uint32_t)w < wave ? v : 0u;
            total += v;
            if ((uint32_t)w < wave) front = reduce_join<RV, U>(front, wv, op);
            all = reduce_join<RV, U>(all, wv, op);
        }
        // the lanes in front of this one: the wave's inclusive scan of the lane before
        ReduceItem<U> lanes;
        lanes.v = pairs_shfl_up<U>(wi.v, 1);
        lanes.f = __shfl_up(wi.f, 1);
        if ((threadIdx.x & (WAVE - 1)) == 0) lanes.f = 0;
        front = reduce_join<RV, U>(front, lanes, op);
        if (t < tiles) {
            tile_base[t] = carry + below + (incl - c);
            tile_carry[t] = (front.f & REDUCE_VALID) ? (uint64_t)front.v : 0ull;  // (tile 0 has nothing in front: never read)
        }
        carry += total;
        open = all;
        __syncthreads();  // the LDS arrays are written again by the next sweep
    }
    if (threadIdx.x == 0) {
        out_num[0] = carry;
        if (out_offsets) out_offsets[carry] = n;
    }
}

// out_keys, out_values and out_offsets may each be null (a uniform branch each)
template <int KB, int VB, int VK>
__global__ __launch_bounds__(REDUCE_WG) void rsx_reduce_write_kernel(const uint8_t* __restrict__ elems, uint64_t n, uint32_t op,
                                                                     const uint64_t* __restrict__ tile_base, const uint64_t* __restrict__ tile_carry,
                                                                     uint8_t* __restrict__ out_keys, uint8_t* __restrict__ out_values,
                                                                     uint64_t* __restrict__ out_offsets, uint32_t kind, uint32_t desc) {
    constexpr int E = (int)reduce_elem(KB, VB), IPT = (int)reduce_ipt(E), VOFF = (int)pairs_voff(KB, VB);
    constexpr int NW = (int)(REDUCE_WG / WAVE);
    using K = typename PairsKey<KB>::type;
    using RV = ReduceVal<VB, VK>;
    using U = typename RV::U;
    __shared__ uint32_t s_wave[NW];
    __shared__ U s_v[NW];
    __shared__ uint32_t s_f[NW];
    uint64_t e0;
    const uint32_t cnt = runs_share<REDUCE_WG, IPT>(n, &e0);
    unsigned char er[E * IPT];
    const uint32_t flags = runs_flags<KB, E, IPT>(elems, e0, cnt, er);
    // bit j: element e0 + j is the last of its run.  Inside the thread that is the next flag; behind the thread's last
    // element it is the successor's key in global memory (a line the neighbouring thread loads anyway), or the array's end.
    uint32_t lasts = flags >> 1;
    if (cnt != 0) {
        bool end = true;
        if (e0 + cnt < n) {  // (then cnt == IPT)
            unsigned char nr[KB];
            pairs_load<KB>(nr, elems + (e0 + cnt) * E);
            K nk, lk;
            __builtin_memcpy(&nk, nr, KB);
            __builtin_memcpy(&lk, er + (IPT - 1) * E, KB);
            end = nk != lk;
        }
        if (end) lasts |= 1u << (cnt - 1);
    }
    U s[IPT];
    const ReduceItem<U> mine = reduce_thread_scan<RV, E, IPT, VOFF, U>(er, flags, cnt, op, s);
    const uint32_t heads = (uint32_t)__popc(flags);
    const uint32_t incl = wave_incl_scan<false>(heads);
    const ReduceItem<U> wi = reduce_wave_scan<RV, U>(mine, op);
    const uint32_t wave = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) {
        s_wave[wave] = incl;
        s_v[wave] = wi.v;
        s_f[wave] = wi.f;
    }
    __syncthreads();
    uint32_t below = 0;
    // what lies in front of this thread: the open run in front of the tile, the waves in front, the lanes in front
    ReduceItem<U> front{0, 0};
    if (blockIdx.x != 0 && out_values) {
        front.v = (U)tile_carry[blockIdx.x];
        front.f = REDUCE_VALID;
    }
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        below += (uint32_t)w < wave ? s_wave[w] : 0u;
        if ((uint32_t)w < wave) front = reduce_join<RV, U>(front, ReduceItem<U>{s_v[w], s_f[w]}, op);
    }
    ReduceItem<U> lanes;
    lanes.v = pairs_shfl_up<U>(wi.v, 1);
    lanes.f = __shfl_up(wi.f, 1);
    if ((threadIdx.x & (WAVE - 1)) == 0) lanes.f = 0;
    front = reduce_join<RV, U>(front, lanes, op);
    if (cnt == 0) return;
    const uint64_t first = tile_base[blockIdx.x] + below + (incl - heads);  // heads in front of element e0
    runs_write_heads<KB, E, IPT>(er, flags, first, e0, out_keys, out_offsets, kind, desc);
    if (out_values) {
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            if (!(lasts >> j & 1u) || (uint32_t)j >= cnt) continue;
            const uint32_t upto = flags & ((2u << j) - 1u);  // the thread's heads up to and including e0 + j
            U v = s[j];
            if (upto == 0 && (front.f & REDUCE_VALID)) v = RV::combine(front.v, v, op);  // the run began in front of the thread
            const uint64_t run = first + (uint32_t)__popc(upto) - 1u;                    // heads up to and including e0 + j, less one
            reinterpret_cast<U*>(out_values)[run] = v;
        }
    }
}

}  // namespace rsx
