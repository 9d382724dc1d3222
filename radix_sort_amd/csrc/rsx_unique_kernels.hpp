// rsx_unique_kernels.hpp -- the run kernels behind rsx_unique_device (rsx.hip; launched by rsx_unique.hip): what follows the sort of
// the joined elements (rsx_pairs_kernels.hpp) when the caller wants the GROUPS of equal keys instead of the sorted columns.
// The input is the sorted array of n joined elements in the context's workspace: the mapped key (complemented for
// descending order) at offset 0 and, on the route with positions, the element's u32 input position behind it.  Element i
// is a HEAD when i == 0 or its mapped key differs from that of element i - 1 (the mapping is a bijection: bit-pattern
// equality of the raw keys).  Three launches, tiled alike (unique_tile elements per workgroup of 256 threads, every thread
// unique_ipt CONSECUTIVE elements: one run of up to 64 bytes, loaded in 16-byte words):
//   rsx_unique_count_kernel  tile t -> tile_heads[t], the heads among its elements
//   rsx_unique_scan_kernel   ONE workgroup: tile_base[t] = heads in front of tile t (UNIQUE_SCAN_SPAN tiles per sweep of its
//                            loop, a running carry); writes out_num[0] = m and out_offsets[m] = n
//   rsx_unique_write_kernel  the flags again, ranked inside the workgroup (wave scan, then the waves' totals through LDS):
//                            a head of rank r at i writes out_keys[r] (mapping undone) and out_offsets[r] = i; every
//                            element writes out_perm[i] = its position and out_inverse[position] = the rank of its run.
// No workgroup waits for another one: the three launches are the only ordering ("Groups of equal
// keys", has the trade against a chained single-pass scan).  A thread's share of the tile, its head flags and the
// write-out of its heads are rsx_runs.hpp's, shared with rsx_reduce_kernels.hpp.  The partial last tile goes element by
// element.  No kernel reads outside the n elements or writes outside tile_heads / tile_base [tiles], out_keys [m],
// out_offsets [m + 1], out_perm [n], out_inverse [n] and out_num [1].
#pragma once

#include "rsx_runs.hpp"

namespace rsx {

constexpr uint32_t UNIQUE_WG = 256;
constexpr uint32_t UNIQUE_SCAN_WG = 512;
constexpr uint32_t UNIQUE_SCAN_SPAN = UNIQUE_SCAN_WG;  // tiles per sweep of the scan kernel: one per thread
// the joined element: the key alone, or (key, u32 position)
constexpr uint32_t unique_elem(uint32_t kb, bool pos) { return pairs_elem(kb, pos ? 4u : 0u); }
// elements per thread: 64 bytes of elements, at most 16 of them (the flags of a thread are bits of one word)
constexpr uint32_t unique_ipt(uint32_t e) { return e <= 4 ? 16u : 64u / e; }
constexpr uint32_t unique_tile(uint32_t e) { return UNIQUE_WG * unique_ipt(e); }

template <int KB, bool POS>
__global__ __launch_bounds__(UNIQUE_WG) void rsx_unique_count_kernel(const uint8_t* __restrict__ elems, uint64_t n,
                                                                     uint32_t* __restrict__ tile_heads) {
    constexpr int E = (int)unique_elem(KB, POS), IPT = (int)unique_ipt(E);
    __shared__ uint32_t s_wave[UNIQUE_WG / WAVE];
    uint64_t e0;
    const uint32_t cnt = runs_share<UNIQUE_WG, IPT>(n, &e0);
    unsigned char er[E * IPT];
    const uint32_t heads = (uint32_t)__popc(runs_flags<KB, E, IPT>(elems, e0, cnt, er));
    const uint32_t incl = wave_incl_scan<false>(heads);
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) s_wave[threadIdx.x / WAVE] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < (int)(UNIQUE_WG / WAVE); ++w) total += s_wave[w];
        tile_heads[blockIdx.x] = total;
    }
}

// out_offsets may be null
__global__ __launch_bounds__(UNIQUE_SCAN_WG) void rsx_unique_scan_kernel(const uint32_t* __restrict__ tile_heads, uint64_t* __restrict__ tile_base,
                                                                         uint64_t tiles, uint64_t n, uint64_t* __restrict__ out_num,
                                                                         uint64_t* __restrict__ out_offsets) {
    constexpr int NW = (int)(UNIQUE_SCAN_WG / WAVE);
    __shared__ uint32_t s_wave[NW];
    const uint32_t wave = threadIdx.x / WAVE;
    uint64_t carry = 0;
    uint32_t next = threadIdx.x < tiles ? tile_heads[threadIdx.x] : 0u;
    for (uint64_t t0 = 0; t0 < tiles; t0 += UNIQUE_SCAN_SPAN) {
        const uint64_t t = t0 + threadIdx.x;
        const uint32_t c = next;
        next = t + UNIQUE_SCAN_SPAN < tiles ? tile_heads[t + UNIQUE_SCAN_SPAN] : 0u;  // the next sweep's count, behind this sweep's work
        const uint32_t incl = wave_incl_scan<false>(c);  // (a sweep's sum is below 2^32: 512 tiles of at most 4096 heads)
        if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) s_wave[wave] = incl;
        __syncthreads();
        uint32_t below = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const uint32_t v = s_wave[w];
            below += (uint32_t)w < wave ? v : 0u;
            total += v;
        }
        if (t < tiles) tile_base[t] = carry + below + (incl - c);
        carry += total;
        __syncthreads();  // s_wave is written again by the next sweep
    }
    if (threadIdx.x == 0) {
        out_num[0] = carry;
        if (out_offsets) out_offsets[carry] = n;
    }
}

// IB: bytes of an index in out_perm / out_inverse (POS only).  Every output pointer may be null (a uniform branch each).
// perm_words: out_perm is 16-byte aligned, a thread's run of indices goes in 16-byte words.
template <int KB, bool POS, int IB>
__global__ __launch_bounds__(UNIQUE_WG) void rsx_unique_write_kernel(const uint8_t* __restrict__ elems, uint64_t n,
                                                                     const uint64_t* __restrict__ tile_base, uint8_t* __restrict__ out_keys,
                                                                     uint64_t* __restrict__ out_offsets, uint8_t* __restrict__ out_perm,
                                                                     uint8_t* __restrict__ out_inverse, uint32_t perm_words, uint32_t kind,
                                                                     uint32_t desc) {
    constexpr int E = (int)unique_elem(KB, POS), IPT = (int)unique_ipt(E), VOFF = (int)pairs_voff(KB, 4);
    using I = typename std::conditional<IB == 4, uint32_t, uint64_t>::type;
    constexpr int NW = (int)(UNIQUE_WG / WAVE);
    __shared__ uint32_t s_wave[NW];
    uint64_t e0;
    const uint32_t cnt = runs_share<UNIQUE_WG, IPT>(n, &e0);
    unsigned char er[E * IPT];
    const uint32_t flags = runs_flags<KB, E, IPT>(elems, e0, cnt, er);
    const uint32_t heads = (uint32_t)__popc(flags);
    const uint32_t incl = wave_incl_scan<false>(heads);
    const uint32_t wave = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    uint32_t below = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) below += (uint32_t)w < wave ? s_wave[w] : 0u;
    if (cnt == 0) return;
    const uint64_t first = tile_base[blockIdx.x] + below + (incl - heads);  // heads in front of element e0
    runs_write_heads<KB, E, IPT>(er, flags, first, e0, out_keys, out_offsets, kind, desc);
    if constexpr (POS) {
        if (out_perm) {
            if (perm_words && cnt == (uint32_t)IPT) {
                unsigned char ir[IB * IPT];
#pragma unroll
                for (int j = 0; j < IPT; ++j) {
                    uint32_t pos;
                    __builtin_memcpy(&pos, er + j * E + VOFF, 4);
                    const I wide = (I)pos;
                    __builtin_memcpy(ir + j * IB, &wide, IB);
                }
                pairs_store<IB * IPT>(out_perm + e0 * IB, ir);
            } else {
#pragma unroll
                for (int j = 0; j < IPT; ++j) {
                    uint32_t pos;
                    __builtin_memcpy(&pos, er + j * E + VOFF, 4);
                    if ((uint32_t)j < cnt) reinterpret_cast<I*>(out_perm)[e0 + (uint64_t)j] = (I)pos;
                }
            }
        }
        if (out_inverse) {  // a scatter by input position: the one uncoalesced stream of the call
#pragma unroll
            for (int j = 0; j < IPT; ++j) {
                uint32_t pos;
                __builtin_memcpy(&pos, er + j * E + VOFF, 4);
                const uint64_t run = first + (uint32_t)__popc(flags & ((2u << j) - 1u)) - 1u;  // heads up to and including e0 + j, less one
                if ((uint32_t)j < cnt && (uint64_t)pos < n) reinterpret_cast<I*>(out_inverse)[pos] = (I)run;
            }
        }
    }
}

}  // namespace rsx
