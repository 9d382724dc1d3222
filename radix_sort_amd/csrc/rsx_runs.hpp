// rsx_runs.hpp -- what the run kernels of rsx_unique_kernels.hpp and rsx_reduce_kernels.hpp have in common: a thread's
// share of a tile, the head flags of its elements and the write-out of its heads.  The input is the sorted array of n
// joined elements (rsx_pairs_kernels.hpp), the mapped key at offset 0; element i is a HEAD when i == 0 or its mapped key
// differs from that of element i - 1.  Templates and constexpr only: any translation unit may include it.
#pragma once

#include "rsx_device.hpp"
#include "rsx_pairs_kernels.hpp"

namespace rsx {

// this thread's first element and how many of the tile's it holds (0: none, behind the end of the array); a tile is
// WG threads of IPT consecutive elements each
template <uint32_t WG, int IPT>
__device__ __forceinline__ uint32_t runs_share(uint64_t n, uint64_t* e0) {
    *e0 = ((uint64_t)blockIdx.x * WG + threadIdx.x) * IPT;
    if (*e0 >= n) return 0;
    const uint64_t left = n - *e0;
    return left < (uint64_t)IPT ? (uint32_t)left : (uint32_t)IPT;
}

// One thread's elements [e0, e0 + cnt) into `er` (cnt <= IPT; the whole run in 16-byte words when cnt == IPT, zeros behind
// cnt) and its head flags: bit j set when element e0 + j is a head.  The key in front of e0 comes from global memory (a
// line the neighbouring thread loads anyway); element 0 has none.
template <int KB, int E, int IPT>
__device__ __forceinline__ uint32_t runs_flags(const uint8_t* __restrict__ elems, uint64_t e0, uint32_t cnt, unsigned char* er) {
    using K = typename PairsKey<KB>::type;
    if (cnt == (uint32_t)IPT) {
        pairs_load<E * IPT>(er, elems + e0 * E);
    } else {
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            if ((uint32_t)j < cnt) pairs_load<E>(er + j * E, elems + (e0 + (uint64_t)j) * E);
            else __builtin_memset(er + j * E, 0, E);
        }
    }
    K prev{};
    if (cnt != 0 && e0 != 0) {
        unsigned char pr[KB];
        pairs_load<KB>(pr, elems + (e0 - 1) * E);
        __builtin_memcpy(&prev, pr, KB);
    }
    uint32_t flags = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        K k;
        __builtin_memcpy(&k, er + j * E, KB);
        const bool head = (j == 0 && e0 == 0) || k != prev;
        if ((uint32_t)j < cnt && head) flags |= 1u << j;
        prev = k;
    }
    return flags;
}

// The heads among one thread's elements (`er` and `flags` of runs_flags; `first`: the heads in front of element e0): a
// head of rank r at e0 + j writes out_keys[r] (mapping undone) and out_offsets[r] = e0 + j.  Either output may be null.
template <int KB, int E, int IPT>
__device__ __forceinline__ void runs_write_heads(const unsigned char* er, uint32_t flags, uint64_t first, uint64_t e0,
                                                 uint8_t* __restrict__ out_keys, uint64_t* __restrict__ out_offsets, uint32_t kind,
                                                 uint32_t desc) {
    using K = typename PairsKey<KB>::type;
    if (!out_keys && !out_offsets) return;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        if (!(flags >> j & 1u)) continue;
        const uint64_t r = first + (uint32_t)__popc(flags & ((1u << j) - 1u));
        if (out_keys) {
            K k;
            __builtin_memcpy(&k, er + j * E, KB);
            k = pairs_unmap<K>(k, kind, desc);
            unsigned char kr[KB];
            __builtin_memcpy(kr, &k, KB);
            pairs_store<KB>(out_keys + r * KB, kr);
        }
        if (out_offsets) out_offsets[r] = e0 + (uint64_t)j;
    }
}

}  // namespace rsx
