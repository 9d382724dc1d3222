// rsx_pairs_kernels.hpp -- the kernels that let SEPARATE key and value arrays reach the sort kernels (rsx.hip,
// pairs_locked): rsx_sort_pairs_device and rsx_argsort_device sort joined (mapped key, value) elements in the context's
// workspace.
//   rsx_pairs_join_kernel   keys[i], values[i] -> element i: the key MAPPED to its order-preserving unsigned form
//                           (radix_digits.rs: sign flip, float total order) and, for descending order, complemented, at
//                           offset 0; the value behind it at pairs_voff; padding zero.  GEN: the value is the element's
//                           position (argsort, proxies) and no value column is read.
//   rsx_pairs_split_kernel  element i -> keys[i] (complement and mapping undone), values[i]; or the keys alone; or the
//                           position alone, widened to the caller's index type.
// Both are typed on the key and value widths (1, 2, 4, 8, 16 bytes; the element size follows from the two) and move
// whole words: a thread handles pairs_vec consecutive elements so that its part of every column and of the element
// array is one run of up to 16 bytes per load or store (elements below 16 bytes), or whole 16-byte words of a 48-byte
// run (12- and 24-byte elements).  Adjacent lanes hold adjacent runs: every access of a wave is one contiguous range.
// The host takes this form when all base addresses are 16-byte aligned; the partial last group goes element by element.
//   rsx_pairs_join_any_kernel / rsx_pairs_split_any_kernel  the same for value widths without a typed instance (3, 12,
//                           20 ... bytes) and for arrays that are only naturally aligned: one thread per element, the
//                           value moved in dwords or bytes.
// No kernel reads or writes outside the n keys, n values (indices) and n elements.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsx {

constexpr uint32_t PAIRS_SIGNED = 1, PAIRS_FLOAT = 2;  // RSX_KEY_SIGNED, RSX_KEY_FLOAT
enum : uint32_t { PAIRS_SPLIT_BOTH = 0, PAIRS_SPLIT_KEYS = 1, PAIRS_SPLIT_INDEX = 2 };

// the value's offset in the joined element: behind the key, aligned to the value's own alignment (at most 4)
constexpr uint32_t pairs_voff(uint32_t kb, uint32_t vb) {
    const uint32_t a = vb == 0 ? 1u : vb % 4 == 0 ? 4u : vb % 2 == 0 ? 2u : 1u;
    return (kb + a - 1) / a * a;
}
// the joined element's size: the smallest size with sort kernels that holds both and is a multiple of the key width
// (0: none, the pair goes by proxies)
constexpr uint32_t pairs_elem(uint32_t kb, uint32_t vb) {
    const uint32_t need = pairs_voff(kb, vb) + vb;
    const uint32_t sizes[8] = {1, 2, 4, 8, 12, 16, 24, 32};
    for (uint32_t i = 0; i < 8; ++i)
        if (sizes[i] >= need && sizes[i] % kb == 0) return sizes[i];
    return 0;
}
// elements per thread of the typed kernels
constexpr uint32_t pairs_vec(uint32_t e) { return e == 12 ? 4u : e == 24 ? 2u : e < 16 ? 16u / e : 1u; }

template <int W> struct PairsWord;
template <> struct PairsWord<1> { using type = uint8_t; };
template <> struct PairsWord<2> { using type = uint16_t; };
template <> struct PairsWord<4> { using type = uint32_t; };
template <> struct PairsWord<8> { using type = uint2; };
template <> struct PairsWord<16> { using type = uint4; };
constexpr int pairs_word(int nbytes) { return nbytes % 16 == 0 ? 16 : nbytes % 8 == 0 ? 8 : nbytes % 4 == 0 ? 4 : nbytes % 2 == 0 ? 2 : 1; }

// N bytes at p (aligned to pairs_word(N)) <-> registers, in the widest words that divide N
template <int N>
__device__ __forceinline__ void pairs_load(unsigned char* r, const uint8_t* __restrict__ p) {
    constexpr int W = pairs_word(N);
    using T = typename PairsWord<W>::type;
#pragma unroll
    for (int i = 0; i < N / W; ++i) {
        const T w = reinterpret_cast<const T*>(p)[i];
        __builtin_memcpy(r + i * W, &w, W);
    }
}
template <int N>
__device__ __forceinline__ void pairs_store(uint8_t* __restrict__ p, const unsigned char* r) {
    constexpr int W = pairs_word(N);
    using T = typename PairsWord<W>::type;
#pragma unroll
    for (int i = 0; i < N / W; ++i) {
        T w;
        __builtin_memcpy(&w, r + i * W, W);
        reinterpret_cast<T*>(p)[i] = w;
    }
}

struct PairsU128 {
    uint64_t lo, hi;
};
__device__ __forceinline__ bool operator!=(const PairsU128& a, const PairsU128& b) { return a.lo != b.lo || a.hi != b.hi; }
__device__ __forceinline__ bool operator<(const PairsU128& a, const PairsU128& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
template <int KB> struct PairsKey;
template <> struct PairsKey<1> { using type = uint8_t; };
template <> struct PairsKey<2> { using type = uint16_t; };
template <> struct PairsKey<4> { using type = uint32_t; };
template <> struct PairsKey<8> { using type = uint64_t; };
template <> struct PairsKey<16> { using type = PairsU128; };

// radix_digits.rs:55-124 on the whole key: signed x ^ MIN; float: negative -> all bits flipped, else the sign bit
template <typename K>
__device__ __forceinline__ K pairs_map(K k, uint32_t kind, uint32_t desc) {
    constexpr K MIN = (K)((K)1 << (8 * sizeof(K) - 1));
    if (kind == PAIRS_SIGNED) k = (K)(k ^ MIN);
    else if (kind == PAIRS_FLOAT) k = (K)(k ^ ((k & MIN) ? (K)~(K)0 : MIN));
    return desc ? (K)~k : k;
}
template <typename K>
__device__ __forceinline__ K pairs_unmap(K k, uint32_t kind, uint32_t desc) {
    constexpr K MIN = (K)((K)1 << (8 * sizeof(K) - 1));
    if (desc) k = (K)~k;
    if (kind == PAIRS_SIGNED) k = (K)(k ^ MIN);
    else if (kind == PAIRS_FLOAT) k = (K)(k ^ ((k & MIN) ? MIN : (K)~(K)0));
    return k;
}
template <>
__device__ __forceinline__ PairsU128 pairs_map<PairsU128>(PairsU128 k, uint32_t kind, uint32_t desc) {
    if (kind == PAIRS_SIGNED) k.hi ^= 1ull << 63;
    if (desc) {
        k.lo = ~k.lo;
        k.hi = ~k.hi;
    }
    return k;
}
template <>
__device__ __forceinline__ PairsU128 pairs_unmap<PairsU128>(PairsU128 k, uint32_t kind, uint32_t desc) {
    if (desc) {
        k.lo = ~k.lo;
        k.hi = ~k.hi;
    }
    if (kind == PAIRS_SIGNED) k.hi ^= 1ull << 63;
    return k;
}

// A wave shuffle of a key or value of any width up to 16 bytes (an integer or PairsU128): 32-bit words, each on its own
template <typename T, typename F>
__device__ __forceinline__ T pairs_shfl(T x, F&& word) {
    if constexpr (sizeof(T) <= 4) {
        return (T)word((uint32_t)x);
    } else {
        uint32_t w[sizeof(T) / 4];
        __builtin_memcpy(w, &x, sizeof(T));
#pragma unroll
        for (int i = 0; i < (int)(sizeof(T) / 4); ++i) w[i] = word(w[i]);
        __builtin_memcpy(&x, w, sizeof(T));
        return x;
    }
}
template <typename T>
__device__ __forceinline__ T pairs_shfl_up(T x, int o) {
    return pairs_shfl(x, [o](uint32_t w) { return (uint32_t)__shfl_up(w, o); });
}
template <typename T>
__device__ __forceinline__ T pairs_shfl_xor(T x, int o) {
    return pairs_shfl(x, [o](uint32_t w) { return (uint32_t)__shfl_xor(w, o); });
}

// V consecutive elements from e0 on
template <int KB, int VB, bool GEN, int V>
__device__ __forceinline__ void pairs_join_group(const uint8_t* __restrict__ keys, const uint8_t* __restrict__ values,
                                                 uint8_t* __restrict__ elems, uint64_t e0, uint32_t kind, uint32_t desc) {
    constexpr int E = (int)pairs_elem(KB, VB), VOFF = (int)pairs_voff(KB, VB);
    using K = typename PairsKey<KB>::type;
    unsigned char kr[KB * V];
    unsigned char vr[VB > 0 ? VB * V : 1];
    unsigned char er[E * V];
    pairs_load<KB * V>(kr, keys + e0 * KB);
    if constexpr (VB > 0 && !GEN) pairs_load<VB * V>(vr, values + e0 * VB);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        K k;
        __builtin_memcpy(&k, kr + j * KB, KB);
        k = pairs_map<K>(k, kind, desc);
        __builtin_memcpy(er + j * E, &k, KB);
#pragma unroll
        for (int b = KB; b < VOFF; ++b) er[j * E + b] = 0;
        if constexpr (GEN) {
            const uint64_t pos = e0 + (uint64_t)j;
            __builtin_memcpy(er + j * E + VOFF, &pos, VB);  // (little-endian: the low VB bytes)
        } else if constexpr (VB > 0) {
            __builtin_memcpy(er + j * E + VOFF, vr + j * VB, VB);
        }
#pragma unroll
        for (int b = VOFF + VB; b < E; ++b) er[j * E + b] = 0;
    }
    pairs_store<E * V>(elems + e0 * E, er);
}

template <int KB, int VB, bool GEN>
__global__ __launch_bounds__(256) void rsx_pairs_join_kernel(const uint8_t* __restrict__ keys, const uint8_t* __restrict__ values,
                                                             uint8_t* __restrict__ elems, uint64_t n, uint32_t kind, uint32_t desc) {
    constexpr int VEC = (int)pairs_vec(pairs_elem(KB, VB));
    const uint64_t e0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e0 >= n) return;
    if (e0 + VEC <= n) {
        pairs_join_group<KB, VB, GEN, VEC>(keys, values, elems, e0, kind, desc);
    } else {
        for (uint64_t e = e0; e < n; ++e) pairs_join_group<KB, VB, GEN, 1>(keys, values, elems, e, kind, desc);
    }
}

// MODE PAIRS_SPLIT_INDEX: the element's VB-byte position is written as IB bytes (IB >= VB); IB is unused otherwise
template <int KB, int VB, int MODE, int IB, int V>
__device__ __forceinline__ void pairs_split_group(const uint8_t* __restrict__ elems, uint8_t* __restrict__ keys,
                                                  uint8_t* __restrict__ values, uint64_t e0, uint32_t kind, uint32_t desc) {
    constexpr int E = (int)pairs_elem(KB, VB), VOFF = (int)pairs_voff(KB, VB);
    using K = typename PairsKey<KB>::type;
    unsigned char er[E * V];
    pairs_load<E * V>(er, elems + e0 * E);
    if constexpr (MODE != PAIRS_SPLIT_INDEX) {
        unsigned char kr[KB * V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            K k;
            __builtin_memcpy(&k, er + j * E, KB);
            k = pairs_unmap<K>(k, kind, desc);
            __builtin_memcpy(kr + j * KB, &k, KB);
        }
        pairs_store<KB * V>(keys + e0 * KB, kr);
    }
    if constexpr (MODE == PAIRS_SPLIT_BOTH && VB > 0) {
        unsigned char vr[VB * V];
#pragma unroll
        for (int j = 0; j < V; ++j) __builtin_memcpy(vr + j * VB, er + j * E + VOFF, VB);
        pairs_store<VB * V>(values + e0 * VB, vr);
    }
    if constexpr (MODE == PAIRS_SPLIT_INDEX) {
        unsigned char ir[IB * V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            uint64_t pos = 0;
            __builtin_memcpy(&pos, er + j * E + VOFF, VB);
            __builtin_memcpy(ir + j * IB, &pos, IB);
        }
        pairs_store<IB * V>(values + e0 * IB, ir);
    }
}

template <int KB, int VB, int MODE, int IB>
__global__ __launch_bounds__(256) void rsx_pairs_split_kernel(const uint8_t* __restrict__ elems, uint8_t* __restrict__ keys,
                                                              uint8_t* __restrict__ values, uint64_t n, uint32_t kind, uint32_t desc) {
    constexpr int VEC = (int)pairs_vec(pairs_elem(KB, VB));
    const uint64_t e0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e0 >= n) return;
    if (e0 + VEC <= n) {
        pairs_split_group<KB, VB, MODE, IB, VEC>(elems, keys, values, e0, kind, desc);
    } else {
        for (uint64_t e = e0; e < n; ++e) pairs_split_group<KB, VB, MODE, IB, 1>(elems, keys, values, e, kind, desc);
    }
}

// ---- any value width, natural alignment: one thread per element, the value in words of W (1 or 4 bytes) ----
// values == nullptr: the value is the element's position (vb 4 or 8, W = uint32_t)
template <int KB, typename W>
__global__ __launch_bounds__(256) void rsx_pairs_join_any_kernel(const uint8_t* __restrict__ keys, const uint8_t* __restrict__ values,
                                                                 uint8_t* __restrict__ elems, uint64_t n, uint32_t vb, uint32_t voff,
                                                                 uint32_t es, uint32_t kind, uint32_t desc) {
    using K = typename PairsKey<KB>::type;
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    uint8_t* d = elems + e * es;
    *reinterpret_cast<K*>(d) = pairs_map<K>(reinterpret_cast<const K*>(keys)[e], kind, desc);
    for (uint32_t b = KB; b < voff; ++b) d[b] = 0;
    W* dv = reinterpret_cast<W*>(d + voff);
    const uint32_t words = vb / (uint32_t)sizeof(W);
    if (values) {
        const W* sv = reinterpret_cast<const W*>(values + e * vb);
        for (uint32_t j = 0; j < words; ++j) dv[j] = sv[j];
    } else {
        for (uint32_t j = 0; j < words; ++j) dv[j] = (W)(e >> (8 * (uint32_t)sizeof(W) * j));
    }
    for (uint32_t b = voff + vb; b < es; ++b) d[b] = 0;
}

// mode PAIRS_SPLIT_INDEX: `values` receives the position as ib bytes (W = uint32_t)
template <int KB, typename W>
__global__ __launch_bounds__(256) void rsx_pairs_split_any_kernel(const uint8_t* __restrict__ elems, uint8_t* __restrict__ keys,
                                                                  uint8_t* __restrict__ values, uint64_t n, uint32_t vb, uint32_t voff,
                                                                  uint32_t es, uint32_t mode, uint32_t ib, uint32_t kind, uint32_t desc) {
    using K = typename PairsKey<KB>::type;
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint8_t* s = elems + e * es;
    if (mode != PAIRS_SPLIT_INDEX) reinterpret_cast<K*>(keys)[e] = pairs_unmap<K>(*reinterpret_cast<const K*>(s), kind, desc);
    const W* sv = reinterpret_cast<const W*>(s + voff);
    if (mode == PAIRS_SPLIT_BOTH) {
        W* dv = reinterpret_cast<W*>(values + e * vb);
        const uint32_t words = vb / (uint32_t)sizeof(W);
        for (uint32_t j = 0; j < words; ++j) dv[j] = sv[j];
    } else if (mode == PAIRS_SPLIT_INDEX) {
        W* dv = reinterpret_cast<W*>(values + e * ib);
        const uint32_t have = vb / (uint32_t)sizeof(W), want = ib / (uint32_t)sizeof(W);
        for (uint32_t j = 0; j < want; ++j) dv[j] = j < have ? sv[j] : (W)0;
    }
}

}  // namespace rsx
