// rsx_lex_kernels.hpp -- the join behind rsx_lexsort_device and rsx_sort_columns_device (rsx.hip, lex_locked; launched
// by rsx_lex.hip): SEVERAL key columns, each of its own width, kind and direction, reach the sort kernels as ONE
// compound key.
//   rsx_lex_join_kernel<W, GATHER>  the columns of one round -> element i of pairs_elem(W, 4) bytes: every column's key
//       MAPPED as rsx_pairs_join_kernel maps it (pairs_map: sign flip, float total order, complement for a descending
//       column) and packed at its byte offset inside the W-byte compound key at offset 0 -- the round's most significant
//       column in the highest used bytes, little-endian, the unused top bytes zero -- with a u32 position behind it at
//       pairs_voff(W, 4); padding zero.
//       GATHER = false, the first round: element e is made of key e of every column and carries the position e.  A thread
//         makes pairs_vec consecutive elements; a column whose base is aligned for it gives them in one load of
//         kb * VEC bytes, any other column in VEC loads of kb bytes.
//       GATHER = true, every later round: output slot e takes the position q that the previous round's sorted element e
//         carries (elements of prev_es bytes, the position at prev_voff), loads key q of every column -- one kb-byte load
//         per column, uncoalesced by nature: q is the order the less significant columns gave -- and carries q on.  The
//         stable sort of these elements orders by this round's columns and keeps the previous order among equals.
// The columns travel by value in the kernel arguments (LexArgs): the loop over them and the switch on a column's width
// are wave-uniform.  The compound key is put together in registers as an integer (shift and or), never through a byte
// array indexed at run time, so nothing leaves the registers.  Elements are stored in whole words of up to 16 bytes,
// adjacent lanes adjacent elements.  The partial last group goes element by element, as in rsx_pairs_join_kernel: no
// load goes past the n keys of a column or the n previous elements, no store past the n elements.
#pragma once

#include "rsx_pairs_kernels.hpp"

namespace rsx {

constexpr uint32_t LEX_MAX_COLUMNS = 16;  // RSX_LEX_MAX_COLUMNS

struct LexColumn {
    const uint8_t* keys;  // n keys of kb bytes, aligned to kb
    uint32_t kb;          // 1, 2, 4, 8, 16
    uint32_t kind;        // RSX_KEY_*
    uint32_t desc;        // 1: complemented
    uint32_t off;         // byte offset of this column's key inside the compound key
    uint32_t wide;        // 1: keys is aligned to kb * VEC of the round's kernel (looked at by GATHER = false only)
    uint32_t pad;
};
struct LexArgs {
    LexColumn col[LEX_MAX_COLUMNS];
    uint32_t ncols;
    uint32_t pad;
};
static_assert(sizeof(LexColumn) == 32 && sizeof(LexArgs) == 32 * LEX_MAX_COLUMNS + 8, "LexArgs is laid out without holes");
static_assert(sizeof(LexArgs) + 64 <= 4096, "the columns and the other arguments of rsx_lex_join_kernel fit the kernel-argument segment");

// the compound key of W bytes as an integer: 64 bits up to W = 8, two of them for W = 16
template <int W> struct LexAcc {
    uint64_t v = 0;
    template <typename K> __device__ __forceinline__ void put(K k, uint32_t off) { v |= (uint64_t)k << (8 * off); }
    __device__ __forceinline__ void store(unsigned char* r) const { __builtin_memcpy(r, &v, W); }
};
template <> struct LexAcc<16> {
    uint64_t lo = 0, hi = 0;
    template <typename K> __device__ __forceinline__ void put(K k, uint32_t off) {  // (a key of at most 8 bytes: off + sizeof(K) <= 16)
        const uint64_t v = (uint64_t)k;
        const uint32_t s = 8 * off;
        if (s == 0) {
            lo |= v;
        } else if (s < 64) {
            lo |= v << s;
            hi |= v >> (64 - s);
        } else {
            hi |= v << (s - 64);
        }
    }
    __device__ __forceinline__ void put(PairsU128 k, uint32_t) {  // a 16-byte column fills the key alone
        lo = k.lo;
        hi = k.hi;
    }
    __device__ __forceinline__ void store(unsigned char* r) const {
        __builtin_memcpy(r, &lo, 8);
        __builtin_memcpy(r + 8, &hi, 8);
    }
};

// one column of KB-byte keys into the V compound keys of a thread
template <int KB, int W, bool GATHER, int V>
__device__ __forceinline__ void lex_column(LexAcc<W> (&acc)[V], const LexColumn& c, uint64_t e0, const uint32_t (&q)[V]) {
    if constexpr (KB <= W) {
        using K = typename PairsKey<KB>::type;
        unsigned char kr[KB * V];
        if constexpr (GATHER) {
#pragma unroll
            for (int j = 0; j < V; ++j) pairs_load<KB>(kr + j * KB, c.keys + (uint64_t)q[j] * KB);
        } else if constexpr (V == 1) {
            pairs_load<KB>(kr, c.keys + e0 * KB);
        } else {
            if (c.wide) {
                pairs_load<KB * V>(kr, c.keys + e0 * KB);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) pairs_load<KB>(kr + j * KB, c.keys + (e0 + (uint64_t)j) * KB);
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            K k;
            __builtin_memcpy(&k, kr + j * KB, KB);
            acc[j].put(pairs_map<K>(k, c.kind, c.desc), c.off);
        }
    }
}

// V consecutive elements from e0 on
template <int W, bool GATHER, int V>
__device__ __forceinline__ void lex_join_group(const LexArgs& a, const uint8_t* __restrict__ prev, uint32_t prev_es, uint32_t prev_voff,
                                               uint8_t* __restrict__ elems, uint64_t e0) {
    constexpr int E = (int)pairs_elem(W, 4), VOFF = (int)pairs_voff(W, 4);
    uint32_t q[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if constexpr (GATHER) q[j] = *reinterpret_cast<const uint32_t*>(prev + (e0 + (uint64_t)j) * prev_es + prev_voff);
        else q[j] = (uint32_t)(e0 + (uint64_t)j);
    }
    LexAcc<W> acc[V];
    for (uint32_t i = 0; i < a.ncols; ++i) {
        const LexColumn& c = a.col[i];
        switch (c.kb) {
            case 1: lex_column<1, W, GATHER, V>(acc, c, e0, q); break;
            case 2: lex_column<2, W, GATHER, V>(acc, c, e0, q); break;
            case 4: lex_column<4, W, GATHER, V>(acc, c, e0, q); break;
            case 8: lex_column<8, W, GATHER, V>(acc, c, e0, q); break;
            default: lex_column<16, W, GATHER, V>(acc, c, e0, q); break;
        }
    }
    unsigned char er[E * V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        acc[j].store(er + j * E);
#pragma unroll
        for (int b = W; b < VOFF; ++b) er[j * E + b] = 0;
        __builtin_memcpy(er + j * E + VOFF, &q[j], 4);
#pragma unroll
        for (int b = VOFF + 4; b < E; ++b) er[j * E + b] = 0;
    }
    pairs_store<E * V>(elems + e0 * E, er);
}

template <int W, bool GATHER>
__global__ __launch_bounds__(256) void rsx_lex_join_kernel(const LexArgs a, const uint8_t* __restrict__ prev, uint32_t prev_es,
                                                           uint32_t prev_voff, uint8_t* __restrict__ elems, uint64_t n) {
    constexpr int VEC = (int)pairs_vec(pairs_elem(W, 4));
    const uint64_t e0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e0 >= n) return;
    if (e0 + VEC <= n) {
        lex_join_group<W, GATHER, VEC>(a, prev, prev_es, prev_voff, elems, e0);
    } else {
        for (uint64_t e = e0; e < n; ++e) lex_join_group<W, GATHER, 1>(a, prev, prev_es, prev_voff, elems, e);
    }
}

}  // namespace rsx
