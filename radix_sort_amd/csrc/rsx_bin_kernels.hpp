// rsx_bin_kernels.hpp -- the kernels of rsx_bin_count_device (rsx.hip): how many of the first N keys of an UNSORTED key
// array fall into each of m + 1 bins.  The keys are read once, in the 16-byte words of select_stream; nothing is written
// but the m + 1 counts.
//   rsx_bin_zero_kernel              the m + 1 counts <- 0 (a kernel, not a memset node: rsx_zero16_kernel says why)
//   rsx_bin_edge_kernel<KB, UP>      bins between m sorted edges: the mapped edges (pairs_map: sign flip, float total
//                                    order, complemented for descending order) are staged in LDS once per workgroup
//                                    beside m + 1 four-byte counters; every key is mapped and its bin found by a bound
//                                    search in LDS -- UP: the edges that are <= the key, else those that are < it --
//                                    BIN_GROUP keys of a thread in step (search_in_step_whole), so that as many LDS
//                                    probes are in flight; the counters are flushed with integer atomics, non-zero ones
//                                    only, so the result does not depend on any order.
//   rsx_bin_index_kernel<KB, LDS>    the bin is the key's integer value when it is in 0 .. m - 1, else m.  LDS true
//                                    (m <= BIN_INDEX_WINDOWS * BIN_INDEX_LDS): counters in LDS as above, no search,
//                                    one window of BIN_INDEX_LDS values at a time -- a workgroup walks its share once per
//                                    window and counts the keys whose bin lies in it; the last window counts the
//                                    outside bin beside its values; LDS false: atomics straight into the counts.
// All of them add through select's shortcut: a wave whose lanes all hold the first lane's bin adds their number once.
// The grid is a fixed number of persistent workgroups, each with one share of at least SELECT_SHARE keys (select_share).
// N = n or min(n, *num), read on the device.  m == 0: one bin holds N, and no key is read.
// A four-byte LDS counter cannot wrap: a workgroup walks its share in pieces of at most BIN_PIECE = 2^31 keys and flushes
// after each (bin_pieces).
// What the kernels promise for edges that are NOT sorted: the fixed-length search reads only positions below m and ends
// in 0 .. m, so every counter touched is one of the m + 1.
#pragma once

#include "rsx_search_kernels.hpp"
#include "rsx_select_kernels.hpp"

#include <type_traits>

namespace rsx {

constexpr int BIN_WG = 512;
constexpr uint32_t BIN_LDS_LIMIT = 80 * 1024;  // static LDS of one workgroup: two fit a CU's 160 KiB
// the most edges of the edge form: m mapped keys and m + 1 counters in LDS
constexpr uint32_t bin_max_edges(uint32_t kb) { return kb <= 4 ? 8192u : kb == 8 ? 4096u : 2048u; }
constexpr uint32_t BIN_INDEX_LDS = 16384;      // values of one window of the index form's LDS variant: 64 KiB (+ the outside bin's counter)
// Windows the LDS variant walks before the atomics take over.  Measured at 2^28 u32 ids ("Histogram"):
// a window costs one read of the keys, 0.19-0.21 ms, the atomics 11.3 ms whatever the number of values; 16 windows, 3.10 ms,
// are also where a sort of the ids (radix_unique with counts, 3.4 ms) draws level.
constexpr uint32_t BIN_INDEX_WINDOWS = 16;
constexpr uint64_t BIN_PIECE = 1ull << 31;     // keys of a workgroup between two flushes of its LDS counters
constexpr int BIN_GROUP = 8;                   // searches of one thread in step
static_assert(bin_max_edges(4) * 4 + (bin_max_edges(4) + 1) * 4 <= BIN_LDS_LIMIT, "edges and counters: two workgroups per CU");
static_assert(bin_max_edges(8) * 8 + (bin_max_edges(8) + 1) * 4 <= BIN_LDS_LIMIT, "edges and counters: two workgroups per CU");
static_assert(bin_max_edges(16) * 16 + (bin_max_edges(16) + 1) * 4 <= BIN_LDS_LIMIT, "edges and counters: two workgroups per CU");
static_assert((BIN_INDEX_LDS + 1) * 4 <= BIN_LDS_LIMIT, "the index form's counters: two workgroups per CU");
static_assert(BIN_PIECE % 16 == 0 && BIN_PIECE < (1ull << 32), "a piece keeps a four-byte counter from wrapping and starts on a whole word");

// select_stream, handing the keys over in groups: f(k, integral_constant<int, C>) receives C keys k[0 .. C), C <= BIN_GROUP,
// in no particular order.  The same loads: 16-byte words, VU of them in flight per thread, the streaming hint when asked
// for, the keys ahead of the first 16-byte boundary and behind the last whole word one by one.
template <int KB, int WG, int VU, typename F>
__device__ __forceinline__ void bin_stream(const void* __restrict__ src, uint64_t p0, uint64_t p1, bool stream, F&& f) {
    using K = typename PairsKey<KB>::type;
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    constexpr int VEC = 16 / KB;
    constexpr int GW = VEC < BIN_GROUP ? VEC : BIN_GROUP;                  // group of the keys of one word
    constexpr int GR = VU * VEC < BIN_GROUP ? VU * VEC : BIN_GROUP;        // ... of the keys of a round of VU words
    if (p0 >= p1) return;
    const K* keys = static_cast<const K*>(src);
    const uint32_t tid = threadIdx.x;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(keys + p0);  // (the same in every lane)
    uint64_t head = (uint64_t)(((16u - (uint32_t)(addr & 15u)) & 15u) / (uint32_t)KB);
    if (head > p1 - p0) head = p1 - p0;
    const uint64_t nvec = (p1 - p0 - head) / VEC;
    const v4u* vsrc = reinterpret_cast<const v4u*>(keys + p0 + head);
    auto words = [&](auto nt) {  // (one copy of the loops per kind of load: no test between the loads of a round)
        auto load = [&](uint64_t j) -> v4u {
            if constexpr (decltype(nt)::value) return __builtin_nontemporal_load(vsrc + j);
            else return vsrc[j];
        };
        uint64_t j = tid;
        for (; j + (uint64_t)(VU - 1) * WG < nvec; j += (uint64_t)VU * WG) {
            v4u v[VU];
#pragma unroll
            for (int u = 0; u < VU; ++u) v[u] = load(j + (uint64_t)u * WG);
            K k[VU * VEC];
            __builtin_memcpy(k, v, 16 * VU);
#pragma unroll
            for (int g = 0; g < VU * VEC; g += GR) f(k + g, std::integral_constant<int, GR>{});
        }
        for (; j < nvec; j += WG) {
            const v4u v = load(j);
            K k[VEC];
            __builtin_memcpy(k, &v, 16);
#pragma unroll
            for (int g = 0; g < VEC; g += GW) f(k + g, std::integral_constant<int, GW>{});
        }
    };
    if (stream) words(std::true_type{});
    else words(std::false_type{});
    const uint64_t t0 = p0 + head + nvec * VEC;  // fewer than VEC keys at either end
    if (tid < head) {
        const K k = keys[p0 + tid];
        f(&k, std::integral_constant<int, 1>{});
    }
    if (tid >= 64 && tid - 64 < p1 - t0) {
        const K k = keys[t0 + (tid - 64)];
        f(&k, std::integral_constant<int, 1>{});
    }
}

// the keys that count: n, or min(n, *num) (uniform: a scalar load)
__device__ __forceinline__ uint64_t bin_count_of(uint64_t n, const uint64_t* __restrict__ num) {
    if (!num) return n;
    const uint64_t have = num[0];
    return have < n ? have : n;
}

// counts[b] += c, counts of cb = 4 or 8 bytes
__device__ __forceinline__ void bin_flush_add(void* __restrict__ counts, uint32_t cb, uint32_t b, uint64_t c) {
    if (cb == 8) atomicAdd(static_cast<unsigned long long*>(counts) + b, (unsigned long long)c);
    else atomicAdd(static_cast<uint32_t*>(counts) + b, (uint32_t)c);
}

// select's add: a wave whose active lanes all hold the first lane's bin adds their number once through one(bin, count)
template <typename A>
__device__ __forceinline__ void bin_add(uint32_t bin, A&& one) {
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
    const bool same = bin == b0;
    const uint64_t m = __builtin_amdgcn_ballot_w64(same);
    if (same) {
        if (mbcnt64(m) == 0) one(b0, (uint32_t)__popcll(m));
    } else {
        one(bin, 1u);
    }
}

// A workgroup's share [p0, p1) in pieces of at most BIN_PIECE keys, with `bins` LDS counters zeroed before and flushed
// into counts[base ..] behind each piece: no counter receives 2^32 adds between two flushes.
template <typename W>
__device__ __forceinline__ void bin_pieces(uint32_t* cnt, uint32_t bins, uint64_t p0, uint64_t p1, void* __restrict__ counts, uint32_t cb,
                                           uint32_t base, W&& walk) {
    const uint32_t tid = threadIdx.x;
    for (uint64_t c0 = p0; c0 < p1; c0 += BIN_PIECE) {
        const uint64_t c1 = p1 - c0 > BIN_PIECE ? c0 + BIN_PIECE : p1;
        for (uint32_t i = tid; i < bins; i += BIN_WG) cnt[i] = 0;
        __syncthreads();
        walk(c0, c1);
        __syncthreads();
        for (uint32_t i = tid; i < bins; i += BIN_WG) {
            const uint32_t c = cnt[i];
            if (c) bin_flush_add(counts, cb, base + i, c);
        }
        __syncthreads();
    }
}

// m == 0: every one of the N keys is in bin 0
__device__ __forceinline__ void bin_all_in_one(uint64_t N, void* __restrict__ counts, uint32_t cb) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && N != 0) bin_flush_add(counts, cb, 0, N);
}

__global__ __launch_bounds__(256) void rsx_bin_zero_kernel(void* __restrict__ counts, uint32_t bins, uint32_t cb) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < bins; i += (uint64_t)gridDim.x * 256) {
        if (cb == 8) static_cast<uint64_t*>(counts)[i] = 0;
        else static_cast<uint32_t*>(counts)[i] = 0;
    }
}

template <int KB, bool UP>
__global__ __launch_bounds__(BIN_WG) void rsx_bin_edge_kernel(const void* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ num,
                                                              const void* __restrict__ edges, uint32_t m, void* __restrict__ counts, uint32_t cb,
                                                              uint32_t kind, uint32_t desc, uint32_t stream) {
    using K = typename PairsKey<KB>::type;
    constexpr uint32_t E = bin_max_edges(KB);
    __shared__ __attribute__((aligned(16))) K s_edge[E];
    __shared__ uint32_t cnt[E + 1];
    const uint64_t N = bin_count_of(n, num);
    if (m > E) return;  // (the host refuses it)
    if (m == 0) return bin_all_in_one(N, counts, cb);
    uint64_t p0, p1;
    select_share(N, &p0, &p1);
    if (p0 >= p1) return;
    for (uint32_t i = threadIdx.x; i < m; i += BIN_WG) s_edge[i] = search_hay<KB>(static_cast<const uint8_t*>(edges), i, kind, desc);
    // (bin_pieces synchronises before the first key is looked at)
    const auto at = [&](uint32_t i) -> K { return s_edge[i]; };
    const auto one = [&](uint32_t b, uint32_t c) { atomicAdd(&cnt[b], c); };
    bin_pieces(cnt, m + 1, p0, p1, counts, cb, 0u, [&](uint64_t c0, uint64_t c1) {
        bin_stream<KB, BIN_WG, 4>(keys, c0, c1, stream != 0, [&](const K* raw, auto count) {
            constexpr int C = decltype(count)::value;
            K key[C];
            uint32_t bin[C];
#pragma unroll
            for (int g = 0; g < C; ++g) {
                key[g] = pairs_map<K>(raw[g], kind, desc);
                bin[g] = 0;
            }
            search_in_step_whole<K, UP, C, uint32_t>(at, bin, m, key);
#pragma unroll
            for (int g = 0; g < C; ++g) bin_add(bin[g], one);
        });
    });
}

// the bin of an integer key: its value in 0 .. m - 1, else m (negative keys of a signed kind too)
template <typename K>
__device__ __forceinline__ uint32_t bin_index_of(K raw, uint32_t m, uint32_t kind) {
    constexpr K MIN = (K)((K)1 << (8 * sizeof(K) - 1));
    const bool outside = (kind == PAIRS_SIGNED && (raw & MIN) != 0) || (uint64_t)raw >= (uint64_t)m;
    return outside ? m : (uint32_t)raw;
}

template <int KB, bool LDS>
__global__ __launch_bounds__(BIN_WG) void rsx_bin_index_kernel(const void* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ num, uint32_t m,
                                                               void* __restrict__ counts, uint32_t cb, uint32_t kind, uint32_t stream) {
    using K = typename PairsKey<KB>::type;
    __shared__ uint32_t cnt[LDS ? BIN_INDEX_LDS + 1 : 1];
    const uint64_t N = bin_count_of(n, num);
    if (m == 0) return bin_all_in_one(N, counts, cb);
    uint64_t p0, p1;
    select_share(N, &p0, &p1);
    if (p0 >= p1) return;
    if constexpr (LDS) {
        if (m > BIN_INDEX_WINDOWS * BIN_INDEX_LDS) return;  // (the host sends these to the other variant)
        const bool hint = stream != 0 && m <= BIN_INDEX_LDS;  // (a share that is read again should stay in the caches)
        const auto one = [&](uint32_t b, uint32_t c) { atomicAdd(&cnt[b], c); };
        for (uint32_t base = 0; base < m; base += BIN_INDEX_LDS) {
            const uint32_t values = m - base < BIN_INDEX_LDS ? m - base : BIN_INDEX_LDS;
            const uint32_t span = values + (base + values == m ? 1u : 0u);  // the last window: bin m sits right behind its values
            bin_pieces(cnt, span, p0, p1, counts, cb, base, [&](uint64_t c0, uint64_t c1) {
                bin_stream<KB, BIN_WG, 4>(keys, c0, c1, hint, [&](const K* raw, auto count) {
#pragma unroll
                    for (int g = 0; g < decltype(count)::value; ++g) {
                        const uint32_t b = bin_index_of<K>(raw[g], m, kind) - base;  // (below the window: wraps to a large value; bin m in an earlier window: beyond it)
                        if (b < span) bin_add(b, one);
                    }
                });
            });
        }
    } else {
        const auto one = [&](uint32_t b, uint32_t c) { bin_flush_add(counts, cb, b, c); };
        bin_stream<KB, BIN_WG, 4>(keys, p0, p1, stream != 0, [&](const K* raw, auto count) {
#pragma unroll
            for (int g = 0; g < decltype(count)::value; ++g) bin_add(bin_index_of<K>(raw[g], m, kind), one);
        });
    }
}

}  // namespace rsx
