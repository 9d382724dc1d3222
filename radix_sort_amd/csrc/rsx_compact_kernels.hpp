// rsx_compact_kernels.hpp -- the kernels behind rsx_compact_device (rsx.hip; launched by rsx_unique.hip, whose scan kernel
// they share): the rows of an UNSORTED table that pass a predicate, in input order, and optionally the others behind them.
// include/rsx.h has the definition: row i < N passes when its flag byte is non-zero (flags given) and its mapped key lies
// in [M(lo), M(hi)) (either bound given); INVERT keeps the rows that do not pass.
// Three launches, the shape of rsx_unique_kernels.hpp and rsx_setop_kernels.hpp, over tiles of compact_tile(KB, VB)
// consecutive rows, COMPACT_WG threads each, a thread owning IPT = tile / COMPACT_WG CONSECUTIVE rows:
//   rsx_compact_count_kernel<KB, IPT>   tile t -> tile_count[t], its kept rows.  It reads only what the predicate needs: the
//                                       thread's IPT flag bytes as one word, its IPT keys in 16-byte words; neither when
//                                       there is no predicate.  Tiles at or behind N store 0.
//   rsx_unique_scan_kernel              ONE workgroup: tile_base[t] = kept in front of tile t; their sum m -> out_num[0]
//   rsx_compact_write_kernel<KB, VB>    the keep bits again, as a register mask; the thread's rank by a wave scan and the
//                                       waves' totals through LDS; the kept rows go into LDS at their rank in the tile --
//                                       raw key, value, u16 source slot -- and, under PARTITION, the others behind them at
//                                       total + their rank; then thread t stores outputs t, t + COMPACT_WG, ...: every
//                                       store of a wave is one contiguous range.  Kept output o goes to tile_base + o, a
//                                       rejected one of rank u to m + (tile_start - tile_base) + u, m read from out_num,
//                                       which the scan wrote earlier in the stream.
//   rsx_compact_gather_kernel           values of a width without a typed instance: out_values row r = values row pos[r]
//                                       for r < m (PARTITION: r < N), the bound read on the device, pos the u32 or u64
//                                       positions the write kernel left
// KB 0: the call has no use for the keys (no bound and no key output); VB 0: no values.  The instantiated forms are
// KB in {0, 1, 2, 4, 8, 16} x VB in {0, 1, 2, 4, 8, 16} of the write kernel and, of the count kernel, every KB with the
// IPT its tiles have (compact_tile).
// N = n or min(n, *num), read on the device.  No workgroup waits for another one and there are no atomics: the same
// bytes on every call.
// Bases that are not 16-byte aligned: a thread's flag word is put together from the two aligned words around it (no byte
// outside the aligned words that hold flags of rows below n is read); keys and values are then loaded one by one.
#pragma once

#include "rsx_device.hpp"
#include "rsx_pairs_kernels.hpp"

#include <type_traits>

namespace rsx {

constexpr int COMPACT_WG = 256;
constexpr uint32_t COMPACT_LDS_LIMIT = 80 * 1024;  // static LDS of one workgroup: two fit a CU's 160 KiB
constexpr uint32_t COMPACT_INVERT = 1, COMPACT_PARTITION = 2;  // RSX_COMPACT_*
// rows of one tile: 16 per thread while a key, a value and a u16 slot per row (and the waves' totals) fit the limit, else 8
constexpr uint32_t compact_lds_bytes(uint32_t kb, uint32_t vb, uint32_t tile) { return tile * (kb + vb + 2u) + 64u; }
constexpr uint32_t compact_tile(uint32_t kb, uint32_t vb) { return compact_lds_bytes(kb, vb, 4096u) <= COMPACT_LDS_LIMIT ? 4096u : 2048u; }
static_assert(compact_lds_bytes(16, 16, compact_tile(16, 16)) <= COMPACT_LDS_LIMIT, "two workgroups per CU");
static_assert(compact_lds_bytes(16, 2, compact_tile(16, 2)) <= COMPACT_LDS_LIMIT && compact_lds_bytes(8, 8, compact_tile(8, 8)) <= COMPACT_LDS_LIMIT,
              "two workgroups per CU");
static_assert(compact_tile(0, 0) % COMPACT_WG == 0 && compact_tile(16, 16) % COMPACT_WG == 0 && compact_tile(0, 0) <= 4096u,
              "whole rows per thread; rsx_unique_scan_kernel: at most 4096 per tile");

template <int B> struct CompactCell { using type = typename PairsWord<B>::type; };
template <> struct CompactCell<0> { using type = uint8_t; };

// the rows that count: n, or min(n, *num) (uniform: a scalar load)
__device__ __forceinline__ uint64_t compact_rows_of(uint64_t n, const uint64_t* __restrict__ num) {
    if (!num) return n;
    const uint64_t have = num[0];
    return have < n ? have : n;
}

// cnt <= IPT consecutive cells of B bytes from row r0 on -> registers: whole words when the base is 16-byte aligned and the
// thread has all its rows (r0 is a multiple of IPT, IPT * B of 8), else one by one
template <int B, int IPT>
__device__ __forceinline__ void compact_load(unsigned char* r, const uint8_t* __restrict__ base, uint64_t r0, uint32_t cnt) {
    using T = typename PairsWord<B>::type;
    if ((reinterpret_cast<uintptr_t>(base) & 15) == 0 && cnt == (uint32_t)IPT) {
        pairs_load<B * IPT>(r, base + r0 * B);
    } else {
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            T w{};
            if ((uint32_t)j < cnt) w = reinterpret_cast<const T*>(base)[r0 + (uint64_t)j];
            __builtin_memcpy(r + j * B, &w, B);
        }
    }
}

// bit j: flag byte r0 + j is non-zero, j < IPT (8 or 16); rows from cnt on give 0.  One aligned word of IPT bytes when the
// base is aligned to it; else the two aligned words around the thread's bytes, shifted together.  The second word is read
// only when it holds the flag of a row below n.
template <int IPT>
__device__ __forceinline__ uint32_t compact_flag_bits(const uint8_t* __restrict__ flags, uint64_t r0, uint32_t cnt, uint64_t n) {
    static_assert(IPT == 8 || IPT == 16, "a thread's flags are one or two 8-byte words");
    constexpr int W = IPT / 8;
    uint64_t f[W];
    const uint8_t* at = flags + r0;
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(at) & (IPT - 1));
    const uint8_t* word = at - shift;  // holds byte r0 (r0 < n: the caller's cnt >= 1)
    if (shift == 0) {
        pairs_load<IPT>(reinterpret_cast<unsigned char*>(f), word);
    } else {
        uint64_t lo[W], hi[W];
        pairs_load<IPT>(reinterpret_cast<unsigned char*>(lo), word);
#pragma unroll
        for (int w = 0; w < W; ++w) hi[w] = 0;
        if (r0 + (IPT - shift) < n) pairs_load<IPT>(reinterpret_cast<unsigned char*>(hi), word + IPT);
        const uint32_t bits = (shift & 7u) * 8u;
        if constexpr (W == 1) {
            f[0] = lo[0] >> bits | hi[0] << (64u - bits);  // (shift 1 .. 7: bits 8 .. 56)
        } else {
            // the four 8-byte words as one 32-byte string, read from byte `shift` on
            const bool far = shift >= 8;
            const uint64_t a = far ? lo[1] : lo[0], b = far ? hi[0] : lo[1], c = far ? hi[1] : hi[0];
            f[0] = bits ? a >> bits | b << (64u - bits) : a;
            f[1] = bits ? b >> bits | c << (64u - bits) : b;
        }
    }
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) m |= ((f[j / 8] >> (8 * (j % 8)) & 0xFFu) != 0 ? 1u : 0u) << j;
    return cnt >= (uint32_t)IPT ? m : m & ((1u << cnt) - 1u);
}

// bit j: M(lo) <= M(key j) < M(hi), each bound only when given (null: none)
template <int KB, int IPT>
__device__ __forceinline__ uint32_t compact_range_bits(const typename PairsKey<KB>::type* k, const void* __restrict__ lo, const void* __restrict__ hi,
                                                       uint32_t kind, uint32_t desc) {
    using K = typename PairsKey<KB>::type;
    K mlo{}, mhi{};
    if (lo) mlo = pairs_map<K>(*static_cast<const K*>(lo), kind, desc);  // (uniform: scalar loads)
    if (hi) mhi = pairs_map<K>(*static_cast<const K*>(hi), kind, desc);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const K x = pairs_map<K>(k[j], kind, desc);
        const bool ok = (!lo || !(x < mlo)) && (!hi || x < mhi);
        m |= (ok ? 1u : 0u) << j;
    }
    return m;
}

// The keep bits of the thread's rows r0 .. r0 + cnt - 1 (cnt >= 1); `raw` receives the keys when they are loaded: for a
// bound, or because the caller wants them (want_keys).
template <int KB, int IPT>
__device__ __forceinline__ uint32_t compact_keep_bits(const uint8_t* __restrict__ keys, const uint8_t* __restrict__ flags, const void* __restrict__ lo,
                                                      const void* __restrict__ hi, uint64_t r0, uint32_t cnt, uint64_t n, uint32_t kind,
                                                      uint32_t desc, uint32_t mode, bool want_keys,
                                                      typename std::conditional<KB == 0, uint8_t, typename PairsKey<(KB ? KB : 1)>::type>::type* raw) {
    const uint32_t valid = (1u << (cnt < (uint32_t)IPT ? cnt : (uint32_t)IPT)) - 1u;  // (IPT <= 16)
    uint32_t pass = valid;
    if (flags) pass &= compact_flag_bits<IPT>(flags, r0, cnt, n);
    if constexpr (KB > 0) {
        const bool range = lo || hi;
        if (range || want_keys) compact_load<KB, IPT>(reinterpret_cast<unsigned char*>(raw), keys, r0, cnt);
        if (range) pass &= compact_range_bits<KB, IPT>(raw, lo, hi, kind, desc);
    }
    return (mode & COMPACT_INVERT ? ~pass : pass) & valid;
}

template <int KB, int IPT>
__global__ __launch_bounds__(COMPACT_WG) void rsx_compact_count_kernel(const uint8_t* __restrict__ keys, const uint8_t* __restrict__ flags,
                                                                       const void* __restrict__ lo, const void* __restrict__ hi, uint64_t n,
                                                                       const uint64_t* __restrict__ num, uint32_t kind, uint32_t desc, uint32_t mode,
                                                                       uint32_t* __restrict__ tile_count) {
    using K = typename std::conditional<KB == 0, uint8_t, typename PairsKey<(KB ? KB : 1)>::type>::type;
    constexpr int NW = COMPACT_WG / WAVE;
    constexpr uint32_t TILE = (uint32_t)(IPT * COMPACT_WG);
    __shared__ uint32_t s_wave[NW];
    const uint64_t N = compact_rows_of(n, num);
    const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
    if (t0 >= N) {  // the whole workgroup: a tile behind the device count
        if (threadIdx.x == 0) tile_count[blockIdx.x] = 0;
        return;
    }
    const uint32_t L = N - t0 < TILE ? (uint32_t)(N - t0) : TILE;
    if (!flags && !lo && !hi) {  // no predicate: every row passes
        if (threadIdx.x == 0) tile_count[blockIdx.x] = mode & COMPACT_INVERT ? 0u : L;
        return;
    }
    const uint32_t s0 = threadIdx.x * IPT;
    const uint32_t cnt = s0 >= L ? 0u : L - s0 < (uint32_t)IPT ? L - s0 : (uint32_t)IPT;
    uint32_t kept = 0;
    if (cnt) {
        K raw[IPT];
        kept = (uint32_t)__popc(compact_keep_bits<KB, IPT>(keys, flags, lo, hi, t0 + s0, cnt, n, kind, desc, mode, false, raw));
    }
    // the wave's sum, then the waves' sums through LDS
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    if ((threadIdx.x & (WAVE - 1)) == 0) s_wave[threadIdx.x / WAVE] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) total += s_wave[w];
        tile_count[blockIdx.x] = total;
    }
}

// ib: bytes of an index in out_index (4 or 8).  Every output pointer may be null (a uniform branch each); VB > 0: values
// and out_values are given.  out_num holds the scan's sum.
template <int KB, int VB>
__global__ __launch_bounds__(COMPACT_WG) void rsx_compact_write_kernel(const uint8_t* __restrict__ keys, const uint8_t* __restrict__ flags,
                                                                       const void* __restrict__ lo, const void* __restrict__ hi,
                                                                       const uint8_t* __restrict__ values, uint64_t n,
                                                                       const uint64_t* __restrict__ num, uint32_t kind, uint32_t desc, uint32_t mode,
                                                                       const uint64_t* __restrict__ tile_base, const uint64_t* __restrict__ out_num,
                                                                       uint8_t* __restrict__ out_keys, uint8_t* __restrict__ out_values,
                                                                       uint8_t* __restrict__ out_index, uint32_t ib) {
    using K = typename std::conditional<KB == 0, uint8_t, typename PairsKey<(KB ? KB : 1)>::type>::type;
    using KC = typename CompactCell<KB>::type;
    using VC = typename CompactCell<VB>::type;
    constexpr uint32_t TILE = compact_tile(KB, VB);
    constexpr int IPT = (int)(TILE / COMPACT_WG), NW = COMPACT_WG / WAVE;
    static_assert(compact_lds_bytes(KB, VB, TILE) <= COMPACT_LDS_LIMIT, "two workgroups per CU");
    __shared__ KC s_key[KB > 0 ? TILE : 1];
    __shared__ VC s_val[VB > 0 ? TILE : 1];
    __shared__ uint16_t s_slot[TILE];
    __shared__ uint32_t s_wave[NW];
    const uint64_t N = compact_rows_of(n, num);
    const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
    if (t0 >= N) return;  // the whole workgroup
    const uint32_t L = N - t0 < TILE ? (uint32_t)(N - t0) : TILE;
    const bool part = (mode & COMPACT_PARTITION) != 0;
    const bool key_out = KB > 0 && out_keys != nullptr;
    const uint32_t s0 = threadIdx.x * IPT < L ? threadIdx.x * IPT : L;
    const uint32_t cnt = L - s0 < (uint32_t)IPT ? L - s0 : (uint32_t)IPT;
    K raw[IPT];
    uint32_t keep = 0;
    if (cnt) keep = compact_keep_bits<KB, IPT>(keys, flags, lo, hi, t0 + s0, cnt, n, kind, desc, mode, key_out, raw);
    const uint32_t kept = (uint32_t)__popc(keep);
    const uint32_t incl = wave_incl_scan<false>(kept);
    const uint32_t wave = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    uint32_t below = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const uint32_t v = s_wave[w];
        below += (uint32_t)w < wave ? v : 0u;
        total += v;
    }
    // kept rows of the tile in front of this thread's: q + kept <= total <= L; rejected ones in front of them: s0 - q, and
    // total + (s0 - q) + (cnt - kept) <= L
    uint32_t q = below + (incl - kept);
    uint32_t u = total + (s0 - q);
    if (cnt && (kept || part)) {
        unsigned char vr[VB > 0 ? VB * IPT : 1];
        if constexpr (VB > 0) compact_load<VB, IPT>(vr, values, t0 + s0, cnt);
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const bool k = keep >> j & 1u;
            if ((uint32_t)j < cnt && (k || part)) {
                const uint32_t at = k ? q : u;
                s_slot[at] = (uint16_t)(s0 + (uint32_t)j);
                if constexpr (KB > 0) {
                    if (key_out) __builtin_memcpy(&s_key[at], &raw[j], KB);
                }
                if constexpr (VB > 0) __builtin_memcpy(&s_val[at], vr + j * VB, VB);
                q += k ? 1u : 0u;
                u += k ? 0u : 1u;
            }
        }
    }
    __syncthreads();
    const uint64_t base = tile_base[blockIdx.x];              // kept in front of the tile: base <= t0
    const uint64_t rest = part ? out_num[0] + (t0 - base) : 0;  // where the tile's rejected rows begin
    const uint32_t outs = part ? L : total;
#pragma unroll 4
    for (uint32_t o = threadIdx.x; o < outs; o += COMPACT_WG) {
        const uint64_t dst = o < total ? base + o : rest + (o - total);
        if (dst >= n) continue;  // (never, while the inputs are what the count launch read)
        if constexpr (KB > 0) {
            if (key_out) reinterpret_cast<KC*>(out_keys)[dst] = s_key[o];
        }
        if constexpr (VB > 0) reinterpret_cast<VC*>(out_values)[dst] = s_val[o];
        if (out_index) {
            const uint64_t src = t0 + s_slot[o];
            if (ib == 8) reinterpret_cast<uint64_t*>(out_index)[dst] = src;
            else reinterpret_cast<uint32_t*>(out_index)[dst] = (uint32_t)src;
        }
    }
}

// out_values row r = values row pos[r] for r < *rows_num (PARTITION: r < min(n, *num)), rows of `words` words of W; pos:
// n positions of pb bytes (4 or 8).  A grid-stride loop over the words of the rows that count.
template <typename W>
__global__ __launch_bounds__(256) void rsx_compact_gather_kernel(const uint8_t* __restrict__ values, const uint8_t* __restrict__ pos, uint32_t pb,
                                                                 uint64_t n, const uint64_t* __restrict__ num, const uint64_t* __restrict__ out_num,
                                                                 uint32_t mode, uint32_t words, uint8_t* __restrict__ out_values) {
    const uint64_t N = compact_rows_of(n, num);
    uint64_t rows = mode & COMPACT_PARTITION ? N : out_num[0];
    if (rows > N) rows = N;
    const uint64_t total = rows * words;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint64_t r = i / words, w = i - r * words;
        const uint64_t src = pb == 8 ? reinterpret_cast<const uint64_t*>(pos)[r] : (uint64_t)reinterpret_cast<const uint32_t*>(pos)[r];
        if (src < n) reinterpret_cast<W*>(out_values)[i] = reinterpret_cast<const W*>(values)[src * words + w];
    }
}

}  // namespace rsx
