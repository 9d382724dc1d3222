// rsx_msplit_kernels.hpp -- the kernels behind rsx_multisplit_device (rsx.hip, beside the bin kernels whose body the count
// launch shares; values of a width without a typed instance go through the compact call's row gather): the first N rows
// of an UNSORTED table regrouped by bin, in input order inside each bin, and the m + 2 offsets of the bins.  bin(key) is
// rsx_bin_count_device's: the edges that are <= the
// mapped key (MSPLIT_UPPER) or < it (MSPLIT_LOWER), or the key's integer value in 0 .. m - 1, else m (MSPLIT_INDEX).
// Four launches over G = min(ceil(n / SELECT_SHARE), 2 * CUs) persistent workgroups, workgroup g owning select_share's
// share g of the N rows -- the count and the write launch read the same N and so cut the same shares:
//   rsx_msplit_count_kernel<KB, MODE>      the bin kernels' body (edges mapped into LDS, bin_stream, eight searches in step,
//                                          bin_add into LDS counters); every workgroup then STORES all m + 1 counters into
//                                          its column of cnt[b * G + g], u32 each: no zeroing launch and no atomics on
//                                          global memory.  A workgroup whose share is empty stores zeros.
//   rsx_msplit_scan_kernel                 a wave per bin: row b of cnt <- its exclusive sums across g, tot[b] <- its sum
//   rsx_msplit_offsets_kernel              ONE workgroup: out_offsets[0 .. m + 1] <- the exclusive sums of tot, and N
//   rsx_msplit_write_kernel<KB, VB, MODE>  MSPLIT_WG threads.  cur[b] <- offsets[b] + cnt[b * G + g], then the share in
//                                          tiles of MSPLIT_TILE rows, in order.  Wave w owns a contiguous quarter of the
//                                          tile; in round j its lane l holds row w * 64 * IPT + j * 64 + l.  Per round: the
//                                          key, its bin again, the lanes of the wave with the same bin (match_digit), the
//                                          rank among them (mbcnt64); every lane reads the wave's own counter wc[w][bin]
//                                          and the group's first lane adds the group's size -- only this wave touches its
//                                          counters, so the rounds need no barrier.  Then thread b turns wc[0 .. 3][b] into
//                                          start positions from cur[b] and advances cur[b], and every row goes to
//                                          wc[w][bin] + its rank in the wave's quarter: raw key, value, position.
// Both kernels find a key's bin through msplit_bins, so they agree on it whatever the edges hold: for edges that are NOT
// sorted the grouping is unspecified, but every one of the N rows is still written exactly once below N, the search reads
// only positions below m and every counter touched is one of the m + 1.
// No counter wraps: the call takes n < 2^32 rows, so no count and no position reaches 2^32 whatever the share (one
// workgroup may own all of them).  N = n or min(n, *num), read on the device.  No workgroup waits for another one: the
// same bytes on every call.
// LDS of the write kernel at the cap, 16-byte keys: 2047 edges 32 KiB, cur 8 KiB, wc 32 KiB -- 72 KiB, two workgroups a CU.
#pragma once

#include "rsx_bin_kernels.hpp"

#include <type_traits>

namespace rsx {

constexpr int MSPLIT_WG = 256;
constexpr int MSPLIT_WAVES = MSPLIT_WG / WAVE;
constexpr int MSPLIT_IPT = 16;                                    // rounds of a wave per tile
constexpr uint32_t MSPLIT_TILE = MSPLIT_WG * MSPLIT_IPT;          // rows of one tile
constexpr uint32_t MSPLIT_MAX_EDGES = 2047;                       // m of an edge mode, and of the index mode: m + 1 <= 2048 bins
constexpr uint32_t MSPLIT_BINS = MSPLIT_MAX_EDGES + 1;
constexpr uint32_t MSPLIT_LDS_LIMIT = 80 * 1024;                  // static LDS of one workgroup: two fit a CU's 160 KiB
constexpr int MSPLIT_UPPER = 0, MSPLIT_LOWER = 1, MSPLIT_INDEX = 2;  // RSX_BIN_*
constexpr int MSPLIT_OFFSETS_WG = 256;
constexpr int MSPLIT_OFFSETS_PER = (int)(MSPLIT_BINS / MSPLIT_OFFSETS_WG);
static_assert(MSPLIT_MAX_EDGES * 16 + MSPLIT_BINS * 4 + MSPLIT_WAVES * MSPLIT_BINS * 4 <= MSPLIT_LDS_LIMIT, "edges, cursors, wave counters: two workgroups per CU");
static_assert(MSPLIT_BINS == (uint32_t)(MSPLIT_OFFSETS_WG * MSPLIT_OFFSETS_PER), "the offsets kernel: whole bins per thread");
static_assert(MSPLIT_BINS <= (1u << 11) && WAVE * MSPLIT_IPT <= (1u << 20), "a bin and a rank in the wave's quarter share one word");
static_assert(MSPLIT_IPT % BIN_GROUP == 0, "whole groups of searches in step");

template <int B> struct MsplitCell { using type = typename PairsWord<B>::type; };
template <> struct MsplitCell<0> { using type = uint8_t; };

// the bins of C keys: the one place both passes take them from
template <int KB, int MODE, int C>
__device__ __forceinline__ void msplit_bins(const typename PairsKey<KB>::type* raw, uint32_t* bin, const typename PairsKey<KB>::type* s_edge, uint32_t m,
                                            uint32_t kind, uint32_t desc) {
    using K = typename PairsKey<KB>::type;
    if constexpr (MODE == MSPLIT_INDEX) {
#pragma unroll
        for (int g = 0; g < C; ++g) bin[g] = bin_index_of<K>(raw[g], m, kind);
    } else {
        K key[C];
        uint32_t at_[C];
#pragma unroll
        for (int g = 0; g < C; ++g) {
            key[g] = pairs_map<K>(raw[g], kind, desc);
            at_[g] = 0;
        }
        if (m != 0) {  // (uniform)
            const auto at = [&](uint32_t i) -> K { return s_edge[i]; };
            search_in_step_whole<K, MODE == MSPLIT_UPPER, C, uint32_t>(at, at_, m, key);
        }
#pragma unroll
        for (int g = 0; g < C; ++g) bin[g] = at_[g];
    }
}

// the lanes of the wave that hold my bin, bins of nb bits: a uniform choice among three widths of the match
__device__ __forceinline__ uint64_t msplit_match(uint32_t bin, uint32_t nb) {
    if (nb <= 4) return match_digit<4>(bin);
    if (nb <= 8) return match_digit<8>(bin);
    return match_digit<11>(bin);
}

// the lane's round bits again, as a value the compiler takes for a new one
__device__ __forceinline__ uint32_t msplit_rounds(uint32_t have) {
    asm volatile("" : "+v"(have));
    return have;
}

template <int KB, int MODE>
__global__ __launch_bounds__(BIN_WG) void rsx_msplit_count_kernel(const void* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ num,
                                                                  const void* __restrict__ edges, uint32_t m, uint32_t* __restrict__ cntm, uint32_t kind,
                                                                  uint32_t desc, uint32_t stream) {
    using K = typename PairsKey<KB>::type;
    __shared__ __attribute__((aligned(16))) K s_edge[MODE == MSPLIT_INDEX ? 1 : MSPLIT_MAX_EDGES];
    __shared__ uint32_t cnt[MSPLIT_BINS];
    if (m > MSPLIT_MAX_EDGES) return;  // (the host refuses it)
    const uint64_t N = bin_count_of(n, num);
    uint64_t p0, p1;
    select_share(N, &p0, &p1);
    if (p1 < p0) p1 = p0;  // a share behind the device count: m + 1 zeros
    if constexpr (MODE != MSPLIT_INDEX)
        for (uint32_t i = threadIdx.x; i < m; i += BIN_WG) s_edge[i] = search_hay<KB>(static_cast<const uint8_t*>(edges), i, kind, desc);
    for (uint32_t i = threadIdx.x; i <= m; i += BIN_WG) cnt[i] = 0;
    __syncthreads();
    if (m == 0) {  // one bin holds the share, and no key is read
        if (threadIdx.x == 0) cnt[0] = (uint32_t)(p1 - p0);
    } else {
        const auto one = [&](uint32_t b, uint32_t c) { atomicAdd(&cnt[b], c); };
        bin_stream<KB, BIN_WG, 4>(keys, p0, p1, stream != 0, [&](const K* raw, auto count) {
            constexpr int C = decltype(count)::value;
            uint32_t bin[C];
            msplit_bins<KB, MODE, C>(raw, bin, s_edge, m, kind, desc);
#pragma unroll
            for (int g = 0; g < C; ++g) bin_add(bin[g], one);
        });
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= m; i += BIN_WG) cntm[(uint64_t)i * gridDim.x + blockIdx.x] = cnt[i];
}

// a wave per bin: row b of the matrix (G words) <- its exclusive sums, tot[b] <- its sum
__global__ __launch_bounds__(MSPLIT_WG) void rsx_msplit_scan_kernel(uint32_t* __restrict__ cntm, uint32_t bins, uint32_t G, uint32_t* __restrict__ tot) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t b = blockIdx.x * MSPLIT_WAVES + threadIdx.x / WAVE;
    if (b >= bins) return;  // (the whole wave)
    uint32_t* row = cntm + (uint64_t)b * G;
    uint32_t carry = 0;
    for (uint32_t c = 0; c < G; c += WAVE) {
        const uint32_t i = c + lane;
        const uint32_t v = i < G ? row[i] : 0u;
        const uint32_t incl = wave_incl_scan<false>(v);
        if (i < G) row[i] = carry + (incl - v);
        carry += (uint32_t)__shfl((int)incl, WAVE - 1);
    }
    if (lane == 0) tot[b] = carry;
}

// ONE workgroup: offsets[b] = the rows of the bins below b, b = 0 .. bins (bins <= MSPLIT_BINS)
__global__ __launch_bounds__(MSPLIT_OFFSETS_WG) void rsx_msplit_offsets_kernel(const uint32_t* __restrict__ tot, uint32_t bins,
                                                                               uint64_t* __restrict__ offsets) {
    __shared__ uint32_t s_wave[MSPLIT_OFFSETS_WG / WAVE];
    const uint32_t b0 = threadIdx.x * MSPLIT_OFFSETS_PER;
    uint32_t v[MSPLIT_OFFSETS_PER];
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < MSPLIT_OFFSETS_PER; ++j) {
        v[j] = b0 + j < bins ? tot[b0 + j] : 0u;
        sum += v[j];
    }
    const uint32_t incl = wave_incl_scan<false>(sum);
    const uint32_t wave = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    uint64_t run = incl - sum;
#pragma unroll
    for (int w = 0; w < MSPLIT_OFFSETS_WG / WAVE; ++w) run += (uint32_t)w < wave ? s_wave[w] : 0u;
#pragma unroll
    for (int j = 0; j < MSPLIT_OFFSETS_PER; ++j) {
        const uint32_t b = b0 + j;
        if (b < bins) offsets[b] = run;
        run += v[j];
        if (b + 1 == bins) offsets[bins] = run;
    }
}

// ib: bytes of a position in out_index (4 or 8).  Every output pointer may be null (a uniform branch each); VB > 0: values
// and out_values are given.  cntm and offsets are what the scan launches left.
template <int KB, int VB, int MODE>
__global__ __launch_bounds__(MSPLIT_WG) void rsx_msplit_write_kernel(const void* __restrict__ keys, const uint8_t* __restrict__ values, uint64_t n,
                                                                     const uint64_t* __restrict__ num, const void* __restrict__ edges, uint32_t m,
                                                                     const uint32_t* __restrict__ cntm, const uint64_t* __restrict__ offsets,
                                                                     uint32_t kind, uint32_t desc, uint8_t* __restrict__ out_keys,
                                                                     uint8_t* __restrict__ out_values, uint8_t* __restrict__ out_index, uint32_t ib) {
    using K = typename PairsKey<KB>::type;
    using KC = typename MsplitCell<KB>::type;
    using VC = typename MsplitCell<VB>::type;
    constexpr int IPT = MSPLIT_IPT;
    __shared__ __attribute__((aligned(16))) K s_edge[MODE == MSPLIT_INDEX ? 1 : MSPLIT_MAX_EDGES];
    __shared__ uint32_t cur[MSPLIT_BINS];
    __shared__ uint32_t wc[MSPLIT_WAVES][MSPLIT_BINS];
    if (m > MSPLIT_MAX_EDGES) return;  // (the host refuses it)
    const uint64_t N = bin_count_of(n, num);
    uint64_t p0, p1;
    select_share(N, &p0, &p1);
    if (p0 >= p1) return;  // the whole workgroup
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    if constexpr (MODE != MSPLIT_INDEX)
        for (uint32_t i = tid; i < m; i += MSPLIT_WG) s_edge[i] = search_hay<KB>(static_cast<const uint8_t*>(edges), i, kind, desc);
    for (uint32_t i = tid; i <= m; i += MSPLIT_WG) cur[i] = (uint32_t)offsets[i] + cntm[(uint64_t)i * gridDim.x + blockIdx.x];
    const uint32_t nb = 32u - (uint32_t)__builtin_clz(m | 1u);  // bits of a bin, 0 .. m
    const KC* kin = static_cast<const KC*>(keys);
    for (uint64_t t0 = p0; t0 < p1; t0 += MSPLIT_TILE) {
        for (uint32_t i = tid; i <= m; i += MSPLIT_WG) {
#pragma unroll
            for (int w = 0; w < MSPLIT_WAVES; ++w) wc[w][i] = 0;
        }
        __syncthreads();  // (the first tile: the edges and the cursors too)
        const uint64_t r0 = t0 + (uint64_t)wave * (WAVE * IPT) + lane;  // the lane's row of round 0
        // bit j: the lane has a row in round j.  Each phase tests an opaque copy (msplit_rounds), so that no phase keeps
        // sixteen lane masks alive in scalar registers for the next one.
        const uint64_t left = p1 > r0 ? p1 - r0 : 0;
        const uint32_t have = left >= (uint64_t)(WAVE * IPT) ? (1u << IPT) - 1u : (1u << (((uint32_t)left + WAVE - 1) / WAVE)) - 1u;
        K raw[IPT];
        uint32_t br[IPT];  // bin | rank in the wave's quarter << 12, later the row's position in the output
        uint32_t rounds = msplit_rounds(have);
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const uint64_t row = r0 + (uint64_t)j * WAVE;
            KC c{};
            if (rounds >> j & 1u) c = kin[row];
            __builtin_memcpy(&raw[j], &c, KB);
        }
#pragma unroll
        for (int j = 0; j < IPT; j += BIN_GROUP) msplit_bins<KB, MODE, BIN_GROUP>(raw + j, br + j, s_edge, m, kind, desc);
        rounds = msplit_rounds(have);
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const bool valid = (rounds >> j & 1u) != 0;
            const uint32_t bin = br[j];
            const uint64_t same = msplit_match(bin, nb) & __builtin_amdgcn_ballot_w64(valid);
            const uint32_t below = mbcnt64(same);
            const uint32_t old = wc[wave][bin];  // (every lane of the group reads it before the first one adds)
            if (valid && below == 0) wc[wave][bin] = old + (uint32_t)__popcll(same);
            br[j] = bin | (old + below) << 12;
        }
        unsigned char vr[VB > 0 ? VB * IPT : 1];
        if constexpr (VB > 0) {
            rounds = msplit_rounds(have);
#pragma unroll
            for (int j = 0; j < IPT; ++j) {
                const uint64_t row = r0 + (uint64_t)j * WAVE;
                VC v{};
                if (rounds >> j & 1u) v = reinterpret_cast<const VC*>(values)[row];
                __builtin_memcpy(vr + j * VB, &v, VB);
            }
        }
        __syncthreads();
        for (uint32_t b = tid; b <= m; b += MSPLIT_WG) {
            uint32_t c = cur[b];
#pragma unroll
            for (int w = 0; w < MSPLIT_WAVES; ++w) {
                const uint32_t x = wc[w][b];
                wc[w][b] = c;
                c += x;
            }
            cur[b] = c;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < IPT; ++j) br[j] = wc[wave][br[j] & 0xFFFu] + (br[j] >> 12);
        __syncthreads();  // (the next tile's zeros come behind these reads)
        rounds = msplit_rounds(have);
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const uint64_t row = r0 + (uint64_t)j * WAVE;
            const uint64_t dst = br[j];
            if (!(rounds >> j & 1u) || dst >= n) continue;  // (dst >= n: never, while the inputs are what the count launch read)
            if (out_keys) {
                KC c;
                __builtin_memcpy(&c, &raw[j], KB);
                reinterpret_cast<KC*>(out_keys)[dst] = c;
            }
            if constexpr (VB > 0) {
                VC v;
                __builtin_memcpy(&v, vr + j * VB, VB);
                reinterpret_cast<VC*>(out_values)[dst] = v;
            }
            if (out_index) {
                if (ib == 8) reinterpret_cast<uint64_t*>(out_index)[dst] = row;
                else reinterpret_cast<uint32_t*>(out_index)[dst] = (uint32_t)row;
            }
        }
    }
}

}  // namespace rsx
