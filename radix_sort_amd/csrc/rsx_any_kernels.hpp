// rsx_any_kernels.hpp -- the kernels that let layouts without a sort kernel of their own (any element size, keys of
// 1..16 bytes) reach the existing ones (rsx.hip, sort_any_locked):
//   rsx_any_move_kernel   streams elements of one size into elements of another through LDS, byte by byte after a
//                         per-layout map (route A's re-layout and restore, route B's key-index proxies), and can write
//                         a verbatim copy of what it read on the way (route B's copy of the input into d_tmp);
//   rsx_row_gather_kernel d_data[i] = d_tmp[proxy[i].index], a lane group per row (route B's last step).
// Both read and write at any byte alignment without touching a byte outside the n elements.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsx {

constexpr uint32_t ANY_MAP_MAX = 32;  // output elements of the mapped form have at most 32 bytes
constexpr int16_t ANY_ZERO = -1;      // map codes (>= 0: that byte of the source element)
constexpr int16_t ANY_SIGN = -2;      // 0xFF if the source's key is negative, else 0 (sign extension)
constexpr int16_t ANY_INDEX = -8;     // ANY_INDEX - b: byte b of the element's u32 position in the array

struct AnyMap {
    int16_t m[ANY_MAP_MAX];  // per output byte
    uint32_t sign_off;       // source byte whose top bit ANY_SIGN repeats (the key's most significant byte)
};

// k / s for k < 2^24 (tile offsets): float reciprocal, then one correction either way
__device__ __forceinline__ uint32_t any_div(uint32_t k, uint32_t s, float rcp) {
    uint32_t e = (uint32_t)((float)k * rcp);
    if (e * s > k) --e;
    else if ((e + 1) * s <= k) ++e;
    return e;
}

// Writes `bytes` output bytes at d (any alignment): whole aligned dwords where they lie inside, single bytes at the
// two ends.  value4(k) gives the 4 bytes at output offsets k..k+3, value1(k) one byte.
template <class F4, class F1>
__device__ __forceinline__ void any_emit(uint8_t* __restrict__ d, uint32_t bytes, F4 value4, F1 value1) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(d), hi = lo + bytes;
    const uintptr_t w0 = lo & ~(uintptr_t)3;
    const uint32_t nw = (uint32_t)((((hi + 3) & ~(uintptr_t)3) - w0) / 4);
    for (uint32_t w = threadIdx.x; w < nw; w += blockDim.x) {
        const uintptr_t a = w0 + 4u * (uintptr_t)w;
        if (a >= lo && a + 4 <= hi) {
            *reinterpret_cast<uint32_t*>(a) = value4((uint32_t)(a - lo));
        } else {
            for (uint32_t j = 0; j < 4; ++j)
                if (a + j >= lo && a + j < hi) *reinterpret_cast<uint8_t*>(a + j) = value1((uint32_t)(a + j - lo));
        }
    }
}

// One tile of `tile` elements per step: the tile's source bytes are staged in LDS by aligned 16-byte loads (bytes at
// the two ends one by one, so nothing outside [src, src + n * s_in) is read), then
//   MAPPED: every output element of s_out bytes is assembled from its source element after `map`, into dst;
//   COPY:   the source bytes are written unchanged to dst2 (same element size, any alignment).
template <bool MAPPED, bool COPY>
__global__ __launch_bounds__(256) void rsx_any_move_kernel(const uint8_t* __restrict__ src, uint32_t s_in, uint8_t* __restrict__ dst,
                                                           uint32_t s_out, uint8_t* __restrict__ dst2, uint64_t n, uint32_t tile,
                                                           AnyMap map, float rcp_out) {
    extern __shared__ uint4 any_lds[];
    __shared__ int16_t smap[ANY_MAP_MAX];
    const uint8_t* lb = reinterpret_cast<const uint8_t*>(any_lds);
    if (MAPPED && threadIdx.x < ANY_MAP_MAX) smap[threadIdx.x] = map.m[threadIdx.x];
    const uint64_t tiles = (n + tile - 1) / tile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t e0 = t * tile;
        const uint32_t ne = (uint32_t)(n - e0 < tile ? n - e0 : tile);
        const uintptr_t lo = reinterpret_cast<uintptr_t>(src) + e0 * s_in, hi = lo + (uint64_t)ne * s_in;
        const uintptr_t c0 = lo & ~(uintptr_t)15;
        const uint32_t head = (uint32_t)(lo - c0);
        const uint32_t nch = (uint32_t)((((hi + 15) & ~(uintptr_t)15) - c0) / 16);
        for (uint32_t c = threadIdx.x; c < nch; c += blockDim.x) {
            const uintptr_t a = c0 + 16u * (uintptr_t)c;
            uint4 v;
            if (a >= lo && a + 16 <= hi) {
                v = *reinterpret_cast<const uint4*>(a);
            } else {
                uint32_t w[4] = {0, 0, 0, 0};
                for (uint32_t j = 0; j < 16; ++j)
                    if (a + j >= lo && a + j < hi) w[j >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(a + j) << (8 * (j & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            any_lds[c] = v;
        }
        __syncthreads();
        if constexpr (MAPPED) {
            // byte o of output element e (tile-local)
            auto byte_of = [&](uint32_t e, uint32_t o) -> uint32_t {
                const int16_t m = smap[o];
                const uint32_t base = head + e * s_in;
                if (m >= 0) return lb[base + (uint32_t)m];
                if (m == ANY_ZERO) return 0u;
                if (m == ANY_SIGN) return (lb[base + map.sign_off] & 0x80u) ? 0xFFu : 0u;
                return (uint32_t)((e0 + e) >> (8 * (uint32_t)(ANY_INDEX - m))) & 0xFFu;
            };
            auto value4 = [&](uint32_t k) -> uint32_t {
                uint32_t e = any_div(k, s_out, rcp_out), o = k - e * s_out, v = 0;
                for (uint32_t j = 0; j < 4; ++j) {
                    v |= byte_of(e, o) << (8 * j);
                    if (++o == s_out) { o = 0; ++e; }
                }
                return v;
            };
            auto value1 = [&](uint32_t k) -> uint8_t {
                const uint32_t e = any_div(k, s_out, rcp_out);
                return (uint8_t)byte_of(e, k - e * s_out);
            };
            any_emit(dst + e0 * s_out, ne * s_out, value4, value1);
        }
        if constexpr (COPY) {
            uint8_t* d2 = dst2 + e0 * s_in;
            if (((reinterpret_cast<uintptr_t>(d2) - lo) & 3) == 0) {  // same alignment mod 4: dwords straight from LDS
                any_emit(d2, ne * s_in, [&](uint32_t k) { return *reinterpret_cast<const uint32_t*>(lb + head + k); },
                         [&](uint32_t k) { return lb[head + k]; });
            } else {
                any_emit(d2, ne * s_in,
                         [&](uint32_t k) {
                             return (uint32_t)lb[head + k] | (uint32_t)lb[head + k + 1] << 8 | (uint32_t)lb[head + k + 2] << 16 |
                                    (uint32_t)lb[head + k + 3] << 24;
                         },
                         [&](uint32_t k) { return lb[head + k]; });
            }
        }
        __syncthreads();
    }
}

// dst row r = src row proxy[r].index (rows of `words` W-sized words; W divides the row size and both base addresses).
// 2^gshift lanes per row (at most 16: four or more rows in flight per wave); the stores run in row order.
template <typename W>
__global__ __launch_bounds__(256) void rsx_row_gather_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t words,
                                                             const uint8_t* __restrict__ proxy, uint32_t p, uint32_t idx_off, uint64_t n,
                                                             uint32_t gshift) {
    const uint32_t G = 1u << gshift;
    const uint32_t lane = threadIdx.x & (G - 1);
    const uint64_t groups = ((uint64_t)gridDim.x * blockDim.x) >> gshift;
    const uint64_t row = (uint64_t)words * sizeof(W);
    for (uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> gshift; r < n; r += groups) {
        const uint32_t idx = *reinterpret_cast<const uint32_t*>(proxy + r * p + idx_off);
        if (idx >= n) continue;  // (a permutation of 0..n-1 by construction)
        const W* s = reinterpret_cast<const W*>(src + (uint64_t)idx * row);
        W* d = reinterpret_cast<W*>(dst + r * row);
        for (uint32_t j = lane; j < words; j += G) d[j] = s[j];
    }
}

}  // namespace rsx
