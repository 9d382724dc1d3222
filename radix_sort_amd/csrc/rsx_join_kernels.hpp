// rsx_join_kernels.hpp -- the kernels behind rsx_join_device (rsx.hip; launched by rsx_search.hip): the sort-merge join
// of two key arrays a and b that are each sorted by mapped key.  With lo(i) / hi(i) the lower and upper bound of a[i] in
// b, m(i) = hi(i) - lo(i) and c(i) the rows a[i] contributes (include/rsx.h: m, max(m, 1), m > 0, m == 0 for inner, left,
// semi, anti), S(i) = c(0) + ... + c(i - 1), row t = S(i) + r is (A(i), B(lo(i) + r)).  Three launches:
//   1. rsx_join_count_kernel<KB>: one workgroup per JOIN_TILE consecutive keys of a.  Steps a-c are rsx_search_kernel's,
//      through its own functions: the window of the tile's smallest and largest key by two wave searches, the window
//      staged in LDS when it holds at most search_window(KB) keys, both bounds of the thread's four keys in step.  a is
//      sorted, so its keys are ordered needles: the search kernel's streaming case.  Then c(i) from the bounds (0 for
//      i >= N_a) and its exclusive sum inside the tile in ELEMENT order: the search layout is strided (thread t holds
//      t, t + 256, ...), so the four strides are four block scans, each a wave scan by shuffles, and the sixteen wave
//      totals go through LDS once.  It writes ws_lo[i] (u32: lo(i), or NONE for an unmatched key of a left join, so that
//      the write kernel needs no second flag), ws_local[i] (u64) and tile_total[tile] (u64), for every i < na.
//   2. rsx_join_scan_kernel: one workgroup, the exclusive sum of tile_total into tile_base[0 .. tiles]; tile_base[tiles]
//      = T also goes to out_num[0].
//   3. rsx_join_write_kernel<IB>: untyped in the key.  One workgroup per JOIN_ROWS consecutive OUTPUT rows [t0, t1), t1 =
//      min(t0 + JOIN_ROWS, T, capacity); a workgroup whose t0 lies behind that leaves at once.  Row t belongs to the
//      largest i with S(i) <= t, S(i) = tile_base[i / JOIN_TILE] + ws_local[i]; since S(i + 1) > t that key has c(i) > 0,
//      and keys that contribute nothing fall out of the search by themselves.  Wave 0 finds the key of row t0 and wave 1
//      that of row t1 - 1, each by two 64-ary searches (tile_base, then the ws_local of one count tile).  When the keys
//      between them are at most JOIN_SPAN = 4 * JOIN_ROWS (a join in which one key of a in four finds a match still
//      stays below it), their S(i) - t0, clamped to [0, JOIN_ROWS], go to LDS as u16 and every row does one binary search
//      there, eight rows of a thread in step; otherwise every row does the two-level binary search in global memory.
//      Thread k stores rows t0 + k, t0 + k + 256, ...: every store of a wave is one contiguous range.
// No workgroup waits for another one and there are no atomics: the same input gives the same bytes on every call.  What
// the kernels promise for inputs that are NOT sorted: the bounds come from rsx_search_kernel's clamped searches, so
// lo(i) <= hi(i) <= N_b and c(i) <= max(N_b, 1); S is then still the exact prefix sum of c, every row finds a key with
// r < c(i), every b position is below N_b (and clamped below nb once more before b_index is read), every a position is
// below na.
#pragma once

#include "rsx_search_kernels.hpp"

namespace rsx {

constexpr uint32_t JOIN_WG = SEARCH_WG;
constexpr uint32_t JOIN_TILE = search_tile(4);    // keys of a per count workgroup (one value for every key width)
static_assert(search_tile(1) == JOIN_TILE && search_tile(2) == JOIN_TILE && search_tile(8) == JOIN_TILE && search_tile(16) == JOIN_TILE,
              "the write kernel knows one count tile");
constexpr uint32_t JOIN_RPT = 8;                  // rows per thread of the write kernel
constexpr uint32_t JOIN_ROWS = JOIN_WG * JOIN_RPT;  // rows per write workgroup
constexpr uint32_t JOIN_SPAN = 4 * JOIN_ROWS;     // keys of a whose S the write kernel stages in LDS at most (u16: 16 KiB)
static_assert(JOIN_ROWS <= 0xFFFFu, "a staged S - t0 is 16 bits wide");
constexpr uint32_t JOIN_SCAN_IPT = 8;             // tile totals per thread and sweep of the scan kernel
constexpr uint32_t JOIN_NONE = 0xFFFFFFFFu;
enum : uint32_t { JOIN_INNER = 0, JOIN_LEFT = 1, JOIN_SEMI = 2, JOIN_ANTI = 3 };  // RSX_JOIN_*

// inclusive sum over the wave
__device__ __forceinline__ uint64_t join_wave_scan(uint64_t x) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
#pragma unroll
    for (int o = 1; o < (int)WAVE; o <<= 1) {
        const uint64_t y = pairs_shfl_up<uint64_t>(x, o);
        if (lane >= (uint32_t)o) x += y;
    }
    return x;
}

template <int KB>
__global__ __launch_bounds__(JOIN_WG) void rsx_join_count_kernel(const uint8_t* __restrict__ a, uint64_t na, const uint64_t* __restrict__ a_num,
                                                                 const uint8_t* __restrict__ b, uint64_t nb, const uint64_t* __restrict__ b_num,
                                                                 uint32_t kind, uint32_t desc, uint32_t how, uint32_t* __restrict__ ws_lo,
                                                                 uint64_t* __restrict__ ws_local, uint64_t* __restrict__ tile_total) {
    using K = typename PairsKey<KB>::type;
    constexpr int IPT = (int)search_ipt(KB), NW = (int)(JOIN_WG / WAVE);
    constexpr uint32_t WINDOW = search_window(KB);
    __shared__ K s_win[WINDOW];
    __shared__ K s_min[NW], s_max[NW];
    __shared__ uint64_t s_bound[2];
    __shared__ uint64_t s_tot[IPT][NW];

    uint64_t NA = na, NB = nb;
    if (a_num) {
        const uint64_t have = a_num[0];
        NA = have < na ? have : na;
    }
    if (b_num) {
        const uint64_t have = b_num[0];
        NB = have < nb ? have : nb;
    }
    // a. the keys of this thread, mapped, and the tile's key range
    const uint64_t i0 = (uint64_t)blockIdx.x * JOIN_TILE + threadIdx.x;
    K key[IPT];
    bool valid[IPT];
    K kmin = search_key_max<K>(), kmax{};
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const uint64_t i = i0 + (uint64_t)j * JOIN_WG;
        key[j] = K{};
        valid[j] = i < NA;
        if (valid[j]) {
            key[j] = search_hay<KB>(a, i, kind, desc);
            if (key[j] < kmin) kmin = key[j];
            if (kmax < key[j]) kmax = key[j];
        }
    }
    // (a tile without a valid key holds kmin = all ones, kmax = 0: an empty window, every count 0)
#pragma unroll
    for (int w = WAVE / 2; w > 0; w >>= 1) {
        const K x = pairs_shfl_xor<K>(kmin, w), y = pairs_shfl_xor<K>(kmax, w);
        if (x < kmin) kmin = x;
        if (kmax < y) kmax = y;
    }
    const uint32_t wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (lane == 0) {
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
        const uint64_t r = wave == 0 ? search_wave_bound<KB, false>(b, NB, k, kind, desc) : search_wave_bound<KB, true>(b, NB, k, kind, desc);
        if (lane == 0) s_bound[wave] = r;
    }
    __syncthreads();
    const uint64_t lo = s_bound[0];
    const uint64_t hi = s_bound[1] < lo ? lo : s_bound[1];  // unsorted inputs: the end is clamped, not trusted
    const uint64_t cnt = hi - lo;
    // c. both bounds of the four keys, in step: lower first, upper from lower on
    uint64_t lower[IPT], m[IPT];
    if (cnt == 0) {
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            lower[j] = lo;
            m[j] = 0;
        }
    } else if (cnt <= (uint64_t)WINDOW) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)cnt; i += JOIN_WG) s_win[i] = search_hay<KB>(b, lo + i, kind, desc);
        __syncthreads();
        const auto at = [&](uint32_t i) -> K { return s_win[i]; };
        uint32_t base[IPT], len[IPT];
#pragma unroll
        for (int j = 0; j < IPT; ++j) base[j] = 0;
        search_in_step_whole<K, false, IPT, uint32_t>(at, base, (uint32_t)cnt, key);
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            lower[j] = lo + base[j];
            len[j] = (uint32_t)cnt - base[j];
        }
        search_in_step<K, true, IPT, uint32_t>(at, base, len, (uint32_t)cnt, (uint32_t)cnt, key);
#pragma unroll
        for (int j = 0; j < IPT; ++j) m[j] = lo + base[j] - lower[j];
    } else {
        const auto at = [&](uint64_t i) -> K { return search_hay<KB>(b, lo + i, kind, desc); };
        uint64_t base[IPT], len[IPT];
#pragma unroll
        for (int j = 0; j < IPT; ++j) base[j] = 0;
        search_in_step_whole<K, false, IPT, uint64_t>(at, base, cnt, key);
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            lower[j] = lo + base[j];
            len[j] = cnt - base[j];
        }
        search_in_step<K, true, IPT, uint64_t>(at, base, len, cnt, cnt, key);
#pragma unroll
        for (int j = 0; j < IPT; ++j) m[j] = lo + base[j] - lower[j];
    }
    // the rows of every key, and their sums in element order: stride j is one block scan behind the strides before it
    uint64_t c[IPT], incl[IPT];
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        c[j] = !valid[j] ? 0u : how == JOIN_INNER ? m[j] : how == JOIN_LEFT ? (m[j] ? m[j] : 1u) : how == JOIN_SEMI ? (m[j] ? 1u : 0u) : (m[j] ? 0u : 1u);
        incl[j] = join_wave_scan(c[j]);
        if (lane == WAVE - 1) s_tot[j][wave] = incl[j];
    }
    __syncthreads();
    uint64_t run = 0;  // the rows of the strides in front of stride j
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        uint64_t front = run;  // ... and of the waves in front of this one
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const uint64_t t = s_tot[j][w];
            if ((uint32_t)w < wave) front += t;
            run += t;
        }
        const uint64_t i = i0 + (uint64_t)j * JOIN_WG;
        if (i < na) {
            ws_lo[i] = (how == JOIN_LEFT && m[j] == 0) ? JOIN_NONE : (uint32_t)lower[j];
            ws_local[i] = front + incl[j] - c[j];
        }
    }
    if (threadIdx.x == 0) tile_total[blockIdx.x] = run;
}

// tile_base[0 .. tiles]: the exclusive sums of tile_total[0 .. tiles) and, in tile_base[tiles] and out_num[0], their sum
__global__ __launch_bounds__(JOIN_WG) void rsx_join_scan_kernel(const uint64_t* __restrict__ tile_total, uint64_t* __restrict__ tile_base, uint64_t tiles,
                                                                uint64_t* __restrict__ out_num) {
    constexpr int IPT = (int)JOIN_SCAN_IPT, NW = (int)(JOIN_WG / WAVE);
    __shared__ uint64_t s_tot[NW];
    const uint32_t wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    uint64_t carry = 0;
    for (uint64_t s0 = 0; s0 < tiles; s0 += (uint64_t)JOIN_WG * IPT) {
        const uint64_t e0 = s0 + (uint64_t)threadIdx.x * IPT;  // IPT consecutive tiles per thread
        uint64_t v[IPT], sum = 0;
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            v[j] = e0 + j < tiles ? tile_total[e0 + j] : 0u;
            sum += v[j];
        }
        const uint64_t incl = join_wave_scan(sum);
        if (lane == WAVE - 1) s_tot[wave] = incl;
        __syncthreads();
        uint64_t front = carry, all = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const uint64_t t = s_tot[w];
            if ((uint32_t)w < wave) front += t;
            all += t;
        }
        uint64_t x = front + incl - sum;
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            if (e0 + j < tiles) tile_base[e0 + j] = x;
            x += v[j];
        }
        carry += all;
        __syncthreads();  // s_tot is written again by the next sweep
    }
    if (threadIdx.x == 0) {
        tile_base[tiles] = carry;
        out_num[0] = carry;
    }
}

// na >= 1 keys in `tiles` = ceil(na / JOIN_TILE) count tiles.  a_index / b_index: null, or the IB-byte words to emit in
// place of positions.  out_b null: semi and anti joins.
template <int IB>
__global__ __launch_bounds__(JOIN_WG) void rsx_join_write_kernel(const uint32_t* __restrict__ ws_lo, const uint64_t* __restrict__ ws_local,
                                                                 const uint64_t* __restrict__ tile_base, uint64_t tiles, uint64_t na, uint64_t nb,
                                                                 const uint8_t* __restrict__ a_index, const uint8_t* __restrict__ b_index,
                                                                 uint8_t* __restrict__ out_a, uint8_t* __restrict__ out_b, uint64_t capacity) {
    using I = typename std::conditional<IB == 4, uint32_t, uint64_t>::type;
    constexpr int G = (int)JOIN_RPT;
    __shared__ uint16_t s_rel[JOIN_SPAN];
    __shared__ uint64_t s_end[2];  // the keys of rows t0 and t1 - 1

    const uint64_t T = tile_base[tiles];
    const uint64_t stop = T < capacity ? T : capacity;
    const uint64_t t0 = (uint64_t)blockIdx.x * JOIN_ROWS;
    if (t0 >= stop) return;
    const uint64_t t1 = stop - t0 < JOIN_ROWS ? stop : t0 + JOIN_ROWS;
    const uint32_t wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    // the largest i with S(i) <= t: the last tile whose base is not above t, then the last key of it whose sum is not
    if (wave < 2) {
        const uint64_t t = wave == 0 ? t0 : t1 - 1;
        uint64_t k = search_wave_count(tiles, [&](uint64_t p) { return tile_base[p] <= t; });
        k = k == 0 ? 0 : k - 1;  // (tile_base[0] == 0: k >= 1)
        const uint64_t first = k * JOIN_TILE;
        const uint64_t in_tile = na - first < JOIN_TILE ? na - first : JOIN_TILE;
        const uint64_t rest = t - tile_base[k];
        uint64_t e = search_wave_count(in_tile, [&](uint64_t p) { return ws_local[first + p] <= rest; });
        e = e == 0 ? 0 : e - 1;  // (ws_local[first] == 0: e >= 1)
        if (lane == 0) s_end[wave] = first + e;
    }
    __syncthreads();
    const uint64_t e_lo = s_end[0];
    const uint64_t e_hi = s_end[1] < e_lo ? e_lo : s_end[1];
    const uint64_t span = e_hi - e_lo + 1;

    uint64_t t[G], i[G], r[G];
#pragma unroll
    for (int g = 0; g < G; ++g) t[g] = t0 + threadIdx.x + (uint64_t)g * JOIN_WG;  // (rows at t1 and beyond are searched like the others, not stored)
    if (span <= (uint64_t)JOIN_SPAN) {
        // S(i) - t0 of the keys e_lo .. e_hi, clamped to [0, JOIN_ROWS]: only e_lo can lie below t0, and a key above
        // t1 - 1 is never the answer
        for (uint32_t p = threadIdx.x; p < (uint32_t)span; p += JOIN_WG) {
            const uint64_t e = e_lo + p;
            const uint64_t S = tile_base[e / JOIN_TILE] + ws_local[e];
            s_rel[p] = (uint16_t)(S <= t0 ? 0u : S - t0 >= JOIN_ROWS ? JOIN_ROWS : (uint32_t)(S - t0));
        }
        __syncthreads();
        const uint64_t S_first = tile_base[e_lo / JOIN_TILE] + ws_local[e_lo];
        const auto at = [&](uint32_t p) -> uint16_t { return s_rel[p]; };
        uint32_t base[G];
        uint16_t rel[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            base[g] = 0;
            rel[g] = (uint16_t)(t[g] - t0);  // (below JOIN_ROWS)
        }
        search_in_step_whole<uint16_t, true, G, uint32_t>(at, base, (uint32_t)span, rel);  // base: the keys with S - t0 <= rel, >= 1
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const uint32_t p = base[g] == 0 ? 0u : base[g] - 1;
            i[g] = e_lo + p;
            r[g] = p == 0 ? t[g] - S_first : (uint64_t)((uint32_t)rel[g] - (uint32_t)s_rel[p]);
        }
    } else {
        // too many keys between the two ends (most of them contribute nothing): every row searches tile_base[k_lo ..
        // k_hi], then the ws_local of its tile
        const uint64_t k_lo = e_lo / JOIN_TILE, k_hi = e_hi / JOIN_TILE;
        const auto at = [&](uint64_t p) -> uint64_t { return tile_base[k_lo + p]; };
        uint64_t kt[G];
#pragma unroll
        for (int g = 0; g < G; ++g) kt[g] = 0;
        search_in_step_whole<uint64_t, true, G, uint64_t>(at, kt, k_hi - k_lo + 1, t);
        uint64_t first[G], rest[G];
        uint32_t pos[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const uint64_t k = k_lo + (kt[g] == 0 ? 0 : kt[g] - 1);
            first[g] = k * JOIN_TILE;
            const uint64_t tb = tile_base[k];
            rest[g] = t[g] < tb ? 0 : t[g] - tb;
            pos[g] = 0;
        }
        // the number of p in [0, JOIN_TILE) with first + p < na and ws_local[first + p] <= rest
        for (uint32_t len = JOIN_TILE; len > 1; len -= len >> 1) {
            const uint32_t half = len >> 1;
            uint64_t probe[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const uint64_t e = first[g] + pos[g] + half - 1;
                probe[g] = ws_local[e < na ? e : na - 1];
            }
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (first[g] + pos[g] + half - 1 < na && probe[g] <= rest[g]) pos[g] += half;
        }
        uint64_t sum[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const uint64_t e = first[g] + pos[g];
            if (e < na && ws_local[e] <= rest[g]) ++pos[g];
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            i[g] = first[g] + (pos[g] == 0 ? 0u : pos[g] - 1);
            sum[g] = ws_local[i[g]];
            r[g] = rest[g] < sum[g] ? 0 : rest[g] - sum[g];
        }
    }
    // the stores
    constexpr I NONE = (I)~(I)0;
    uint32_t lo[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (i[g] >= na) i[g] = na - 1;
        lo[g] = ws_lo[i[g]];
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (t[g] >= t1) continue;
        reinterpret_cast<I*>(out_a)[t[g]] = a_index ? reinterpret_cast<const I*>(a_index)[i[g]] : (I)i[g];
        if (out_b) {
            I v = NONE;
            if (lo[g] != JOIN_NONE) {
                uint64_t j = (uint64_t)lo[g] + r[g];
                if (j >= nb) j = nb - 1;  // (never, while S is the sum of c: r < c(i) <= N_b - lo)
                v = b_index ? reinterpret_cast<const I*>(b_index)[j] : (I)j;
            }
            reinterpret_cast<I*>(out_b)[t[g]] = v;
        }
    }
}

}  // namespace rsx
