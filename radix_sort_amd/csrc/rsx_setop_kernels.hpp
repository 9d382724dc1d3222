// rsx_setop_kernels.hpp -- the kernel behind rsx_setop_device (rsx.hip; launched by rsx_setops.hip): union, intersection,
// difference and symmetric difference of two key arrays a[N_a] and b[N_b] that are sorted by mapped key (complemented for
// descending order), as multisets (std::set_union and its siblings), with optional values and optional source positions.
// include/rsx.h has the definition: a[i] of rank r inside its run of equal keys is MATCHED when b holds more than r keys
// equal to it, b[j] likewise against a, and an operation keeps the matched or the unmatched elements of a side; the kept
// elements come out in the order of the stable merge (equal keys of a first).
// Three launches, the shape of rsx_unique_kernels.hpp, over tiles of setop_tile(KB) consecutive positions of the MERGE:
//   rsx_setop_kernel<KB, 0, 0, false>   the count form: tile t -> tile_count[t], its kept elements; it also saves the
//                                       tile's two cuts and the global lower bounds of its first key (tile_save)
//   rsx_unique_scan_kernel              ONE workgroup: tile_base[t] = kept in front of tile t, and their sum
//   rsx_setop_kernel<KB, VB, IB, true>  the write form: the flags again from the saved cuts, ranked inside the workgroup,
//                                       keys and source slots compacted in LDS, stored as contiguous ranges from tile_base[t]
// The kernel runs steps a to c of rsx_merge_kernel through the functions of rsx_merge_kernels.hpp (the cuts, the clamp, the
// staging, the thread's cut, the serial merge) and decides every element while it merges:
//   e. the keep flag.  A thread carries la, lb: the lower bounds, relative to the staged a-range and b-range, of the key
//      it is on.  At its first output they come from two binary searches in LDS; at every change of key they are the
//      current ai, bi (everything smaller has been taken, and a goes first among ties).  Only the tile's FIRST key can
//      have its run begin in front of the tile: for that key waves 0 and 1 find the global A_lo and B_lo in a[0, a0) and
//      b[0, b0) by the 64-ary search (search_wave_bound), each only when the key in front of its range equals it, and
//      la = A_lo - a0, lb = B_lo - b0 (zero or negative).  a[a0 + ai] then probes position lb + (ai - la) of the b-range,
//      b[b0 + bi] position la + (bi - lb) of the a-range: one read, from LDS when the position lies in the staged range,
//      else from global memory with the position checked against N_b / N_a.  A run that goes on behind the tile needs
//      nothing more: its probes land behind the staged range.
//   f. count form: the flags summed (wave_incl_scan, the waves' totals through LDS).  Write form: a kept output of rank q
//      puts its mapped key and u16 source slot at q in LDS; thread t then stores outputs t, t + MERGE_WG, ... as step d of
//      the merge kernel does, so every store of a wave is one contiguous range.
// N_a = na or min(na, *a_num), N_b likewise, read on the device; the grid comes from the host's na + nb and the tiles at or
// past N_a + N_b store a zero count and leave.  No workgroup waits for another one and there are no atomics.
// What is promised when the inputs are NOT sorted: merge_clamp keeps both staged ranges inside the arrays, every LDS read
// is bounded by acnt / bcnt, every global probe by N_a / N_b, every store by `cap` rows, and out_num[0] = min(sum, cap);
// every position is below na + nb.
#pragma once

#include "rsx_merge_kernels.hpp"

namespace rsx {

constexpr uint32_t SETOP_UNION = 0, SETOP_INTERSECTION = 1, SETOP_DIFFERENCE = 2, SETOP_SYMMETRIC_DIFFERENCE = 3;
// the merge's tile: the same LDS, the same chain of latencies per tile
constexpr uint32_t setop_tile(uint32_t kb) { return merge_tile(kb, 0); }
constexpr uint32_t SETOP_SAVE = 4;  // u64 words of tile_save per tile: cut(d0), cut(d1), A_lo, B_lo
// static LDS of one workgroup at most: keys, slots, the two cuts, the two bounds, the waves' totals
constexpr uint32_t setop_lds_bytes(uint32_t kb) { return setop_tile(kb) * (kb + 2u) + 64u; }
static_assert(setop_tile(1) <= 4096u && setop_tile(8) <= 4096u && setop_tile(16) <= 4096u, "rsx_unique_scan_kernel: at most 4096 per tile");

template <typename K>
__device__ __forceinline__ bool setop_same(const K& a, const K& b) {
    return !(a != b);
}

// the number of keys before `key` in s[0, cnt) (sorted); reads below cnt only
template <typename K>
__device__ __forceinline__ uint32_t setop_lower(const K* s, uint32_t cnt, const K& key) {
    uint32_t lo = 0, len = cnt;
    while (len > 0) {
        const uint32_t half = len >> 1;
        if (s[lo + half] < key) {
            lo += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return lo;
}

// WRITE false (VB = IB = 0): tile_count and tile_save are written.  WRITE true: tile_save, tile_base and raw_num (the
// scan's sum) are read; out_keys may be null, VB > 0: a_values and out_values are given, and b_values when the operation
// emits from b; IB > 0: out_index is.
template <int KB, int VB, int IB, bool WRITE>
__global__ __launch_bounds__(MERGE_WG) void rsx_setop_kernel(const uint8_t* __restrict__ a_keys, const uint8_t* __restrict__ a_values, uint64_t na,
                                                             const uint64_t* __restrict__ a_num, const uint8_t* __restrict__ b_keys,
                                                             const uint8_t* __restrict__ b_values, uint64_t nb, const uint64_t* __restrict__ b_num,
                                                             uint32_t op, uint32_t kind, uint32_t desc, uint32_t* __restrict__ tile_count,
                                                             uint64_t* tile_save, const uint64_t* __restrict__ tile_base,
                                                             const uint64_t* __restrict__ raw_num, uint64_t cap, uint8_t* __restrict__ out_keys,
                                                             uint8_t* __restrict__ out_values, uint8_t* __restrict__ out_index,
                                                             uint64_t* __restrict__ out_num) {
    using K = typename PairsKey<KB>::type;
    using I = typename std::conditional<IB == 4, uint32_t, uint64_t>::type;
    constexpr int IPT = (int)merge_ipt(KB), NW = (int)(MERGE_WG / WAVE);
    constexpr uint32_t TILE = setop_tile(KB);
    constexpr bool SLOTS = WRITE && (VB > 0 || IB > 0);
    static_assert(WRITE || (VB == 0 && IB == 0), "the count form moves nothing");
    static_assert(IPT <= 32, "a thread's flags are bits of one word");
    __shared__ K s_key[TILE];
    __shared__ uint16_t s_slot[SLOTS ? TILE : 1];
    __shared__ uint64_t s_cut[2];
    __shared__ uint64_t s_lo[2];
    __shared__ uint32_t s_wave[NW];

    uint64_t Na = na, Nb = nb;
    if (a_num) {
        const uint64_t have = a_num[0];
        Na = have < na ? have : na;
    }
    if (b_num) {
        const uint64_t have = b_num[0];
        Nb = have < nb ? have : nb;
    }
    const uint64_t n = Na + Nb;
    if constexpr (WRITE) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const uint64_t sum = raw_num[0];
            out_num[0] = sum < cap ? sum : cap;  // (sorted inputs: the sum itself)
        }
    }
    const uint64_t d0 = (uint64_t)blockIdx.x * TILE;
    if (d0 >= n) {  // the whole workgroup: a tile behind the device counts
        if constexpr (!WRITE) {
            if (threadIdx.x == 0) tile_count[blockIdx.x] = 0;
        }
        return;
    }
    const uint64_t d1 = d0 + TILE < n ? d0 + TILE : n;
    const uint32_t L = (uint32_t)(d1 - d0);
    const uint32_t wave = threadIdx.x / WAVE;
    uint64_t* save = tile_save + (uint64_t)blockIdx.x * SETOP_SAVE;
    // a, b. the two cuts (searched once, by the count form) and the clamp
    uint64_t a0, a1;
    if constexpr (!WRITE) {
        merge_cuts<KB>(a_keys, Na, b_keys, Nb, d0, d1, kind, desc, s_cut);
        __syncthreads();
        a0 = s_cut[0];
        a1 = s_cut[1];
    } else {
        a0 = save[0];
        a1 = save[1];
    }
    uint64_t b0;
    uint32_t acnt, bcnt;
    merge_clamp(a0, a1, d0, L, Na, Nb, &b0, &acnt, &bcnt);
    // c. both ranges -> LDS
    merge_stage<KB, IPT>(a_keys, a0, acnt, b_keys, b0, L, kind, desc, s_key);
    __syncthreads();
    // e. the tile's first key (L >= 1) and the global lower bounds of its run
    const K ka0 = s_key[0], kb0 = s_key[bcnt > 0 ? acnt : 0u];
    const K k0 = merge_pick<K>(acnt > 0 && (bcnt == 0 || !(kb0 < ka0)), ka0, kb0);
    uint64_t A_lo, B_lo;
    if constexpr (!WRITE) {
        if (wave < 2) {
            const uint8_t* keys = wave == 0 ? a_keys : b_keys;
            const uint64_t start = wave == 0 ? a0 : b0;  // a0 <= N_a, b0 <= N_b: every read below is inside the array
            uint64_t lo = start;
            if (start > 0 && setop_same<K>(search_hay<KB>(keys, start - 1, kind, desc), k0)) lo = search_wave_bound<KB, false>(keys, start, k0, kind, desc);
            if ((threadIdx.x & (WAVE - 1)) == 0) s_lo[wave] = lo;
        }
        __syncthreads();
        A_lo = s_lo[0];
        B_lo = s_lo[1];
        if (threadIdx.x == 0) {
            save[0] = a0;
            save[1] = a1;
            save[2] = A_lo;
            save[3] = B_lo;
        }
    } else {
        A_lo = save[2];
        B_lo = save[3];
    }
    // this thread's outputs [dt, dt + IPT) of the tile, merged serially, each with its flag.  la, lb: the lower bounds of the
    // key the thread is on, as positions relative to a0 and b0 (negative where the first key's run begins in front of the tile)
    const uint32_t dt = threadIdx.x * IPT < L ? threadIdx.x * IPT : L;
    uint32_t ai, bi;
    merge_thread_cut<K>(s_key, dt, acnt, bcnt, &ai, &bi);
    const uint32_t ai0 = ai, bi0 = bi;
    K key[WRITE ? IPT : 1];
    K ka{}, kb{};
    if (ai < acnt) ka = s_key[ai];
    if (bi < bcnt) kb = s_key[acnt + bi];
    int64_t la = 0, lb = 0;
    uint32_t flags = 0, sides = 0;  // bit k: output dt + k is kept; it comes from a
    K cur{};
    if (dt < L) {
        cur = merge_pick<K>(RSX_MERGE_TAKE_A(ka, kb, ai, bi, acnt, bcnt), ka, kb);
        if (setop_same<K>(cur, k0)) {  // A_lo <= a0, B_lo <= b0
            la = -(int64_t)(a0 - A_lo);
            lb = -(int64_t)(b0 - B_lo);
        } else {
            la = (int64_t)setop_lower<K>(s_key, ai, cur);
            lb = (int64_t)setop_lower<K>(s_key + acnt, bi, cur);
        }
    }
    const bool probe_a = op != SETOP_UNION;                                     // an element of a is decided by its probe
    const bool emit_b = op == SETOP_UNION || op == SETOP_SYMMETRIC_DIFFERENCE;  // an element of b can be kept
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        if constexpr (WRITE) key[k] = K{};
        if (dt + k < L) {
            const bool take_a = RSX_MERGE_TAKE_A(ka, kb, ai, bi, acnt, bcnt);
            const K kk = merge_pick<K>(take_a, ka, kb);
            if (kk != cur) {
                la = (int64_t)ai;
                lb = (int64_t)bi;
                cur = kk;
            }
            bool matched = false;
            if (take_a ? probe_a : emit_b) {
                // the element's rank in its run (ai - la, bi - lb: la <= ai and lb <= bi always), then the position of that
                // rank in the other array's run, relative to the other staged range: b0 + lb >= B_lo >= 0, a0 + la >= A_lo >= 0
                const uint64_t pl = (uint64_t)(take_a ? lb + ((int64_t)ai - la) : la + ((int64_t)bi - lb));
                const uint32_t ocnt = take_a ? bcnt : acnt, obase = take_a ? acnt : 0u;
                if (pl < (uint64_t)ocnt) {
                    matched = setop_same<K>(s_key[obase + (uint32_t)pl], kk);
                } else {
                    const uint64_t p = (take_a ? b0 : a0) + pl;
                    if (p < (take_a ? Nb : Na)) matched = setop_same<K>(search_hay<KB>(take_a ? b_keys : a_keys, p, kind, desc), kk);
                }
            }
            const bool keep = take_a ? (!probe_a || (op == SETOP_INTERSECTION) == matched) : (emit_b && !matched);
            flags |= (keep ? 1u : 0u) << k;
            sides |= (take_a ? 1u : 0u) << k;
            if constexpr (WRITE) key[k] = kk;
            merge_advance<K>(s_key, take_a, acnt, bcnt, ai, bi, ka, kb);
        }
    }
    // f. the flags summed; every thread is behind its last read of the staged keys at the barrier
    const uint32_t kept = (uint32_t)__popc(flags);
    const uint32_t incl = wave_incl_scan<false>(kept);
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    uint32_t below = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const uint32_t v = s_wave[w];
        below += (uint32_t)w < wave ? v : 0u;
        total += v;
    }
    if constexpr (!WRITE) {
        if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
    } else {
        uint32_t q = below + (incl - kept);  // kept outputs of the tile in front of this thread's: q + kept <= total <= L
        uint32_t sa = ai0, sb = acnt + bi0;  // the source slots again: two ascending runs from the thread's cut on
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            const bool from_a = sides >> k & 1u;
            if (flags >> k & 1u) {
                s_key[q] = key[k];
                if constexpr (SLOTS) s_slot[q] = (uint16_t)(from_a ? sa : sb);
                ++q;
            }
            sa += from_a ? 1u : 0u;
            sb += from_a ? 0u : 1u;
        }
        __syncthreads();
        const uint64_t base = tile_base[blockIdx.x];
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const uint32_t o = threadIdx.x + (uint32_t)j * MERGE_WG;
            if (o >= total || base + o >= cap) continue;
            if (out_keys) {
                const K k = pairs_unmap<K>(s_key[o], kind, desc);
                unsigned char r[KB];
                __builtin_memcpy(r, &k, KB);
                pairs_store<KB>(out_keys + (base + o) * KB, r);
            }
            if constexpr (SLOTS) {
                const uint32_t s = s_slot[o];  // s < acnt: a[a0 + s]; else b[b0 + s - acnt], s - acnt < bcnt
                const bool from_a = s < acnt;
                const uint64_t at = from_a ? a0 + s : b0 + (s - acnt);
                if constexpr (VB > 0) {
                    unsigned char v[VB];
                    pairs_load<VB>(v, (from_a ? a_values : b_values) + at * VB);
                    pairs_store<VB>(out_values + (base + o) * VB, v);
                }
                if constexpr (IB > 0) reinterpret_cast<I*>(out_index)[base + o] = (I)(from_a ? at : na + at);  // (the host's na)
            }
        }
    }
}

}  // namespace rsx
