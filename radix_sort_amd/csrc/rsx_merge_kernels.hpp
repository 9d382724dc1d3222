// rsx_merge_kernels.hpp -- the kernels behind rsx_merge_device (rsx.hip; launched by rsx_merge.hip): the stable merge of two
// key arrays a[na] and b[nb] that are sorted by mapped key (complemented for descending order), with optional values and
// optional source positions.  With c = a ++ b and p the stable permutation that sorts c by mapped key (equal keys of a in
// front of equal keys of b):  out_keys[t] = c[p[t]],  out_values[t] = (a_values ++ b_values)[p[t]],  out_index[t] = p[t].
// One kernel, rsx_merge_kernel<KB, VB, IB> (VB 0: no values, IB 0: no positions; its steps a to c are functions that the
// set-operation kernel of rsx_setop_kernels.hpp calls too); one workgroup of MERGE_WG threads per tile
// of merge_tile(KB, VB) consecutive OUTPUT positions [d0, d1):
//   a. the tile's two cuts on the merge path: cut(d) = the number of elements of a among the first d outputs = the largest
//      i in [max(0, d - nb), min(d, na)] with i == 0, or d - i >= nb, or M(a[i-1]) <= M(b[d-i]) (monotone in i; the <= is
//      what puts a first among ties).  Wave 0 finds cut(d0) and wave 1 cut(d1) at the same time, each by the 64-ary ballot
//      search of the search kernel (search_wave_count), a probe per lane and round and two loads per probe.  The tile
//      behind this one computes cut(d1) again: the price of not waiting for a neighbour.
//   b. the clamp (merge_clamp): the tile takes a[a0 .. a0 + acnt) and b[b0 .. b0 + bcnt), acnt + bcnt = d1 - d0.
//   c. the mapped keys of both ranges go to LDS with coalesced loads; every thread finds the cut of its own IPT consecutive
//      outputs by the same predicate in LDS and merges IPT elements serially, keeping the mapped key of every output and
//      storing its tile-local source slot in LDS, in output order; every LDS read is bounded by acnt / bcnt.
//   d. the keys go back through LDS in output order too; thread t then holds outputs t, t + MERGE_WG, ... so that every
//      store of a wave is one contiguous range: the key mapped back, the value loaded from a_values / b_values by the slot
//      (within the tile two ascending streams, so a wave touches two contiguous ranges), the position from the slot.
// No workgroup waits for another one, there are no atomics, and the kernel needs no workspace.
// What is promised when the inputs are NOT sorted: the counts of the probes keep every cut inside its range, and the clamp
// of step b keeps [a0, a0 + acnt) and [b0, b0 + bcnt) inside the arrays, so every read stays inside the two inputs, every
// write inside the n-entry outputs, and every position is below n.  The output need not be a permutation then.
//   rsx_merge_gather_kernel  the values of any other width (3, 12, 24 ... 32768 bytes): out row r = row pos[r] of
//      a_values ++ b_values, a lane group per row in 16-byte words or bytes (rsx_row_gather_kernel with two sources), from
//      the u64 positions rsx_merge_kernel<KB, 0, 8> left in the context's workspace; it also narrows them into out_index.
// Known weak spots: a call of few tiles pays the two dependent cut searches in full, and the gather of wide values
// reads its rows wherever they lie.
#pragma once

#include "rsx_search_kernels.hpp"

namespace rsx {

constexpr uint32_t MERGE_WG = 256;
// Outputs per thread, by key width.  LDS of a tile: merge_tile * (KB + 2) bytes (mapped keys and u16 slots).  A larger tile
// pays the tile's chain of dependent latencies -- five rounds of the cut search, the loads, the thread's own binary search
// in LDS -- less often, until its LDS and its longer serial merge cost more than that saves.  Measured on one MI355X
// (profiles/merge_variants.jsonl; ms, interleaved keys / all of a below b):
//   4-byte keys, 2^27 + 2^27:   8: 1.94 / 0.97   12: 1.52 / 0.80   16: 1.20 / 0.80   24: 1.09 / 0.82
//   ... with 4-byte values:     8: 2.33 / 1.33   12: 1.97 / 1.29   16: 1.77 / 1.45   24: 1.98 / 1.80
//   ... 2^28 + 2^20, keys:      8: 1.00 / 0.73   12: 0.85 / 0.69   16: 0.87 / 0.74   24: 0.91 / 0.79
//   ... 2^16 + 2^16, keys:      8: 0.021         12: 0.023         16: 0.025         24: 0.028
//   8-byte keys with 4-byte values, 2^26 + 2^26:   4: 2.10 / 1.13   8: 1.39 / 0.91   12: 1.21 / 0.90   16: 1.61 / 1.44
// 16-byte keys were not measured: 4 keeps their tile at 18 KiB of LDS.
#ifndef RSX_MERGE_IPT4
#define RSX_MERGE_IPT4 16  // 1-, 2- and 4-byte keys
#endif
#ifndef RSX_MERGE_IPT8
#define RSX_MERGE_IPT8 12
#endif
#ifndef RSX_MERGE_IPT16
#define RSX_MERGE_IPT16 4
#endif
constexpr uint32_t merge_ipt(uint32_t kb) { return kb == 16 ? RSX_MERGE_IPT16 : kb == 8 ? RSX_MERGE_IPT8 : RSX_MERGE_IPT4; }
// (the value moves through registers only: its width does not change the tile)
constexpr uint32_t merge_tile(uint32_t kb, uint32_t /*vb*/) { return MERGE_WG * merge_ipt(kb); }
// static LDS of one workgroup at most: keys, slots, the two cuts
constexpr uint32_t merge_lds_bytes(uint32_t kb, uint32_t vb) { return merge_tile(kb, vb) * (kb + 2u) + 16u; }

// c ? x : y, on the words of a 16-byte key one by one (the struct as a whole would go through the stack)
template <typename K>
__device__ __forceinline__ K merge_pick(bool c, const K& x, const K& y) {
    return c ? x : y;
}
template <>
__device__ __forceinline__ PairsU128 merge_pick<PairsU128>(bool c, const PairsU128& x, const PairsU128& y) {
    return PairsU128{c ? x.lo : y.lo, c ? x.hi : y.hi};
}

// Step b.  THE WHOLE OF THE IN-BOUNDS PROMISE: whatever the two cut searches returned, the tile reads a[a0 .. a0 + acnt)
// and b[b0 .. b0 + bcnt) with acnt + bcnt = L, and both ranges lie inside their arrays.  a0 is a cut of d0, so
// max(0, d0 - nb) <= a0 <= min(d0, na) and b0 = d0 - a0 is in [0, nb].  acnt is then forced into
// [max(0, L - (nb - b0)), min(L, na - a0)], which is never empty because d0 + L <= na + nb.  For sorted inputs the cuts
// are exact and the clamp changes nothing.
__device__ __forceinline__ void merge_clamp(uint64_t a0, uint64_t a1, uint64_t d0, uint32_t L, uint64_t na, uint64_t nb, uint64_t* b0,
                                            uint32_t* acnt, uint32_t* bcnt) {
    const uint64_t bb = d0 - a0;
    const uint64_t brest = nb - bb, arest = na - a0;
    const uint64_t lo = (uint64_t)L > brest ? (uint64_t)L - brest : 0;
    const uint64_t hi = (uint64_t)L < arest ? (uint64_t)L : arest;
    uint64_t c = a1 > a0 ? a1 - a0 : 0;
    c = c < lo ? lo : c;
    c = c > hi ? hi : c;
    *b0 = bb;
    *acnt = (uint32_t)c;
    *bcnt = L - (uint32_t)c;
}

// Step a, the waves 0 and 1 of the workgroup: cut(d0) and cut(d1) -> s_cut[0], s_cut[1] (the caller's barrier follows).
template <int KB>
__device__ __forceinline__ void merge_cuts(const uint8_t* __restrict__ a_keys, uint64_t na, const uint8_t* __restrict__ b_keys, uint64_t nb, uint64_t d0,
                                           uint64_t d1, uint32_t kind, uint32_t desc, uint64_t* s_cut) {
    using K = typename PairsKey<KB>::type;
    const uint32_t wave = threadIdx.x / WAVE;
    if (wave < 2) {
        const uint64_t d = wave == 0 ? d0 : d1;
        const uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
        // i = lo + 1 + x for x in [0, hi - lo): a[i-1] = a[lo + x] with lo + x < hi <= na, b[d-i] = b[d - lo - 1 - x] with
        // 0 <= d - hi <= d - lo - 1 - x <= d - lo - 1 < nb
        const uint64_t c = search_wave_count(hi - lo, [&](uint64_t x) {
            const K ka = search_hay<KB>(a_keys, lo + x, kind, desc);
            const K kb = search_hay<KB>(b_keys, d - lo - 1 - x, kind, desc);
            return !(kb < ka);
        });
        if ((threadIdx.x & (WAVE - 1)) == 0) s_cut[wave] = lo + c;
    }
}

// Step c, first part: both ranges -> LDS, a's mapped keys at [0, acnt), b's behind them (L = acnt + bcnt <= IPT * MERGE_WG).
template <int KB, int IPT>
__device__ __forceinline__ void merge_stage(const uint8_t* __restrict__ a_keys, uint64_t a0, uint32_t acnt, const uint8_t* __restrict__ b_keys, uint64_t b0,
                                            uint32_t L, uint32_t kind, uint32_t desc, typename PairsKey<KB>::type* s_key) {
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const uint32_t i = threadIdx.x + (uint32_t)j * MERGE_WG;
        if (i < L) s_key[i] = i < acnt ? search_hay<KB>(a_keys, a0 + i, kind, desc) : search_hay<KB>(b_keys, b0 + (i - acnt), kind, desc);
    }
}

// ... second part: the cut of the tile's output dt in LDS, the largest i in [lo, hi] with i == lo or sa[i-1] <= sb[dt-i]
template <typename K>
__device__ __forceinline__ void merge_thread_cut(const K* s_key, uint32_t dt, uint32_t acnt, uint32_t bcnt, uint32_t* ai, uint32_t* bi) {
    uint32_t lo = dt > bcnt ? dt - bcnt : 0, hi = dt < acnt ? dt : acnt;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;  // lo < mid <= hi: mid - 1 < acnt, 0 <= dt - mid < bcnt
        if (!(s_key[acnt + (dt - mid)] < s_key[mid - 1])) lo = mid;
        else hi = mid - 1;
    }
    *ai = lo;
    *bi = dt - lo;
}

// ... third part, one output of the serial merge.  ka = sa[ai] when ai < acnt, kb = sb[bi] when bi < bcnt, and one side at
// least has an element left: which side gives the output (the <= that puts a first among ties).  One definition for both
// kernels, as a macro: through a function the 16-byte-key instantiations of the merge kernel took 2 to 4 more SGPRs.
#define RSX_MERGE_TAKE_A(ka, kb, ai, bi, acnt, bcnt) ((ai) < (acnt) && ((bi) >= (bcnt) || !((kb) < (ka))))
// ... and the step behind it: the next key of the side taken, one LDS read per output whichever side it is (no divergent branch)
template <typename K>
__device__ __forceinline__ void merge_advance(const K* s_key, bool take_a, uint32_t acnt, uint32_t bcnt, uint32_t& ai, uint32_t& bi, K& ka, K& kb) {
    ai += take_a ? 1u : 0u;
    bi += take_a ? 0u : 1u;
    const bool more = take_a ? ai < acnt : bi < bcnt;
    const K next = s_key[more ? (take_a ? ai : acnt + bi) : 0u];
    ka = merge_pick<K>(take_a, next, ka);
    kb = merge_pick<K>(take_a, kb, next);
}

// VB > 0: a_values (na > 0), b_values (nb > 0) and out_values are given; IB > 0: out_index is; out_keys may be null.
template <int KB, int VB, int IB>
__global__ __launch_bounds__(MERGE_WG) void rsx_merge_kernel(const uint8_t* __restrict__ a_keys, const uint8_t* __restrict__ a_values, uint64_t na,
                                                             const uint8_t* __restrict__ b_keys, const uint8_t* __restrict__ b_values, uint64_t nb,
                                                             uint8_t* __restrict__ out_keys, uint8_t* __restrict__ out_values,
                                                             uint8_t* __restrict__ out_index, uint32_t kind, uint32_t desc) {
    using K = typename PairsKey<KB>::type;
    using I = typename std::conditional<IB == 4, uint32_t, uint64_t>::type;
    constexpr int IPT = (int)merge_ipt(KB);
    constexpr uint32_t TILE = merge_tile(KB, VB);
    constexpr bool SLOTS = VB > 0 || IB > 0;
    static_assert(TILE <= 65536u, "slots are u16");
    __shared__ K s_key[TILE];
    __shared__ uint16_t s_slot[SLOTS ? TILE : 1];
    __shared__ uint64_t s_cut[2];

    const uint64_t n = na + nb;
    const uint64_t d0 = (uint64_t)blockIdx.x * TILE;  // (the host launches ceil(n / TILE) tiles: d0 < n)
    const uint64_t d1 = d0 + TILE < n ? d0 + TILE : n;
    const uint32_t L = (uint32_t)(d1 - d0);
    // a. the two cuts
    merge_cuts<KB>(a_keys, na, b_keys, nb, d0, d1, kind, desc, s_cut);
    __syncthreads();
    // b. the clamp
    const uint64_t a0 = s_cut[0];
    uint64_t b0;
    uint32_t acnt, bcnt;
    merge_clamp(a0, s_cut[1], d0, L, na, nb, &b0, &acnt, &bcnt);
    // c. both ranges -> LDS: a's keys at [0, acnt), b's behind them
    merge_stage<KB, IPT>(a_keys, a0, acnt, b_keys, b0, L, kind, desc, s_key);
    __syncthreads();
    // this thread's outputs [dt, dt + IPT) of the tile and their cut
    const uint32_t dt = threadIdx.x * IPT < L ? threadIdx.x * IPT : L;
    uint32_t ai, bi;
    merge_thread_cut<K>(s_key, dt, acnt, bcnt, &ai, &bi);
    K key[IPT];
    K ka{}, kb{};
    if (ai < acnt) ka = s_key[ai];
    if (bi < bcnt) kb = s_key[acnt + bi];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        key[k] = K{};
        if (dt + k < L) {  // ai + bi = dt + k < acnt + bcnt: one side at least has an element left
            const bool take_a = RSX_MERGE_TAKE_A(ka, kb, ai, bi, acnt, bcnt);
            key[k] = merge_pick<K>(take_a, ka, kb);
            // (the slots have an array of their own that nobody reads before the barriers below: stored at once, in output order)
            if constexpr (SLOTS) s_slot[dt + k] = (uint16_t)(take_a ? ai : acnt + bi);
            merge_advance<K>(s_key, take_a, acnt, bcnt, ai, bi, ka, kb);
        }
    }
    __syncthreads();
    // d. the keys in output order, then the stores
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        if (dt + k < L) {
            s_key[dt + k] = key[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const uint32_t o = threadIdx.x + (uint32_t)j * MERGE_WG;
        if (o >= L) continue;
        if (out_keys) {
            const K k = pairs_unmap<K>(s_key[o], kind, desc);
            unsigned char r[KB];
            __builtin_memcpy(r, &k, KB);
            pairs_store<KB>(out_keys + (d0 + o) * KB, r);
        }
        if constexpr (SLOTS) {
            const uint32_t s = s_slot[o];  // s < acnt: a[a0 + s]; else b[b0 + s - acnt], s - acnt < bcnt
            const bool from_a = s < acnt;
            const uint64_t at = from_a ? a0 + s : b0 + (s - acnt);
            if constexpr (VB > 0) {
                unsigned char v[VB];
                pairs_load<VB>(v, (from_a ? a_values : b_values) + at * VB);
                pairs_store<VB>(out_values + (d0 + o) * VB, v);
            }
            if constexpr (IB > 0) reinterpret_cast<I*>(out_index)[d0 + o] = (I)(from_a ? at : na + at);
        }
    }
}

// out row r = row pos[r] of a_values ++ b_values (rows of `words` W-sized words; W divides the row size and the three
// base addresses); 2^gshift lanes per row, the stores in row order.  A position of n or more is not moved (none occurs:
// rsx_merge_kernel writes positions below n whatever its inputs).  out_index != nullptr: pos[r] is also stored there as
// ib (4 or 8) bytes.
template <typename W>
__global__ __launch_bounds__(256) void rsx_merge_gather_kernel(const uint8_t* __restrict__ a_values, const uint8_t* __restrict__ b_values, uint64_t na,
                                                               uint8_t* __restrict__ out_values, uint32_t words, const uint64_t* __restrict__ pos,
                                                               uint64_t n, uint32_t gshift, uint8_t* __restrict__ out_index, uint32_t ib) {
    const uint32_t G = 1u << gshift;
    const uint32_t lane = threadIdx.x & (G - 1);
    const uint64_t groups = ((uint64_t)gridDim.x * blockDim.x) >> gshift;
    const uint64_t row = (uint64_t)words * sizeof(W);
    for (uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> gshift; r < n; r += groups) {
        const uint64_t idx = pos[r];
        if (idx >= n) continue;
        if (out_index && lane == 0) {
            if (ib == 4) reinterpret_cast<uint32_t*>(out_index)[r] = (uint32_t)idx;
            else reinterpret_cast<uint64_t*>(out_index)[r] = idx;
        }
        const W* s = reinterpret_cast<const W*>(idx < na ? a_values + idx * row : b_values + (idx - na) * row);
        W* d = reinterpret_cast<W*>(out_values + r * row);
        for (uint32_t j = lane; j < words; j += G) d[j] = s[j];
    }
}

}  // namespace rsx
