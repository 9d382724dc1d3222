// rsx_topk_kernels.hpp -- the first k of every row's stable sort without sorting the row (rsx_topk_rows_device): a radix
// SELECT in LDS, then the sort of the k chosen elements alone.
//
// One workgroup handles one CHUNK of a row: at most cape<ES, KPT, WG>() joined (mapped key, u32 position in the row)
// elements, held in registers in the slot order of local_load.
//   load     first round: keys[row * row_len + p] joined with the generated position p (segp_join: the key mapped, and
//            complemented for descending order, so "smallest mapped key first" is the only case); later rounds: the
//            joined candidates an earlier round wrote.
//   select   digits from the most significant down: a 256-bin count of the digit of the elements still live (the wave
//            counters of local_passes, free at this point), the bin that holds rank k', what lies below it is taken, what
//            lies above it dropped, the bin itself stays live (a bit mask over the thread's KPT registers).  Ends as soon
//            as the bin holds exactly the k' still wanted; when the digits run out with more equal keys than wanted, the
//            first k' of them in array order are taken (ballot prefixes in slot order plus the waves' totals).
//   compact  the taken elements go to LDS in array order (the same ballot prefix), are read back in slot order with
//            n = k and sorted by local_passes / segp_passes_skip: stable, so equal keys stay in array order.
//   store    final round: the unmapped key to out_keys and the position (u32 / u64) to out_index; earlier rounds: the
//            joined elements to the round's candidate array, chunk after chunk.
// Array order is position order in every round: candidates of a chunk are sorted by (key, position) and chunks follow each
// other by position, so equal keys -- the only elements whose order the tie rule decides -- lie in position order.
// The result is the first k columns of rsx_argsort_rows_device, byte for byte.  Nothing is written outside the k
// outputs (candidates) of the chunk; the key column is only read.
#pragma once
#include "rsx_segment_pairs_kernels.hpp"

namespace rsx {

struct TopkArgs {
    const uint8_t* keys;    // first round: rows x row_len keys; later rounds: nullptr
    const void* cand_in;    // later rounds: rows x m joined candidates
    void* cand_out;         // every round but the last: rows x m_next joined candidates; last round: nullptr
    uint8_t* out_keys;      // last round: rows x k keys, or nullptr
    uint8_t* out_index;     // last round: rows x k positions of ib bytes, or nullptr
    uint64_t rows;
    uint64_t row_len;       // of the key column
    uint32_t m;             // this round's row length (first round: row_len)
    uint32_t chunk;         // elements per chunk (every chunk of a row but its last is full)
    uint32_t cpr;           // chunks per row
    uint32_t m_next;        // the next round's row length: (cpr - 1) * k + min(k, length of the last chunk)
    uint32_t k;
    uint32_t kind, desc, ib;
};

// set bits of `mask` bit j over the workgroup's slots in front of this thread's slot j: the caller adds the ballot prefix
// of round j to `run` and advances it.  Wave totals go through s_misc; ends with every thread past its read of them.
template <int KPT, int WG>
__device__ __forceinline__ uint32_t topk_wave_base(const uint32_t mask, const uint32_t kp, uint32_t* s_misc) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t tot = 0;
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if ((uint32_t)j < kp) tot += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(((mask >> j) & 1u) != 0));
    if (lane == 0) s_misc[wave] = tot;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < wave; ++w) base += s_misc[w];
    return base;
}

// One chunk: elements [c * chunk, ...) of row `row` of this round's array.
template <int ES, int KB, int KPT, int WG>
__device__ __forceinline__ void topk_one(const SmallArgs& a, const TopkArgs& t, const uint64_t row, const uint32_t c, unsigned char* smem,
                                         uint32_t& skip_ok) {
    static_assert(pairs_elem(KB, 4) == (uint32_t)ES, "the joined (key, u32 position) element of this key width");
    static_assert(KPT <= 32, "the live set is a 32-bit mask");
    using E = Elem<ES>;
    using C = WaveCnt<ES>;
    static_assert(!C::HALF, "the select counts in whole words");
    using K = typename PairsKey<KB>::type;
    constexpr int NWAVE = WG / WAVE;
    constexpr int VOFF = (int)pairs_voff(KB, 4);
    using Tile = LdsTile<ES, KPT, WG>;
    E* s_elems = Tile::elems(smem);
    uint32_t* s_cnt = Tile::cnt(smem);
    uint32_t* s_misc = Tile::misc(smem);
    uint32_t* s_flag = Tile::flag(smem);
    uint32_t* s_sel = s_flag + 4;  // [3] the chosen bin, the live elements below it, the live elements in it
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t c0 = c * t.chunk;
    const uint32_t len = t.m - c0 < t.chunk ? t.m - c0 : t.chunk;
    const uint32_t kk = t.k < len ? t.k : len;
    uint32_t n = len;  // what the passes sort
    E e[KPT];
    {   // the slot order (slots_of)
        const Slots sl = slots_of<WG>(len);
        const uint32_t kp = sl.kp, seg = sl.seg;
        uint32_t live = 0;
        if (t.keys) {
            SegPairsArgs s{};
            s.keys = const_cast<uint8_t*>(t.keys);
            s.kind = t.kind;
            s.desc = t.desc;
            s.mode = SEGP_LOCAL;
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                e[j] = E{};
                if ((uint32_t)j < kp) {
                    const uint32_t p = seg + (uint32_t)j * WAVE;
                    if (p < len) {
                        e[j] = segp_join<ES, KB, 4>(s, row * t.row_len, c0 + p);  // (the position in the row: c0 + p)
                        live |= 1u << j;
                    }
                }
            }
        } else {
            const E* src = static_cast<const E*>(t.cand_in) + row * (uint64_t)t.m + c0;
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                e[j] = E{};
                if ((uint32_t)j < kp) {
                    const uint32_t p = seg + (uint32_t)j * WAVE;
                    if (p < len) {
                        e[j] = src[p];
                        live |= 1u << j;
                    }
                }
            }
        }
        if (kk < len) {  // (uniform) select: otherwise everything is wanted and the chunk is sorted as it is
            uint32_t* my = s_cnt + wave * RADIX;
            uint32_t take = 0, kr = kk;
            bool ties = true;  // the digits ran out with more equal keys live than wanted
            for (uint32_t d = a.passes; d-- > 0;) {
                const DigitSpec spec = a.spec[d];
                C::zero(my, lane);
#pragma unroll
                for (int j = 0; j < KPT; ++j)
                    if ((uint32_t)j < kp) {
                        const bool lv = ((live >> j) & 1u) != 0;
                        const uint32_t dg = elem_digit<ES, false>(e[j], spec);
                        // (the lanes that share the first live lane's digit -- all of them where the keys agree on this
                        // byte -- are counted by one add; same-address LDS atomics would serialise)
                        const uint64_t lm = __builtin_amdgcn_ballot_w64(lv);
                        if (lm != 0) {
                            const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)dg, (int)__builtin_ctzll(lm));
                            const uint64_t same = __builtin_amdgcn_ballot_w64(lv && dg == d0);
                            if (lv) {
                                if (dg != d0) atomicAdd(&my[dg], 1u);
                                else if (mbcnt64(same) == 0) atomicAdd(&my[d0], (uint32_t)__popcll(same));
                            }
                        }
                    }
                __syncthreads();
                uint32_t tcount = 0, incl = 0;
                if (tid < RADIX) {
#pragma unroll
                    for (int w = 0; w < NWAVE; ++w) tcount += s_cnt[w * RADIX + tid];
                    incl = wave_incl_scan<true>(tcount);
                    if (lane == 63) s_misc[wave] = incl;
                }
                __syncthreads();
                if (tid < RADIX) {
                    uint32_t below = incl - tcount;
                    for (uint32_t w = 0; w < wave; ++w) below += s_misc[w];
                    if (below < kr && kr <= below + tcount) {  // (one bin: at least kr elements are live)
                        s_sel[0] = tid;
                        s_sel[1] = below;
                        s_sel[2] = tcount;
                    }
                }
                __syncthreads();
                const uint32_t bin = s_sel[0], below = s_sel[1], inbin = s_sel[2];
#pragma unroll
                for (int j = 0; j < KPT; ++j)
                    if ((uint32_t)j < kp && ((live >> j) & 1u)) {
                        const uint32_t dg = elem_digit<ES, false>(e[j], spec);
                        if (dg < bin) take |= 1u << j;
                        if (dg != bin) live &= ~(1u << j);
                    }
                kr -= below;
                if (inbin == kr) {  // the bin is wanted whole
                    take |= live;
                    ties = false;
                    break;
                }
            }
            if (ties) {  // equal keys: the first kr of them in array order
                uint32_t run = topk_wave_base<KPT, WG>(live, kp, s_misc);
#pragma unroll
                for (int j = 0; j < KPT; ++j)
                    if ((uint32_t)j < kp) {
                        const bool lv = ((live >> j) & 1u) != 0;
                        const uint64_t bm = __builtin_amdgcn_ballot_w64(lv);
                        if (lv && run + mbcnt64(bm) < kr) take |= 1u << j;
                        run += (uint32_t)__popcll(bm);
                    }
                __syncthreads();  // s_misc belongs to the compaction
            }
            {   // compact in array order, read back in slot order
                uint32_t run = topk_wave_base<KPT, WG>(take, kp, s_misc);
#pragma unroll
                for (int j = 0; j < KPT; ++j)
                    if ((uint32_t)j < kp) {
                        const bool tk = ((take >> j) & 1u) != 0;
                        const uint64_t bm = __builtin_amdgcn_ballot_w64(tk);
                        const uint32_t dst = run + mbcnt64(bm);
                        if (tk && dst < kk) s_elems[dst] = e[j];
                        run += (uint32_t)__popcll(bm);
                    }
                __syncthreads();
                n = kk;
                const Slots sl2 = slots_of<WG>(n);
                const uint32_t kp2 = sl2.kp, seg2 = sl2.seg;
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    e[j] = E{};
                    if ((uint32_t)j < kp2) {
                        const uint32_t p = seg2 + (uint32_t)j * WAVE;
                        if (p < n) e[j] = s_elems[p];
                    }
                }
                __syncthreads();  // s_elems and s_misc belong to the passes
            }
        }
    }
    if constexpr (ES < 8) {
        local_passes<ES, KPT, WG>(a, e, n, smem);
    } else {
        PassPlan pp;
        pp.end = a.passes;
        pp.first = (a.no_skip || !skip_ok) ? 0u : first_digit_for(n, 8u * a.passes, a.passes);
        pp.set_masks(0u, (uint32_t)KB);
        const uint32_t first = pp.first;
        segp_passes_skip<ES, KPT, WG>(a, e, n, smem, pp, s_flag);
        if (pp.first != first) skip_ok = 0;
    }
    // the first kk of the sorted elements
    for (uint32_t i = tid; i < kk; i += WG) {
        const E x = s_elems[i];
        if (t.cand_out) {
            static_cast<E*>(t.cand_out)[row * (uint64_t)t.m_next + (uint64_t)c * t.k + i] = x;
        } else {
            unsigned char r[ES];
            __builtin_memcpy(r, &x, ES);
            const uint64_t o = row * (uint64_t)t.k + i;
            if (t.out_keys) {
                K key;
                __builtin_memcpy(&key, r, KB);
                reinterpret_cast<K*>(t.out_keys)[o] = pairs_unmap<K>(key, t.kind, t.desc);
            }
            if (t.out_index) {
                uint32_t pos;
                __builtin_memcpy(&pos, r + VOFF, 4);
                if (t.ib == 8) reinterpret_cast<uint64_t*>(t.out_index)[o] = pos;
                else reinterpret_cast<uint32_t*>(t.out_index)[o] = pos;
            }
        }
    }
}

// grid: any; the workgroups take the rows x cpr chunks round-robin.
template <int ES, int KB, int KPT, int WG>
__global__ __launch_bounds__(WG) void rsx_topk_kernel(const SmallArgs a, const TopkArgs t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint64_t total = t.rows * (uint64_t)t.cpr;
    uint32_t skip_ok = 1;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const uint64_t row = w / t.cpr;
        topk_one<ES, KB, KPT, WG>(a, t, row, (uint32_t)(w - row * t.cpr), smem, skip_ok);
        __syncthreads();  // smem belongs to the next chunk
    }
}

}  // namespace rsx
