// rsx_segment_pairs_kernels.hpp -- many independent segments of SEPARATE key and value arrays sorted by one call
// (rsx_sort_segments_pairs_device, rsx_argsort_segments_device and their row forms): the segmented sort of
// rsx_segment_kernels.hpp whose load reads a segment from the key column and the value column (or makes positions) and
// whose store writes the columns back.  The joined (mapped key, value) elements of rsx_pairs_kernels.hpp exist only in
// registers and LDS: the LDS classes read every column once and write it once.
//
//   load    slot order of local_load (wave, round, lane): keys[beg + p] as one KB-wide word, mapped (pairs_map: sign flip,
//           float total order, complement for descending order); values[beg + p] as one VB-wide word, or the position p
//           (argsort) / beg + p (proxies of wider values); both packed at offsets 0 and pairs_voff of an Elem<ES>.
//   passes  local_passes unchanged (ES < 8); the skip-and-mend plan of segment_sort_one on the mapped key, sorted as an
//           unsigned key at offset 0 (ES >= 8).
//   store   from s_elems[i]: the key unmapped to keys[beg + i], the value word to values[beg + i], or the position to the
//           index column (u32 / u64) or to the proxy array.
// Kind, order, mode and index width are uniform arguments that act in the load and the store only.
//
// Size classes, dispatch and the distrust of the offsets are those of rsx_segment_sort_kernel.  The through-memory class
// (MEM) joins its segment into the context's pairs workspace, runs stream_pass between the two workspace arrays and
// splits the result back.  Nothing outside the n keys / values / indices (and the n workspace elements) is touched.
#pragma once
#include "rsx_pairs_kernels.hpp"
#include "rsx_segment_kernels.hpp"

namespace rsx {

struct SegPairsArgs {
    uint8_t* keys;            // n keys (SEGP_LOCAL: only read)
    uint8_t* values;          // SEGP_VALUES: n values; SEGP_LOCAL: n indices of ib bytes; SEGP_GLOBAL: n proxies of ES bytes
    void* w0;                 // MEM: the two workspace arrays of n joined elements
    void* w1;
    SegWalk w;                // n: of keys, values and workspace elements
    uint32_t kind, desc, mode, ib;
};

// element p of the segment at `beg`, joined in registers
template <int ES, int KB, int VB>
__device__ __forceinline__ Elem<ES> segp_join(const SegPairsArgs& s, const uint64_t beg, const uint32_t p) {
    static_assert(pairs_elem(KB, VB) == (uint32_t)ES, "the joined element of these widths");
    constexpr int VOFF = (int)pairs_voff(KB, VB);
    using K = typename PairsKey<KB>::type;
    unsigned char r[ES];
#pragma unroll
    for (int b = 0; b < ES; ++b) r[b] = 0;
    K k = reinterpret_cast<const K*>(s.keys)[beg + p];
    k = pairs_map<K>(k, s.kind, s.desc);
    __builtin_memcpy(r, &k, KB);
    if constexpr (VB > 0) {
        using V = typename PairsWord<VB>::type;
        bool column = true;
        if constexpr (VB == 4) {
            if (s.mode != SEGP_VALUES) {
                const uint32_t pos = s.mode == SEGP_LOCAL ? p : (uint32_t)(beg + p);
                __builtin_memcpy(r + VOFF, &pos, 4);
                column = false;
            }
        }
        if (column) {
            const V v = reinterpret_cast<const V*>(s.values)[beg + p];
            __builtin_memcpy(r + VOFF, &v, VB);
        }
    }
    Elem<ES> e;
    __builtin_memcpy(&e, r, ES);
    return e;
}

// sorted element i of the segment at `beg` back to its columns
template <int ES, int KB, int VB>
__device__ __forceinline__ void segp_split(const SegPairsArgs& s, const uint64_t beg, const uint32_t i, const Elem<ES>& x) {
    constexpr int VOFF = (int)pairs_voff(KB, VB);
    using K = typename PairsKey<KB>::type;
    unsigned char r[ES];
    __builtin_memcpy(r, &x, ES);
    if (s.mode != SEGP_LOCAL) {
        K k;
        __builtin_memcpy(&k, r, KB);
        reinterpret_cast<K*>(s.keys)[beg + i] = pairs_unmap<K>(k, s.kind, s.desc);
    }
    if constexpr (VB > 0) {
        using V = typename PairsWord<VB>::type;
        bool column = true;
        if constexpr (VB == 4) {
            if (s.mode != SEGP_VALUES) {
                uint32_t pos;
                __builtin_memcpy(&pos, r + VOFF, 4);
                if (s.mode == SEGP_GLOBAL) *reinterpret_cast<uint32_t*>(s.values + (beg + i) * ES + VOFF) = pos;
                else if (s.ib == 8) reinterpret_cast<uint64_t*>(s.values)[beg + i] = pos;
                else reinterpret_cast<uint32_t*>(s.values)[beg + i] = pos;
                column = false;
            }
        }
        if (column) {
            V v;
            __builtin_memcpy(&v, r + VOFF, VB);
            reinterpret_cast<V*>(s.values)[beg + i] = v;
        }
    }
}

// local_sort_skip's middle on elements already in registers: the passes [pp.first, pp.end), the check, the mending or --
// if the runs are too long for that -- every pass.  The sorted array is left in LDS.
template <int ES, int KPT, int WG>
__device__ __forceinline__ void segp_passes_skip(const SmallArgs& a, Elem<ES> (&e)[KPT], const uint32_t n, unsigned char* smem, PassPlan& pp,
                                                 uint32_t* s_flag) {
    using E = Elem<ES>;
    local_passes<ES, KPT, WG>(a, e, n, smem, pp.first, pp.end);
    if (pp.first == 0) return;
    uint32_t ties;
    bool mended;
    {
        E x[KPT];
        mended = !local_check<ES, KPT, WG>(pp, n, smem, x, ties);
    }
    if (!mended) mended = local_mend_listed<ES, KPT, WG>(n, smem, pp, s_flag, ties);
    if (!mended) {
        pp.first = 0;
        const uint32_t kp = (n + WG - 1) / WG, seg = (threadIdx.x >> 6) * (WAVE * kp) + (threadIdx.x & 63u);  // (as in local_sort_skip)
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if ((uint32_t)j < kp) e[j] = reinterpret_cast<const E*>(smem)[seg + (uint32_t)j * WAVE];
        __syncthreads();
        local_passes<ES, KPT, WG>(a, e, n, smem, 0, pp.end);
    }
}

// One segment [beg, beg + len).  MEM == false: len <= cape<ES, KPT, WG>().
template <int ES, int KB, int VB, int KPT, int WG, bool MEM>
__device__ __forceinline__ void segp_sort_one(const SmallArgs& a, const SegPairsArgs& s, const uint64_t beg, const uint32_t len, unsigned char* smem,
                                              uint32_t& skip_ok) {
    using E = Elem<ES>;
    if constexpr (MEM) {
        E* src = static_cast<E*>(s.w0) + beg;
        E* dst = static_cast<E*>(s.w1) + beg;
        for (uint32_t i = threadIdx.x; i < len; i += WG) src[i] = segp_join<ES, KB, VB>(s, beg, i);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        for (uint32_t pass = 0; pass < a.passes; ++pass) {  // the mapped key: plain digits
            const DigitSpec spec = a.spec[pass];
            uint32_t bs = 0, bc = 0;
            stream_pass<ES, KPT, WG>(a, src, dst, len, smem, [&](const E& x) { return elem_digit<ES, false>(x, spec); }, false, bs, bc);
            E* t = src;
            src = dst;
            dst = t;
        }
        // (stream_pass ended with a release, a barrier and an acquire: src is visible to every thread)
        for (uint32_t i = threadIdx.x; i < len; i += WG) segp_split<ES, KB, VB>(s, beg, i, src[i]);
    } else {
        E e[KPT];
        {   // the slot order: slots_of(len), written out (through the call three of these kernels are scheduled otherwise)
            const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
            const uint32_t kp = (len + WG - 1) / WG;
            const uint32_t seg = wave * (WAVE * kp) + lane;
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                e[j] = E{};
                if ((uint32_t)j < kp) {
                    const uint32_t p = seg + (uint32_t)j * WAVE;
                    if (p < len) e[j] = segp_join<ES, KB, VB>(s, beg, p);
                }
            }
        }
        if constexpr (ES < 8) {
            local_passes<ES, KPT, WG>(a, e, len, smem);
        } else {
            PassPlan pp;
            pp.end = a.passes;
            pp.first = (a.no_skip || !skip_ok) ? 0u : first_digit_for(len, 8u * a.passes, a.passes);
            pp.set_masks(0u, (uint32_t)KB);
            const uint32_t first = pp.first;
            uint32_t* s_flag = LdsTile<ES, KPT, WG>::flag(smem);
            segp_passes_skip<ES, KPT, WG>(a, e, len, smem, pp, s_flag);
            if (pp.first != first) skip_ok = 0;
        }
        const E* s_elems = reinterpret_cast<const E*>(smem);
        for (uint32_t i = threadIdx.x; i < len; i += WG) segp_split<ES, KB, VB>(s, beg, i, s_elems[i]);
    }
}

template <int ES, int KB, int VB, int KPT, int WG, bool MEM>
__global__ __launch_bounds__(WG) void rsx_segment_pairs_kernel(const SmallArgs a, const SegPairsArgs s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // (the dispatch loop of rsx_segment_sort_kernel, which says why it is written out twice)
    __shared__ uint64_t s_beg[SEG_BLOCK];
    __shared__ uint32_t s_len[SEG_BLOCK];
    __shared__ uint64_t s_members;
    const uint32_t tid = threadIdx.x;
    const bool rows = s.w.offsets == nullptr;
    const uint32_t team = rows ? 1u : s.w.team;
    const uint32_t r = blockIdx.x & (team - 1u);
    const uint64_t step = gridDim.x / team;
    const uint64_t nblocks = rows ? s.w.nseg : (s.w.nseg + SEG_BLOCK - 1) / SEG_BLOCK;
    uint32_t skip_ok = 1;
    for (uint64_t blk = blockIdx.x / team; blk < nblocks; blk += step) {
        if (!rows) {
            if (tid < SEG_BLOCK) {
                const uint64_t i = blk * SEG_BLOCK + tid;
                bool member = false;
                uint64_t b = 0, e = 0;
                if (i < s.w.nseg) {
                    b = s.w.offsets[i];
                    e = s.w.offsets[i + 1];
                    const bool valid = b <= e && e <= s.w.n && e - b < (1ull << 32);
                    if (!valid) __hip_atomic_store(s.w.error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    member = valid && e - b > s.w.lo && e - b <= s.w.hi;
                }
                s_beg[tid] = b;
                s_len[tid] = member ? (uint32_t)(e - b) : 0u;
                const uint64_t m = __ballot(member);
                if (tid == 0) s_members = m;
            }
            __syncthreads();
        }
        uint64_t m = 1;
        if (!rows) {
            const uint64_t v = s_members;
            m = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)v) | (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32;
        }
        uint32_t k = 0;
        for (; m != 0; m &= m - 1ull) {
            if ((k++ & (team - 1u)) != r) continue;
            uint64_t beg = blk * s.w.row_len;
            uint32_t len = (uint32_t)s.w.row_len;
            if (!rows) {
                const uint32_t bit = (uint32_t)__builtin_ctzll(m);
                const uint64_t v = s_beg[bit];
                beg = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)v) | (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32;
                len = __builtin_amdgcn_readfirstlane(s_len[bit]);
            }
            segp_sort_one<ES, KB, VB, KPT, WG, MEM>(a, s, beg, len, smem, skip_ok);
            __syncthreads();  // smem belongs to the next segment
        }
        __syncthreads();  // s_beg, s_len and s_members belong to the next block
    }
}

}  // namespace rsx
