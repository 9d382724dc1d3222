// rsx_segment_kernels.hpp -- many independent segments of ONE array sorted by one call (rsx_sort_segments_device,
// rsx_sort_rows_device): every segment is the array of one workgroup, sorted by the device functions of
// rsx_small_kernel.hpp -- local_sort / local_sort_skip (all passes in LDS) for segments that fit a workgroup's LDS,
// stream_pass (one workgroup, pass by pass between the data and the caller's scratch array) for longer ones.
//
// Size classes.  One instantiation of rsx_segment_sort_kernel per class: 256 threads x KPT elements, 1024 threads x KPT
// elements (KPT = bucket_kpt_for(ES): 7168 / 28672 4-byte, 4352 / 17408 8-byte elements), and 1024 threads through
// memory.  A class takes the segments whose length lies in (lo, hi]; segments of 0 and 1 elements belong to no class.
//
// Dispatch.  The segment lengths are on the device and the host never reads them.  Every class is a persistent grid of
// `teams` x `team` workgroups that walks the offsets a BLOCK of 64 segments at a time: lane t of a workgroup's first wave
// loads the pair of offsets of segment block * 64 + t (coalesced), a ballot names the members of the workgroup's class,
// and workgroup r of a team sorts the members r, r + team, ... of the block (team = 1 when there are blocks enough for
// every workgroup; a power of two up to 64 when there are few segments).  A million segments of another class cost a
// workgroup a few dozen coalesced loads.  No classification pass, no lists, no counters, no workspace.  Rows of one length
// (offsets == nullptr) are computed instead of loaded, one row per block.
//
// Offsets are not trusted: a segment with begin > end, end > n or 2^32 elements and more belongs to no class, is left as
// it is and sets the context's host-visible error word.  Nothing outside [0, n) of `data` and `tmp` is read or written.
#pragma once
#include "rsx_small_kernel.hpp"

namespace rsx {

// What the walk over the segments reads; the kernels' argument blocks hold one behind their arrays.
struct SegWalk {
    uint64_t n;               // elements in the arrays
    const uint64_t* offsets;  // nseg + 1 element offsets, or nullptr: segment i = [i * row_len, (i + 1) * row_len)
    uint64_t nseg;
    uint64_t row_len;
    uint64_t lo, hi;          // this launch sorts the segments of lo < length <= hi
    uint32_t team;            // workgroups that share a block of SEG_BLOCK segments (a power of two, <= SEG_BLOCK)
    uint32_t* error;          // host-visible error word of the context
};
struct SegArgs {
    void* data;  // n elements
    void* tmp;   // n elements: the ping-pong array of the sort through memory
    SegWalk w;
};

// One segment [0, len) at `seg`, in place (scratch at `scr`).  MEM == false: len <= cape<ES, KPT, WG>().
template <int ES, int KPT, int WG, bool MEM>
__device__ __forceinline__ void segment_sort_one(const SmallArgs& a, Elem<ES>* seg, Elem<ES>* scr, const uint32_t len, unsigned char* smem,
                                                 uint32_t& skip_ok) {
    using E = Elem<ES>;
    if constexpr (MEM) {
        // a.passes LSD passes through memory.  The keys stay RAW (a.spec are the raw key's digit specs, with their flip
        // and float sign: elem_digit<ES, true>), so no pass maps anything; an odd number of passes ends in `scr`.
        E* src = seg;
        E* dst = scr;
        for (uint32_t pass = 0; pass < a.passes; ++pass) {
            const DigitSpec spec = a.spec[pass];
            uint32_t bs = 0, bc = 0;
            stream_pass<ES, KPT, WG>(a, src, dst, len, smem, [&](const E& x) { return elem_digit<ES, true>(x, spec); }, false, bs, bc);
            E* t = src;
            src = dst;
            dst = t;
        }
        if (src != seg)  // (stream_pass ended with a release, a barrier and an acquire: scr is visible to every thread)
            for (uint32_t i = threadIdx.x; i < len; i += WG) seg[i] = scr[i];
    } else if constexpr (ES < 8) {  // (keys of more than five bytes only: narrower elements never skip)
        local_sort<ES, KPT, WG>(a, seg, seg, len, smem);
    } else {
        // As rsx_bucket_sort_kernel: the passes start at the digit a uniform array of this length is told apart by, the
        // neighbours that still agree are mended by the digits skipped.  A workgroup that meets a segment where that
        // fails (keys that agree on their high digits: small integers in wide keys) runs every pass from then on.
        // (These lines stand at four sites -- here, segp_sort_one, topk_one, rsx_bucket_sort_kernel: as one helper four kernels compile otherwise.)
        PassPlan pp;
        pp.end = a.passes;
        pp.first = (a.no_skip || !skip_ok) ? 0u : first_digit_for(len, 8u * a.passes, a.passes);
        pp.set_masks(a.key_offset, a.key_bytes);
        const uint32_t first = pp.first;
        uint32_t* s_flag = LdsTile<ES, KPT, WG>::flag(smem);
        local_sort_skip<ES, KPT, WG>(a, seg, seg, len, smem, pp, s_flag);
        if (pp.first != first) skip_ok = 0;
    }
}

constexpr uint32_t SEG_BLOCK = 64;  // segments a workgroup examines at a time: one wave's ballot

template <int ES, int KPT, int WG, bool MEM>
__global__ __launch_bounds__(WG) void rsx_segment_sort_kernel(const SmallArgs a, const SegArgs s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // (The loop below reads SegWalk alone and is the same, token for token, in rsx_segment_pairs_kernel.  It stays in
    // both kernels: as one function that takes the body, the through-memory fused kernels gained 8-128 bytes of scratch.)
    // the block's segments as its first wave read and judged them (every thread takes a member's place from here: the
    // offsets are read once, by vector loads, and what was judged is what is sorted)
    __shared__ uint64_t s_beg[SEG_BLOCK];
    __shared__ uint32_t s_len[SEG_BLOCK];
    __shared__ uint64_t s_members;
    using E = Elem<ES>;
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
        uint32_t k = 0;  // members of the block so far (uniform, as everything from here on)
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
            segment_sort_one<ES, KPT, WG, MEM>(a, static_cast<E*>(s.data) + beg, static_cast<E*>(s.tmp) + beg, len, smem, skip_ok);
            __syncthreads();  // smem belongs to the next segment
        }
        __syncthreads();  // s_beg, s_len and s_members belong to the next block
    }
}

}  // namespace rsx
