// rsx_scan_kernels.hpp -- the kernels behind rsx_scan_by_key_device (rsx.hip; launched by rsx_scan.hip): a result for
// EVERY element, the inclusive or exclusive (+) of the values of its group up to it, stored at the element's input
// position.  The run kernels of rsx_reduce_kernels.hpp compute exactly this segmented scan and keep only the last
// element of every run; these keep all of it.  Three launches, tiled alike (scanbk_ipt elements per thread, 256 threads):
//   rsx_scanbk_count_kernel  tile t -> tile_heads[t] and tile_tail[t], with the meaning they have in
//                            rsx_reduce_count_kernel
//   rsx_reduce_scan_kernel   (rsx_reduce_kernels.hpp, as it is) tile_base[t], tile_carry[t] and the number of heads
//   rsx_scanbk_write_kernel  the flags and the segmented scan again; every element stores its result
// Both kernels are templated on where a thread's elements come from and where its results go (SRC):
//   SCANBK_COLUMNS    RSX_SCAN_RUNS: keys and values straight from the caller's columns, a head being a key that differs
//                     from the key in front of it AS THEY LIE.  A thread takes scanbk_ipt CONSECUTIVE rows, a whole number
//                     of 16-byte words of BOTH columns, loaded and stored as such when the column's base is 16-byte
//                     aligned (a uniform branch per column: ScanArgs::wide) and element by element otherwise -- the same
//                     rows per thread either way, so the same bytes.  Results are stored coalesced.
//   SCANBK_POSITIONS  the grouped form: the sorted (mapped key, u32 position) elements of rsx_argsort_device.  The count
//                     kernel gathers values[position] -- the call's one uncoalesced read -- and stores what it gathered,
//                     coalesced, into a workspace column of n values; the write kernel streams that column and scatters
//                     out[position], the one uncoalesced write.
// VK is the value kind (0 unsigned, PAIRS_SIGNED, PAIRS_FLOAT) or SCANBK_ONES, the count form: every value is the integer
// 1, no value is read anywhere and the workspace column does not exist.  The operator, the exclusive bit and `first` are
// uniform run-time arguments.
//
// The results of element e0 + j of a thread, s[j] being the thread's own segmented scan (reduce_thread_scan) and `front`
// the item in front of the thread (the open run in front of the tile, the waves and the lanes in front):
//   inclusive  I[j] = s[j], with front on its left while the thread has had no head up to j;
//   exclusive  `first` at a head (stored, never combined), else I[j - 1] -- for j == 0 front's value itself, which is valid
//              then: an element that is no head has its run's elements in front of it.
// The association of a float sum is therefore the reduce kernels': ((carry (+) in front of the thread) (+) in the
// thread), fixed by the tiling.  No identity element is ever combined.
//
// ALIASING.  out may be the value column.  SCANBK_COLUMNS: the write kernel's thread loads the values of its own rows
// [e0, e0 + cnt) into registers before its first store and stores those rows only; what it takes from other rows comes
// through tile_carry (written by the launch before) and through registers and LDS (waves' totals), never from the value
// column -- a thread stores only positions whose values it has itself already loaded, and nobody else reads them.  The
// count kernel, which reads every value too, has finished: stream order.  SCANBK_POSITIONS: the write kernel does not read
// the caller's values at all (the count kernel gathered them into the workspace), and the positions are a permutation:
// every out[position] is stored once.  out must not overlap the keys: the key in front of a thread's rows is read from
// global memory while other threads store.
// No workgroup waits for another one.  No kernel reads outside the n keys (elements) and n values or writes outside
// tile_heads / tile_tail [tiles], the workspace column [n] and out [n].
#pragma once

#include "rsx_reduce_kernels.hpp"

namespace rsx {

constexpr uint32_t SCANBK_WG = REDUCE_WG;
enum : int { SCANBK_COLUMNS = 0, SCANBK_POSITIONS = 1 };
constexpr int SCANBK_ONES = 3;  // VK of the count form
enum : uint32_t { SCANBK_EXCLUSIVE = 1, SCANBK_RUNS = 2 };                    // RSX_SCAN_*
enum : uint32_t { SCANBK_WIDE_KEYS = 1, SCANBK_WIDE_VALUES = 2, SCANBK_WIDE_OUT = 4 };  // ScanArgs::wide

// the sorted element of the grouped form: (mapped key, u32 position)
constexpr uint32_t scanbk_elem(uint32_t kb) { return pairs_elem(kb, 4); }
// elements per thread.  Columns: the fewest rows that are whole 16-byte words of the key column and of a 4-byte value
// column (so of an 8-byte one too), twice that for 4-byte keys (32 bytes of keys); positions: the reduce kernels' share of
// the sorted elements
constexpr uint32_t scanbk_ipt(int src, uint32_t kb) {
    return src == SCANBK_COLUMNS ? (kb == 1 ? 16u : kb <= 4 ? 8u : 4u) : reduce_ipt(scanbk_elem(kb));
}
constexpr uint32_t scanbk_tile(int src, uint32_t kb) { return SCANBK_WG * scanbk_ipt(src, kb); }

struct ScanArgs {
    const uint8_t* keys;    // columns: the caller's n keys; positions: the n sorted (mapped key, u32 position) elements
    const uint8_t* values;  // the caller's n values (unused in the count form; positions: read by the count kernel only)
    uint8_t* column;        // positions: the workspace column of n values in sorted order
    uint8_t* out;           // n results, by input position
    uint32_t wide;          // columns: SCANBK_WIDE_* of the columns whose base is 16-byte aligned
};

// IPT consecutive entries of W bytes from entry e0 of `col` on into r (zeros behind cnt): whole words when the thread has
// all IPT and `wide`, else entry by entry
template <int W, int IPT>
__device__ __forceinline__ void scanbk_load(unsigned char* r, const uint8_t* col, uint64_t e0, uint32_t cnt, bool wide) {
    if (cnt == (uint32_t)IPT && wide) {
        pairs_load<W * IPT>(r, col + e0 * W);
    } else {
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            if ((uint32_t)j < cnt) pairs_load<W>(r + j * W, col + (e0 + (uint64_t)j) * W);
            else __builtin_memset(r + j * W, 0, W);
        }
    }
}
template <int W, int IPT>
__device__ __forceinline__ void scanbk_store(uint8_t* col, uint64_t e0, uint32_t cnt, bool wide, const unsigned char* r) {
    if (cnt == (uint32_t)IPT && wide) {
        pairs_store<W * IPT>(col + e0 * W, r);
    } else {
#pragma unroll
        for (int j = 0; j < IPT; ++j)
            if ((uint32_t)j < cnt) pairs_store<W>(col + (e0 + (uint64_t)j) * W, r + j * W);
    }
}

// One thread's head flags and values (as bit patterns in v, zeros behind cnt) and, for SCANBK_POSITIONS, its positions.
// GATHER (the count kernel of the positions source): the values come from the caller's column through the positions and
// are stored into the workspace column; otherwise that column is read.
template <int SRC, int KB, int VB, int VK, bool GATHER, int IPT, typename U>
__device__ __forceinline__ uint32_t scanbk_take(const ScanArgs& a, uint64_t e0, uint32_t cnt, U* v, uint32_t* pos) {
    uint32_t flags = 0;
    if constexpr (SRC == SCANBK_COLUMNS) {
        unsigned char kr[KB * IPT];
        if (a.wide & SCANBK_WIDE_KEYS) {
            flags = runs_flags<KB, KB, IPT>(a.keys, e0, cnt, kr);
        } else {  // natural alignment only: row by row, each with the key in front of it
#pragma unroll
            for (int j = 0; j < IPT; ++j) flags |= runs_flags<KB, KB, 1>(a.keys, e0 + (uint64_t)j, (uint32_t)j < cnt ? 1u : 0u, kr + j * KB) << j;
        }
        if constexpr (VK != SCANBK_ONES) scanbk_load<VB, IPT>(reinterpret_cast<unsigned char*>(v), a.values, e0, cnt, (a.wide & SCANBK_WIDE_VALUES) != 0);
    } else {
        constexpr int E = (int)scanbk_elem(KB), VOFF = (int)pairs_voff(KB, 4);
        unsigned char er[E * IPT];
        flags = runs_flags<KB, E, IPT>(a.keys, e0, cnt, er);
#pragma unroll
        for (int j = 0; j < IPT; ++j) __builtin_memcpy(&pos[j], er + j * E + VOFF, 4);
        if constexpr (VK != SCANBK_ONES) {
            if constexpr (GATHER) {
#pragma unroll
                for (int j = 0; j < IPT; ++j) v[j] = (uint32_t)j < cnt ? reinterpret_cast<const U*>(a.values)[pos[j]] : (U)0;
                scanbk_store<VB, IPT>(a.column, e0, cnt, true, reinterpret_cast<const unsigned char*>(v));
            } else {
                scanbk_load<VB, IPT>(reinterpret_cast<unsigned char*>(v), a.column, e0, cnt, true);
            }
        }
    }
    if constexpr (VK == SCANBK_ONES) {
#pragma unroll
        for (int j = 0; j < IPT; ++j) v[j] = (U)1;
    }
    return flags;
}

// the count form adds unsigned ones
template <int VB, int VK>
using ScanVal = ReduceVal<VB, VK == SCANBK_ONES ? 0 : VK>;

template <int SRC, int KB, int VB, int VK>
__global__ __launch_bounds__(SCANBK_WG) void rsx_scanbk_count_kernel(ScanArgs a, uint64_t n, uint32_t op, uint32_t* __restrict__ tile_heads,
                                                                     uint64_t* __restrict__ tile_tail) {
    constexpr int IPT = (int)scanbk_ipt(SRC, KB);
    constexpr int NW = (int)(SCANBK_WG / WAVE);
    using RV = ScanVal<VB, VK>;
    using U = typename RV::U;
    __shared__ uint32_t s_wave[NW];
    __shared__ U s_v[NW];
    __shared__ uint32_t s_f[NW];
    uint64_t e0;
    const uint32_t cnt = runs_share<SCANBK_WG, IPT>(n, &e0);
    U v[IPT];
    uint32_t pos[IPT];
    const uint32_t flags = scanbk_take<SRC, KB, VB, VK, true, IPT, U>(a, e0, cnt, v, pos);
    U s[IPT];
    const ReduceItem<U> mine = reduce_thread_scan<RV, VB, IPT, 0, U>(reinterpret_cast<const unsigned char*>(v), flags, cnt, op, s);
    const uint32_t incl = wave_incl_scan<false>((uint32_t)__popc(flags));
    const ReduceItem<U> wi = reduce_wave_scan<RV, U>(mine, op);
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) {
        s_wave[threadIdx.x / WAVE] = incl;
        s_v[threadIdx.x / WAVE] = wi.v;
        s_f[threadIdx.x / WAVE] = wi.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        ReduceItem<U> acc{0, 0};
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            total += s_wave[w];
            acc = reduce_join<RV, U>(acc, ReduceItem<U>{s_v[w], s_f[w]}, op);
        }
        tile_heads[blockIdx.x] = total;
        tile_tail[blockIdx.x] = (uint64_t)acc.v;  // (the tile holds an element: valid)
    }
}

template <int SRC, int KB, int VB, int VK>
__global__ __launch_bounds__(SCANBK_WG) void rsx_scanbk_write_kernel(ScanArgs a, uint64_t n, uint32_t op, uint32_t exclusive, uint64_t first,
                                                                     const uint64_t* __restrict__ tile_carry) {
    constexpr int IPT = (int)scanbk_ipt(SRC, KB);
    constexpr int NW = (int)(SCANBK_WG / WAVE);
    using RV = ScanVal<VB, VK>;
    using U = typename RV::U;
    __shared__ U s_v[NW];
    __shared__ uint32_t s_f[NW];
    uint64_t e0;
    const uint32_t cnt = runs_share<SCANBK_WG, IPT>(n, &e0);
    U v[IPT];
    uint32_t pos[IPT];
    const uint32_t flags = scanbk_take<SRC, KB, VB, VK, false, IPT, U>(a, e0, cnt, v, pos);
    U s[IPT];
    const ReduceItem<U> mine = reduce_thread_scan<RV, VB, IPT, 0, U>(reinterpret_cast<const unsigned char*>(v), flags, cnt, op, s);
    const ReduceItem<U> wi = reduce_wave_scan<RV, U>(mine, op);
    const uint32_t wave = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) {
        s_v[wave] = wi.v;
        s_f[wave] = wi.f;
    }
    __syncthreads();
    // what lies in front of this thread: the open run in front of the tile, the waves in front, the lanes in front
    ReduceItem<U> front{0, 0};
    if (blockIdx.x != 0) {
        front.v = (U)tile_carry[blockIdx.x];
        front.f = REDUCE_VALID;
    }
#pragma unroll
    for (int w = 0; w < NW; ++w)
        if ((uint32_t)w < wave) front = reduce_join<RV, U>(front, ReduceItem<U>{s_v[w], s_f[w]}, op);
    ReduceItem<U> lanes;
    lanes.v = pairs_shfl_up<U>(wi.v, 1);
    lanes.f = __shfl_up(wi.f, 1);
    if ((threadIdx.x & (WAVE - 1)) == 0) lanes.f = 0;
    front = reduce_join<RV, U>(front, lanes, op);
    if (cnt == 0) return;
    // (from here on v is the thread's results: every value it holds has been consumed into s)
    U before = front.v;  // the inclusive result of the element in front of e0 + j
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        U inc = s[j];
        if ((flags & ((2u << j) - 1u)) == 0 && (front.f & REDUCE_VALID)) inc = RV::combine(front.v, inc, op);  // the run began in front of the thread
        v[j] = exclusive ? ((flags >> j & 1u) ? (U)first : before) : inc;
        before = inc;
    }
    if constexpr (SRC == SCANBK_COLUMNS) {
        scanbk_store<VB, IPT>(a.out, e0, cnt, (a.wide & SCANBK_WIDE_OUT) != 0, reinterpret_cast<const unsigned char*>(v));
    } else {
#pragma unroll
        for (int j = 0; j < IPT; ++j)
            if ((uint32_t)j < cnt) reinterpret_cast<U*>(a.out)[pos[j]] = v[j];
    }
}

}  // namespace rsx
