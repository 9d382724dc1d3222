// rsx_binred_kernels.hpp -- the kernels behind rsx_bin_reduce_device (rsx.hip, beside the bin and multisplit kernels whose
// bin search, wave match and shares they take): a value column of an UNSORTED table combined per bin -- sum, minimum or
// maximum of values[i] over the rows whose key falls into bin b, for b = 0 .. m -- without sorting anything.  bin(key) is
// rsx_bin_count_device's (msplit_bins); the operators are rsx_reduce_by_key_device's (ReduceVal: wrapping integer sums,
// IEEE float sums, min and max by the total order on bit patterns).  Two launches, no zeroing launch:
//   rsx_binred_part_kernel<KB, VB, FLT, IDX>  G = min(ceil(n / SELECT_SHARE), 2 * CUs) persistent workgroups of BINRED_WG
//                                             threads, workgroup g owning select_share's share g of the N rows.  LDS: the
//                                             mapped edges, one row of m + 1 accumulators PER WAVE, one row of m + 1 counters.
//                                             The share goes in tiles of binred_tile rows; wave w owns a contiguous quarter
//                                             of the tile and in round j its lane l holds row w * 64 * IPT + j * 64 + l.
//                                             A round whose 64 lanes hold ONE bin costs one combine per lane: every lane
//                                             keeps a register accumulator for the wave's current bin, and only a change of
//                                             that bin (or the end of the share) reduces the 64 registers (a fixed xor tree)
//                                             into the wave's LDS row.  Any other round: the lanes with my bin
//                                             (msplit_match), their values combined along the peer mask by pointer jumping
//                                             -- lane i takes the value of the next peer above it, then of the peer two
//                                             above, four above, ...: at most six steps, fewer when the groups are short --
//                                             and the group's first lane alone updates its wave's row by a plain LDS read,
//                                             combine and write.  Only wave w touches row w, so the rounds need no barrier
//                                             and no two waves ever write one word.  The counters take integer LDS atomics
//                                             (order-free).  At the end the four rows are combined in wave order and STORED
//                                             into the workgroup's column of part[b * G + g]; the counters into cntm likewise.
//                                             A workgroup whose share is empty stores identities and zeros.
//   rsx_binred_final_kernel<VB, FLT>          a wave per bin: lane l combines part[b * G + l], [l + 64], ... in that order,
//                                             the 64 lanes by the same xor tree; lane 0 stores the value -- or combines it
//                                             onto what the output held (accumulate) -- and the count.
// The kernels know two kinds of value, floats and integers (FLT).  Signed integers differ from unsigned ones in the order
// of MIN and MAX alone, so the host hands those calls `flip`, the sign bit: the first launch flips it in every value it
// loads and works in the unsigned order, the second flips it back in what it stores (and in what it accumulates onto).
// The edge modes differ in the search alone and share a kernel (IDX false, `up` a uniform argument).
// Rows beyond the share's end take part as the operator's identity in the bin of the round's first row: a float sum's
// identity is +0.0 and every row of accumulators starts from it, so a bin of -0.0 values ends as +0.0 and a padded lane
// changes no bit of any result.  The association of a float sum is therefore a function of the keys' bins, N and G alone:
// which wave or workgroup runs first changes nothing, there are no floating-point atomics and the same input gives the
// same bytes on every call.
// Edges that are NOT sorted: msplit_bins reads only positions below m and ends in 0 .. m, so every accumulator touched is
// one of the m + 1.  No counter wraps: the call takes n < 2^32 rows.  N = n or min(n, *num), read on the device.
// LDS at the caps (binred_max_edges): m * KB + 4 * (m + 1) * VB + 4 * (m + 1) + BINRED_LDS_PAD <= 80 KiB, two workgroups a CU.
#pragma once

#include "rsx_msplit_kernels.hpp"
#include "rsx_reduce_kernels.hpp"

namespace rsx {

constexpr int BINRED_WG = 256;
constexpr int BINRED_WAVES = BINRED_WG / WAVE;
constexpr uint32_t BINRED_LDS_LIMIT = 80 * 1024;  // static LDS of one workgroup: two fit a CU's 160 KiB
constexpr uint32_t BINRED_NONE = 0xFFFFFFFFu;     // no current bin
// the most edges: bins fit the 11 bits of the widest wave match, and the edges, four rows of accumulators and the counters fit the LDS
// (BINRED_LDS_PAD: what the alignment of the three arrays may cost)
constexpr uint32_t BINRED_LDS_PAD = 32;
constexpr uint32_t binred_max_edges(uint32_t kb, uint32_t vb) {
    const uint32_t per = kb + BINRED_WAVES * vb + 4u, fit = (BINRED_LDS_LIMIT - BINRED_LDS_PAD - BINRED_WAVES * vb - 4u) / per;
    return fit < MSPLIT_MAX_EDGES ? fit : MSPLIT_MAX_EDGES;
}
constexpr uint32_t binred_max_index(uint32_t vb) { return binred_max_edges(0, vb); }  // no edges in LDS
// rounds of a wave per tile: what keeps the keys, values and bins of a tile in registers
constexpr int binred_ipt(int kb, int vb) { return kb + vb <= 12 ? 16 : 8; }
constexpr uint32_t binred_tile(int kb, int vb) { return (uint32_t)(BINRED_WG * binred_ipt(kb, vb)); }
static_assert(binred_max_edges(16, 8) >= 1023 && binred_max_edges(16, 4) >= 1023 && binred_max_edges(8, 8) >= 1023, "at least 1023 edges for every key and value width");
static_assert(binred_max_edges(4, 4) == MSPLIT_MAX_EDGES && binred_max_edges(16, 4) == MSPLIT_MAX_EDGES && binred_max_index(8) == MSPLIT_MAX_EDGES && binred_max_index(4) == MSPLIT_MAX_EDGES, "the narrow forms reach the match's 11 bits");
static_assert(binred_max_edges(16, 8) * 16 + (binred_max_edges(16, 8) + 1) * (BINRED_WAVES * 8 + 4) + BINRED_LDS_PAD <= BINRED_LDS_LIMIT, "edges, four rows, counters: two workgroups per CU");
static_assert(binred_max_edges(4, 8) * 4 + (binred_max_edges(4, 8) + 1) * (BINRED_WAVES * 8 + 4) + BINRED_LDS_PAD <= BINRED_LDS_LIMIT, "edges, four rows, counters: two workgroups per CU");
static_assert(binred_ipt(16, 8) % BIN_GROUP == 0 && binred_ipt(4, 4) % BIN_GROUP == 0, "whole groups of searches in step");

// the identity of the operator: what an empty bin holds
// (integers in the unsigned order, where the sign flip has taken the signed ones: 0 and all ones are the signed minimum
// and maximum, flipped)
template <int VB, bool FLT>
using BinredVal = ReduceVal<VB, FLT ? (int)PAIRS_FLOAT : 0>;
template <int VB, bool FLT>
__device__ __forceinline__ typename BinredVal<VB, FLT>::U binred_identity(uint32_t op) {
    using U = typename BinredVal<VB, FLT>::U;
    // the lowest value of the order: the float of all ones (a -NaN), the integer 0; the highest: the float of all ones
    // below the sign bit (a +NaN), the unsigned maximum
    constexpr U MIN = BinredVal<VB, FLT>::MIN;
    constexpr U LOWEST = FLT ? (U) ~(U)0 : (U)0;
    constexpr U HIGHEST = FLT ? (U)~MIN : (U) ~(U)0;
    if (op == REDUCE_SUM) return (U)0;  // integer 0, +0.0
    return op == REDUCE_MIN ? HIGHEST : LOWEST;
}

// the 64 lanes' values in lane 0 (every lane: a fixed tree, the lower lane on the left)
template <typename RV>
__device__ __forceinline__ typename RV::U binred_wave(typename RV::U x, uint32_t op) {
    using U = typename RV::U;
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) x = RV::combine(x, pairs_shfl_xor<U>(x, o), op);
    return x;
}

// part and cntm: (m + 1) x gridDim.x, the workgroup's column STORED; cntm may be null (a uniform branch).  m == 0: no key
// is read.  IDX: the index mode; else `up` chooses between RSX_BIN_UPPER and RSX_BIN_LOWER.  flip: see above.
template <int KB, int VB, bool FLT, bool IDX>
__global__ __launch_bounds__(BINRED_WG) void rsx_binred_part_kernel(const void* __restrict__ keys, const void* __restrict__ values, uint64_t n,
                                                                    const uint64_t* __restrict__ num, const void* __restrict__ edges, uint32_t m,
                                                                    uint32_t up, uint32_t kind, uint32_t desc, uint32_t op, uint64_t flip,
                                                                    void* __restrict__ part, uint32_t* __restrict__ cntm) {
    using K = typename PairsKey<KB>::type;
    using KC = typename MsplitCell<KB>::type;
    using RV = BinredVal<VB, FLT>;
    using U = typename RV::U;
    constexpr int IPT = binred_ipt(KB, VB);
    constexpr uint32_t TILE = binred_tile(KB, VB);
    constexpr uint32_t E = IDX ? binred_max_index(VB) : binred_max_edges(KB, VB);
    __shared__ __attribute__((aligned(16))) K s_edge[IDX ? 1 : E];
    __shared__ U acc[BINRED_WAVES][E + 1];
    __shared__ uint32_t s_cnt[E + 1];
    if (m > E) return;  // (the host refuses it)
    const uint64_t N = bin_count_of(n, num);
    uint64_t p0, p1;
    select_share(N, &p0, &p1);
    if (p1 < p0) p1 = p0;  // a share behind the device count: m + 1 identities
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const U ident = binred_identity<VB, FLT>(op);
    const U sign = (U)flip;
    const bool counting = cntm != nullptr;
    if constexpr (!IDX)
        for (uint32_t i = tid; i < m; i += BINRED_WG) s_edge[i] = search_hay<KB>(static_cast<const uint8_t*>(edges), i, kind, desc);
    for (uint32_t i = tid; i <= m; i += BINRED_WG) {
#pragma unroll
        for (int w = 0; w < BINRED_WAVES; ++w) acc[w][i] = ident;
        s_cnt[i] = 0;
    }
    __syncthreads();
    const uint32_t nb = 32u - (uint32_t)__builtin_clz(m | 1u);  // bits of a bin, 0 .. m
    const KC* kin = static_cast<const KC*>(keys);
    const U* vin = static_cast<const U*>(values);
    U* row = acc[wave];
    // the wave's current bin (uniform), every lane's accumulator for it and the rows it stands for
    uint32_t cur = BINRED_NONE, cur_rows = 0;
    U mine = ident;
    const auto flush = [&]() {
        if (cur == BINRED_NONE) return;  // (uniform)
        const U r = binred_wave<RV>(mine, op);
        if (lane == 0) {
            row[cur] = RV::combine(row[cur], r, op);
            if (counting) atomicAdd(&s_cnt[cur], cur_rows);
        }
        mine = ident;
        cur_rows = 0;
    };
    for (uint64_t t0 = p0; t0 < p1; t0 += TILE) {
        const uint64_t r0 = t0 + (uint64_t)wave * (WAVE * IPT) + lane;  // the lane's row of round 0
        const uint64_t left = p1 > r0 ? p1 - r0 : 0;
        // bit j: the lane has a row in round j; lane 0's bits cover every other lane's
        const uint32_t have = left >= (uint64_t)(WAVE * IPT) ? (1u << IPT) - 1u : (1u << (((uint32_t)left + WAVE - 1) / WAVE)) - 1u;
        const uint32_t any = (uint32_t)__builtin_amdgcn_readfirstlane((int)have);
        if (any == 0) continue;  // (the whole wave: its quarter lies behind the share's end)
        K raw[IPT];
        U val[IPT];
        uint32_t bin[IPT];
        uint32_t rounds = msplit_rounds(have);
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const uint64_t at = r0 + (uint64_t)j * WAVE;
            KC c{};
            if (m != 0 && (rounds >> j & 1u)) c = kin[at];
            __builtin_memcpy(&raw[j], &c, KB);
        }
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const uint64_t at = r0 + (uint64_t)j * WAVE;
            val[j] = ident;
            if (rounds >> j & 1u) val[j] = (U)(vin[at] ^ sign);
        }
        if (m != 0) {  // (uniform, as is the choice of the search)
#pragma unroll
            for (int j = 0; j < IPT; j += BIN_GROUP) {
                if constexpr (IDX) msplit_bins<KB, MSPLIT_INDEX, BIN_GROUP>(raw + j, bin + j, s_edge, m, kind, desc);
                else if (up) msplit_bins<KB, MSPLIT_UPPER, BIN_GROUP>(raw + j, bin + j, s_edge, m, kind, desc);
                else msplit_bins<KB, MSPLIT_LOWER, BIN_GROUP>(raw + j, bin + j, s_edge, m, kind, desc);
            }
        } else {
#pragma unroll
            for (int j = 0; j < IPT; ++j) bin[j] = 0;
        }
        rounds = msplit_rounds(have);
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            if (!(any >> j & 1u)) break;  // (uniform: no lane has a row in this round or a later one)
            const bool valid = (rounds >> j & 1u) != 0;
            const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin[j]);  // lane 0 has a row
            const uint32_t b = valid ? bin[j] : b0;
            const U v = val[j];  // (the identity where the lane has no row)
            const uint64_t live = __builtin_amdgcn_ballot_w64(valid);
            if (__builtin_amdgcn_ballot_w64(b != b0) == 0) {  // one bin: no cross-lane work
                if (b0 != cur) {
                    flush();
                    cur = b0;
                }
                mine = RV::combine(mine, v, op);
                cur_rows += (uint32_t)__popcll(live);
                continue;
            }
            const uint64_t same = msplit_match(b, nb);
            const uint64_t above = (same >> lane) >> 1;  // my peers in higher lanes
            uint32_t next = above ? lane + 1u + (uint32_t)__builtin_ctzll(above) : (uint32_t)WAVE;
            U x = v;
            while (__builtin_amdgcn_ballot_w64(next < (uint32_t)WAVE) != 0) {  // x: my value and those of 2^step - 1 peers above me
                const int src = (int)(next < (uint32_t)WAVE ? next : lane);
                const U y = pairs_shfl<U>(x, [src](uint32_t w) { return (uint32_t)__shfl((int)w, src); });
                const uint32_t nn = (uint32_t)__shfl((int)next, src);
                if (next < (uint32_t)WAVE) {
                    x = RV::combine(x, y, op);
                    next = nn;
                }
            }
            if (mbcnt64(same) == 0) {  // the group's first lane: bins differ between first lanes, and the row is this wave's
                row[b] = RV::combine(row[b], x, op);
                if (counting) {
                    const uint32_t c = (uint32_t)__popcll(same & live);
                    if (c) atomicAdd(&s_cnt[b], c);
                }
            }
        }
    }
    flush();
    __syncthreads();
    U* out = static_cast<U*>(part);
    for (uint32_t i = tid; i <= m; i += BINRED_WG) {
        U r = acc[0][i];
#pragma unroll
        for (int w = 1; w < BINRED_WAVES; ++w) r = RV::combine(r, acc[w][i], op);
        const uint64_t at = (uint64_t)i * gridDim.x + blockIdx.x;
        out[at] = r;
        if (counting) cntm[at] = s_cnt[i];
    }
}

// A wave per bin: out_values[b] <- the G partials of row b of part, in a fixed order; out_counts[b] (may be null, cb = 4 or
// 8 bytes) <- the sum of row b of cntm.  accumulate: combined onto / added to what the outputs held; with no row at all
// (N == 0) nothing is touched.  G == 0 (n == 0): the identities and zeros.  flip: see above.
template <int VB, bool FLT>
__global__ __launch_bounds__(BINRED_WG) void rsx_binred_final_kernel(const void* __restrict__ part, const uint32_t* __restrict__ cntm, uint32_t bins, uint32_t G,
                                                                     uint64_t n, const uint64_t* __restrict__ num, uint32_t op, uint64_t flip,
                                                                     uint32_t accumulate, void* __restrict__ out_values, void* __restrict__ out_counts, uint32_t cb) {
    using RV = BinredVal<VB, FLT>;
    using U = typename RV::U;
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t b = blockIdx.x * BINRED_WAVES + threadIdx.x / WAVE;
    if (b >= bins) return;  // (the whole wave)
    if (accumulate && bin_count_of(n, num) == 0) return;
    const U* prow = static_cast<const U*>(part) + (uint64_t)b * G;
    const uint32_t* crow = cntm + (uint64_t)b * G;
    U x = binred_identity<VB, FLT>(op);
    uint64_t c = 0;
    for (uint32_t i = lane; i < G; i += WAVE) {
        x = RV::combine(x, prow[i], op);
        if (out_counts) c += crow[i];
    }
    x = binred_wave<RV>(x, op);
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) c += pairs_shfl_xor<uint64_t>(c, o);
    if (lane != 0) return;
    U* ov = static_cast<U*>(out_values);
    const U sign = (U)flip;
    ov[b] = (U)((accumulate ? RV::combine((U)(ov[b] ^ sign), x, op) : x) ^ sign);
    if (out_counts) {
        if (cb == 8) {
            uint64_t* oc = static_cast<uint64_t*>(out_counts);
            oc[b] = accumulate ? oc[b] + c : c;
        } else {
            uint32_t* oc = static_cast<uint32_t*>(out_counts);
            oc[b] = accumulate ? oc[b] + (uint32_t)c : (uint32_t)c;
        }
    }
}

}  // namespace rsx
