// rsx_select_kernels.hpp -- the kernels of rsx_select_device (rsx.hip): the elements at given ranks of the stable sort of
// an UNSORTED key array, found by counting.  Nothing is moved: the levels walk the digits of the mapped key (sign flip,
// float total order, complemented for descending order: pairs_map) from the top, SELECT_BITS bits each, and keep, per
// rank, the bucket that holds it.
//   rsx_select_count_kernel<KB>    streams the current source -- the caller's keys, or the candidate buffer once one
//                                  exists -- in 16-byte words and adds every key's digit into LDS counters, one row of
//                                  2^SELECT_BITS counters per SLOT (a slot is one distinct key prefix among the ranks;
//                                  level 0 has one slot and no prefix test); the rows are flushed into global u64 bins
//                                  with integer atomics, non-zero counters only, so the result is order-free.
//   rsx_select_pick_kernel         one workgroup: per rank the bin that holds its residual rank; extends the rank's
//                                  prefix, adds the keys below the bin to its `less`, zeroes the bins it read, merges
//                                  ranks with equal prefixes into slots, and opens the gate when the source is still the
//                                  caller's array and the candidates C (the picked bins of the distinct slots) fit the
//                                  candidate buffer.
//   rsx_select_compact_kernel<KB>  gated: the mapped keys under any slot's prefix -> the candidate buffer, keys only, in
//                                  arbitrary order (one wave-aggregated returning atomic per round: ballot, popcount,
//                                  leader add).  From then on the count kernel reads the buffer.
// After the last level every rank's mapped value v and the number of keys below it are known on the device; the wanted
// element is occurrence e = rank - less of v in position order.  With an index asked for, three launches without atomics
// find it, and no workgroup waits for another:
//   rsx_select_tile_kernel<KB>     per tile of SELECT_TILE keys and per rank, the keys equal to v
//   rsx_select_scan_kernel         one workgroup per rank: the tile that holds occurrence e, and e inside it
//   rsx_select_find_kernel<KB>     one workgroup per rank: the position inside that tile; stores it and keys[position]
// Without one, rsx_select_write_kernel<KB> un-maps v into out_keys.
// No kernel writes outside the context's workspace and the nranks output keys and indices.
#pragma once

#include "rsx_device.hpp"
#include "rsx_pairs_kernels.hpp"

#include <type_traits>

namespace rsx {

constexpr uint32_t SELECT_MAX_RANKS = 8;   // ranks of one call: rows of LDS counters, uniform prefixes of a level
constexpr uint32_t SELECT_BITS = 11;       // bits of a level's digit
constexpr uint32_t SELECT_BINS = 1u << SELECT_BITS;
constexpr uint32_t SELECT_TILE = 4096;     // keys per workgroup of the tile kernel
constexpr uint32_t SELECT_CAND_DIV = 16;   // the candidate buffer holds n / SELECT_CAND_DIV + SELECT_CAND_FLOOR keys
constexpr uint32_t SELECT_CAND_FLOOR = 1024;
constexpr int SELECT_COUNT_WG = 512;       // 64 KiB of counters: two workgroups per CU
constexpr uint32_t SELECT_SHARE = 16384;   // fewest keys worth a workgroup of the count and compact kernels
static_assert(SELECT_MAX_RANKS * SELECT_BINS * 4 <= 80 * 1024, "the count kernel's counters leave no room for two workgroups per CU");
static_assert(SELECT_TILE % 256 == 0, "the find kernel gives every thread the same number of keys");

// What the kernels of one call hand each other: the front of the call's workspace, zeroed with the bins before level 0.
struct SelectState {
    uint32_t from_buffer;  // the count kernel's source: 0 the caller's keys, 1 the candidate buffer
    uint32_t compacted;    // 0: never; else 1 + the level after which the candidates were compacted
    uint32_t gate;         // the compact kernel behind this pick runs
    uint32_t nslots;
    uint64_t candidates;   // C of the last pick; once from_buffer is set, the keys in the buffer
    uint64_t cursor;       // the compact kernel's write cursor
    uint64_t v[SELECT_MAX_RANKS][2];       // per rank: the mapped key so far (lo, hi), undecided bits zero
    uint64_t resid[SELECT_MAX_RANKS];      // ... its rank among the keys under its prefix
    uint64_t less[SELECT_MAX_RANKS];       // ... and the keys below that prefix
    uint64_t slot_v[SELECT_MAX_RANKS][2];  // per slot: its prefix
    uint32_t slot_of[SELECT_MAX_RANKS];
    uint64_t tile[SELECT_MAX_RANKS];       // the scan kernel's answer: the tile of the wanted occurrence ...
    uint32_t within[SELECT_MAX_RANKS];     // ... and the occurrences of v ahead of it in that tile
    uint32_t found[SELECT_MAX_RANKS];      // (1: tile and within are valid; the state is zeroed before every call)
};
struct SelectRanks {
    uint64_t r[SELECT_MAX_RANKS];
};
// one level: the digit is bits [shift, shift + width) of the mapped key; the prefix is what lies above (none at level 0)
struct SelectLevel {
    uint32_t index, shift, width, last;
};

// ---- the mapped key as (lo, hi) words, its digit, and the test "the bits from `sh` up are those of p" (0 < sh < bits) ----
template <typename K>
__device__ __forceinline__ K select_key(uint64_t lo, uint64_t hi) {
    (void)hi;
    return (K)lo;
}
template <>
__device__ __forceinline__ PairsU128 select_key<PairsU128>(uint64_t lo, uint64_t hi) {
    return PairsU128{lo, hi};
}
template <typename K>
__device__ __forceinline__ uint32_t select_digit(K k, uint32_t shift, uint32_t mask) {
    return (uint32_t)((uint64_t)k >> shift) & mask;
}
template <>
__device__ __forceinline__ uint32_t select_digit<PairsU128>(PairsU128 k, uint32_t shift, uint32_t mask) {
    const uint64_t w = shift >= 64 ? k.hi >> (shift - 64) : shift == 0 ? k.lo : (k.lo >> shift) | (k.hi << (64 - shift));
    return (uint32_t)w & mask;
}
template <typename K>
__device__ __forceinline__ bool select_under(K k, K p, uint32_t sh) {
    return (((uint64_t)k ^ (uint64_t)p) >> sh) == 0;
}
template <>
__device__ __forceinline__ bool select_under<PairsU128>(PairsU128 k, PairsU128 p, uint32_t sh) {
    const uint64_t xl = k.lo ^ p.lo, xh = k.hi ^ p.hi;
    return sh >= 64 ? (xh >> (sh - 64)) == 0 : (xh | (xl >> sh)) == 0;
}
template <typename K>
__device__ __forceinline__ bool select_equal(K a, K b) {
    return !(a != b);
}

// Calls f(key) for every key of [p0, p1) of `src`, in no particular order: 16-byte words, VU of them in flight per
// thread, with the streaming hint when NT; the keys ahead of the first 16-byte boundary and those behind the last whole
// word go one by one (the C-ABI promises key alignment only).  All WG threads of the workgroup call it.
template <int KB, int WG, int VU, typename F>
__device__ __forceinline__ void select_stream(const void* __restrict__ src, uint64_t p0, uint64_t p1, bool stream, F&& f) {
    using K = typename PairsKey<KB>::type;
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    constexpr uint32_t VEC = 16 / KB;
    if (p0 >= p1) return;
    const K* keys = static_cast<const K*>(src);
    const uint32_t tid = threadIdx.x;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(keys + p0);  // (the same in every lane)
    uint64_t head = (uint64_t)(((16u - (uint32_t)(addr & 15u)) & 15u) / (uint32_t)KB);
    if (head > p1 - p0) head = p1 - p0;
    const uint64_t nvec = (p1 - p0 - head) / VEC;
    const v4u* vsrc = reinterpret_cast<const v4u*>(keys + p0 + head);
    auto word = [&](const v4u& v) {
        K k[VEC];
        __builtin_memcpy(k, &v, 16);
#pragma unroll
        for (uint32_t e = 0; e < VEC; ++e) f(k[e]);
    };
    auto words = [&](auto nt) {  // (one copy of the loops per kind of load: no test between the loads of a round)
        auto load = [&](uint64_t j) -> v4u {
            if constexpr (decltype(nt)::value) return __builtin_nontemporal_load(vsrc + j);
            else return vsrc[j];
        };
        uint64_t j = tid;
        for (; j + (uint64_t)(VU - 1) * WG < nvec; j += (uint64_t)VU * WG) {
            v4u v[VU];
#pragma unroll
            for (int u = 0; u < VU; ++u) v[u] = load(j + (uint64_t)u * WG);
#pragma unroll
            for (int u = 0; u < VU; ++u) word(v[u]);
        }
        for (; j < nvec; j += WG) word(load(j));
    };
    if (stream) words(std::true_type{});
    else words(std::false_type{});
    const uint64_t t0 = p0 + head + nvec * VEC;  // fewer than VEC keys at either end
    if (tid < head) f(keys[p0 + tid]);
    if (tid >= 64 && tid - 64 < p1 - t0) f(keys[t0 + (tid - 64)]);
}

// the share [p0, p1) of workgroup b when `count` keys are cut into shares of at least SELECT_SHARE keys
__device__ __forceinline__ void select_share(uint64_t count, uint64_t* p0, uint64_t* p1) {
    uint64_t per = (count + gridDim.x - 1) / gridDim.x;
    if (per < SELECT_SHARE) per = SELECT_SHARE;
    per = (per + 15u) & ~(uint64_t)15u;
    *p0 = (uint64_t)blockIdx.x * per;
    *p1 = *p0 + per < count ? *p0 + per : count;
}

template <int KB>
__global__ __launch_bounds__(SELECT_COUNT_WG) void rsx_select_count_kernel(const void* __restrict__ keys, uint64_t n, const void* __restrict__ buffer,
                                                                          const SelectState* __restrict__ state,
                                                                          unsigned long long* __restrict__ bins, uint64_t cand_cap, SelectLevel lv,
                                                                          uint32_t kind, uint32_t desc, uint32_t stream) {
    using K = typename PairsKey<KB>::type;
    __shared__ __attribute__((aligned(16))) uint32_t cnt[SELECT_MAX_RANKS * SELECT_BINS];
    const uint32_t tid = threadIdx.x;
    const bool first = lv.index == 0;
    const bool from_buffer = !first && state->from_buffer != 0;  // (uniform: scalar loads)
    const uint64_t count = from_buffer ? (state->candidates < cand_cap ? state->candidates : cand_cap) : n;  // (never past the buffer)
    uint64_t p0, p1;
    select_share(count, &p0, &p1);
    if (p0 >= p1) return;
    uint32_t nslots = first ? 1u : state->nslots;
    if (nslots > SELECT_MAX_RANKS) nslots = SELECT_MAX_RANKS;
    K pre[SELECT_MAX_RANKS];
#pragma unroll
    for (uint32_t s = 0; s < SELECT_MAX_RANKS; ++s) pre[s] = first ? select_key<K>(0, 0) : select_key<K>(state->slot_v[s][0], state->slot_v[s][1]);
    for (uint32_t i = tid; i < nslots * SELECT_BINS / 4u; i += SELECT_COUNT_WG) reinterpret_cast<uint4*>(cnt)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const uint32_t mask = (1u << lv.width) - 1u, sh = lv.shift + lv.width;
    const uint32_t mkind = from_buffer ? 0u : kind, mdesc = from_buffer ? 0u : desc;  // the buffer holds mapped keys
    // Equal digits across a wave (all keys equal, a few values) would queue up on one counter: a wave whose lanes all
    // hold the first lane's bin adds their number once.
    auto add = [&](bool hit, uint32_t bin) {
        const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
        const bool same = hit && bin == b0;
        const uint64_t m = __builtin_amdgcn_ballot_w64(same);
        if (same) {
            if (mbcnt64(m) == 0) atomicAdd(&cnt[b0], (uint32_t)__popcll(m));
        } else if (hit) {
            atomicAdd(&cnt[bin], 1u);
        }
    };
    const void* src = from_buffer ? buffer : keys;
    if (first) {
        select_stream<KB, SELECT_COUNT_WG, KB == 16 ? 2 : 4>(src, p0, p1, stream != 0, [&](K raw) {
            const K k = pairs_map<K>(raw, mkind, mdesc);
            add(true, select_digit<K>(k, lv.shift, mask));
        });
    } else {
        select_stream<KB, SELECT_COUNT_WG, KB == 16 ? 2 : 4>(src, p0, p1, stream != 0 && !from_buffer, [&](K raw) {
            const K k = pairs_map<K>(raw, mkind, mdesc);
            uint32_t row = SELECT_MAX_RANKS;  // (the slots' prefixes differ: at most one holds the key)
#pragma unroll
            for (uint32_t s = 0; s < SELECT_MAX_RANKS; ++s)
                if (s < nslots && select_under<K>(k, pre[s], sh)) row = s;
            add(row < SELECT_MAX_RANKS, (row & (SELECT_MAX_RANKS - 1u)) * SELECT_BINS + select_digit<K>(k, lv.shift, mask));
        });
    }
    __syncthreads();
    for (uint32_t i = tid; i < nslots * SELECT_BINS; i += SELECT_COUNT_WG) {
        const uint32_t c = cnt[i];
        if (c) atomicAdd(&bins[i], (unsigned long long)c);
    }
}

// One workgroup of 1024 threads, two bins each.
__global__ __launch_bounds__(1024) void rsx_select_pick_kernel(SelectState* __restrict__ state, unsigned long long* __restrict__ bins, SelectRanks ranks,
                                                               uint32_t nranks, SelectLevel lv, uint64_t cand_cap) {
    __shared__ uint64_t s_wave[16];
    __shared__ uint64_t s_resid[SELECT_MAX_RANKS], s_below[SELECT_MAX_RANKS], s_count[SELECT_MAX_RANKS];
    __shared__ uint64_t s_v[SELECT_MAX_RANKS][2];
    __shared__ uint32_t s_slot[SELECT_MAX_RANKS], s_bin[SELECT_MAX_RANKS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const bool first = lv.index == 0;
    const uint32_t nslots = first ? 1u : (state->nslots < SELECT_MAX_RANKS ? state->nslots : SELECT_MAX_RANKS);
    if (tid < SELECT_MAX_RANKS) {
        uint64_t r = 0;
#pragma unroll
        for (uint32_t q = 0; q < SELECT_MAX_RANKS; ++q)
            if (tid == q) r = ranks.r[q];
        s_resid[tid] = first ? r : state->resid[tid];
        s_slot[tid] = first ? 0u : state->slot_of[tid];
        s_below[tid] = 0;
        s_count[tid] = 0;
        s_bin[tid] = 0;
    }
    __syncthreads();
    for (uint32_t s = 0; s < nslots; ++s) {
        unsigned long long* row = bins + (size_t)s * SELECT_BINS;
        const uint64_t b0 = row[2 * tid], b1 = row[2 * tid + 1];
        row[2 * tid] = 0;  // clean for the next level's count
        row[2 * tid + 1] = 0;
        const uint64_t pair = b0 + b1;
        uint64_t incl = pair;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t up = pairs_shfl_up<uint64_t>(incl, o);
            if (lane >= (uint32_t)o) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint64_t excl = incl - pair;
        for (uint32_t w = 0; w < wave; ++w) excl += s_wave[w];
        for (uint32_t q = 0; q < nranks; ++q) {
            if (s_slot[q] != s) continue;
            const uint64_t r = s_resid[q];
            if (r >= excl && r - excl < pair) {  // exactly one thread: the counts of a slot sum to more than its ranks
                const bool lowbin = r - excl < b0;
                s_bin[q] = 2 * tid + (lowbin ? 0u : 1u);
                s_below[q] = lowbin ? excl : excl + b0;
                s_count[q] = lowbin ? b0 : b1;
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    for (uint32_t q = 0; q < nranks; ++q) {
        uint64_t lo = first ? 0 : state->v[q][0], hi = first ? 0 : state->v[q][1];
        const uint64_t d = s_bin[q];
        if (lv.shift >= 64) {
            hi |= d << (lv.shift - 64);
        } else {
            lo |= d << lv.shift;
            if (lv.shift + lv.width > 64) hi |= d >> (64 - lv.shift);
        }
        s_v[q][0] = lo;
        s_v[q][1] = hi;
        state->v[q][0] = lo;
        state->v[q][1] = hi;
        state->less[q] = (first ? 0 : state->less[q]) + s_below[q];
        state->resid[q] = s_resid[q] - s_below[q];
    }
    uint32_t slots = 0;
    uint64_t cands = 0;
    for (uint32_t q = 0; q < nranks; ++q) {  // ranks with equal prefixes share a slot
        uint32_t s = slots;
        for (uint32_t p = 0; p < q; ++p)
            if (s_v[p][0] == s_v[q][0] && s_v[p][1] == s_v[q][1]) {
                s = s_slot[p];
                break;
            }
        if (s == slots) {
            state->slot_v[s][0] = s_v[q][0];
            state->slot_v[s][1] = s_v[q][1];
            cands += s_count[q];
            ++slots;
        }
        s_slot[q] = s;  // (the old slots are done with)
        state->slot_of[q] = s;
    }
    state->nslots = slots;
    const bool from_buffer = !first && state->from_buffer != 0;
    const bool open = !from_buffer && !lv.last && cands <= cand_cap;
    state->gate = open ? 1u : 0u;
    if (open) {  // (the compact kernel behind this launch reads the caller's keys whatever this says)
        state->from_buffer = 1u;
        state->compacted = 1u + lv.index;
    }
    if (!from_buffer) state->candidates = cands;  // the buffer's length, once it exists
}

template <int KB>
__global__ __launch_bounds__(256) void rsx_select_compact_kernel(const void* __restrict__ keys, uint64_t n, void* __restrict__ buffer, uint64_t cap,
                                                                 SelectState* __restrict__ state, SelectLevel lv, uint32_t kind, uint32_t desc,
                                                                 uint32_t stream) {
    using K = typename PairsKey<KB>::type;
    if (state->gate == 0) return;
    uint64_t p0, p1;
    select_share(n, &p0, &p1);
    if (p0 >= p1) return;
    uint32_t nslots = state->nslots;
    if (nslots > SELECT_MAX_RANKS) nslots = SELECT_MAX_RANKS;
    // (through LDS: eight uniform 128-bit prefixes and the lane masks of their tests do not fit the scalar registers)
    __shared__ K pre[SELECT_MAX_RANKS];
    if (threadIdx.x < SELECT_MAX_RANKS) pre[threadIdx.x] = select_key<K>(state->slot_v[threadIdx.x][0], state->slot_v[threadIdx.x][1]);
    __syncthreads();
    const uint32_t sh = lv.shift;  // the prefixes now include this level's digit
    K* out = static_cast<K*>(buffer);
    unsigned long long* cursor = reinterpret_cast<unsigned long long*>(&state->cursor);
    select_stream<KB, 256, KB == 16 ? 2 : 4>(keys, p0, p1, stream != 0, [&](K raw) {
        const K k = pairs_map<K>(raw, kind, desc);
        bool hit = false;
#pragma unroll
        for (uint32_t s = 0; s < SELECT_MAX_RANKS; ++s) hit = hit || (s < nslots && select_under<K>(k, pre[s], sh));
        const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
        if (hit) {  // (the first active lane in here is the lowest lane of m: the leader)
            const uint32_t below = mbcnt64(m);
            unsigned long long base = 0;
            if (below == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
            const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
            const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
            const uint64_t at = ((uint64_t)bhi << 32 | blo) + below;
            if (at < cap) out[at] = k;  // (the pick kernel counted them: they fit)
        }
        __builtin_amdgcn_sched_barrier(0);  // (one key's tests at a time: their lane masks are scalar registers)
    });
}

template <int KB>
__global__ __launch_bounds__(256) void rsx_select_tile_kernel(const void* __restrict__ keys, uint64_t n, const SelectState* __restrict__ state,
                                                              uint32_t* __restrict__ tile_count, uint64_t tiles, uint32_t nranks, uint32_t kind,
                                                              uint32_t desc, uint32_t stream) {
    using K = typename PairsKey<KB>::type;
    __shared__ uint32_t s_part[4][SELECT_MAX_RANKS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    K want[SELECT_MAX_RANKS];  // the raw bytes of every rank's value (uniform)
#pragma unroll
    for (uint32_t q = 0; q < SELECT_MAX_RANKS; ++q) want[q] = pairs_unmap<K>(select_key<K>(state->v[q][0], state->v[q][1]), kind, desc);
    uint32_t c[SELECT_MAX_RANKS];
#pragma unroll
    for (uint32_t q = 0; q < SELECT_MAX_RANKS; ++q) c[q] = 0;
    const uint64_t p0 = (uint64_t)blockIdx.x * SELECT_TILE;
    const uint64_t p1 = p0 + SELECT_TILE < n ? p0 + SELECT_TILE : n;
    auto run = [&](auto nr) {  // (one rank, the common call, compares once per key)
        constexpr uint32_t NR = decltype(nr)::value;
        select_stream<KB, 256, KB == 16 ? 2 : 4>(keys, p0, p1, stream != 0, [&](K raw) {
#pragma unroll
            for (uint32_t q = 0; q < NR; ++q) c[q] += select_equal<K>(raw, want[q]) ? 1u : 0u;
            __builtin_amdgcn_sched_barrier(0);  // (one key's compares at a time: their lane masks are scalar registers)
        });
    };
    if (nranks == 1) run(std::integral_constant<uint32_t, 1>{});
    else run(std::integral_constant<uint32_t, SELECT_MAX_RANKS>{});
#pragma unroll
    for (uint32_t q = 0; q < SELECT_MAX_RANKS; ++q) {
        uint32_t x = c[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o);
        if (lane == 0) s_part[wave][q] = x;
    }
    __syncthreads();
    if (tid < nranks) tile_count[(uint64_t)tid * tiles + blockIdx.x] = s_part[0][tid] + s_part[1][tid] + s_part[2][tid] + s_part[3][tid];
}

// Workgroup q: the first tile at which the running number of keys equal to rank q's value exceeds its occurrence.
__global__ __launch_bounds__(1024) void rsx_select_scan_kernel(SelectState* __restrict__ state, const uint32_t* __restrict__ tile_count, uint64_t tiles) {
    __shared__ uint64_t s_wave[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, q = blockIdx.x;
    const uint32_t* cnt = tile_count + (uint64_t)q * tiles;
    const uint64_t e = state->resid[q];
    uint64_t running = 0;
    for (uint64_t base = 0; base < tiles; base += 1024u) {
        const uint64_t t = base + tid;
        const uint64_t c = t < tiles ? cnt[t] : 0u;
        uint64_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t up = pairs_shfl_up<uint64_t>(incl, o);
            if (lane >= (uint32_t)o) incl += up;
        }
        __syncthreads();  // (the previous round's totals have been read)
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint64_t excl = running + incl - c, total = 0;
        for (uint32_t w = 0; w < 16; ++w) {
            if (w < wave) excl += s_wave[w];
            total += s_wave[w];
        }
        if (e >= excl && e - excl < c) {
            state->tile[q] = t;
            state->within[q] = (uint32_t)(e - excl);
            state->found[q] = 1;
        }
        if (e < running + total) return;  // (uniform)
        running += total;
    }
}

// Workgroup q: thread t looks at keys [t * PER, (t + 1) * PER) of the tile, so the threads' counts are in position order.
template <int KB>
__global__ __launch_bounds__(256) void rsx_select_find_kernel(const void* __restrict__ keys, uint64_t n, const SelectState* __restrict__ state,
                                                              void* __restrict__ out_keys, void* __restrict__ out_index, uint32_t ib, uint32_t kind,
                                                              uint32_t desc) {
    using K = typename PairsKey<KB>::type;
    constexpr uint32_t PER = SELECT_TILE / 256;
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, q = blockIdx.x;
    if (state->found[q] == 0) return;  // (uniform)
    const K want = pairs_unmap<K>(select_key<K>(state->v[q][0], state->v[q][1]), kind, desc);
    const K* src = static_cast<const K*>(keys);
    const uint64_t first = state->tile[q] * SELECT_TILE + (uint64_t)tid * PER;
    const uint32_t e = state->within[q];
    uint32_t hits = 0;  // bit j: key first + j is the value
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j)
        if (first + j < n && select_equal<K>(src[first + j], want)) hits |= 1u << j;
    const uint32_t mine = (uint32_t)__popc(hits);
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= (uint32_t)o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t excl = incl - mine;
    for (uint32_t w = 0; w < wave; ++w) excl += s_wave[w];
    if (e < excl || e - excl >= mine) return;
    uint32_t left = e - excl, j = 0;
    for (; j < PER; ++j)
        if ((hits >> j) & 1u) {
            if (left == 0) break;
            --left;
        }
    const uint64_t pos = first + j;
    if (out_index) {
        if (ib == 4) static_cast<uint32_t*>(out_index)[q] = (uint32_t)pos;
        else static_cast<uint64_t*>(out_index)[q] = pos;
    }
    if (out_keys) static_cast<K*>(out_keys)[q] = src[pos];
}

template <int KB>
__global__ __launch_bounds__(64) void rsx_select_write_kernel(const SelectState* __restrict__ state, void* __restrict__ out_keys, uint32_t nranks,
                                                              uint32_t kind, uint32_t desc) {
    using K = typename PairsKey<KB>::type;
    const uint32_t q = threadIdx.x;
    if (q < nranks) static_cast<K*>(out_keys)[q] = pairs_unmap<K>(select_key<K>(state->v[q][0], state->v[q][1]), kind, desc);
}

}  // namespace rsx
