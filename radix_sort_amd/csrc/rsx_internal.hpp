// rsx_internal.hpp -- host-side state and helpers shared by the sixteen translation units of librsx.so:
//   rsx.hip         the C-ABI of include/rsx.h (context, pass loop, multi-GPU driver, harness)
//   rsx_es.hip      the kernel launchers of ONE element size (compiled once per size with -DRSX_ES=n,
//                   so the eight sizes build in parallel), reached through that size's EsLaunchers table
//   rsx_pairs.hip   the join and split kernels of the key / value calls
//   rsx_unique.hip  the run kernels of rsx_unique_device and, around their tile scan, the kernels of rsx_compact_device
//   rsx_scan.hip    the kernels of rsx_scan_by_key_device and, through rsx_reduce.hip, which it includes, the run kernels
//                   of rsx_reduce_by_key_device
//   rsx_search.hip  the kernel of rsx_search_sorted_device and, built from its functions, those of rsx_join_device
//   rsx_merge.hip   the kernels of rsx_merge_device
//   rsx_setops.hip  the kernel of rsx_setop_device
//   rsx_lex.hip     the join of several key columns (rsx_lexsort_device, rsx_sort_columns_device)
// and what they agree on before a kernel is picked: the dispatch on a key width (for_key_width) and on the value and
// index widths of the merge and set-operation kernels, the fused value widths, and the tile count of one launch.
#pragma once
#include "rsx_device.hpp"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <algorithm>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rsx.h"

namespace rsxh {
using namespace rsx;

// aux block layout (one hipMalloc, zeroed at creation).
// What a sort ACCUMULATES into before any of its kernels could clear it -- every pass's ticket / roll-call words, the
// count matrix of the most significant digit (middle sizes) and count matrix 0 -- lives in a CONTROL BLOCK, and there
// are three of them: sort k uses block k % 2 and its count kernel, on its way, zeroes the block sort k - 1 used, so
// that no memset launch stands between two sorts (3.5 us of 60 at 2^16 keys).  Block 2 belongs to sorts that are being
// captured into a graph: a replay cannot alternate, so those zero their block themselves, with a memset, as every
// sort did before.  Count matrices 1 and 2 are cleared by the kernels of the sort itself (count kernel, first sweep).
// A count matrix is kept in J_REPL replicas (rsx_device.hpp): [J_REPL][num_regions][256] u64.
constexpr int MAX_PASSES = 16;                                                   // u128 keys
constexpr size_t J_BYTES = (size_t)J_REPL * MAX_REGIONS * RADIX * sizeof(uint64_t);  // one count matrix, all replicas
constexpr size_t TICKET_WORDS = ROLL_SHARDS + (size_t)ROLL_SHARD_COUNT * ROLL_SHARD_STRIDE;  // per pass (rsx_device.hpp)
constexpr uint32_t PART_MAX_SUB = 16;  // sub-ranges of rsx_partition_count_device / rsx_partition_scatter_device
constexpr uint32_t MID_MAX_REGIONS = 16;  // middle-size sorts: regions of the most significant digit's count matrix
constexpr size_t CB_TICKETS = 0;                                                 // [MAX_PASSES][TICKET_WORDS] u32
constexpr size_t CB_JT = ((MAX_PASSES * TICKET_WORDS * 4 + 255) / 256) * 256;    // count matrix of the most significant digit
constexpr size_t JT_BYTES = (size_t)J_REPL * MID_MAX_REGIONS * RADIX * sizeof(uint64_t);
constexpr size_t CB_J0 = CB_JT + JT_BYTES;                                       // count matrix 0
constexpr size_t CB_BYTES = CB_J0 + J_BYTES;
static_assert(CB_BYTES % 16 == 0, "control blocks are zeroed with 16-byte stores");
constexpr int CB_COUNT = 3;
constexpr size_t OFF_J1 = CB_COUNT * CB_BYTES;
constexpr size_t OFF_J2 = OFF_J1 + J_BYTES;
constexpr size_t OFF_PART_TICKETS = OFF_J2 + J_BYTES;                            // control words of rsx_partition_scatter_device
constexpr size_t OFF_BASE = OFF_PART_TICKETS + ((TICKET_WORDS * 4 + 255) / 256) * 256;  // scratch of the context self-tests
constexpr size_t OFF_FLAGS = OFF_BASE + 4096;                                    // self-test verdicts
constexpr size_t OFF_DBG = OFF_FLAGS + 256;                                      // 16 waves x 8 diagnostic counters
constexpr size_t AUX_BYTES = OFF_DBG + 1024;
// words of the host-visible block (rsx_ctx::host_err, 64 bytes): a kernel that gives up a bounded wait sets the first; the
// second word group holds what the last middle-size sort and the last wide-key try reported, for the host's forecasts
constexpr uint32_t HV_ERROR = 0, HV_MID_HINT = 8, HV_WIDE_HINT = 9;
// rsx_sort_host: bytes of one pinned staging buffer -- the largest chunk RSX_OPT_HOST_CHUNK takes, and its default
constexpr size_t HOST_CHUNK = 32u << 20;
constexpr int HOST_RING = 4;
// every array carved out of a workspace starts on a 256-byte boundary
constexpr size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// rsx_ctx::last_path, what the last call ran.  The values are frozen: RSX_INFO_LAST_PASSES reports them in bits 24..27 (PATH_BIN, PATH_COMPACT, PATH_MSPLIT, PATH_BINRED: 24..28).
enum : uint32_t {
    PATH_LSD = 0,        // general passes
    PATH_SMALL = 1,      // one-launch sort
    PATH_MID_SPLIT = 2,  // middle-size bucket split
    PATH_COUNT8 = 3,     // one-byte counting
    PATH_COUNT16 = 4,    // two-byte counting
    PATH_WIDE = 5,       // wide-key hybrid (the device's verdict says whether it ran)
    PATH_SEGMENTS = 6,   // segmented and row sorts
    PATH_TOPK = 7,
    PATH_UNIQUE = 8,
    PATH_REDUCE = 9,
    PATH_SEARCH = 10,
    PATH_MERGE = 11,
    PATH_SETOP = 12,
    PATH_JOIN = 13,
    PATH_SCAN = 14,      // scan by key
    PATH_SELECT = 15,    // order statistics (the last value the four bits hold)
    PATH_BIN = 16,       // keys per bin: it takes bit 28 with it, where the sorts report their route (it has none)
    PATH_COMPACT = 17,   // rows that pass a predicate: bits 24 and 28, as PATH_BIN
    PATH_MSPLIT = 18,    // rows regrouped by bin: bits 25 and 28
    PATH_BINRED = 19,    // a value column combined per bin: bits 24, 25 and 28
};

// option bits (rsx_ctx_set_option): alternative kernel paths, all bit-exact
enum : uint32_t {
    OPT_DYNAMIC_TILES = 1u << 0,   // ticketed tiles, no roll call
    OPT_BALLOT_RANKS = 1u << 1,    // never rank by returned LDS atomics
    OPT_ATOMIC_RANKS = 1u << 2,    // atomics whatever the skew
    OPT_AGENT_STATUS = 1u << 3,    // agent-scope status stores everywhere
    OPT_NO_XCD_MAJOR = 1u << 4,    // plain blockIdx numbering
    OPT_GENERAL_BYTES = 1u << 5,   // one-byte elements through the general pass
    OPT_VERBOSE = 1u << 6,
    OPT_RANK_CHECK = 1u << 7,      // cross-check atomic ranks against ballots on real tiles (tests)
    OPT_NO_SMALL_SORT = 1u << 8,   // arrays of at most one tile through the general path too
    OPT_NO_MID_SORT = 1u << 9,     // middle sizes through the general path too (no bucket split)
};

}  // namespace rsxh

struct rsx_ctx {
    int device = 0;
    std::mutex mu;
    std::string err = "";
    void* status = nullptr;  // tile status words: two halves, alternating per pass
    size_t status_bytes = 0;
    char* aux = nullptr;
    uint32_t* host_err = nullptr;  // pinned, device-mapped: a kernel that gives up sets it (no sync needed to see it)
    uint32_t* host_err_dev = nullptr;
    // staging for rsx_sort_host
    void* host_buf[2] = {nullptr, nullptr};
    size_t host_bytes = 0;
    hipStream_t copy_stream = nullptr;
    void* pinned[4] = {nullptr, nullptr, nullptr, nullptr};  // ring of pinned bounce chunks
    size_t host_chunk = rsxh::HOST_CHUNK;  // RSX_OPT_HOST_CHUNK: bytes of one piece of the copy pipeline (the buffers keep their size)
    hipEvent_t copy_event[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t wide_skip = 0;     // sorts to go without trying the wide-key hybrid (the last try was refused on the device)
    char* wide_buf = nullptr;   // wide-key hybrid: bin totals [65536] u64, bin-block sums [256] u64, bucket starts [65537] u64, verdict u32
    uint32_t wide_mode = 1;     // RSX_OPT_WIDE_SORT: 0 off, 1 auto, 2 always, 3 auto without the size floor
    std::vector<const void*> lds_attr;  // kernels whose dynamic-LDS limit was raised on this context's device (ensure_lds)
    uint64_t wide_tried_sig = 0, wide_refused_sig = 0;  // (layout, n) of the last hybrid try / of the last refusal
    uint32_t bucket_no_skip = 0;  // RSX_OPT_BUCKET_SKIP == 0
    uint32_t bucket_group = 1;    // RSX_OPT_BUCKET_GROUP: small buckets of the hybrid are sorted in groups
    uint32_t bucket_direct = 1;   // RSX_OPT_BUCKET_DIRECT: key-only elements go through rsx_bucket16_direct_kernel
    uint32_t last_direct = 0;     // the last hybrid sort enqueued that kernel (RSX_INFO_LAST_DIRECT)
    uint32_t* ovf16 = nullptr;  // u16 / i16 counting path: 65536 overflow counters, all zero between sorts
    unsigned long long* part_J = nullptr;  // rsx_partition_count_device: one count matrix per sub-range (PART_MAX_SUB x J_BYTES)
    // multi-GPU driver (rsx_sort_sharded): per-slice stream and splitter-search scratch, made once
    hipStream_t shard_stream = nullptr;
    uint64_t* shard_q = nullptr;     // device: queries (lo, hi) + ranges (begin, end)
    uint64_t* shard_out = nullptr;   // device: answers
    uint64_t* shard_hist = nullptr;  // device: 256 digit counts
    uint64_t* shard_host = nullptr;  // pinned: answers, then the 256 counts
    std::vector<uint64_t> shard_stage;
    int num_cu = 256;
    uint32_t last_path = 0;    // rsxh::PATH_*
    uint32_t last_sort_passes = 0;  // sweep passes of the last sort (RSX_INFO_LAST_PASSES)
    uint32_t last_route = 0;   // how the last sort reached the kernels: 0 direct, 1 packed re-layout, 2 key-index proxy
    char* any_buf = nullptr;   // routes 1 / 2: the re-laid-out elements or the proxies, and their ping-pong array
    size_t any_bytes = 0;
    uint32_t last_pairs = 0;   // RSX_INFO_LAST_PAIRS: route of the last pairs / argsort call (1 joined, 2 proxies) | joined element size << 8
    uint32_t last_lex = 0;     // RSX_INFO_LAST_LEX: rounds of the last lexsort / sort-columns call | element size of its last round << 8
    uint64_t cb_used[2][2] = {{0, 0}, {0, 0}};  // per alternating block: bytes of the top-digit matrix / of count matrix 0 its last sort used
    uint32_t cb_alt = 0;       // which of the two alternating blocks the last uncaptured sort used
    uint32_t cb_last = 0;      // control block of the last sort that ran sweeps (RSX_INFO_LAST_PASSES)
    bool cb_dirty = false;     // an enqueue failed half way: both alternating blocks are zeroed by memset before the next sort
    uint32_t mid_choice = 0;   // what the last middle-size sort was enqueued as (1 / 2)
    uint32_t mid_force = 0;    // RSX_OPT_MID_SORT 2 / 3: always split (1) / always LSD passes (2)
    uint32_t mid_cooldown = 0; // sorts to go by LSD passes after a bucket split met a skewed input
    bool rank_atomic = false;  // LDS atomic ordering self-test passed (set when the workspace is first made)
    bool l2_local = false;     // same-XCD hand-off self-test passed: chains may keep status words in their L2
    uint32_t hot_lanes = 16;
    uint32_t options = 0;      // OPT_* (rsx_ctx_set_option)
    uint32_t max_regions = 0;  // 0 = default per element size
    uint32_t dbg = 0;          // RSX_TUNING builds only: timing ablations (wrong output by design)
    // stream-ordered reuse: work of this context on another stream waits for the last enqueue
    hipStream_t last_stream = nullptr;
    hipEvent_t last_event = nullptr;
    bool busy = false;
    // per-launch HIP-event timing (rsx_ctx_profile)
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pending[RSX_PROF_KINDS];
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_free;
    double prof_ms[RSX_PROF_KINDS] = {0, 0, 0, 0};
    uint64_t prof_n[RSX_PROF_KINDS] = {0, 0, 0, 0};
    std::vector<float> prof_each;  // per-launch sweep times (rsx_debug_sweep_times)
};

namespace rsxh {

// What belongs to ONE sort (or lone pass) while it is being enqueued: made on the stack by the entry point's body and
// handed down to the launchers, so that nothing of one call is left behind on the context for the next.
struct SortRun {
    uint32_t cb = 0;  // control block of this sort (aux layout above)
    CleanList clean = {{nullptr, nullptr, nullptr}, {0, 0, 0}};  // what the first count kernel zeroes on its way (the previous sort's control block)
    Gate gate = {nullptr, 0, 0};  // of a gated kernel sequence (wide keys)
    const DigitSpec* spec_dev = nullptr;  // the hybrid's sweeps read their digits from the device's plan (WidePlan::specs)
    uint32_t* tickets_override = nullptr;  // rsx_partition_scatter_device: control words outside the blocks
};
// ... and to one sweep within it
struct SweepPass {
    uint32_t index;  // of the sweep within its sort (selects the status half, the ticket words)
    bool last;       // no pass follows: nothing to clean
    uint32_t mid;    // middle-size sort, first sweep (MID instantiation): 1 = bucket split by the top digit, 2 = first LSD pass
};

inline int fail(rsx_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
    if (c) {
        c->err = what;
        if (e != hipSuccess) {
            c->err += ": ";
            c->err += hipGetErrorString(e);
        }
    }
    return code;
}

#define RSX_HIP(call)                                                   \
    do {                                                                \
        hipError_t _e = (call);                                         \
        if (_e != hipSuccess) return fail(ctx, RSX_ERR_HIP, #call, _e); \
    } while (0)

// Records a start/stop event pair around one launch when profiling is on.
struct LaunchTimer {
    rsx_ctx* c;
    int kind;
    hipStream_t st;
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    LaunchTimer(rsx_ctx* ctx, int k, hipStream_t s) : c(ctx), kind(k), st(s) {
        if (!c->prof) return;
        if (!c->prof_free.empty()) {
            ev = c->prof_free.back();
            c->prof_free.pop_back();
        } else if (hipEventCreate(&ev.first) != hipSuccess || hipEventCreate(&ev.second) != hipSuccess) {
            ev = {nullptr, nullptr};
            return;
        }
        (void)hipEventRecord(ev.first, st);
    }
    ~LaunchTimer() {
        if (!ev.first) return;
        (void)hipEventRecord(ev.second, st);
        c->prof_pending[kind].push_back(ev);
    }
};

// Keys per thread by element size.  Tiles need not be powers of two (the last tile of a region is
// partial anyway); bigger tiles mean longer output runs per digit (fewer partial cache lines, the
// memory system's real cost here) and fewer look-backs per key, as long as two or three workgroups
// still fit a CU: u32 28 x 512 = 14336 keys (56 KiB), u64 14 x 512 (56 KiB), 16-byte 5 x 512 (40 KiB),
// 12-byte 10 x 512 (60 KiB), 24-byte 5 x 512 (60 KiB), 32-byte 3 x 512 (48 KiB).
// Measured against 16 / 8 / 4: 1B u32 117 -> 136, 1B u64 32 -> 34.9, 128M (u64,u64) 17.3 -> 18 Gkeys/s.
#ifndef RSX_REGION_FLOOR
#define RSX_REGION_FLOOR 6  // log2 of the fewest tiles worth a region of their own
#endif
#ifndef RSX_KPT4
#define RSX_KPT4 28
#endif
#ifndef RSX_KPT2
#define RSX_KPT2 RSX_KPT4  // 1- and 2-byte elements
#endif
#ifndef RSX_WG4
#define RSX_WG4 512
#endif
#ifndef RSX_KPT8
#define RSX_KPT8 14  // 56 KiB tiles, still two workgroups per CU with 16 regions: 1B u64 30.8 -> 30.15 ms, Zipf u64 -3.4 % (12: round 1)
#endif
#ifndef RSX_KPT16
#define RSX_KPT16 5
#endif
#ifndef RSX_KPT12
#define RSX_KPT12 10
#endif
#ifndef RSX_KPT32
#define RSX_KPT32 3
#endif
#ifndef RSX_KPT24
#define RSX_KPT24 5  // with 8 regions: 60 KiB tiles at two workgroups per CU: 2 GiB of (u64,[u64;2]) 8.34 -> 7.53 ms (3 x 512, 16 regions)
#endif
#ifndef RSX_WG8
#define RSX_WG8 512
#endif
// rsx_bucket_sort_kernel: 1024 threads x BKPT elements in registers, the bucket in LDS (<= 112 KiB, 8-byte elements
// 136 KiB) beside 16 KiB of wave counters
constexpr int bucket_kpt_for(int es) { return es <= 4 ? 28 : es == 8 ? 17 : es == 12 ? 9 : es == 16 ? 7 : es == 24 ? 4 : 3; }
// ... and of the hybrid's 1024-thread form, which fills the LDS: as many registers as hold what 160 KiB leave beside the
// wave counters (bucket_cape: 16-byte elements 9020 of 9216 slots); its smaller forms and the middle sizes keep the shorter
// unrolled loops.
constexpr int wide_kpt_for(int es) { return es <= 4 ? 28 : es == 8 ? 17 : es == 12 ? 12 : es == 16 ? 9 : es == 24 ? 6 : 5; }
// ... and of rsx_bucket16_medium_kernel (1024 threads).  It inlines the split, the LDS sort and the sort through memory: with
// the bucket kernel's 17 eight-byte elements per thread it spilled 113-141 registers into 950-970 bytes of scratch per lane
// (16 per thread: 792 bytes; 15: 32), and a kernel with that much scratch takes 20-25 us to DISPATCH even when its gate sends
// it home at once -- every hybrid sort of 8-byte elements paid that (6 % of a 2^23-key sort).
#ifndef RSX_KMED8
#define RSX_KMED8 15
#endif
constexpr int medium_kpt_for(int es) { return es == 8 ? RSX_KMED8 : wide_kpt_for(es); }
// whether an array's 1024-thread form is the longer one: when the average bucket is above 7/8 of what the shorter holds
constexpr bool wide_big_form(int es, uint64_t n) { return n / 65536u > (uint64_t)1024 * (uint64_t)bucket_kpt_for(es) * 7u / 8u; }
// The dynamic LDS of a workgroup that sorts in LDS (rsx_small_kernel.hpp, LdsTile, which carves it): the elements, the
// wave counters [wg / 64][256], 64 bytes of the waves' totals and the 3 KiB of the sort through memory.
constexpr uint32_t LDS_PER_CU = 163840u;  // gfx950: 160 KiB
constexpr size_t bucket_cnt_bytes() { return 4; }
constexpr uint32_t lds_tile_fixed(int wg) { return (uint32_t)(wg / 64) * 256u * (uint32_t)bucket_cnt_bytes() + 64u + 3u * 256u * 4u; }
// elements a workgroup of `wg` threads x `kpt` registers holds there: wg * kpt, or what 160 KiB leave beside the rest and
// 1 KiB for the kernels' static LDS (1024 threads of 16-byte elements: 9020 of 9216 slots)
constexpr uint32_t bucket_cape(int es, int kpt, int wg) {
    const uint32_t slots = (uint32_t)wg * (uint32_t)kpt;
    const uint32_t room = ((LDS_PER_CU - 1024u - lds_tile_fixed(wg)) / (uint32_t)es) & ~3u;
    return slots < room ? slots : room;
}
constexpr size_t lds_tile_bytes(int es, int kpt, int wg) { return (size_t)bucket_cape(es, kpt, wg) * (size_t)es + lds_tile_fixed(wg); }
// the LDS size classes of a segmented sort (rsx_segment_kernels.hpp): 256 and 1024 threads x bucket_kpt_for(es) elements
constexpr uint32_t segment_cap(int es, int cls) { return bucket_cape(es, bucket_kpt_for(es), cls == 0 ? 256 : 1024); }
// the hybrid's buffer (ctx->wide_buf): bucket totals [65536], block totals [256], starts [65537] (u64), then its WidePlan
constexpr size_t WIDE_PLAN_OFFSET = (65536 + 256 + 65537 + 1) * sizeof(uint64_t);
// ... then what rsx_bucket16_direct_kernel hands over to the kernels behind it: `left`, the number of buckets it left
// unsorted (a line of its own; cleared by rsx_scan16_kernel in every hybrid sort), and done[65536], a byte per bucket
constexpr size_t WIDE_LEFT_OFFSET = (WIDE_PLAN_OFFSET + sizeof(WidePlan) + 127) / 128 * 128;
constexpr size_t WIDE_DONE_OFFSET = WIDE_LEFT_OFFSET + 128;
constexpr size_t WIDE_BUF_BYTES = WIDE_DONE_OFFSET + 65536;
constexpr uint32_t bucket_cap(int es) { return 1024u * (uint32_t)bucket_kpt_for(es); }
// Largest array taken by the middle-size path: the average bucket is 4/7 of the capacity, so uniform top digits
// pass with a wide margin (2^22 4-byte, 2^20 16-byte elements); skewed ones fall back to LSD passes.  8-byte elements
// go up to 2^22 as well (the general path needs 275 us there, this one 90): the average bucket is then 16384 of 17408,
// eight standard deviations of a uniform top digit below the capacity; a bucket that overflows all the same is sorted
// through memory by its workgroup, which costs about what the general path would have.
// One-byte elements have no such path (their one digit is counted, never split): 0.
constexpr uint64_t mid_max_elems(int es) { return es == 1 ? 0 : es == 8 ? (1ull << 22) : (uint64_t)bucket_cap(es) * 256u * 4u / 7u; }
constexpr int kpt_for(int es) { return es <= 2 ? RSX_KPT2 : es <= 4 ? RSX_KPT4 : es == 8 ? RSX_KPT8 : es == 12 ? RSX_KPT12 : es == 16 ? RSX_KPT16 : es == 24 ? RSX_KPT24 : RSX_KPT32; }
constexpr int wg_for(int es) { return es <= 4 ? RSX_WG4 : es == 8 ? RSX_WG8 : 512; }
constexpr uint32_t tile_elems(int es) { return wg_for(es) * kpt_for(es); }
// The wide-key hybrid's SECOND sweep counts for no next pass (the bucket kernel follows), so the 16 KiB that the count
// matrix s_jn[16][256] takes beside a 512 x 14 tile of 8-byte elements hold four more keys per thread there:
// 512 x 18 x 8 + 4096 (wave counters) + 128 = 77952 B, to the byte what the first sweep asks for, still two workgroups
// per CU (19 does not fit).  Other element sizes keep kpt_for: 16-byte elements are capped at 80 VGPRs.
#ifndef RSX_HYB_KPT8
#define RSX_HYB_KPT8 18
#endif
constexpr int hyb_kpt_for(int es) { return es == 8 ? RSX_HYB_KPT8 : kpt_for(es); }
static_assert((size_t)RSX_WG8 * RSX_HYB_KPT8 * 8 + (RSX_WG8 / 64) * 256 * 2 + 128 <= LDS_PER_CU / 2, "the deep tile leaves no room for two workgroups per CU");
// The bucket split of a middle-size sort (rsx_mid_kernels.hpp) works on SMALL tiles, one workgroup each (a tile is one
// workgroup's serial work: 13 us for 14336 u32 keys, and 2^16 keys are five of those): 512 x 8 4-byte, 512 x 4 8-byte,
// 512 x 2 16-byte elements.
constexpr int mid_kpt_for(int es) { return es <= 4 ? 8 : es == 8 ? 4 : es == 12 ? 3 : 2; }
constexpr uint32_t mid_tile_elems(int es) { return 512u * (uint32_t)mid_kpt_for(es); }

inline uint32_t log2u(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }

// Regions: smallest power-of-two length (>= one tile) that covers n with <= cap of them.
// small_tiles: tile count of a middle-size sort's bucket split (mid_tile_elems): only its status_rows() is used, to size
// the workspace that holds the split's two tiles x 256 tables.
inline RegionGeom make_geom(const rsx_ctx* ctx, uint64_t n, uint32_t es, bool small_tiles = false) {
    RegionGeom g;
    g.n = n;
    g.tile = small_tiles ? mid_tile_elems((int)es) : tile_elems((int)es);
    uint32_t k = log2u(g.tile);
    if ((1ull << k) < g.tile) ++k;  // tiles need not be a power of two; regions are
    // A region is worth having from about 64 tiles on: every region ends with a partial tile and a workgroup of its
    // own, and widens every workgroup's count-matrix flush.  Measured with one region per 2^k keys: 2^18 u32
    // 109 -> 87 us, 2^22 u32 148 -> 134 us, 2^18 u64 249 -> 166 us, 2^22 u64 360 -> 275 us; large inputs are
    // bounded by `cap` as before.
    k += small_tiles ? 3 : RSX_REGION_FLOOR;
    // the next pass's count matrix costs 1 KiB of LDS per region: 8 where the tile needs the room.  (True of every sweep
    // that counts for a next pass -- all LSD passes but the last, the hybrid's first sweep; a last pass and the hybrid's
    // second sweep have no such matrix, and the latter spends the room on a deeper tile: hyb_geom.)
    const uint64_t cap = small_tiles ? MID_MAX_REGIONS : ctx->max_regions ? ctx->max_regions : (es == 8 || es == 32) ? 16 : 8;
    while (((n + (1ull << k) - 1) >> k) > cap) ++k;
    g.region_shift = k;
    g.num_regions = (uint32_t)((n + (1ull << k) - 1) >> k);
    if (g.num_regions == 0) g.num_regions = 1;
    return g;
}
inline uint64_t tiles_per_region(const RegionGeom& g) {
    return ((1ull << g.region_shift) + g.tile - 1) / g.tile;
}
inline uint64_t status_rows(const RegionGeom& g) {
    return (uint64_t)g.num_regions * tiles_per_region(g);
}
// The geometry of the hybrid's second sweep: the regions of `g` (same n, region_shift, num_regions) cut into the deeper
// tiles of hyb_kpt_for.  Its status rows are reg * tiles_per_region(deep) + kt, and they have to be rows that the first
// sweep zeroed (each of ITS tiles zeroes row reg * tiles_per_region(g) + kt of the next pass's half).  They are: every
// region but the last is full, so the first sweep zeroes all tiles_per_region(g) rows of it and, for the last, as many as
// that region has tiles -- one unbroken range [0, (NR - 1) * tpr + tiles(last)) --, and a deeper tile makes neither
// number larger, so the second sweep's rows are a prefix of that range (sort_wide checks the two numbers).
inline RegionGeom hyb_geom(const RegionGeom& g, uint32_t es) {
    RegionGeom d = g;
    d.tile = (uint32_t)wg_for((int)es) * (uint32_t)hyb_kpt_for((int)es);
    return d;
}
// rows of a sweep's status array in use: up to the last tile of the last region
inline uint64_t status_rows_used(const RegionGeom& g) {
    const uint64_t last = g.n - ((uint64_t)(g.num_regions - 1) << g.region_shift);
    return (uint64_t)(g.num_regions - 1) * tiles_per_region(g) + (last + g.tile - 1) / g.tile;
}
// chain prefixes are relative to the region: 30 value bits suffice up to 2^30-element regions
inline bool status32(const RegionGeom& g) { return g.region_shift <= 30; }

// More than 64 KiB of dynamic LDS has to be asked for, per kernel and per DEVICE: once per context.
inline void ensure_lds(rsx_ctx* ctx, const void* kernel, size_t bytes) {
    for (const void* k : ctx->lds_attr)
        if (k == kernel) return;
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    ctx->lds_attr.push_back(kernel);
}

inline DigitSpec make_spec(const rsx_layout* L, uint32_t digit) {
    DigitSpec s;
    const uint32_t byte = L->key_offset + digit;
    const uint32_t top = L->key_offset + L->key_bytes - 1;
    if (L->elem_bytes >= 4) {
        s.word = byte >> 2;
        s.shift = 8 * (byte & 3);
        s.top_word = top >> 2;
        s.top_shift = 8 * (top & 3) + 7;
    } else {  // 1- and 2-byte elements live in one register
        s.word = 0;
        s.shift = 8 * byte;
        s.top_word = 0;
        s.top_shift = 8 * top + 7;
    }
    s.flip = (L->key_kind != RSX_KEY_UNSIGNED && digit == L->key_bytes - 1) ? 0x80u : 0u;
    s.fsign = L->key_kind == RSX_KEY_FLOAT ? ~0u : 0u;
    return s;
}

// the three count matrices rotate: pass d reads J_of(d % 3), accumulates the next pass's into
// J_of((d + 1) % 3) and zeroes J_of((d + 2) % 3) for the pass after
inline char* cb_of(rsx_ctx* c, uint32_t which) { return c->aux + (size_t)which * CB_BYTES; }
inline unsigned long long* J_of(rsx_ctx* c, const SortRun& run, uint32_t which) {
    char* p = which == 0 ? cb_of(c, run.cb) + CB_J0 : which == 1 ? c->aux + OFF_J1 : c->aux + OFF_J2;
    return reinterpret_cast<unsigned long long*>(p);
}
inline unsigned long long* JT_of(rsx_ctx* c, const SortRun& run) { return reinterpret_cast<unsigned long long*>(cb_of(c, run.cb) + CB_JT); }
inline uint32_t* tickets_of(rsx_ctx* c, const SortRun& run, uint32_t pass) {
    return reinterpret_cast<uint32_t*>(cb_of(c, run.cb) + CB_TICKETS) + (size_t)pass * TICKET_WORDS;
}
inline uint32_t* part_tickets_of(rsx_ctx* c) { return reinterpret_cast<uint32_t*>(c->aux + OFF_PART_TICKETS); }
inline uint32_t* flags_of(rsx_ctx* c) { return reinterpret_cast<uint32_t*>(c->aux + OFF_FLAGS); }
inline volatile uint32_t& host_word(rsx_ctx* c, uint32_t w) { return reinterpret_cast<volatile uint32_t*>(c->host_err)[w]; }  // HV_*

// The wide-key hybrid sorts its small buckets in groups of 2^gs (0: none), about 3/4 of what a 512-thread workgroup of the
// bucket kernel holds (keys of at least 8 bytes): rsx_scan16_kernel is offered this shift and launch_bucket16 enqueues the
// form that goes with it, so both ask here.
inline uint32_t group_shift(const rsx_ctx* ctx, size_t n, const rsx_layout* L) {
    const uint64_t avg = (uint64_t)n / 65536u;
    uint32_t gs = 0;
    if (L->key_bytes >= 8 && ctx->bucket_group)
        while (gs < 6 && (avg << (gs + 1)) <= (uint64_t)512 * bucket_kpt_for((int)L->elem_bytes) * 3 / 4) ++gs;
    return gs >= 2 ? gs : 0;
}

// What one fused segmented key / value sort is asked to do (rsx.hip -> launch_segment_pairs of the joined element size).
struct SegPairsCall {
    void* keys;               // n keys of kb bytes (mode 1: only read)
    void* values;             // mode 0: n values of vb bytes (vb 0: none); mode 1: n indices of ib bytes; mode 2: n proxies (w0)
    void* w0;                 // the two workspace arrays of n joined elements (through-memory class only)
    void* w1;
    size_t n;
    uint32_t kb, vb;          // widths inside the joined element (modes 1 and 2: vb 4, the position)
    uint32_t kind, desc;
    uint32_t mode;            // rsx::SEGP_VALUES / SEGP_LOCAL / SEGP_GLOBAL
    uint32_t ib;
    const uint64_t* offsets;  // or nullptr: nseg rows of row_len
    uint64_t nseg, row_len, max_len;
};
// whether a segment above the largest LDS class can occur (the through-memory class is launched, its workspace needed)
inline bool segment_pairs_mem(uint32_t es, const uint64_t* offsets, uint64_t row_len, uint64_t max_len) {
    const uint64_t cap = segment_cap((int)es, 1);
    return offsets ? (max_len == 0 || max_len > cap) : row_len > cap;
}

// What one rsx_topk_rows_device call is asked to do (rsx.hip -> launch_topk of the joined (key, u32 position) element size).
struct TopkCall {
    const void* keys;         // rows x row_len keys of kb bytes, only read
    void* out_keys;           // rows x k keys, or nullptr
    void* out_index;          // rows x k positions of ib bytes, or nullptr
    void* w0;                 // rows longer than the largest LDS class: the two candidate arrays (topk_workspace_half bytes each)
    void* w1;
    uint64_t rows, row_len, k;
    uint32_t kb, kind, desc, ib;
};
// the largest k a row above the largest LDS class is selected with: every round of the tournament then shrinks the row
inline uint32_t topk_max_k(uint32_t es) { return segment_cap((int)es, 1) / 2u; }
// bytes of ONE candidate array: what the first round leaves, min(k, length) joined elements per chunk (0: no round needs one)
inline size_t topk_workspace_half(uint32_t es, uint64_t rows, uint64_t row_len, uint64_t k) {
    const uint64_t L = segment_cap((int)es, 1);
    if (row_len <= L) return 0;
    const uint64_t cpr = (row_len + L - 1) / L, last = row_len - (cpr - 1) * L;
    const uint64_t m1 = (cpr - 1) * k + (k < last ? k : last);
    return round256((size_t)(rows * m1) * es);
}

// ---- per-element-size launchers: defined in rsx_launch_impl.hpp; rsx_es.hip fills ONE size's table with them (which
// instantiates them), rsx.hip looks the table up by element size once per call (launchers_for).  A unit's kernels are emitted
// in the order of the members here: keeping it keeps the code objects comparable from one build to the next. ----
struct EsLaunchers {
    // every segment (offsets, or rows of row_len when offsets == nullptr) sorted by one workgroup: one launch per size class
    int (*segment_sort)(rsx_ctx* ctx, void* data, void* tmp, size_t n, const rsx_layout* L, const uint64_t* offsets, uint64_t nseg,
                        uint64_t row_len, uint64_t max_len, uint32_t* launched, hipStream_t st);
    // count phase of a first pass: J[rep][r][v] for `digit` over the input regions (J zeroed by the caller);
    // jclear: a second count matrix to clear on the way (or null); clear_status: zero the tile status words of
    // the sweep that follows (first half of the workspace).  Like every count launcher it hands run.clean to its kernel
    // and empties it: done once per sort.
    int (*hist)(rsx_ctx* ctx, SortRun& run, const void* src, const RegionGeom& g, const rsx_layout* L, uint32_t digit,
                unsigned long long* J, unsigned long long* jclear, bool clear_status, hipStream_t st);
    // the same counting a second digit (`digit2` into `J2`) on the same read (middle-size path)
    int (*hist2)(rsx_ctx* ctx, SortRun& run, const void* src, const RegionGeom& g, const rsx_layout* L, uint32_t digit,
                 unsigned long long* J, uint32_t digit2, unsigned long long* J2, unsigned long long* jclear, hipStream_t st);
    // wide keys, large arrays: the top 16 bits of the mapped key counted per workgroup (P[parts][32768]); the 65536
    // buckets (starts[65537]) sorted by the lower digits in LDS, in place
    int (*wideplan)(rsx_ctx* ctx, const void* src, size_t n, const rsx_layout* L, WidePlan* plan, hipStream_t st);
    int (*count16top)(rsx_ctx* ctx, const void* src, size_t n, const rsx_layout* L, WidePlan* plan, uint32_t* P, uint32_t parts,
                      uint32_t region_shift, uint32_t k, hipStream_t st);
    int (*marginal16)(rsx_ctx* ctx, SortRun& run, const uint32_t* P, uint32_t parts, uint32_t k, const RegionGeom& g, unsigned long long* J,
                      unsigned long long* jclear, hipStream_t st);
    int (*bucket16)(rsx_ctx* ctx, const SortRun& run, void* data, void* scratch, size_t n, const rsx_layout* L, const uint64_t* starts,
                    const WidePlan* plan, hipStream_t st);
    // first half of a middle-size sort: stable split of `src` into `dst` by the most significant digit (three launches)
    int (*mid_split)(rsx_ctx* ctx, const void* src, void* dst, size_t n, const rsx_layout* L, hipStream_t st);
    // second half: the 256 top-digit buckets of `src` sorted by the lower digits into `dst`; small: 256-thread workgroups
    int (*bucket_sort)(rsx_ctx* ctx, const void* src, void* dst, const rsx_layout* L, bool small, hipStream_t st);
    // one sweep pass.  J: this pass's count matrix; jnext: accumulated for the next pass (or null);
    // jzero: matrix to clear for the pass after next (or null); xf: bit 0 = map signed/float keys on
    // load (first pass), bit 1 = map back on store (last pass)
    int (*sweep)(rsx_ctx* ctx, const SortRun& run, const SweepPass& pass, const void* src, void* dst, const RegionGeom& g, const rsx_layout* L,
                 uint32_t digit, const unsigned long long* J, unsigned long long* jnext, unsigned long long* jzero, int xf, hipStream_t st);
    // arrays of at most one tile (tile_elems(ES)): the whole sort in one launch of one workgroup, in place
    int (*small_sort)(rsx_ctx* ctx, void* data, size_t n, const rsx_layout* L, hipStream_t st);
    int (*segcopy)(rsx_ctx* ctx, const void* src, void* dst, const uint64_t* so, const uint64_t* dof, const uint64_t* len, uint32_t nseg,
                   hipStream_t st);
    // every segment of separate key and value columns sorted by one workgroup (rsx_segment_pairs_kernels.hpp), for the
    // joined element size of this table: one launch per size class
    int (*segment_pairs)(rsx_ctx* ctx, const SegPairsCall& call, uint32_t* launched, hipStream_t st);
    // the first k of every row's stable sort (rsx_topk_kernels.hpp), for the joined (key, u32 position) element size of
    // this table (8, 16, 32): one launch per round, *launched receives their number
    int (*topk)(rsx_ctx* ctx, const TopkCall& call, uint32_t* launched, hipStream_t st);
};
template <int ES>
const EsLaunchers& es_launchers();  // specialised in rsx_es.hip

// ---- what the launcher units and rsx.hip agree on before a kernel is picked ----
template <int N>
using Width = std::integral_constant<int, N>;
// The key widths with kernels: calls f(Width<KB>{}) for kb = 1, 2, 4, 8, 16 and returns true; any other width: false, f
// is not called.  A launcher reads KB off its generic lambda's argument (decltype(kb)::value) as a template argument.
template <class F>
bool for_key_width(uint32_t kb, F&& f) {
    switch (kb) {
        case 1: f(Width<1>{}); return true;
        case 2: f(Width<2>{}); return true;
        case 4: f(Width<4>{}); return true;
        case 8: f(Width<8>{}); return true;
        case 16: f(Width<16>{}); return true;
        default: return false;
    }
}
// a value width that the typed kernels of the pairs, segment, merge and set-operation calls move themselves (0: no values)
constexpr bool value_width_fused(uint32_t vb) { return vb == 0 || vb == 1 || vb == 2 || vb == 4 || vb == 8 || vb == 16; }
// The merge and set-operation write kernels, per fused value width (taken as 16 when it is none of the others) and index
// width (0: no index; else 4 or 8): calls f(Width<VB>{}, Width<IB>{}).
template <class F>
void for_value_index_width(uint32_t vb, uint32_t ib, F&& f) {
    auto index = [&](auto v) {
        if (ib == 0) f(v, Width<0>{});
        else if (ib == 4) f(v, Width<4>{});
        else f(v, Width<8>{});
    };
    switch (vb) {
        case 0: index(Width<0>{}); break;
        case 1: index(Width<1>{}); break;
        case 2: index(Width<2>{}); break;
        case 4: index(Width<4>{}); break;
        case 8: index(Width<8>{}); break;
        default: index(Width<16>{}); break;
    }
}
// whether ceil(n / tile) tiles, one workgroup each, fit one launch
constexpr bool tiles_fit(uint64_t n, uint32_t tile) { return (n + tile - 1) / tile < (1ull << 31); }

// separate key and value arrays <-> joined elements (rsx_pairs.hip, rsx_pairs_kernels.hpp); split modes: 0 keys and
// values, 1 keys only, 2 the position alone as ib bytes
int launch_pairs_join(rsx_ctx* ctx, const void* keys, const void* values, void* elems, size_t n, uint32_t kb, uint32_t vb, bool gen,
                      uint32_t kind, uint32_t desc, hipStream_t st);
int launch_pairs_split(rsx_ctx* ctx, const void* elems, void* keys, void* values, size_t n, uint32_t kb, uint32_t vb, uint32_t mode, uint32_t ib,
                       uint32_t kind, uint32_t desc, hipStream_t st);
uint32_t pairs_elem_bytes(uint32_t kb, uint32_t vb);    // joined element size, 0: none (proxy route)
uint32_t pairs_value_offset(uint32_t kb, uint32_t vb);  // of the value in the joined element

// The columns of ONE round of rsx_lexsort_device / rsx_sort_columns_device -> joined (compound key, u32 position) elements
// (rsx_lex.hip, rsx_lex_kernels.hpp).
struct LexJoinCol {
    const void* keys;         // n keys of kb bytes, aligned to kb
    uint32_t kb, kind, desc;
    uint32_t off;             // byte offset of the mapped key inside the compound key
};
struct LexJoinCall {
    LexJoinCol col[RSX_LEX_MAX_COLUMNS];
    uint32_t ncols;
    uint32_t w;               // bytes of the compound key: 1, 2, 4, 8, 16; the element is pairs_elem_bytes(w, 4)
    const void* prev;         // null: the first round; else the previous round's n sorted elements of prev_es bytes,
    uint32_t prev_es;         // whose positions (u32 at prev_voff) say which key of every column slot i takes
    uint32_t prev_voff;
    void* elems;              // out: n elements, 16-byte aligned
    size_t n;                 // 1 .. 2^32 - 1
};
int launch_lex_join(rsx_ctx* ctx, const LexJoinCall& call, hipStream_t st);

// What one rsx_unique_device call asks of the run kernels (rsx_unique.hip, rsx_unique_kernels.hpp) once its joined
// elements are sorted.
struct UniqueCall {
    const void* elems;        // n sorted joined elements: the mapped key alone (pos false) or (mapped key, u32 position)
    uint32_t* tile_heads;     // per tile of unique_tile_elems: its heads, and ...
    uint64_t* tile_base;      // ... the heads in front of it
    size_t n;
    uint32_t kb, kind, desc;
    bool pos;
    uint32_t ib;              // bytes of an index in out_perm / out_inverse
    void* out_keys;           // every output but out_num may be null
    uint64_t* out_offsets;
    void* out_perm;
    void* out_inverse;
    uint64_t* out_num;
};
int launch_unique(rsx_ctx* ctx, const UniqueCall& call, uint32_t* launched, hipStream_t st);
uint32_t unique_tile_elems(uint32_t kb, bool pos);  // elements per workgroup of the count and write kernels
uint32_t unique_scan_span();                        // tiles per sweep of the scan kernel's loop

// What one rsx_reduce_by_key_device call asks of the run kernels (rsx_reduce.hip, rsx_reduce_kernels.hpp) once its
// joined (mapped key, value) elements are sorted.
struct ReduceCall {
    const void* elems;        // n sorted joined elements
    uint32_t* tile_heads;     // per tile of reduce_tile_elems: its heads, ...
    uint64_t* tile_base;      // ... the heads in front of it, ...
    uint64_t* tile_tail;      // ... the value of its elements from its last head on, and ...
    uint64_t* tile_carry;     // ... the value of the open run in front of it
    size_t n;
    uint32_t kb, kind, desc;
    uint32_t vb, vkind, op;
    void* out_keys;           // every output but out_num may be null
    void* out_values;
    uint64_t* out_offsets;
    uint64_t* out_num;
};
int launch_reduce(rsx_ctx* ctx, const ReduceCall& call, uint32_t* launched, hipStream_t st);
uint32_t reduce_tile_elems(uint32_t kb, uint32_t vb);  // elements per workgroup of the count and write kernels
uint32_t reduce_scan_span();                           // tiles per sweep of the scan kernel's loop

// What one rsx_scan_by_key_device call asks of the scan kernels (rsx_scan.hip, rsx_scan_kernels.hpp).
struct ScanCall {
    bool runs;                // RSX_SCAN_RUNS: the keys as they lie; else the sorted elements of the grouped form
    const void* keys;         // runs: the caller's n keys; else n sorted joined (mapped key, u32 position) elements
    const void* values;       // the caller's n values, only read; null: the count form, every value the integer 1
    void* column;             // grouped form with values: the workspace column of n values in sorted order
    uint32_t* tile_heads;     // per tile of scan_tile_elems, with the meaning they have in ReduceCall
    uint64_t* tile_base;
    uint64_t* tile_tail;
    uint64_t* tile_carry;
    size_t n;
    uint32_t kb;
    uint32_t vb, vkind, op;
    bool exclusive;
    uint64_t first;           // its low vb bytes: what the first element of every group receives (exclusive)
    void* out;                // n results of vb bytes by input position; may be `values`
    uint64_t* out_num;        // the number of groups (runs): the caller's word or a workspace word
};
int launch_scan_by_key(rsx_ctx* ctx, const ScanCall& call, uint32_t* launched, hipStream_t st);
uint32_t scan_tile_elems(uint32_t kb, bool runs);  // elements per workgroup of the count and write kernels

// What one rsx_search_sorted_device call asks of the search kernel (rsx_search.hip, rsx_search_kernels.hpp).
struct SearchCall {
    const void* sorted;          // n keys of kb bytes, sorted by mapped key in the call's order
    size_t n;
    const uint64_t* sorted_num;  // null, or one device word: only the first min(n, *sorted_num) keys count
    const void* needles;         // m keys as given (pos false) or m sorted joined (mapped key, u32 position) elements
    size_t m;
    uint32_t kb, kind, desc;
    bool pos;
    uint32_t ib;                 // bytes of an index in out_lower / out_upper
    void* out_lower;             // either may be null
    void* out_upper;
};
int launch_search(rsx_ctx* ctx, const SearchCall& call, uint32_t* launched, hipStream_t st);
uint32_t search_tile_elems(uint32_t kb);     // needles per workgroup
uint32_t search_window_elems(uint32_t kb);  // haystack keys a workgroup stages in LDS at most

// What one rsx_join_device call asks of the join kernels (rsx_search.hip, rsx_join_kernels.hpp).
struct JoinCall {
    uint32_t how;                // RSX_JOIN_*
    const void* a_keys;          // na keys of kb bytes, sorted by mapped key in the call's order; b likewise
    size_t na;                   // 1 .. 2^32 - 1
    const uint64_t* a_num;       // null, or one device word: only the first min(na, *a_num) keys count; b_num likewise
    const void* a_index;         // null, or na words of ib bytes to emit in place of positions in a; b_index likewise
    const void* b_keys;
    size_t nb;                   // 0 .. 2^32 - 1
    const uint64_t* b_num;
    const void* b_index;
    uint32_t kb, kind, desc;
    uint32_t ib;                 // bytes of a word of out_a / out_b / a_index / b_index
    uint32_t* ws_lo;             // per key of a: its lower bound in b (or all ones), ...
    uint64_t* ws_local;          // ... and the rows of the keys in front of it in its count tile
    uint64_t* tile_total;        // per count tile of join_tile_elems: its rows, and ...
    uint64_t* tile_base;         // ... [tiles + 1] those in front of it; the last word is the number of rows
    bool write;                  // false: the count-only form, two launches
    uint64_t write_groups;       // workgroups of the write launch (1 .. 2^31)
    void* out_a;
    void* out_b;                 // null: semi and anti joins
    size_t capacity;             // rows of out_a / out_b
    uint64_t* out_num;           // the number of rows, whatever the capacity
};
int launch_join(rsx_ctx* ctx, const JoinCall& call, uint32_t* launched, hipStream_t st);
uint32_t join_tile_elems();  // keys of a per count workgroup
uint32_t join_rows();        // output rows per write workgroup

// What one rsx_merge_device call asks of the merge kernel (rsx_merge.hip, rsx_merge_kernels.hpp).
struct MergeCall {
    const void* a_keys;          // na keys of kb bytes, sorted by mapped key in the call's order; b likewise
    const void* a_values;        // na values of vb bytes (read only when out_values is given)
    size_t na;
    const void* b_keys;
    const void* b_values;
    size_t nb;
    uint32_t kb, kind, desc;
    uint32_t vb;                 // launch_merge: a fused width (value_width_fused) when out_values is given
    uint32_t ib;                 // bytes of a position in out_index
    void* out_keys;              // each may be null
    void* out_values;
    void* out_index;
};
int launch_merge(rsx_ctx* ctx, const MergeCall& call, uint32_t* launched, hipStream_t st);
// the values of any other width: out_values row r = row pos[r] of a_values ++ b_values; out_index (or null) receives pos
int launch_merge_gather(rsx_ctx* ctx, const MergeCall& call, const uint64_t* pos, void* out_values, void* out_index, hipStream_t st);
uint32_t merge_tile_elems(uint32_t kb, uint32_t vb);  // outputs per workgroup

// What one rsx_setop_device call asks of the set-operation kernel (rsx_setops.hip, rsx_setop_kernels.hpp).
struct SetopCall {
    const void* a_keys;          // na keys of kb bytes, sorted by mapped key in the call's order; b likewise
    const void* a_values;        // na values of vb bytes (read only when out_values is given)
    size_t na;
    const uint64_t* a_num;       // null, or one device word: only the first min(na, *a_num) keys count; b_num likewise
    const void* b_keys;
    const void* b_values;        // may be null when the operation never emits from b
    size_t nb;
    const uint64_t* b_num;
    uint32_t op;                 // RSX_SETOP_*
    uint32_t kb, kind, desc;
    uint32_t vb;                 // a fused width (value_width_fused)
    uint32_t ib;                 // bytes of a position in out_index
    uint32_t* tile_count;        // per tile of setop_tile_elems: its kept elements, ...
    uint64_t* tile_base;         // ... those in front of it, and ...
    uint64_t* tile_save;         // ... setop_save_words() words the count launch leaves for the write launch
    uint64_t* raw_num;           // one word: the scan's sum
    size_t cap;                  // rows of every output
    void* out_keys;              // each may be null
    void* out_values;
    void* out_index;
    uint64_t* out_num;           // min(the scan's sum, cap)
};
int launch_setop(rsx_ctx* ctx, const SetopCall& call, uint32_t* launched, hipStream_t st);
uint32_t setop_tile_elems(uint32_t kb);  // merge positions per workgroup
uint32_t setop_save_words();
// rsx_unique_scan_kernel over another call's per-tile counts (rsx_unique.hip): tile_base[t] and their sum -> out_num[0]
void launch_run_scan(const uint32_t* tile_count, uint64_t* tile_base, uint64_t tiles, uint64_t* out_num, hipStream_t st);

// What one rsx_compact_device call asks of the compaction kernels (rsx_unique.hip, rsx_compact_kernels.hpp).
struct CompactCall {
    const void* keys;            // n keys of kb bytes; null (kb 0) when the call neither compares nor emits keys
    const uint8_t* flags;        // null, or n flag bytes
    const void* lo;              // null, or one key on the device: the bounds of the key range
    const void* hi;
    const void* values;          // n values of vb bytes (read only when out_values is given)
    size_t n;                    // 1 .. 2^32 - 1
    const uint64_t* num;         // null, or one device word: only the first min(n, *num) rows count
    uint32_t kb, kind, desc;
    uint32_t vb;                 // 0, or a fused width (value_width_fused): what the write kernel moves itself
    uint32_t ib;                 // bytes of a position in out_index
    uint32_t mode;               // RSX_COMPACT_* bits
    uint32_t* tile_count;        // per tile of compact_tile_elems: its kept rows, and ...
    uint64_t* tile_base;         // ... those in front of it
    void* out_keys;              // each may be null
    void* out_values;
    void* out_index;
    uint64_t* out_num;           // the number of kept rows
};
int launch_compact(rsx_ctx* ctx, const CompactCall& call, uint32_t* launched, hipStream_t st);
// out_values row r = row pos[r] (pb bytes each) of `values`, rows of vb bytes, for the rows the call wrote
int launch_compact_gather(rsx_ctx* ctx, const CompactCall& call, const void* pos, uint32_t pb, uint32_t vb, void* out_values, hipStream_t st);
uint32_t compact_tile_elems(uint32_t kb, uint32_t vb);  // rows per workgroup of the count and write kernels

}  // namespace rsxh
