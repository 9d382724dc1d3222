// rsx_launch_impl.hpp -- definitions of the per-element-size launchers behind EsLaunchers
// (rsx_internal.hpp).  Included only by rsx_es.hip, which instantiates them for ONE element size.
#pragma once
#include <cstdlib>
#include "rsx_internal.hpp"
#include "rsx_small_kernel.hpp"
#include "rsx_mid_kernels.hpp"
#include "rsx_segment_kernels.hpp"
#include "rsx_segment_pairs_kernels.hpp"
#include "rsx_topk_kernels.hpp"

#ifndef RSX_HIST_BLOCKS_PER_CU
#define RSX_HIST_BLOCKS_PER_CU 8
#endif

namespace rsxh {

inline uint32_t rank_atomic_of(const rsx_ctx* ctx) { return (ctx->rank_atomic && !(ctx->options & OPT_BALLOT_RANKS)) ? 1u : 0u; }
constexpr CleanList CLEAN_NONE = {{nullptr, nullptr, nullptr}, {0, 0, 0}};

// ---- count phase of a first pass: J[r][v] for `digit` over the input regions ------------------
// the count kernels' grid: workgroups per region, each region cut into blocks of 512 x 16 elements
inline uint64_t hist_blocks_per_region(const rsx_ctx* ctx, const RegionGeom& g) {
    const uint64_t per_block = 512ull * 16;
    uint64_t bpr = ((1ull << g.region_shift) + per_block - 1) / per_block;
    const uint64_t cap = ((uint64_t)ctx->num_cu * RSX_HIST_BLOCKS_PER_CU + g.num_regions - 1) / g.num_regions;
    if (bpr > cap) bpr = cap;
    return bpr == 0 ? 1 : bpr;
}
template <int ES, bool FLT>
int launch_hist_t(rsx_ctx* ctx, SortRun& run, const void* src, const RegionGeom& g, const rsx_layout* L, uint32_t digit,
                  unsigned long long* J, unsigned long long* jclear, bool clear_status, hipStream_t st) {
    // the status words of the sweep that follows (its first half of the workspace) are zeroed by this kernel
    const uint64_t zero16_n = clear_status ? status_rows(g) * RADIX * (status32(g) ? 4u : 8u) / 16u : 0u;
    const uint64_t bpr = hist_blocks_per_region(ctx, g);
    LaunchTimer lt(ctx, RSX_PROF_HIST, st);
    hipLaunchKernelGGL((rsx_hist_kernel<ES, FLT>), dim3((uint32_t)(bpr * g.num_regions)), dim3(512), 0, st,
                       static_cast<const Elem<ES>*>(src), g, make_spec(L, digit), (uint32_t)bpr, J, jclear, status32(g) ? 1u : 0u,
                       static_cast<uint4*>(ctx->status), zero16_n, run.clean, run.gate, DigitSpec{}, nullptr, run.spec_dev);
    RSX_HIP(hipGetLastError());
    run.clean = CLEAN_NONE;  // done once per sort
    return RSX_OK;
}
template <int ES>
int launch_hist(rsx_ctx* ctx, SortRun& run, const void* src, const RegionGeom& g, const rsx_layout* L, uint32_t digit,
                unsigned long long* J, unsigned long long* jclear, bool clear_status, hipStream_t st) {
    if (L->key_kind == RSX_KEY_FLOAT || (L->key_kind == RSX_KEY_SIGNED && (digit + 1 == L->key_bytes || run.spec_dev != nullptr)))
        return launch_hist_t<ES, true>(ctx, run, src, g, L, digit, J, jclear, clear_status, st);
    return launch_hist_t<ES, false>(ctx, run, src, g, L, digit, J, jclear, clear_status, st);
}

template <int ES>
int launch_hist2(rsx_ctx* ctx, SortRun& run, const void* src, const RegionGeom& g, const rsx_layout* L, uint32_t digit,
                 unsigned long long* J, uint32_t digit2, unsigned long long* J2, unsigned long long* jclear, hipStream_t st) {
    const uint64_t zero16_n = status_rows(g) * RADIX * (status32(g) ? 4u : 8u) / 16u;
    const uint64_t bpr = hist_blocks_per_region(ctx, g);
    LaunchTimer lt(ctx, RSX_PROF_HIST, st);
    // one instantiation per key kind class: the general digit map is the identity for unsigned keys' specs
    if (L->key_kind != RSX_KEY_UNSIGNED)
        hipLaunchKernelGGL((rsx_hist_kernel<ES, true, true>), dim3((uint32_t)(bpr * g.num_regions)), dim3(512), 0, st,
                           static_cast<const Elem<ES>*>(src), g, make_spec(L, digit), (uint32_t)bpr, J, jclear, status32(g) ? 1u : 0u,
                           static_cast<uint4*>(ctx->status), zero16_n, run.clean, run.gate, make_spec(L, digit2), J2);
    else
        hipLaunchKernelGGL((rsx_hist_kernel<ES, false, true>), dim3((uint32_t)(bpr * g.num_regions)), dim3(512), 0, st,
                           static_cast<const Elem<ES>*>(src), g, make_spec(L, digit), (uint32_t)bpr, J, jclear, status32(g) ? 1u : 0u,
                           static_cast<uint4*>(ctx->status), zero16_n, run.clean, run.gate, make_spec(L, digit2), J2);
    RSX_HIP(hipGetLastError());
    run.clean = CLEAN_NONE;
    return RSX_OK;
}

// ---- scatter phase: one sweep pass -------------------------------------------------------------
// the per-dword masks of the signed/float key map (KeyXform in rsx_device.hpp)
inline KeyXform make_xform(const rsx_layout* L) {
    KeyXform x;
    std::memset(&x, 0, sizeof x);
    if (L->key_kind == RSX_KEY_UNSIGNED) return x;
    const uint32_t top = L->key_offset + L->key_bytes - 1;
    auto word_of = [&](uint32_t byte) { return L->elem_bytes >= 4 ? byte >> 2 : 0u; };
    auto bit_of = [&](uint32_t byte) { return L->elem_bytes >= 4 ? 8 * (byte & 3) : 8 * byte; };
    const uint32_t sw = word_of(top);
    const uint32_t sbit = 1u << (bit_of(top) + 7);
    x.sign[sw] = sbit;
    x.xpos[sw] = sbit;
    if (L->key_kind == RSX_KEY_SIGNED) {
        x.xneg[sw] = sbit;
    } else {
        for (uint32_t b = L->key_offset; b <= top; ++b) x.xneg[word_of(b)] |= 0xFFu << bit_of(b);
    }
    return x;
}

// KPT: keys per thread of the tile; the geometry has to be one of that tile size (every sweep at kpt_for(ES) but the
// hybrid's second, at hyb_kpt_for(ES): launch_sweep_n).  The dynamic LDS size and the occupancy cached with it follow it.
template <int ES, typename S, int XF, bool NEXT, bool MID = false, bool STR = false, int KPT = kpt_for(ES)>
int launch_sweep_t(rsx_ctx* ctx, const SortRun& run, const SweepPass& pass, const void* src, void* dst, const RegionGeom& g, const rsx_layout* L,
                   uint32_t digit, const unsigned long long* J, unsigned long long* jnext, unsigned long long* jzero,
                   hipStream_t st) {
    static_assert(KPT == kpt_for(ES) || (STR && !NEXT && !MID), "only the hybrid's sweep that counts nothing has room for a deeper tile");
    if (g.tile != (uint32_t)(wg_for(ES) * KPT)) return fail(ctx, RSX_ERR_INTERNAL, "launch_sweep: geometry of another tile size");
    constexpr int SWEEP_WG = wg_for(ES);
    constexpr int TILE = SWEEP_WG * KPT;
    // Status words alternate between the two halves of the workspace.  The first half is zeroed by the
    // count kernel that precedes the first sweep; every pass zeroes, tile by tile, the half of the next.
    char* const half[2] = {static_cast<char*>(ctx->status), static_cast<char*>(ctx->status) + ctx->status_bytes};
    const uint32_t which = pass.index & 1u;
    SweepArgs a;
    a.status_clean = pass.last ? nullptr : half[which ^ 1u];
    a.src = src;
    a.dst = dst;
    a.g = g;
    a.J = J;
    a.status = half[which];
    a.tickets = run.tickets_override ? run.tickets_override : tickets_of(ctx, run, pass.index);
    a.prev_mode = pass.index ? tickets_of(ctx, run, pass.index - 1) + ROLL_SHARDS + 1 : nullptr;
    a.jnext = jnext;
    a.jzero = jzero;
    a.error = ctx->host_err_dev;
    a.spec = make_spec(L, digit);
    a.next = make_spec(L, NEXT ? digit + 1 : digit);
    a.spec.flip = a.next.flip = 0;  // the sweep sees mapped keys: plain digits
    a.xf = make_xform(L);
    a.tiles_per_region = (uint32_t)tiles_per_region(g);
    a.opts = ((ctx->options & OPT_DYNAMIC_TILES) ? SWEEP_OPT_DYNAMIC : 0u) |
             ((ctx->options & OPT_NO_XCD_MAJOR) ? SWEEP_OPT_NO_XCD_MAJOR : 0u) |
             ((ctx->options & OPT_AGENT_STATUS) || !ctx->l2_local ? SWEEP_OPT_AGENT_STATUS : 0u) |
             ((ctx->options & OPT_RANK_CHECK) ? SWEEP_OPT_RANK_CHECK : 0u) |
             ((uint64_t)g.n * ES <= (2ull << 30) ? SWEEP_OPT_PREREAD : 0u);  // measured: a gain up to 2 GiB of data, a loss at 4 GiB
    a.dbg = ctx->dbg;
    a.mid_J = nullptr;
    a.mid_spec = a.spec;
    a.mid_cap = 0;
    a.gate = run.gate;
    a.spec_dev = run.spec_dev;
    a.mid_mode = pass.mid;
    a.mid_hint = ctx->host_err_dev + HV_MID_HINT;
    if constexpr (MID) {
        a.mid_J = JT_of(ctx, run);
        a.mid_spec = make_spec(L, L->key_bytes - 1);
        a.mid_spec.flip = 0;
        a.mid_cap = bucket_cap(ES);
    }
    a.rank_atomic = rank_atomic_of(ctx);
    a.hot_lanes = (ctx->options & OPT_ATOMIC_RANKS) ? 65u : ctx->hot_lanes;
    a.dbg_cnt = reinterpret_cast<unsigned long long*>(ctx->aux + OFF_DBG);
    const size_t lds = (size_t)TILE * ES + (SWEEP_WG / WAVE) * RADIX * (sweep_wide_cnt(ES, KPT, SWEEP_WG) ? sizeof(uint32_t) : sizeof(uint16_t)) +
                       (NEXT ? (size_t)g.num_regions * RADIX * sizeof(uint32_t) : 0) + 128;
    auto kern = rsx_sweep_kernel<ES, KPT, SWEEP_WG, S, XF, NEXT, MID, STR>;
    // resident workgroups per CU for this kernel at this LDS size (the count matrix of the next pass
    // makes the LDS size depend on the number of regions): cached per instantiation and thread
    thread_local size_t occ_lds = ~(size_t)0;
    thread_local int occ = 0;
    if (occ == 0 || occ_lds != lds) {
        int o = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, kern, SWEEP_WG, lds) != hipSuccess || o < 1) o = 2;
        occ = o;
        occ_lds = lds;
    }
    // persistent workgroups; correctness does not need them co-resident (a workgroup only
    // ever waits for tiles whose tickets were drawn earlier, by workgroups already running)
    // tiles of region r: every region ends with a tile of its own (partial unless the region length is a multiple
    // of the tile), so the total is NOT ceil(n / TILE)
    const uint32_t NR = g.num_regions;
    const uint64_t region_len = 1ull << g.region_shift;
    auto tiles_of = [&](uint32_t r) -> uint64_t {
        const uint64_t beg = (uint64_t)r << g.region_shift;
        const uint64_t len = g.n - beg < region_len ? g.n - beg : region_len;
        return (len + TILE - 1) / TILE;
    };
    uint64_t real_tiles = 0;
    for (uint32_t r = 0; r < NR; ++r) real_tiles += tiles_of(r);
    uint64_t grid = (uint64_t)ctx->num_cu * occ;
    if (grid > real_tiles) grid = real_tiles;
    if (grid < NR) grid = NR;
#ifdef RSX_TUNING
    if (const char* o = std::getenv("RSX_OCC")) {
        const long v = std::atol(o);
        if (v >= 1 && v <= 8) grid = (uint64_t)ctx->num_cu * (uint64_t)v;
    }
#endif
    if (grid > 0xFFFFu) grid = 0xFFFFu;  // wg_first entries are 16 bit
    {   // static mode: workgroups per region, proportional to the region's tile count, >= 1 each
        uint64_t cum = 0;
        for (uint32_t r = 0; r < NR; ++r) {
            a.wg_first[r] = (uint16_t)(cum * grid / real_tiles);
            cum += tiles_of(r);
        }
        a.wg_first[NR] = (uint16_t)grid;
        for (uint32_t r = 0; r < NR; ++r)  // at least one workgroup per region
            if (a.wg_first[r + 1] <= a.wg_first[r]) a.wg_first[r + 1] = a.wg_first[r] + 1;
        for (uint32_t r = NR; r-- > 0;) {
            const uint32_t cap = (uint32_t)grid - (NR - r);
            if (a.wg_first[r] > cap) a.wg_first[r] = (uint16_t)cap;
        }
        a.wg_first[NR] = (uint16_t)grid;
        for (uint32_t r = NR + 1; r <= (uint32_t)MAX_REGIONS; ++r) a.wg_first[r] = (uint16_t)grid;
        // regions whose workgroups fall into one class of the kernel's XCD-major numbering
        // (class = index / (grid/8) = blockIdx % 8): candidates for L2-local status words
        a.local_mask = 0;
        if (grid % 8 == 0 && !(ctx->options & OPT_NO_XCD_MAJOR))
            for (uint32_t r = 0; r < NR; ++r)
                if (a.wg_first[r] / (grid / 8) == (a.wg_first[r + 1] - 1u) / (grid / 8)) a.local_mask |= 1u << r;
    }
    if (ctx->options & OPT_VERBOSE) std::fprintf(stderr, "[rsx] sweep ES=%d NEXT=%d occ=%d grid=%llu lds=%zu tiles=%llu regions=%u\n", ES, (int)NEXT, occ, (unsigned long long)grid, lds, (unsigned long long)real_tiles, g.num_regions);
    LaunchTimer lt(ctx, RSX_PROF_SWEEP, st);
    hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(SWEEP_WG), lds, st, a);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}

template <int ES, typename S, int XF>
int launch_sweep_n(rsx_ctx* ctx, const SortRun& run, const SweepPass& pass, const void* src, void* dst, const RegionGeom& g, const rsx_layout* L,
                   uint32_t digit, const unsigned long long* J, unsigned long long* jnext, unsigned long long* jzero,
                   hipStream_t st) {
    if (run.spec_dev != nullptr) {  // the hybrid's two sweeps: window digits at any bit offset (the STR instantiation)
        if constexpr (ES >= 8 && (XF & 2) == 0) {
            if (jnext) return launch_sweep_t<ES, S, XF, true, false, true>(ctx, run, pass, src, dst, g, L, digit, J, jnext, jzero, st);
            if constexpr (XF == 0) {  // the second sweep: a geometry of the deeper tile (hyb_geom) picks the deeper kernel
                if constexpr (hyb_kpt_for(ES) != kpt_for(ES)) {
                    if (g.tile == (uint32_t)(wg_for(ES) * hyb_kpt_for(ES)))
                        return launch_sweep_t<ES, S, 0, false, false, true, hyb_kpt_for(ES)>(ctx, run, pass, src, dst, g, L, digit, J, nullptr, jzero, st);
                }
                return launch_sweep_t<ES, S, 0, false, false, true>(ctx, run, pass, src, dst, g, L, digit, J, nullptr, jzero, st);
            }
        }
        return fail(ctx, RSX_ERR_INTERNAL, "launch_sweep: no kernel for this pass of the hybrid");
    }
    if constexpr ((XF & 2) == 0) {  // a pass that maps the keys back is a last pass: nothing to count for
        if constexpr (sizeof(S) == 4 && ES != 1) {  // the first sweep of a middle-size sort (regions of <= 2^30 elements by far)
            if (jnext && pass.mid != 0) return launch_sweep_t<ES, S, XF, true, true>(ctx, run, pass, src, dst, g, L, digit, J, jnext, jzero, st);
        }
        if (jnext) return launch_sweep_t<ES, S, XF, true>(ctx, run, pass, src, dst, g, L, digit, J, jnext, jzero, st);
    } else if (jnext) {
        return fail(ctx, RSX_ERR_ARG, "a last pass cannot count for a next one");
    }
    return launch_sweep_t<ES, S, XF, false>(ctx, run, pass, src, dst, g, L, digit, J, nullptr, jzero, st);
}

template <int ES, typename S>
int launch_sweep_x(rsx_ctx* ctx, const SortRun& run, const SweepPass& pass, const void* src, void* dst, const RegionGeom& g, const rsx_layout* L,
                   uint32_t digit, const unsigned long long* J, unsigned long long* jnext, unsigned long long* jzero,
                   int xf, hipStream_t st) {
    switch (L->key_kind == RSX_KEY_UNSIGNED ? 0 : xf) {
        case 1: return launch_sweep_n<ES, S, 1>(ctx, run, pass, src, dst, g, L, digit, J, jnext, jzero, st);
        case 2: return launch_sweep_n<ES, S, 2>(ctx, run, pass, src, dst, g, L, digit, J, jnext, jzero, st);
        case 3: return launch_sweep_n<ES, S, 3>(ctx, run, pass, src, dst, g, L, digit, J, jnext, jzero, st);
        default: return launch_sweep_n<ES, S, 0>(ctx, run, pass, src, dst, g, L, digit, J, jnext, jzero, st);
    }
}

template <int ES>
int launch_sweep(rsx_ctx* ctx, const SortRun& run, const SweepPass& pass, const void* src, void* dst, const RegionGeom& g, const rsx_layout* L,
                 uint32_t digit, const unsigned long long* J, unsigned long long* jnext, unsigned long long* jzero, int xf, hipStream_t st) {
    if (status32(g)) return launch_sweep_x<ES, uint32_t>(ctx, run, pass, src, dst, g, L, digit, J, jnext, jzero, xf, st);
    return launch_sweep_x<ES, uint64_t>(ctx, run, pass, src, dst, g, L, digit, J, jnext, jzero, xf, st);
}

// ---- sorts of one workgroup in LDS (rsx_small_kernel.hpp) ------------------------------------------
// What their SmallArgs share: `passes` digits to sort by, the digits `nspec` of them are described for, and whether the
// keys arrive raw (map_load) or mapped by an earlier sweep.  The bucket kernels start their LDS passes at the digit their
// bucket's size allows (RSX_OPT_BUCKET_SKIP, first_digit_for) and compare neighbours on the key bytes from there up: they
// build their compare masks from key_offset / key_bytes.
inline SmallArgs small_args(const rsx_ctx* ctx, const rsx_layout* L, uint32_t passes, uint32_t nspec, bool map_load) {
    SmallArgs a;
    std::memset(&a, 0, sizeof a);
    a.passes = passes;
    a.rank_atomic = rank_atomic_of(ctx);
    a.map_store = L->key_kind == RSX_KEY_UNSIGNED ? 0u : 1u;
    a.map_load = map_load ? a.map_store : 0u;
    for (uint32_t d = 0; d < nspec; ++d) {
        a.spec[d] = make_spec(L, d);
        a.spec[d].flip = 0;  // the kernel sees mapped keys: plain digits
    }
    a.xf = make_xform(L);
    a.no_skip = ctx->bucket_no_skip;
    a.key_offset = L->key_offset;
    a.key_bytes = L->key_bytes;
    return a;
}

// ---- arrays of at most one tile: all passes in one launch of one workgroup ----------------------
template <int ES>
int launch_small_sort(rsx_ctx* ctx, void* data, size_t n, const rsx_layout* L, hipStream_t st) {
    constexpr int KPT = kpt_for(ES);
    if (n == 0 || n > (size_t)512 * KPT || L->key_bytes > 16) return fail(ctx, RSX_ERR_INTERNAL, "launch_small_sort: size out of range");
    SmallArgs a = small_args(ctx, L, L->key_bytes, L->key_bytes, true);
    a.src = data;
    a.data = data;
    a.n = (uint32_t)n;
    const size_t lds = (size_t)512 * KPT * ES + 8 * RADIX * sizeof(uint32_t) + 64;
    auto kern = rsx_small_sort_kernel<ES, KPT>;
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    hipLaunchKernelGGL(kern, dim3(1), dim3(512), lds, st, a);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}

// ---- middle-size sorts: split by the top digit (count -> scan -> scatter, one launch each) --------
inline uint32_t* mid_totals_of(rsx_ctx* ctx) { return reinterpret_cast<uint32_t*>(ctx->aux + OFF_BASE); }
template <int ES>
int launch_mid_split(rsx_ctx* ctx, const void* src, void* dst, size_t n, const rsx_layout* L, hipStream_t st) {
    if constexpr (ES == 1) {
        return fail(ctx, RSX_ERR_INTERNAL, "launch_mid_split: one-byte elements");
    } else {
        constexpr int KPT = mid_kpt_for(ES);
        constexpr uint32_t TILE = 512u * KPT;
        MidArgs a;
        std::memset(&a, 0, sizeof a);
        a.src = src;
        a.dst = dst;
        a.n = (uint32_t)n;
        a.tiles = (uint32_t)((n + TILE - 1) / TILE);
        if ((size_t)a.tiles * RADIX * sizeof(uint32_t) > ctx->status_bytes) return fail(ctx, RSX_ERR_INTERNAL, "launch_mid_split: workspace");
        a.C = static_cast<uint32_t*>(ctx->status);
        a.X = reinterpret_cast<uint32_t*>(static_cast<char*>(ctx->status) + ctx->status_bytes);
        a.T = mid_totals_of(ctx);
        a.spec = make_spec(L, L->key_bytes - 1);  // count: the raw key's top byte through the digit map
        a.xf = make_xform(L);
        a.map_keys = L->key_kind == RSX_KEY_UNSIGNED ? 0u : 1u;
        a.rank_atomic = rank_atomic_of(ctx);
        {
            LaunchTimer lt(ctx, RSX_PROF_HIST, st);
            if (L->key_kind != RSX_KEY_UNSIGNED) hipLaunchKernelGGL((rsx_tilecount_kernel<ES, KPT, true>), dim3(a.tiles), dim3(512), 0, st, a);
            else hipLaunchKernelGGL((rsx_tilecount_kernel<ES, KPT, false>), dim3(a.tiles), dim3(512), 0, st, a);
            RSX_HIP(hipGetLastError());
        }
        {
            LaunchTimer lt(ctx, RSX_PROF_SCAN, st);
            hipLaunchKernelGGL(rsx_tilescan_kernel<ES>, dim3(RADIX), dim3(256), 0, st, a);
            RSX_HIP(hipGetLastError());
        }
        a.spec.flip = 0;  // scatter: the keys are mapped on load, plain digits from there on
        const size_t lds = (size_t)TILE * ES + 8 * RADIX * sizeof(uint32_t) + 64 + 2 * RADIX * sizeof(uint32_t);
        LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
        hipLaunchKernelGGL((rsx_tilescatter_kernel<ES, KPT>), dim3(a.tiles), dim3(512), lds, st, a);
        RSX_HIP(hipGetLastError());
        return RSX_OK;
    }
}

// ---- ... then the 256 buckets, each sorted by one workgroup --------------------------------------
template <int ES>
int launch_bucket_sort(rsx_ctx* ctx, const void* src, void* dst, const rsx_layout* L, bool small, hipStream_t st) {
    if constexpr (ES == 1) {
        return fail(ctx, RSX_ERR_INTERNAL, "launch_bucket_sort: one-byte elements");
    } else {
        constexpr int KPT = bucket_kpt_for(ES);
        if (L->key_bytes < 2 || L->key_bytes > 16) return fail(ctx, RSX_ERR_INTERNAL, "launch_bucket_sort: key width out of range");
        SmallArgs a = small_args(ctx, L, L->key_bytes - 1, L->key_bytes - 1, false);  // (the split mapped the keys)
        a.src = src;
        a.data = dst;
        a.top_tot = mid_totals_of(ctx);
        a.cap = bucket_cap(ES);
        a.hint = ctx->host_err_dev + HV_MID_HINT;
        LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
        if (small) {  // small buckets, all known to fit: 256 threads each
            constexpr size_t lds = LdsTile<ES, KPT, 256>::bytes();
            hipLaunchKernelGGL((rsx_bucket_sort_kernel<ES, KPT, 256>), dim3(RADIX), dim3(256), lds, st, a);
        } else {
            constexpr size_t lds = LdsTile<ES, KPT, 1024>::bytes();
            auto kern = rsx_bucket_sort_kernel<ES, KPT, 1024>;
            ensure_lds(ctx, reinterpret_cast<const void*>(kern), lds);
            hipLaunchKernelGGL(kern, dim3(RADIX), dim3(1024), lds, st, a);
        }
        RSX_HIP(hipGetLastError());
        return RSX_OK;
    }
}

// ---- wide keys, large arrays: count of the top 16 bits; the buckets sorted in LDS -------------------
// the hybrid's plan: which 16 bits of the mapped key the array is partitioned by (rsx_wideplan_kernel)
template <int ES>
int launch_wideplan(rsx_ctx* ctx, const void* src, size_t n, const rsx_layout* L, WidePlan* plan, hipStream_t st) {
    if constexpr (ES < 4) {
        return fail(ctx, RSX_ERR_INTERNAL, "launch_wideplan: narrow elements");
    } else {
        LaunchTimer lt(ctx, RSX_PROF_SCAN, st);
        if (L->key_kind != RSX_KEY_UNSIGNED)
            hipLaunchKernelGGL((rsx_wideplan_kernel<ES, true>), dim3(WIDEPLAN_BLOCKS), dim3(1024), 0, st, static_cast<const Elem<ES>*>(src), (uint64_t)n, L->key_offset,
                               L->key_bytes, L->key_kind, make_xform(L), plan);
        else
            hipLaunchKernelGGL((rsx_wideplan_kernel<ES, false>), dim3(WIDEPLAN_BLOCKS), dim3(1024), 0, st, static_cast<const Elem<ES>*>(src), (uint64_t)n, L->key_offset,
                               L->key_bytes, L->key_kind, make_xform(L), plan);
        RSX_HIP(hipGetLastError());
        return RSX_OK;
    }
}

template <int ES>
int launch_count16top(rsx_ctx* ctx, const void* src, size_t n, const rsx_layout* L, WidePlan* plan, uint32_t* P, uint32_t parts,
                      uint32_t region_shift, uint32_t k, hipStream_t st) {
    if constexpr (ES < 4) {
        return fail(ctx, RSX_ERR_INTERNAL, "launch_count16top: narrow elements");
    } else {
        LaunchTimer lt(ctx, RSX_PROF_HIST, st);
        if (L->key_kind != RSX_KEY_UNSIGNED) {
            auto kern = rsx_count16top_kernel<ES, true>;
            ensure_lds(ctx, reinterpret_cast<const void*>(kern), 131072);
            hipLaunchKernelGGL(kern, dim3(parts), dim3(1024), 131072, st, static_cast<const Elem<ES>*>(src), (uint64_t)n, plan, make_xform(L), P,
                               ctx->ovf16, region_shift, k);
        } else {
            auto kern = rsx_count16top_kernel<ES, false>;
            ensure_lds(ctx, reinterpret_cast<const void*>(kern), 131072);
            hipLaunchKernelGGL(kern, dim3(parts), dim3(1024), 131072, st, static_cast<const Elem<ES>*>(src), (uint64_t)n, plan, make_xform(L), P,
                               ctx->ovf16, region_shift, k);
        }
        RSX_HIP(hipGetLastError());
        return RSX_OK;
    }
}

// the first sweep's count matrix from the counters of launch_count16top (k chunks per region), + the side jobs of launch_hist
template <int ES>
int launch_marginal16(rsx_ctx* ctx, SortRun& run, const uint32_t* P, uint32_t parts, uint32_t k, const RegionGeom& g, unsigned long long* J,
                      unsigned long long* jclear, hipStream_t st) {
    const uint64_t zero16_n = status_rows(g) * RADIX * (status32(g) ? 4u : 8u) / 16u;
    uint32_t grid = (uint32_t)ctx->num_cu * 8u;
    if (grid < parts) grid = parts;
    LaunchTimer lt(ctx, RSX_PROF_HIST, st);
    hipLaunchKernelGGL(rsx_marginal16_kernel<ES>, dim3(grid), dim3(256), 0, st, P, parts, k, g, J, jclear, status32(g) ? 1u : 0u,
                       static_cast<uint4*>(ctx->status), zero16_n, run.clean, run.gate);
    RSX_HIP(hipGetLastError());
    run.clean = CLEAN_NONE;
    return RSX_OK;
}

template <int ES>
int launch_bucket16(rsx_ctx* ctx, const SortRun& run, void* data, void* scratch, size_t n, const rsx_layout* L, const uint64_t* starts,
                    const WidePlan* plan, hipStream_t st) {
    if constexpr (ES < 4) {
        return fail(ctx, RSX_ERR_INTERNAL, "launch_bucket16: narrow elements");
    } else {
        constexpr int KPT = bucket_kpt_for(ES);
        if (L->key_bytes < 4) return fail(ctx, RSX_ERR_INTERNAL, "launch_bucket16: key width out of range");
        // passes: what the sort THROUGH MEMORY of an oversized bucket runs: an even number, every digit the LDS passes could
        // need; the LDS passes themselves follow the device's plan.  The first sweep mapped the keys.
        SmallArgs a = small_args(ctx, L, L->key_bytes - 2, L->key_bytes, false);
        a.src = data;
        a.data = data;
        a.cap = bucket_cap(ES);
        LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
        // Every form the device's verdict can name is enqueued behind its own gate (rsx_scan16_kernel picks the smallest
        // workgroup that holds all but a handful of THIS input's buckets; a form whose workgroup cannot even hold the
        // average bucket is not enqueued): 256, 512 or 1024 threads x KPT elements, as many workgroups per CU as LDS and
        // registers allow (3, 2, 1); small buckets in groups of 2^gs, about 3/4 of what a 512-thread workgroup holds,
        // sorted by all digits up to the window's top (keys of at least 8 bytes).
        const uint64_t avg = (uint64_t)n / 65536u;
        const uint32_t gs = group_shift(ctx, n, L);
        const Gate base = run.gate;  // (null word: no gates -- never the case for this kernel)
        // Key-only elements (the key is the whole element: equal elements are the same bytes, no order among them shows):
        // rsx_bucket16_direct_kernel of the same form runs ahead of every plain form, behind the same gate, and the old
        // kernel takes what it leaves (done, left: ctx->wide_buf).  Elements with a payload need the stable passes.
        // (Its 2^(B+1) 16-bit counters are the halves of the words where the old kernel keeps its wave counters: the same `lds`.)
        bool direct = false;
        // Not where groups of small buckets are on offer (arrays up to about 2^26 u64 keys: uniform keys take the groups, and
        // every plain form's direct kernel would be one more launch that returns at once, 4-5 us each: 2^23 u64 +2.5 %).
        if constexpr (ES == 8 || ES == 16)
            direct = ctx->bucket_direct != 0 && gs == 0 && L->key_offset == 0 && L->key_bytes == (uint32_t)ES && ctx->wide_buf != nullptr;
        unsigned char* done = direct ? reinterpret_cast<unsigned char*>(ctx->wide_buf + WIDE_DONE_OFFSET) : nullptr;
        uint32_t* left = direct ? reinterpret_cast<uint32_t*>(ctx->wide_buf + WIDE_LEFT_OFFSET) : nullptr;
        ctx->last_direct = direct ? 1u : 0u;
        auto go = [&](auto wgc, auto kc, uint32_t form, uint32_t group_shift) {
            constexpr int WGS = decltype(wgc)::value;
            constexpr int K = decltype(kc)::value;
            SmallArgs b = a;
            b.group_shift = group_shift;
            if (group_shift) b.passes = L->key_bytes;
            constexpr size_t lds = LdsTile<ES, K, WGS>::bytes();
            auto kern = rsx_bucket16_kernel<ES, K, WGS>;
            ensure_lds(ctx, reinterpret_cast<const void*>(kern), lds);
            int per_cu = (int)(LDS_PER_CU / lds);
            if (per_cu < 1) per_cu = 1;
            if (per_cu > 4 * RSX_B16_WAVES(WGS) * 64 / WGS) per_cu = 4 * RSX_B16_WAVES(WGS) * 64 / WGS;
            const Gate g{base.word, VERDICT_PATH_MASK | VERDICT_FORM_MASK, VERDICT_HYBRID | form};
            const bool ahead = direct && group_shift == 0;  // (direct: no groups are enqueued)
            if constexpr (ES == 8 || ES == 16) {
                if (ahead) {
                    auto dkern = rsx_bucket16_direct_kernel<ES, K, WGS>;
                    ensure_lds(ctx, reinterpret_cast<const void*>(dkern), lds);
                    hipLaunchKernelGGL(dkern, dim3((uint32_t)(ctx->num_cu * per_cu)), dim3(WGS), lds, st, b, starts, plan, done, left, g);
                }
            }
            hipLaunchKernelGGL(kern, dim3((uint32_t)(ctx->num_cu * per_cu)), dim3(WGS), lds, st, b, starts, scratch, plan, g,
                               ahead ? static_cast<const unsigned char*>(done) : nullptr, ahead ? static_cast<const uint32_t*>(left) : nullptr);
        };
        using std::integral_constant;
        constexpr int KBIG = wide_kpt_for(ES);  // (the longer form only where the average bucket needs it: wide_big_form)
        if (gs >= 2) go(integral_constant<int, 512>{}, integral_constant<int, KPT>{}, VERDICT_GROUPS, gs);
        if (avg <= (uint64_t)256 * KPT) go(integral_constant<int, 256>{}, integral_constant<int, KPT>{}, VERDICT_WG256, 0);
        if (avg <= (uint64_t)512 * KPT) go(integral_constant<int, 512>{}, integral_constant<int, KPT>{}, VERDICT_WG512, 0);
        const bool big_form = KBIG != KPT && wide_big_form(ES, n);
        if (big_form) go(integral_constant<int, 1024>{}, integral_constant<int, KBIG>{}, VERDICT_WG1024, 0);
        else go(integral_constant<int, 1024>{}, integral_constant<int, KPT>{}, VERDICT_WG1024, 0);
        {   // the buckets above the chosen form's workgroup (VERDICT_MEDIUM): one workgroup of the largest kind each
            constexpr int KMED = medium_kpt_for(ES);
            constexpr size_t lds = LdsTile<ES, KMED, 1024>::bytes();
            auto kern = rsx_bucket16_medium_kernel<ES, KMED, 1024>;
            ensure_lds(ctx, reinterpret_cast<const void*>(kern), lds);
            const Gate g{base.word, VERDICT_PATH_MASK | VERDICT_MEDIUM, VERDICT_HYBRID | VERDICT_MEDIUM};
            hipLaunchKernelGGL(kern, dim3((uint32_t)ctx->num_cu), dim3(1024), lds, st, a, starts, scratch, plan, (uint32_t)(256 * KPT), (uint32_t)(512 * KPT),
                               (uint32_t)(big_form ? cape<ES, KBIG, 1024>() : cape<ES, KPT, 1024>()), g);
        }
        RSX_HIP(hipGetLastError());
        return RSX_OK;
    }
}

template <int ES>
int launch_segcopy(rsx_ctx* ctx, const void* src, void* dst, const uint64_t* so, const uint64_t* dof,
                   const uint64_t* len, uint32_t nseg, hipStream_t st) {
    const uint32_t bps = 8;
    hipLaunchKernelGGL((rsx_segcopy_kernel<ES>), dim3(nseg * bps), dim3(256), 0, st,
                       static_cast<const Elem<ES>*>(src), static_cast<Elem<ES>*>(dst), so, dof, len, nseg, bps);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}

// ---- the classes of the LDS sort: what the segmented sorts and top-k launch ------------------------------------------
// One class is a workgroup size x bucket_kpt_for(ES) elements; its persistent grid fills the device.
struct LdsGeometry {
    size_t lds;     // dynamic LDS of a workgroup
    uint64_t full;  // workgroups that fill the device
};
template <int ES, int KPT, int WG, typename Kern>
LdsGeometry lds_class_geometry(rsx_ctx* ctx, Kern kern) {
    constexpr size_t lds = LdsTile<ES, KPT, WG>::bytes();
    ensure_lds(ctx, reinterpret_cast<const void*>(kern), lds);
    uint32_t per_cu = (uint32_t)(LDS_PER_CU / (lds + 1024));
    if (per_cu > 1024u / WG) per_cu = 1024u / WG;  // (128 registers a lane: 16 waves a CU)
    if (per_cu < 1) per_cu = 1;
    return {lds, (uint64_t)ctx->num_cu * per_cu};
}
// the grid of a segmented class, and the workgroups of a team (rsx_segment_kernels.hpp, Dispatch)
inline uint64_t segment_grid(uint64_t full, const uint64_t* offsets, uint64_t nseg, uint32_t* team) {
    *team = 1;
    if (!offsets) return full > nseg ? nseg : full;
    const uint64_t nblocks = (nseg + SEG_BLOCK - 1) / SEG_BLOCK;  // few blocks: the workgroups of a team share a block's members
    while (*team < SEG_BLOCK && (uint64_t)*team < nseg && nblocks * *team < full) *team *= 2;
    uint64_t teams = full / *team;
    if (teams < 1) teams = 1;
    if (teams > nblocks) teams = nblocks;
    return teams * *team;
}
// The three classes of a segmented launch, segments of lo < length <= hi each: 256 threads in LDS from `lo0`, 1024 threads
// in LDS, 1024 threads through memory.  go(workgroup size, through memory, walk with lo and hi set) launches one; a class
// that `max_len` (0: unknown), or the one row length, leaves no segment is passed over.
template <int ES, typename Go>
int for_segment_classes(const SegWalk& w, uint64_t max_len, uint64_t lo0, Go&& go) {
    constexpr uint32_t CAP0 = segment_cap(ES, 0), CAP1 = segment_cap(ES, 1);
    const uint64_t longest = w.offsets ? (max_len ? max_len : ~0ull) : w.row_len;
    auto one = [&](auto wgc, auto memc, uint64_t lo, uint64_t hi) -> int {
        if (longest <= lo || (!w.offsets && w.row_len > hi)) return RSX_OK;  // no segment of this class can occur
        SegWalk c = w;
        c.lo = lo;
        c.hi = hi;
        return go(wgc, memc, c);
    };
    using std::integral_constant;
    int rc = one(integral_constant<int, 256>{}, integral_constant<bool, false>{}, lo0, CAP0);
    if (rc) return rc;
    rc = one(integral_constant<int, 1024>{}, integral_constant<bool, false>{}, CAP0, CAP1);
    if (rc) return rc;
    return one(integral_constant<int, 1024>{}, integral_constant<bool, true>{}, CAP1, 0xFFFFFFFFull);
}
inline SegWalk seg_walk(rsx_ctx* ctx, uint64_t n, const uint64_t* offsets, uint64_t nseg, uint64_t row_len) {
    return SegWalk{n, offsets, nseg, row_len, 0, 0, 1, ctx->host_err_dev};  // (lo, hi and team: set per class)
}

// ---- many segments of one array (rsx_segment_kernels.hpp) ------------------------------------------
// One launch per size class that `max_len` (0: unknown) leaves possible; rows (offsets == nullptr): the one class of
// row_len.  *launched receives the number of kernels enqueued.
template <int ES>
int launch_segment_sort(rsx_ctx* ctx, void* data, void* tmp, size_t n, const rsx_layout* L, const uint64_t* offsets, uint64_t nseg,
                        uint64_t row_len, uint64_t max_len, uint32_t* launched, hipStream_t st) {
    constexpr int KPT = bucket_kpt_for(ES);
    if (L->key_bytes > 16) return fail(ctx, RSX_ERR_INTERNAL, "launch_segment_sort: key width out of range");
    SmallArgs a = small_args(ctx, L, L->key_bytes, L->key_bytes, true);  // the LDS forms
    if (L->key_bytes < 6) a.no_skip = 1u;
    SmallArgs am = a;  // through memory: the keys stay raw, every pass reads its digit through the key map
    am.map_load = am.map_store = 0;
    for (uint32_t d = 0; d < L->key_bytes; ++d) am.spec[d] = make_spec(L, d);
    return for_segment_classes<ES>(seg_walk(ctx, n, offsets, nseg, row_len), max_len, 1, [&](auto wgc, auto memc, const SegWalk& w) -> int {
        constexpr int WGS = decltype(wgc)::value;
        constexpr bool MEM = decltype(memc)::value;
        auto kern = rsx_segment_sort_kernel<ES, KPT, WGS, MEM>;
        const LdsGeometry g = lds_class_geometry<ES, KPT, WGS>(ctx, kern);
        SegArgs b{data, tmp, w};
        const uint64_t grid = segment_grid(g.full, offsets, nseg, &b.w.team);
        LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
        hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(WGS), g.lds, st, MEM ? am : a, b);
        RSX_HIP(hipGetLastError());
        ++*launched;
        return RSX_OK;
    });
}

// ---- many segments of separate key and value columns (rsx_segment_pairs_kernels.hpp) ----------------------
// One launch per size class of the JOINED element size ES that `max_len` (0: unknown) leaves possible; rows: the one
// class of row_len.  The kernel is typed on the widths (KB, VB) with pairs_elem(KB, VB) == ES.
template <int ES, int KB, int VB>
int launch_segment_pairs_kv(rsx_ctx* ctx, const SegPairsCall& c, uint32_t* launched, hipStream_t st) {
    constexpr int KPT = bucket_kpt_for(ES);
    const rsx_layout L{(uint32_t)ES, 0, (uint32_t)KB, RSX_KEY_UNSIGNED};  // what the passes see: the mapped key in front
    SmallArgs a = small_args(ctx, &L, KB, KB, false);
    if (KB < 6) a.no_skip = 1u;
    // (argsort: a segment of one element gets its one 0, so the first class starts at length 1)
    return for_segment_classes<ES>(seg_walk(ctx, c.n, c.offsets, c.nseg, c.row_len), c.max_len, c.mode == SEGP_LOCAL ? 0 : 1,
                                   [&](auto wgc, auto memc, const SegWalk& w) -> int {
        constexpr int WGS = decltype(wgc)::value;
        constexpr bool MEM = decltype(memc)::value;
        if (MEM && (!c.w0 || !c.w1)) return fail(ctx, RSX_ERR_INTERNAL, "launch_segment_pairs: no workspace for the through-memory class");
        auto kern = rsx_segment_pairs_kernel<ES, KB, VB, KPT, WGS, MEM>;
        const LdsGeometry g = lds_class_geometry<ES, KPT, WGS>(ctx, kern);
        SegPairsArgs b{static_cast<uint8_t*>(c.keys), static_cast<uint8_t*>(c.values), c.w0, c.w1, w, c.kind, c.desc, c.mode, c.ib};
        const uint64_t grid = segment_grid(g.full, c.offsets, c.nseg, &b.w.team);
        LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
        hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(WGS), g.lds, st, a, b);
        RSX_HIP(hipGetLastError());
        ++*launched;
        return RSX_OK;
    });
}

template <int ES, int KB, int VB>
bool segment_pairs_try(rsx_ctx* ctx, const SegPairsCall& c, uint32_t* launched, hipStream_t st, int& rc) {
    if constexpr (pairs_elem(KB, VB) == (uint32_t)ES) {
        if (c.kb == (uint32_t)KB && c.vb == (uint32_t)VB) {
            rc = launch_segment_pairs_kv<ES, KB, VB>(ctx, c, launched, st);
            return true;
        }
    }
    return false;
}
template <int ES, int KB>
bool segment_pairs_try_kb(rsx_ctx* ctx, const SegPairsCall& c, uint32_t* launched, hipStream_t st, int& rc) {
    return segment_pairs_try<ES, KB, 0>(ctx, c, launched, st, rc) || segment_pairs_try<ES, KB, 1>(ctx, c, launched, st, rc) ||
           segment_pairs_try<ES, KB, 2>(ctx, c, launched, st, rc) || segment_pairs_try<ES, KB, 4>(ctx, c, launched, st, rc) ||
           segment_pairs_try<ES, KB, 8>(ctx, c, launched, st, rc) || segment_pairs_try<ES, KB, 16>(ctx, c, launched, st, rc);
}
template <int ES>
int launch_segment_pairs(rsx_ctx* ctx, const SegPairsCall& c, uint32_t* launched, hipStream_t st) {
    int rc = RSX_OK;
    if (c.mode != SEGP_VALUES && c.vb != 4) return fail(ctx, RSX_ERR_INTERNAL, "launch_segment_pairs: positions are four bytes");
    if (segment_pairs_try_kb<ES, 1>(ctx, c, launched, st, rc) || segment_pairs_try_kb<ES, 2>(ctx, c, launched, st, rc) ||
        segment_pairs_try_kb<ES, 4>(ctx, c, launched, st, rc) || segment_pairs_try_kb<ES, 8>(ctx, c, launched, st, rc) ||
        segment_pairs_try_kb<ES, 16>(ctx, c, launched, st, rc))
        return rc;
    return fail(ctx, RSX_ERR_INTERNAL, "launch_segment_pairs: widths without a kernel of this element size");
}

// ---- the first k of every row (rsx_topk_kernels.hpp) ------------------------------------------------
// Rows of at most CAP1 elements: one launch, one workgroup per row, of the class of row_len.  Longer rows: a tournament --
// the row is cut into chunks of CAP1, every chunk leaves its min(k, length) best as joined candidates in a workspace array,
// and the candidates of a row are the row of the next round (k <= CAP1 / 2: every round shrinks the row) until it fits one
// chunk, whose launch writes the outputs.
template <int ES, int KB>
int launch_topk_kb(rsx_ctx* ctx, const TopkCall& c, uint32_t* launched, hipStream_t st) {
    constexpr int KPT = bucket_kpt_for(ES);
    constexpr uint32_t CAP0 = segment_cap(ES, 0), CAP1 = segment_cap(ES, 1);
    const rsx_layout L{(uint32_t)ES, 0, (uint32_t)KB, RSX_KEY_UNSIGNED};  // what the passes see: the mapped key in front
    SmallArgs a = small_args(ctx, &L, KB, KB, false);
    if (KB < 6) a.no_skip = 1u;
    if (c.row_len > CAP1 && (c.k > topk_max_k(ES) || !c.w0 || !c.w1)) return fail(ctx, RSX_ERR_INTERNAL, "launch_topk: long rows without their workspace");
    TopkArgs t;
    std::memset(&t, 0, sizeof t);
    t.rows = c.rows;
    t.row_len = c.row_len;
    t.chunk = CAP1;
    t.k = (uint32_t)c.k;
    t.kind = c.kind;
    t.desc = c.desc;
    t.ib = c.ib;
    auto go = [&](auto wgc) -> int {
        constexpr int WGS = decltype(wgc)::value;
        auto kern = rsx_topk_kernel<ES, KB, KPT, WGS>;
        const LdsGeometry g = lds_class_geometry<ES, KPT, WGS>(ctx, kern);
        const uint64_t total = t.rows * t.cpr;
        LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
        hipLaunchKernelGGL(kern, dim3((uint32_t)(g.full > total ? total : g.full)), dim3(WGS), g.lds, st, a, t);
        RSX_HIP(hipGetLastError());
        ++*launched;
        return RSX_OK;
    };
    uint64_t m = c.row_len;
    void* bufs[2] = {c.w0, c.w1};
    for (uint32_t round = 0;; ++round) {
        const uint64_t cpr = (m + CAP1 - 1) / CAP1, last = m - (cpr - 1) * CAP1;
        const bool final = cpr == 1;
        t.keys = round == 0 ? static_cast<const uint8_t*>(c.keys) : nullptr;
        t.cand_in = round == 0 ? nullptr : bufs[(round - 1) & 1u];
        t.cand_out = final ? nullptr : bufs[round & 1u];
        t.out_keys = final ? static_cast<uint8_t*>(c.out_keys) : nullptr;
        t.out_index = final ? static_cast<uint8_t*>(c.out_index) : nullptr;
        t.m = (uint32_t)m;
        t.cpr = (uint32_t)cpr;
        t.m_next = (uint32_t)((cpr - 1) * c.k + (c.k < last ? c.k : last));
        const int rc = (final && m <= CAP0) ? go(std::integral_constant<int, 256>{}) : go(std::integral_constant<int, 1024>{});
        if (rc) return rc;
        if (final) return RSX_OK;
        m = t.m_next;
    }
}

template <int ES>
int launch_topk(rsx_ctx* ctx, const TopkCall& c, uint32_t* launched, hipStream_t st) {
    if constexpr (ES == 8) {
        if (c.kb == 1) return launch_topk_kb<ES, 1>(ctx, c, launched, st);
        if (c.kb == 2) return launch_topk_kb<ES, 2>(ctx, c, launched, st);
        if (c.kb == 4) return launch_topk_kb<ES, 4>(ctx, c, launched, st);
    } else if constexpr (ES == 16) {
        if (c.kb == 8) return launch_topk_kb<ES, 8>(ctx, c, launched, st);
    } else if constexpr (ES == 32) {
        if (c.kb == 16) return launch_topk_kb<ES, 16>(ctx, c, launched, st);
    }
    return fail(ctx, RSX_ERR_INTERNAL, "launch_topk: no (key, u32 position) element of this size for the key width");
}

}  // namespace rsxh
