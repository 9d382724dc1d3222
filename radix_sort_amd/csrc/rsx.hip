// rsx.hip -- host side of librsx.so: the C-ABI of include/rsx.h over the gfx950
// kernels in rsx_device.hpp.  Plays the role of the body of
// `<[T]>::radix_sort` (reference src/radix_sort/mod.rs:62-175): pass loop,
// ping-pong, odd-D copy-back -- with every phase a stream-ordered launch.
// The per-element-size kernel launchers live in rsx_es.hip (one object per size).
#include "rsx_internal.hpp"
#include "rsx_misc_kernels.hpp"
#include "rsx_any_kernels.hpp"
#include "rsx_select_kernels.hpp"
#include "rsx_bin_kernels.hpp"
#include "rsx_msplit_kernels.hpp"
#include "rsx_binred_kernels.hpp"

#include <cmath>

using namespace rsx;
using namespace rsxh;

namespace {

// any_width: what rsx_sort_device / rsx_sort_host / rsx_ctx_reserve / rsx_generate_device / rsx_verify_device accept: any
// element size and integer keys of any width up to 16 bytes.  Layouts that layout_ok + size_supported refuse reach the
// kernels through sort_any_locked; every other entry point keeps to the key widths with kernels (bounds* and splitter*:
// layout_ok alone, any element size; histogram, partition*, segments and sharded sorts: layout_ok + size_supported).
bool layout_ok(const rsx_layout* L, bool any_width = false) {
    if (!L) return false;
    const uint32_t kb = L->key_bytes;
    if (any_width ? (kb < 1 || kb > 16) : !(kb == 1 || kb == 2 || kb == 4 || kb == 8 || kb == 16)) return false;
    if (L->key_kind > RSX_KEY_FLOAT) return false;
    if (L->key_kind == RSX_KEY_FLOAT && !(kb == 4 || kb == 8)) return false;
    if (L->elem_bytes == 0 || (uint64_t)L->key_offset + kb > L->elem_bytes) return false;
    return true;
}
// the launchers of one element size (rsx_es.hip), looked up once per call; null: a size without kernels, which
// check_common refuses
const EsLaunchers* launchers_for(uint32_t es) {
    switch (es) {
        case 1: return &es_launchers<1>();
        case 2: return &es_launchers<2>();
        case 4: return &es_launchers<4>();
        case 8: return &es_launchers<8>();
        case 12: return &es_launchers<12>();
        case 16: return &es_launchers<16>();
        case 24: return &es_launchers<24>();
        case 32: return &es_launchers<32>();
        default: return nullptr;
    }
}
bool size_supported(uint32_t es) { return launchers_for(es) != nullptr; }
uint32_t elem_align(uint32_t es) {
    switch (es) {
        case 1: return 1;
        case 2: return 2;
        case 4: case 12: return 4;
        case 8: case 24: return 8;
        default: return 16;
    }
}
bool aligned(const void* p, uint32_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

bool capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}

// Brackets the work ONE API call enqueues on `st`: the context's device workspace (count matrices,
// tickets, status words) belongs to one sort at a time, so work arriving on a different stream than
// the context's last enqueue first waits for that enqueue (an event, no host sync).  Inside a stream
// capture nothing is recorded: ordering between replays is the graph owner's business.
struct Enqueue {
    rsx_ctx* c;
    hipStream_t st;
    bool live;
    Enqueue(rsx_ctx* ctx, hipStream_t s) : c(ctx), st(s), live(ctx->last_event != nullptr && !capturing(s)) {
        if (live && c->busy && c->last_stream != st) (void)hipStreamWaitEvent(st, c->last_event, 0);
    }
    ~Enqueue() {
        if (!live) return;
        (void)hipEventRecord(c->last_event, st);
        c->busy = true;
        c->last_stream = st;
    }
};

size_t status_bytes_for(const rsx_ctx* ctx, size_t n, uint32_t es) {
    const RegionGeom g = make_geom(ctx, n, es);
    size_t b = (size_t)status_rows(g) * RADIX * (status32(g) ? 4 : 8);
    if ((uint64_t)n <= mid_max_elems((int)es)) {  // the bucket split of a middle-size sort has more, smaller tiles
        const RegionGeom gs = make_geom(ctx, n, es, true);
        const size_t bs = (size_t)status_rows(gs) * RADIX * 4;
        if (bs > b) b = bs;
    }
    return b;
}

// First use of a context on its device: aux block, host-visible error word, the two device self-tests.
int ensure_aux(rsx_ctx* ctx, hipStream_t st) {
    if (ctx->aux) return RSX_OK;
    if (capturing(st)) return fail(ctx, RSX_ERR_WORKSPACE, "workspace not reserved (rsx_ctx_reserve) before stream capture");
    void* p = nullptr;
    RSX_HIP(hipMalloc(&p, AUX_BYTES));
    ctx->aux = static_cast<char*>(p);
    RSX_HIP(hipMemset(ctx->aux, 0, AUX_BYTES));
    RSX_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->host_err), 64, hipHostMallocMapped));
    std::memset(ctx->host_err, 0, 64);
    RSX_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->host_err_dev), ctx->host_err, 0));
    RSX_HIP(hipEventCreateWithFlags(&ctx->last_event, hipEventDisableTiming));
    uint32_t* flags = flags_of(ctx);  // [0] LDS order failures, [4..6] L2 probe {pairs, cross-CU pairs, failures}, [16..] probe words
    // may the sweep rank by returned LDS atomics on this device?  (see rsx_lds_order_kernel)
    hipLaunchKernelGGL(rsx_lds_order_kernel, dim3(64), dim3(512), 0, nullptr, flags);
    RSX_HIP(hipGetLastError());
    // may a single-XCD chain keep its status words in that XCD's L2?  (see rsx_l2_probe_kernel)
    uint32_t* probe_words = reinterpret_cast<uint32_t*>(ctx->aux + OFF_BASE);  // scratch: 32 pairs x 4 words (zeroed above)
    hipLaunchKernelGGL(rsx_l2_probe_kernel, dim3(64), dim3(64), 0, nullptr, probe_words, flags + 4, 64u);
    RSX_HIP(hipGetLastError());
    uint32_t v[8] = {1, 0, 0, 0, 0, 0, 1, 0};
    RSX_HIP(hipMemcpy(v, flags, sizeof v, hipMemcpyDeviceToHost));
    RSX_HIP(hipMemset(ctx->aux + OFF_BASE, 0, 32 * 4 * sizeof(uint32_t)));
    ctx->rank_atomic = v[0] == 0;
    ctx->l2_local = v[4] > 0 && v[5] > 0 && v[6] == 0;  // some same-XCD pair on two CUs ran, none missed a value
    if (ctx->options & OPT_VERBOSE) {
        std::fprintf(stderr, "[rsx] LDS atomic order self-test %s\n", v[0] ? "FAILED: ballots only" : "passed");
        std::fprintf(stderr, "[rsx] same-XCD hand-off self-test: %u pairs on one XCD, %u of them on two CUs, %u failures -> %s\n",
                     v[4], v[5], v[6], ctx->l2_local ? "passed" : "agent-scope status stores");
    }
    return RSX_OK;
}

int ensure_workspace(rsx_ctx* ctx, size_t n, const rsx_layout* L, hipStream_t st) {
    int rc = ensure_aux(ctx, st);
    if (rc) return rc;
    const size_t need = status_bytes_for(ctx, n, L->elem_bytes);
    if (need > ctx->status_bytes) {
        if (capturing(st)) return fail(ctx, RSX_ERR_WORKSPACE, "workspace too small for this sort and a stream capture is active (rsx_ctx_reserve first)");
        if (ctx->busy) RSX_HIP(hipEventSynchronize(ctx->last_event));  // the old block may still be in use
        if (ctx->status) RSX_HIP(hipFree(ctx->status));
        ctx->status = nullptr;
        ctx->status_bytes = 0;
        hipError_t e = hipMalloc(&ctx->status, 2 * need);  // two arrays: this pass's and the next pass's
        if (e != hipSuccess) return fail(ctx, RSX_ERR_NOMEM, "workspace hipMalloc", e);
        ctx->status_bytes = need;
    }
    return RSX_OK;
}

// the 256 digit totals of a count matrix -> d_counts
int launch_totals(rsx_ctx* ctx, const RegionGeom& g, const unsigned long long* J, uint64_t* d_counts, hipStream_t st) {
    LaunchTimer lt(ctx, RSX_PROF_SCAN, st);
    hipLaunchKernelGGL(rsx_totals_kernel, dim3(1), dim3(RADIX), 0, st, J, g.num_regions, d_counts, status32(g) ? 1u : 0u);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}

// Fills `run` for the sort (or lone pass) being enqueued: picks its control block -- every pass's tickets and roll-call words, the
// top digit's count matrix and count matrix 0, all zero -- and tells the count kernel which block to zero on its way:
// the one the previous sort used (rsx_internal.hpp, aux layout).  A sort that is being captured into a graph uses
// block 2 and zeroes it itself (a replay cannot alternate); so does the sort after a failed enqueue, for both blocks.
int begin_control(rsx_ctx* ctx, SortRun& run, hipStream_t st, const RegionGeom& g, bool uses_jt) {
    run = SortRun{};
    const uint64_t used = (uint64_t)J_REPL * g.num_regions * RADIX * sizeof(uint64_t);  // prefix of a count matrix in use
    if (capturing(st)) {
        run.cb = 2;
        hipLaunchKernelGGL(rsx_zero16_kernel, dim3(64), dim3(256), 0, st, reinterpret_cast<uint4*>(cb_of(ctx, 2)), (uint64_t)(CB_BYTES / 16));
        RSX_HIP(hipGetLastError());
        return RSX_OK;
    }
    if (ctx->cb_dirty) {
        RSX_HIP(hipMemsetAsync(cb_of(ctx, 0), 0, 2 * CB_BYTES, st));
        ctx->cb_used[0][0] = ctx->cb_used[0][1] = ctx->cb_used[1][0] = ctx->cb_used[1][1] = 0;
    }
    const uint32_t prev = ctx->cb_alt;
    ctx->cb_alt ^= 1u;
    run.cb = ctx->cb_alt;
    run.clean.p[0] = reinterpret_cast<uint4*>(cb_of(ctx, prev) + CB_TICKETS);
    run.clean.n16[0] = CB_JT / 16;
    run.clean.p[1] = reinterpret_cast<uint4*>(cb_of(ctx, prev) + CB_JT);
    run.clean.n16[1] = ctx->cb_used[prev][0] / 16;
    run.clean.p[2] = reinterpret_cast<uint4*>(cb_of(ctx, prev) + CB_J0);
    run.clean.n16[2] = ctx->cb_used[prev][1] / 16;
    ctx->cb_used[run.cb][0] = uses_jt ? used : 0;
    ctx->cb_used[run.cb][1] = used;
    ctx->cb_dirty = true;  // until the enqueue has gone through (end_control)
    return RSX_OK;
}
inline void end_control(rsx_ctx* ctx) { ctx->cb_dirty = false; }

int check_common(rsx_ctx* ctx, const rsx_layout* L) {
    if (!ctx) return RSX_ERR_ARG;
    if (!layout_ok(L)) return fail(ctx, RSX_ERR_ARG, "invalid rsx_layout");
    if (!size_supported(L->elem_bytes)) return fail(ctx, RSX_ERR_UNSUPPORTED, "element size has no device kernel");
    return RSX_OK;
}
bool direct_layout(const rsx_layout* L) { return layout_ok(L) && size_supported(L->elem_bytes); }
// the entry points that sort any layout (sort_any_locked)
int check_any(rsx_ctx* ctx, const rsx_layout* L) {
    if (!ctx) return RSX_ERR_ARG;
    if (direct_layout(L)) return RSX_OK;
    if (!layout_ok(L, true)) return fail(ctx, RSX_ERR_ARG, "invalid rsx_layout");
    if (L->elem_bytes > RSX_MAX_ELEM_BYTES) return fail(ctx, RSX_ERR_UNSUPPORTED, "element larger than RSX_MAX_ELEM_BYTES");
    return RSX_OK;
}

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// What an entry point holds from its argument checks to its return: the context's mutex, the context's device as the
// current one, and the caller's stream.  !ok: the device could not be set.
struct Entry {
    std::lock_guard<std::mutex> lk;
    DeviceGuard dev;
    const bool ok;
    const hipStream_t st;
    explicit Entry(rsx_ctx* ctx, void* stream = nullptr) : lk(ctx->mu), dev(ctx->device), ok(dev.ok), st(static_cast<hipStream_t>(stream)) {}
};
int no_device(rsx_ctx* ctx) { return fail(ctx, RSX_ERR_NODEVICE, "hipSetDevice failed"); }
// How every entry point that needs the device takes it: declares `held`, and leaves where the device could not be set.
#define RSX_ENTER(stream)     \
    Entry held(ctx, stream);  \
    if (!held.ok) return no_device(ctx)

// the checks of an `order` and an `index_bytes` argument
int order_desc(rsx_ctx* ctx, int order, uint32_t* desc) {
    if (order != RSX_ORDER_ASCENDING && order != RSX_ORDER_DESCENDING) return fail(ctx, RSX_ERR_ARG, "invalid order");
    *desc = order == RSX_ORDER_DESCENDING ? 1u : 0u;
    return RSX_OK;
}
int check_index_bytes(rsx_ctx* ctx, uint32_t ib) {
    if (ib != 4 && ib != 8) return fail(ctx, RSX_ERR_ARG, "index_bytes must be 4 or 8");
    return RSX_OK;
}

// what the call being enqueued ran, for RSX_INFO_LAST_PASSES
void note_path(rsx_ctx* ctx, uint32_t path, uint32_t passes, uint32_t route = 0) {
    ctx->last_path = path;
    ctx->last_sort_passes = passes;
    ctx->last_route = route;
}

// A kernel of this context gave up a bounded wait (the word is host-visible: no sync needed to see it).
int pending_error(rsx_ctx* ctx) {
    if (ctx->host_err && host_word(ctx, HV_ERROR))
        return fail(ctx, RSX_ERR_INTERNAL, "an earlier sort on this context gave up a device-side wait; its output is invalid (rsx_ctx_check clears the condition)");
    return RSX_OK;
}

// The D LSD passes of mod.rs:84-169 on the device: count phase of pass 0 (later passes are counted by the sweep before
// them), then D sweeps with ping-pong; the prefix phase (mod.rs:110-120) is the prologue of each sweep.  mid: a
// middle-size sort whose first sweep also reports what the top digit looks like (mid_mode 2).
int lsd_passes(rsx_ctx* ctx, const EsLaunchers& K, SortRun& run, void* d_data, void* d_tmp, size_t n, const rsx_layout* L, const RegionGeom& geom,
               bool mid, uint32_t mid_mode, hipStream_t st) {
    const uint32_t D = L->key_bytes;
    int rc;
    if (mid) rc = K.hist2(ctx, run, d_data, geom, L, 0, J_of(ctx, run, 0), D - 1, JT_of(ctx, run), J_of(ctx, run, 1), st);
    else rc = K.hist(ctx, run, d_data, geom, L, 0, J_of(ctx, run, 0), D > 1 ? J_of(ctx, run, 1) : nullptr, true, st);
    if (rc) return rc;
    ctx->last_sort_passes = D;
    ctx->cb_last = run.cb;
    for (uint32_t d = 0; d < D; ++d) {
        const void* src = (d % 2 == 0) ? d_data : d_tmp;
        void* dst = (d % 2 == 0) ? d_tmp : d_data;
        unsigned long long* jnext = (d + 1 < D) ? J_of(ctx, run, (d + 1) % 3) : nullptr;
        unsigned long long* jzero = (d + 2 < D) ? J_of(ctx, run, (d + 2) % 3) : nullptr;
        const int xf = (d == 0 ? 1 : 0) | (d + 1 == D ? 2 : 0);  // key map on at the first, off at the last pass
        const SweepPass pass{d, d + 1 == D, d == 0 ? mid_mode : 0u};  // (mid 2: the first LSD pass also reports whether the top digit's buckets would fit)
        rc = K.sweep(ctx, run, pass, src, dst, geom, L, d, J_of(ctx, run, d % 3), jnext, jzero, xf, st);  // mod.rs:121-168
        if (rc) return rc;
    }
    if (D % 2 == 1)  // odd-D copy-back (mod.rs:170-174)
        RSX_HIP(hipMemcpyAsync(d_data, d_tmp, n * (size_t)L->elem_bytes, hipMemcpyDeviceToDevice, st));
    return RSX_OK;
}

// ---- the paths of a sort, in the order sort_device_locked tries them ----
int ensure_ovf16(rsx_ctx* ctx, hipStream_t st) {
    if (ctx->ovf16) return RSX_OK;
    RSX_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->ovf16), 65536 * sizeof(uint32_t)));
    RSX_HIP(hipMemsetAsync(ctx->ovf16, 0, 65536 * sizeof(uint32_t), st));  // kept all zero between sorts by rsx_total16_kernel
    return RSX_OK;
}

// u16 / i16 arrays of at least 2^23 elements: the element is its two-byte key, so the 65536 counts ARE the sorted
// array: count (one read), write the runs (one write) -- instead of D = 2 passes of each.  The count kernel's
// per-workgroup counters (128 KiB each), the bin totals and the bin-block sums live in d_tmp.
int sort_counting16(rsx_ctx* ctx, void* d_data, void* d_tmp, size_t n, const rsx_layout* L, hipStream_t st) {
    int rc = ensure_ovf16(ctx, st);
    if (rc) return rc;
    const size_t tail = 65536 * sizeof(uint64_t) + 256 * sizeof(uint64_t);
    size_t parts = (n * 2 - tail) / (32768 * sizeof(uint32_t));
    if (parts > (size_t)ctx->num_cu) parts = (size_t)ctx->num_cu;
    uint32_t* P = static_cast<uint32_t*>(d_tmp);
    uint64_t* tot = reinterpret_cast<uint64_t*>(static_cast<char*>(d_tmp) + parts * 32768 * sizeof(uint32_t));
    uint64_t* BT = tot + 65536;
    const uint32_t xor_mask = L->key_kind == RSX_KEY_SIGNED ? 0x8000u : 0u;
    ensure_lds(ctx, reinterpret_cast<const void*>(rsx_count16_kernel), 131072);
    {
        LaunchTimer lt(ctx, RSX_PROF_HIST, st);
        hipLaunchKernelGGL(rsx_count16_kernel, dim3((uint32_t)parts), dim3(1024), 131072, st, static_cast<const uint16_t*>(d_data),
                           (uint64_t)n, xor_mask, P, ctx->ovf16);
        RSX_HIP(hipGetLastError());
    }
    {
        LaunchTimer lt(ctx, RSX_PROF_SCAN, st);
        hipLaunchKernelGGL(rsx_total16_kernel, dim3(256), dim3(256), 0, st, P, (uint32_t)parts, ctx->ovf16, tot, BT);
        RSX_HIP(hipGetLastError());
    }
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    hipLaunchKernelGGL(rsx_expand16_kernel, dim3((uint32_t)ctx->num_cu * 8), dim3(256), 0, st, static_cast<uint16_t*>(d_data), (uint64_t)n, tot,
                       BT, xor_mask);
    RSX_HIP(hipGetLastError());
    ctx->last_path = PATH_COUNT16;
    return RSX_OK;
}

// Wide keys, large arrays (rsx_mid_kernels.hpp): two passes through memory for the top 16 bits, the rest in LDS --
// when the count of those 16 bits says that every bucket fits a workgroup.  That is known on the device only, so
// BOTH kernel sequences are enqueued, gated on the verdict word rsx_scan16_kernel writes (a launch that returns at
// once costs ~5 us: nothing beside milliseconds).  A refused try costs its count (one read of the array): the
// verdict is also written host-visibly, and after a refusal the context goes 15 sorts without trying.
// what the hybrid's largest (1024-thread) workgroup holds
uint32_t wide_cap(uint32_t es) { return bucket_cape((int)es, wide_kpt_for((int)es), 1024); }
// whether this sort is to try it
bool wide_forecast(rsx_ctx* ctx, size_t n, const rsx_layout* L, hipStream_t st) {
    const uint32_t es = L->elem_bytes, D = L->key_bytes;
    // Where it pays (measured, uniform keys, LSD passes / hybrid): keys of 8 and 16 bytes everywhere above the middle
    // sizes -- u64 2^23 x1.34, 2^26 x1.29, 2^28 x1.9; (u64,u64) 2^22 x1.3, 2^26 x1.9; u128 2^22 x2.4, 2^26 x3.8 (small
    // buckets are sorted in groups, rsx_bucket16_kernel) --; 4-byte keys in 8-byte and wider elements (two of four passes
    // in LDS) x1.2 from 2 GiB on; (u32,u32) x1.09 at 1 GiB already (2^27: 1.99 -> 1.83 ms), x0.88 at 2^26.
    const bool wide_type = es >= 8 && D >= 4;
    const size_t wide_floor = D >= 8 ? 0 : es == 8 ? ((size_t)1 << 30) : ((size_t)2 << 30);
    const bool wide_size = wide_type && (uint64_t)n > mid_max_elems((int)es);
    bool wide = false;
    if (ctx->wide_mode == 2) {
        wide = wide_type && n >= 65536;
    } else if (((ctx->wide_mode == 1 && n * (size_t)es >= wide_floor) || ctx->wide_mode == 3) && wide_size &&
               (uint64_t)n / 65536u < (uint64_t)wide_cap(es)) {  // (the real test is the device's, on the actual counts)
        // the last try's verdict (1 taken, 2 refused) counts for arrays like the one it was given on: same layout, n
        // within a factor of two (the multi-GPU drivers sort value ranges of slightly different lengths)
        volatile uint32_t& hint = host_word(ctx, HV_WIDE_HINT);
        const uint64_t sig = 1ull | (uint64_t)(63 - __builtin_clzll((unsigned long long)n)) << 8 | (uint64_t)es << 16 | (uint64_t)L->key_offset << 24 |
                             (uint64_t)D << 32 | (uint64_t)L->key_kind << 40;
        if (ctx->wide_skip > 0 && sig == ctx->wide_refused_sig) {
            --ctx->wide_skip;
        } else if (hint == 2u && sig == ctx->wide_tried_sig) {
            hint = 0;
            ctx->wide_skip = 15;
            ctx->wide_refused_sig = sig;
        } else {
            if (hint == 2u) hint = 0;
            wide = true;
            ctx->wide_tried_sig = sig;
        }
    }
    return wide && !((ctx->ovf16 == nullptr || ctx->wide_buf == nullptr) && capturing(st));
}
int sort_wide(rsx_ctx* ctx, const EsLaunchers& K, void* d_data, void* d_tmp, size_t n, const rsx_layout* L, hipStream_t st) {
    const uint32_t es = L->elem_bytes, D = L->key_bytes;
    int rc = ensure_ovf16(ctx, st);
    if (rc) return rc;
    if (!ctx->wide_buf) {
        RSX_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->wide_buf), WIDE_BUF_BYTES));
        RSX_HIP(hipMemsetAsync(reinterpret_cast<char*>(ctx->wide_buf) + WIDE_PLAN_OFFSET, 0, sizeof(WidePlan), st));  // (plan_or, plan_done)
    }
    uint64_t* tot = reinterpret_cast<uint64_t*>(ctx->wide_buf);
    uint64_t* BT = tot + 65536;
    uint64_t* starts = BT + 256;
    WidePlan* plan = reinterpret_cast<WidePlan*>(reinterpret_cast<char*>(ctx->wide_buf) + WIDE_PLAN_OFFSET);
    const uint32_t* verdict = &plan->verdict;
    const RegionGeom geom = make_geom(ctx, n, es);
    // the count's workgroups: k per region of the sweeps' geometry where the scratch array holds their counters
    // (128 KiB each) -- then the first sweep's count matrix is a marginal of those counters, as long as none of them was
    // parked in the per-bin overflow table.  A bucket that fits LDS cannot park (the assert below), but the verdict also
    // keeps the hybrid with up to 8 buckets of up to medium_max elements, and 0x8000 of one of those inside one count
    // chunk do: the count kernel then sets plan->parked and rsx_scan16_kernel gives the sort to the LSD passes --;
    // else flat shares, and a count kernel of its own for that sweep
    size_t parts = n * (size_t)es / (32768 * sizeof(uint32_t));
    if (parts > (size_t)ctx->num_cu) parts = (size_t)ctx->num_cu;
    static_assert(bucket_cape(8, wide_kpt_for(8), 1024) < 0x8000u && bucket_cape(4, wide_kpt_for(4), 1024) < 0x8000u,
                  "buckets that fit LDS never park a 16-bit counter: uniform inputs must not lose the hybrid to WidePlan::parked");
    uint32_t k = ctx->wide_mode == 2 ? 0u : (uint32_t)(parts / geom.num_regions);
    if (k > 0) parts = (size_t)k * geom.num_regions;
    rc = K.wideplan(ctx, d_data, n, L, plan, st);
    if (rc) return rc;
    rc = K.count16top(ctx, d_data, n, L, plan, static_cast<uint32_t*>(d_tmp), (uint32_t)parts, geom.region_shift, k, st);  // partial counts in d_tmp
    if (rc) return rc;
    {
        LaunchTimer lt(ctx, RSX_PROF_SCAN, st);
        hipLaunchKernelGGL(rsx_total16_kernel, dim3(256), dim3(256), 0, st, static_cast<const uint32_t*>(d_tmp), (uint32_t)parts, ctx->ovf16, tot, BT);
        RSX_HIP(hipGetLastError());
        // which form of the bucket kernel runs is the device's choice too (launch_bucket16 enqueues them all):
        // groups of small buckets are on offer when the AVERAGE bucket is small (group_shift)
        const uint64_t cap1024 = wide_big_form((int)es, n) ? wide_cap(es) : bucket_cap((int)es), cap512 = bucket_cap((int)es) / 2;
        hipLaunchKernelGGL(rsx_scan16_kernel, dim3(256), dim3(256), 0, st, tot, BT, starts, cap512 / 2, cap512, cap1024, group_shift(ctx, n, L),
                           ctx->wide_mode == 2 ? 1u : 0u, (uint64_t)bucket_cape((int)es, medium_kpt_for((int)es), 1024) * 150u, (uint64_t)n / 64u, plan,
                           ctx->host_err_dev + HV_WIDE_HINT, reinterpret_cast<uint32_t*>(ctx->wide_buf + WIDE_LEFT_OFFSET));
        RSX_HIP(hipGetLastError());
    }
    SortRun lsd;
    rc = begin_control(ctx, lsd, st, geom, false);
    if (rc) return rc;
    ctx->cb_last = lsd.cb;
    // Two runs on one control block, each with the clean list: whichever sequence's count kernel runs does the cleaning.
    // sequence 1 (verdict 1): LSD passes on digits D-2 and D-1, then every 16-bit bucket in LDS
    SortRun hyb = lsd;
    hyb.gate = Gate{verdict, VERDICT_PATH_MASK, VERDICT_HYBRID};
    hyb.spec_dev = &plan->specs[0];  // (the two digits of the window come from the plan, not from the digit index given here)
    if (k > 0) {
        rc = K.marginal16(ctx, hyb, static_cast<const uint32_t*>(d_tmp), (uint32_t)parts, k, geom, J_of(ctx, hyb, 0), J_of(ctx, hyb, 1), st);
    } else {  // (forced mode: counters may have overflowed; a count kernel of its own, its digit from the plan)
        rc = K.hist(ctx, hyb, d_data, geom, L, D - 2, J_of(ctx, hyb, 0), J_of(ctx, hyb, 1), true, st);
    }
    if (rc) return rc;
    rc = K.sweep(ctx, hyb, SweepPass{0, false, 0}, d_data, d_tmp, geom, L, D - 2, J_of(ctx, hyb, 0), J_of(ctx, hyb, 1), nullptr, 1, st);  // keys mapped on load
    if (rc) return rc;
    hyb.spec_dev = &plan->specs[1];
    // The second sweep counts nothing, and spends the LDS its count matrix would take on a deeper tile (hyb_geom: 8-byte
    // elements; the forced mode keeps the one geometry).  Its count matrix, cursors and tickets are per region and do not
    // know the tile; its status rows are among those the first sweep zeroed.
    const RegionGeom geom2 = ctx->wide_mode == 2 ? geom : hyb_geom(geom, es);
    if (status_rows_used(geom2) > status_rows_used(geom) || tiles_per_region(geom2) > tiles_per_region(geom))
        return fail(ctx, RSX_ERR_INTERNAL, "sort_wide: the second sweep's status rows are not among those the first one zeroes");
    rc = K.sweep(ctx, hyb, SweepPass{1, true, 0}, d_tmp, d_data, geom2, L, D - 1, J_of(ctx, hyb, 1), nullptr, nullptr, 0, st);  // ... and stay mapped
    if (rc) return rc;
    rc = K.bucket16(ctx, hyb, d_data, d_tmp, n, L, starts, plan, st);
    if (rc) return rc;
    // sequence 2 (verdict 2): the D LSD passes
    lsd.gate = Gate{verdict, VERDICT_PATH_MASK, VERDICT_LSD};
    rc = lsd_passes(ctx, K, lsd, d_data, d_tmp, n, L, geom, false, 0, st);
    if (rc) return rc;
    ctx->last_sort_passes = D;
    ctx->last_path = PATH_WIDE;
    end_control(ctx);
    return RSX_OK;
}

// Middle sizes (more than one tile, up to mid_max_elems): the count kernel also counts the MOST significant digit.
// If that digit spreads the array over its 256 buckets so that each fits a workgroup's LDS, one sweep makes the
// buckets and rsx_bucket_sort_kernel sorts each by the remaining digits: 4 launches and two trips through memory
// instead of D + 2 and D.  Whether it does is known on the device only, and a launch costs ~4 us even when it
// returns at once, so the host FORECASTS from what the previous middle-size sort reported (a host-visible word,
// read without synchronising: it may lag, and either way the result is right -- a bucket that does not fit after
// all is sorted through memory by its one workgroup, slowly, after which the context keeps to LSD passes for a while).
// Returns how this sort is enqueued: 1 bucket split (*bucket_small: by 256-thread workgroups), 2 LSD passes.
uint32_t mid_forecast(rsx_ctx* ctx, size_t n, bool* bucket_small) {
    const uint32_t hint = host_word(ctx, HV_MID_HINT);  // 0 nothing yet, 1 / 3 fits (a small / a large workgroup), 2 does not
    uint32_t mid_mode;
    if (ctx->mid_choice == 1 && hint == 2 && ctx->mid_cooldown == 0) ctx->mid_cooldown = 8;  // a split met a skewed input
    if (ctx->mid_cooldown > 0) {
        --ctx->mid_cooldown;
        mid_mode = 2;
    } else {
        mid_mode = hint == 2 ? 2u : 1u;
    }
    if (ctx->mid_force) mid_mode = ctx->mid_force;
    ctx->mid_choice = mid_mode;
    *bucket_small = hint == 1 && (uint64_t)n <= 256ull * 2048ull;
    return mid_mode;
}
// bucket split (count, scan, scatter: rsx_mid_kernels.hpp), then every bucket sorted in LDS
int sort_mid_split(rsx_ctx* ctx, const EsLaunchers& K, void* d_data, void* d_tmp, size_t n, const rsx_layout* L, bool bucket_small, hipStream_t st) {
    int rc = K.mid_split(ctx, d_data, d_tmp, n, L, st);  // the buckets are made in d_tmp (keys stay mapped) ...
    if (rc) return rc;
    rc = K.bucket_sort(ctx, d_tmp, d_data, L, bucket_small, st);  // ... sorted, they land in d_data
    if (rc) return rc;
    ctx->last_path = PATH_MID_SPLIT;
    return RSX_OK;
}

// the general path; mid: a middle-size sort that the forecast gave to LSD passes (mid_mode 2)
int sort_lsd(rsx_ctx* ctx, const EsLaunchers& K, void* d_data, void* d_tmp, size_t n, const rsx_layout* L, bool mid, uint32_t mid_mode,
             hipStream_t st) {
    const RegionGeom geom = make_geom(ctx, n, L->elem_bytes);
    SortRun run;
    int rc = begin_control(ctx, run, st, geom, mid);
    if (rc) return rc;
    rc = lsd_passes(ctx, K, run, d_data, d_tmp, n, L, geom, mid, mid_mode, st);
    if (rc) return rc;
    end_control(ctx);
    return RSX_OK;
}

// u8 / i8: the element is its digit, so the 256 counts ARE the sorted array (same bytes as the pass + copy-back of
// mod.rs:121-174 would leave): count (mod.rs:90-109), write the runs, skip scatter and copy
int sort_counting8(rsx_ctx* ctx, const EsLaunchers& K, void* d_data, size_t n, const rsx_layout* L, hipStream_t st) {
    const RegionGeom geom = make_geom(ctx, n, L->elem_bytes);
    SortRun run;
    int rc = begin_control(ctx, run, st, geom, false);
    if (rc) return rc;
    rc = K.hist(ctx, run, d_data, geom, L, 0, J_of(ctx, run, 0), nullptr, false, st);
    if (rc) return rc;
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    const uint64_t steps = ((n + 15) / 16 + 255) / 256;  // a block writes 256 chunks of 16 bytes per step
    uint64_t blocks = steps;
    if (blocks > (uint64_t)ctx->num_cu * 16) blocks = (uint64_t)ctx->num_cu * 16;
    hipLaunchKernelGGL(rsx_expand_bytes_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, static_cast<uint8_t*>(d_data),
                       (uint64_t)n, J_of(ctx, run, 0), geom.num_regions, status32(geom) ? 1u : 0u,
                       L->key_kind == RSX_KEY_SIGNED ? 0x80u : 0u);
    RSX_HIP(hipGetLastError());
    end_control(ctx);
    ctx->last_path = PATH_COUNT8;
    return RSX_OK;
}

// body of rsx_sort_device; caller holds ctx->mu and has set the device
int sort_device_locked(rsx_ctx* ctx, void* d_data, void* d_tmp, size_t n, const rsx_layout* L, hipStream_t st) {
    const EsLaunchers* K = launchers_for(L->elem_bytes);
    if (!K) return fail(ctx, RSX_ERR_UNSUPPORTED, "element size has no device kernel");
    int rc = pending_error(ctx);
    if (rc) return rc;
    rc = ensure_workspace(ctx, n, L, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);
    const uint32_t D = L->key_bytes;  // T::NUMBER_OF_DIGITS
    const bool general_bytes = (ctx->options & OPT_GENERAL_BYTES) != 0;
    const bool counting8 = L->elem_bytes == 1 && !general_bytes;  // no sweep follows
    note_path(ctx, PATH_LSD, 0);
    // at most one tile: all D passes in one launch of one workgroup (rsx_small_kernel.hpp)
    if (!counting8 && n <= (size_t)512 * kpt_for((int)L->elem_bytes) && !(ctx->options & OPT_NO_SMALL_SORT)) {  // one 512-thread tile
        ctx->last_path = PATH_SMALL;
        return K->small_sort(ctx, d_data, n, L, st);
    }
    if (L->elem_bytes == 2 && D == 2 && n >= ((size_t)1 << 23) && !general_bytes && (ctx->ovf16 != nullptr || !capturing(st)))
        return sort_counting16(ctx, d_data, d_tmp, n, L, st);
    if (wide_forecast(ctx, n, L, st)) return sort_wide(ctx, *K, d_data, d_tmp, n, L, st);
    const bool mid = !counting8 && D >= 2 && (uint64_t)n <= mid_max_elems((int)L->elem_bytes) && !(ctx->options & OPT_NO_MID_SORT);
    bool bucket_small = false;
    const uint32_t mid_mode = mid ? mid_forecast(ctx, n, &bucket_small) : 0u;
    if (mid_mode == 1) return sort_mid_split(ctx, *K, d_data, d_tmp, n, L, bucket_small, st);
    if (counting8) return sort_counting8(ctx, *K, d_data, n, L, st);
    return sort_lsd(ctx, *K, d_data, d_tmp, n, L, mid, mid_mode, st);
}

// ---- layouts without a kernel of their own (include/rsx.h, "Any layout") ----
// Both routes sort a CANONICAL key: the key at offset 0, widened to kw = the smallest of 1, 2, 4, 8, 16 bytes that holds
// it (unsigned keys zero-extended, signed keys sign-extended: both keep the order, so the existing kernels sort it under
// the layout's own key kind).
//   route 1, packed re-layout: canonical key + the other elem_bytes - key_bytes bytes in their order, c <= 16 bytes,
//     padded to a size with kernels (a multiple of kw); re-laid out into workspace, sorted there, restored into d_data;
//   route 2, key-index proxy: (canonical key, u32 position) proxies are sorted, then d_data[i] = copy[proxy[i].index],
//     the copy made in d_tmp by the same kernel that made the proxies.
struct AnyPlan {
    uint32_t route;    // 1 or 2
    rsx_layout inner;  // what the existing kernels sort
    uint32_t kw;       // canonical key width
    uint32_t idx_off;  // route 2: byte offset of the position in the proxy
};
uint32_t canon_width(uint32_t kb) { return kb <= 1 ? 1 : kb <= 2 ? 2 : kb <= 4 ? 4 : kb <= 8 ? 8 : 16; }
// Route 1 while the canonical element fits 16 bytes: measured at 2^24 and 2^26, route 2 was faster from 20-byte
// elements on ((20,0,4) 4.18 against 4.84 ms at 2^26, (28,0,4) 4.59 against 5.48) and 2.3x slower for (6,0,2)
// (DESIGN.md section 5).
constexpr uint32_t ANY_PACKED_MAX = 16;
AnyPlan any_plan(const rsx_layout* L) {
    AnyPlan P{};
    const uint32_t kb = L->key_bytes, s = L->elem_bytes, kw = canon_width(kb);
    const uint32_t c = kw + s - kb;
    P.kw = kw;
    P.route = c <= ANY_PACKED_MAX ? 1u : 2u;
#if defined(RSX_TUNING) && defined(RSX_ANY_ROUTE)  // measurement builds: force the proxy route where both exist
    if (RSX_ANY_ROUTE == 2) P.route = 2;
#endif
    if (P.route == 1) {
        static const uint32_t sizes[] = {4, 8, 12, 16};
        uint32_t sp = 16;
        for (uint32_t z : sizes)
            if (z >= c && z % (kw < 16 ? kw : 16) == 0) { sp = z; break; }
        P.inner = rsx_layout{sp, 0, kw, L->key_kind};
    } else {
        const uint32_t p = kw <= 4 ? 8 : kw == 8 ? 16 : 32;  // (u32 key, u32) / (u64 key, u64) / (u128 key, u128)
        P.idx_off = kw <= 4 ? 4 : kw;
        P.inner = rsx_layout{p, 0, kw, L->key_kind};
    }
    return P;
}
// byte maps of the move kernel: source element -> canonical (re-layout / proxy), canonical -> source element (restore)
AnyMap map_forward(const rsx_layout* L, const AnyPlan& P) {
    AnyMap m{};
    const uint32_t kb = L->key_bytes, ko = L->key_offset, kw = P.kw, c = kw + L->elem_bytes - kb;
    m.sign_off = ko + kb - 1;
    for (uint32_t o = 0; o < ANY_MAP_MAX; ++o) {
        int16_t v = ANY_ZERO;
        if (o < kb) v = (int16_t)(ko + o);
        else if (o < kw) v = L->key_kind == RSX_KEY_SIGNED ? ANY_SIGN : ANY_ZERO;
        else if (P.route == 1 && o < c) v = (int16_t)(o - kw < ko ? o - kw : o - kw + kb);
        else if (P.route == 2 && o >= P.idx_off && o < P.idx_off + 4) v = (int16_t)(ANY_INDEX - (int16_t)(o - P.idx_off));
        m.m[o] = o < P.inner.elem_bytes ? v : ANY_ZERO;
    }
    return m;
}
AnyMap map_restore(const rsx_layout* L, const AnyPlan& P) {
    AnyMap m{};
    const uint32_t kb = L->key_bytes, ko = L->key_offset;
    for (uint32_t b = 0; b < ANY_MAP_MAX; ++b)
        m.m[b] = b >= L->elem_bytes ? ANY_ZERO : (b >= ko && b < ko + kb) ? (int16_t)(b - ko) : (int16_t)(P.kw + (b < ko ? b : b - kb));
    return m;
}
// Lays the arrays of the second workspace out one behind the other: take() gives the next array's offset, and `bytes`
// is then what ensure_any is asked for.  A call's plan is made of these, and both its reserve entry and its launches
// read that one plan.
struct Carve {
    size_t bytes;  // (no initialiser: the plans stay plain structs; make it with {})
    size_t take(size_t b) {
        const size_t off = bytes;
        bytes += round256(b);
        return off;
    }
};

int ensure_any(rsx_ctx* ctx, size_t bytes, hipStream_t st) {
    if (bytes <= ctx->any_bytes) return RSX_OK;
    if (capturing(st)) return fail(ctx, RSX_ERR_WORKSPACE, "workspace too small for this layout and a stream capture is active (rsx_ctx_reserve first)");
    if (ctx->busy) RSX_HIP(hipEventSynchronize(ctx->last_event));  // the old arrays may still be in use
    if (ctx->any_buf) RSX_HIP(hipFree(ctx->any_buf));
    ctx->any_buf = nullptr;
    ctx->any_bytes = 0;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&ctx->any_buf), bytes);
    if (e != hipSuccess) return fail(ctx, RSX_ERR_NOMEM, "workspace hipMalloc", e);
    ctx->any_bytes = bytes;
    return RSX_OK;
}

int reserve_any(rsx_ctx* ctx, size_t n, const rsx_layout* L, hipStream_t st) {
    const AnyPlan P = any_plan(L);
    int rc = ensure_workspace(ctx, n, &P.inner, st);
    if (rc) return rc;
    return ensure_any(ctx, 2 * round256(n * (size_t)P.inner.elem_bytes), st);
}

int launch_move(rsx_ctx* ctx, const void* src, uint32_t s_in, void* dst, uint32_t s_out, void* dst2, size_t n, const AnyMap& map,
                hipStream_t st) {
    uint32_t tile = 16384u / s_in;
    if (tile > 4096) tile = 4096;
    if (tile < 1) tile = 1;
    const size_t lds = ((size_t)tile * s_in + 47) & ~(size_t)15;  // + the 16-byte chunks the tile's two ends fall into
    uint64_t blocks = (n + tile - 1) / tile;
    const uint64_t cap = (uint64_t)ctx->num_cu * 8;
    if (blocks > cap) blocks = cap;
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    if (dst2) {
        hipLaunchKernelGGL((rsx_any_move_kernel<true, true>), dim3((uint32_t)blocks), dim3(256), lds, st, static_cast<const uint8_t*>(src), s_in,
                           static_cast<uint8_t*>(dst), s_out, static_cast<uint8_t*>(dst2), (uint64_t)n, tile, map, 1.0f / (float)s_out);
    } else {
        hipLaunchKernelGGL((rsx_any_move_kernel<true, false>), dim3((uint32_t)blocks), dim3(256), lds, st, static_cast<const uint8_t*>(src), s_in,
                           static_cast<uint8_t*>(dst), s_out, static_cast<uint8_t*>(nullptr), (uint64_t)n, tile, map, 1.0f / (float)s_out);
    }
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}

// dst[i] = src[position in proxy i]: rows of s bytes; proxies of p bytes with the u32 position at byte idx_off
int launch_gather(rsx_ctx* ctx, const void* src, void* dst, uint32_t s, const void* proxy, uint32_t p, uint32_t idx_off, size_t n, hipStream_t st) {
    const uintptr_t al = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | s;
    const uint32_t w = (al & 15) == 0 ? 16 : (al & 7) == 0 ? 8 : (al & 3) == 0 ? 4 : (al & 1) == 0 ? 2 : 1;
    const uint32_t words = s / w;
    uint32_t gshift = 0;
    while (gshift < 4 && (1u << gshift) < words) ++gshift;  // lanes per row: at most 16, four rows or more per wave
    uint64_t blocks = ((uint64_t)n << gshift) / 256 + 1;
    const uint64_t cap = (uint64_t)ctx->num_cu * 16;
    if (blocks > cap) blocks = cap;
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    const uint8_t* sp = static_cast<const uint8_t*>(src);
    uint8_t* dp = static_cast<uint8_t*>(dst);
    const uint8_t* pp = static_cast<const uint8_t*>(proxy);
    switch (w) {
        case 16: hipLaunchKernelGGL(rsx_row_gather_kernel<uint4>, dim3((uint32_t)blocks), dim3(256), 0, st, sp, dp, words, pp, p, idx_off, (uint64_t)n, gshift); break;
        case 8: hipLaunchKernelGGL(rsx_row_gather_kernel<uint2>, dim3((uint32_t)blocks), dim3(256), 0, st, sp, dp, words, pp, p, idx_off, (uint64_t)n, gshift); break;
        case 4: hipLaunchKernelGGL(rsx_row_gather_kernel<uint32_t>, dim3((uint32_t)blocks), dim3(256), 0, st, sp, dp, words, pp, p, idx_off, (uint64_t)n, gshift); break;
        case 2: hipLaunchKernelGGL(rsx_row_gather_kernel<uint16_t>, dim3((uint32_t)blocks), dim3(256), 0, st, sp, dp, words, pp, p, idx_off, (uint64_t)n, gshift); break;
        default: hipLaunchKernelGGL(rsx_row_gather_kernel<uint8_t>, dim3((uint32_t)blocks), dim3(256), 0, st, sp, dp, words, pp, p, idx_off, (uint64_t)n, gshift); break;
    }
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}

// rsx_sort_device's body for every layout: a layout with kernels of its own goes straight to sort_device_locked (the
// same launches as ever), any other one through route 1 or 2.  Caller holds ctx->mu and has set the device.
int sort_any_locked(rsx_ctx* ctx, void* d_data, void* d_tmp, size_t n, const rsx_layout* L, hipStream_t st) {
    if (direct_layout(L)) return sort_device_locked(ctx, d_data, d_tmp, n, L, st);
    const AnyPlan P = any_plan(L);
    if (P.route == 2 && (uint64_t)n >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more elements wider than 32 bytes");
    int rc = pending_error(ctx);
    if (rc) return rc;
    rc = reserve_any(ctx, n, L, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this sort from the first launch on
    char* w0 = ctx->any_buf;
    char* w1 = ctx->any_buf + round256(n * (size_t)P.inner.elem_bytes);
    const uint32_t s = L->elem_bytes, sp = P.inner.elem_bytes;
    if (P.route == 1) {
        rc = launch_move(ctx, d_data, s, w0, sp, nullptr, n, map_forward(L, P), st);
        if (rc) return rc;
        rc = sort_device_locked(ctx, w0, w1, n, &P.inner, st);
        if (rc) return rc;
        rc = launch_move(ctx, w0, sp, d_data, s, nullptr, n, map_restore(L, P), st);
    } else {
        rc = launch_move(ctx, d_data, s, w0, sp, d_tmp, n, map_forward(L, P), st);
        if (rc) return rc;
        rc = sort_device_locked(ctx, w0, w1, n, &P.inner, st);
        if (rc) return rc;
        rc = launch_gather(ctx, d_tmp, d_data, s, w0, sp, P.idx_off, n, st);
    }
    if (rc) return rc;
    ctx->last_route = P.route;
    return RSX_OK;
}


// ---- separate key and value arrays (include/rsx.h: rsx_sort_pairs_device, rsx_argsort_device) ----
// Both calls sort JOINED elements in the context's second workspace: the mapped key (complemented for descending order)
// at offset 0, sorted as RSX_KEY_UNSIGNED by the kernels every other call uses, with
//   route 1, joined elements: the value (or, for argsort, the element's position) behind the key, when the two fit an
//     element size with sort kernels (rsx_pairs_kernels.hpp, pairs_elem); join, sort, split;
//   route 2, proxies and gather: (mapped key, u32 position) proxies for wider values; the keys are written from the
//     sorted proxies and the values gathered through a copy kept behind the two proxy arrays.
// The two arrays of n joined elements every such call sorts in, at the front of the second workspace; what a call keeps
// behind them it takes from `ws`.
struct JoinedPlan {
    size_t n;
    uint32_t vb;       // bytes of the value inside the element
    rsx_layout inner;  // what the sort kernels see (elem_bytes 0: no joined element for these widths)
    size_t half;       // bytes of each of the two element arrays: the second one's offset
    Carve ws;          // ws.bytes: the whole workspace of the call
};
JoinedPlan joined_plan(size_t n, uint32_t kb, uint32_t vb) {
    JoinedPlan P{};
    const uint32_t es = pairs_elem_bytes(kb, vb);
    P.n = n;
    P.vb = vb;
    P.inner = rsx_layout{es, 0, kb, RSX_KEY_UNSIGNED};
    P.ws.take(n * (size_t)es);
    P.half = P.ws.take(n * (size_t)es);
    return P;
}
int reserve_joined(rsx_ctx* ctx, const JoinedPlan& P, hipStream_t st) {
    int rc = ensure_workspace(ctx, P.n, &P.inner, st);
    if (rc) return rc;
    return ensure_any(ctx, P.ws.bytes, st);
}
// a reserve entry's body once its arguments are checked: a joined sort's two workspaces, or `bytes` of the second alone
int reserve_joined_entry(rsx_ctx* ctx, const JoinedPlan& P) {
    RSX_ENTER(nullptr);
    return reserve_joined(ctx, P, nullptr);
}
int reserve_any_entry(rsx_ctx* ctx, size_t bytes) {
    RSX_ENTER(nullptr);
    int rc = ensure_aux(ctx, nullptr);
    if (rc) return rc;
    return ensure_any(ctx, bytes, nullptr);
}
// Joins keys and values (gen: every key's position) into the first array and sorts them there; *w0 receives the sorted
// elements.  The caller has reserved P (reserve_joined) and opened its Enqueue, in that order.
int joined_sort(rsx_ctx* ctx, const JoinedPlan& P, const void* d_keys, const void* d_values, bool gen, uint32_t kind, uint32_t desc, hipStream_t st,
                char** w0) {
    char* w = ctx->any_buf;
    int rc = launch_pairs_join(ctx, d_keys, d_values, w, P.n, P.inner.key_bytes, P.vb, gen, kind, desc, st);
    if (rc) return rc;
    if (P.n > 1) {
        rc = sort_device_locked(ctx, w, w + P.half, P.n, &P.inner, st);
        if (rc) return rc;
    }
    ctx->last_pairs = 1u | P.inner.elem_bytes << 8;
    *w0 = w;
    return RSX_OK;
}
struct PairsPlan {
    uint32_t route;
    JoinedPlan j;     // route 2: (mapped key, u32 position) proxies
    size_t copy_off;  // route 2: the copy of the values, behind the two proxy arrays
};
// route 2 for n values of vb bytes (the segmented calls take it for every width without a fused kernel)
PairsPlan proxy_plan(size_t n, uint32_t kb, uint32_t vb) {
    PairsPlan P{2u, joined_plan(n, kb, 4), 0};
    P.copy_off = P.j.ws.take(n * (size_t)vb);
    return P;
}
PairsPlan pairs_plan(size_t n, uint32_t kb, uint32_t vb) {
    if (!pairs_elem_bytes(kb, vb)) return proxy_plan(n, kb, vb);
    return PairsPlan{1u, joined_plan(n, kb, vb), 0};
}
bool key_widths_ok(uint32_t kb, uint32_t kind) {  // the key array as a layout of its own
    const rsx_layout L{kb, 0, kb, kind};
    return layout_ok(&L);
}
// ---- the segmented forms of those calls (rsx_segment_pairs_kernels.hpp): values with a fused kernel, or positions ----
// the joined element the fused kernels sort: the value itself, or a four-byte position (argsort; values too wide to join)
uint32_t segment_pairs_elem(uint32_t kb, uint32_t vb, bool argsort) {
    return pairs_elem_bytes(kb, (!argsort && value_width_fused(vb)) ? vb : 4u);
}
uint32_t value_align(uint32_t vb) {
    uint32_t a = 1;
    while (a < 16 && vb % (2 * a) == 0) a *= 2;
    return a;
}

// d_index != nullptr: argsort (d_keys only read, d_values unused, ib = index bytes); otherwise keys and values (vb == 0:
// keys only) sorted in place.  Caller holds ctx->mu, has set the device and checked the arguments; n >= 2.
int pairs_locked(rsx_ctx* ctx, void* d_keys, void* d_values, void* d_index, size_t n, uint32_t kb, uint32_t kind, uint32_t vb, uint32_t ib,
                 uint32_t desc, hipStream_t st) {
    const bool argsort = d_index != nullptr;
    const uint32_t pw = (uint64_t)n < (1ull << 32) ? 4u : 8u;  // bytes of a position
    if (argsort && ib < pw) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys need 8-byte indices");
    const PairsPlan P = pairs_plan(n, kb, argsort ? pw : vb);
    if (P.route == 2 && (uint64_t)n >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more pairs with values too wide to join");
    int rc = pending_error(ctx);
    if (rc) return rc;
    rc = reserve_joined(ctx, P.j, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* w0 = ctx->any_buf;
    const uint32_t es = P.j.inner.elem_bytes;
    if (!argsort && vb == 0 && !desc) {  // ascending keys alone: the sort of one array, the workspace as its ping-pong
        const rsx_layout L{kb, 0, kb, kind};
        rc = sort_device_locked(ctx, d_keys, w0, n, &L, st);
        if (rc) return rc;
        ctx->last_pairs = 1u | es << 8;
        return RSX_OK;
    }
    if (P.route == 1) {
        rc = joined_sort(ctx, P.j, d_keys, d_values, argsort, kind, desc, st, &w0);
        if (rc) return rc;
        if (argsort) rc = launch_pairs_split(ctx, w0, nullptr, d_index, n, kb, P.j.vb, 2, ib, kind, desc, st);
        else rc = launch_pairs_split(ctx, w0, d_keys, d_values, n, kb, P.j.vb, 0, 0, kind, desc, st);
    } else {  // (the copy of the values stands between the join and the sort: not joined_sort)
        char* cp = w0 + P.copy_off;
        rc = launch_pairs_join(ctx, d_keys, nullptr, w0, n, kb, 4, true, kind, desc, st);
        if (rc) return rc;
        RSX_HIP(hipMemcpyAsync(cp, d_values, n * (size_t)vb, hipMemcpyDeviceToDevice, st));
        rc = sort_device_locked(ctx, w0, w0 + P.j.half, n, &P.j.inner, st);
        if (rc) return rc;
        rc = launch_pairs_split(ctx, w0, d_keys, nullptr, n, kb, 4, 1, 0, kind, desc, st);
        if (rc) return rc;
        rc = launch_gather(ctx, cp, d_values, vb, w0, es, pairs_value_offset(kb, 4), n, st);
    }
    if (rc) return rc;
    ctx->last_pairs = P.route | es << 8;
    return RSX_OK;
}

}  // namespace

extern "C" {

int rsx_version(void) { return RSX_VERSION; }

const char* rsx_strerror(int status) {
    switch (status) {
        case RSX_OK: return "ok";
        case RSX_ERR_ARG: return "invalid argument";
        case RSX_ERR_UNSUPPORTED: return "unsupported element layout";
        case RSX_ERR_HIP: return "HIP runtime error";
        case RSX_ERR_NOMEM: return "out of device memory";
        case RSX_ERR_NODEVICE: return "no usable device";
        case RSX_ERR_WORKSPACE: return "workspace not reserved";
        case RSX_ERR_INTERNAL: return "device-side protocol error";
        default: return "unknown status";
    }
}

const char* rsx_last_error(const rsx_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int rsx_ctx_create(int device, rsx_ctx** out) try {
    if (!out) return RSX_ERR_ARG;
    *out = nullptr;
    const char* verbose = std::getenv("RSX_VERBOSE");
    const bool loud = verbose && verbose[0] && verbose[0] != '0';
    int count = 0;
    hipError_t he = hipGetDeviceCount(&count);
    if (he != hipSuccess || count <= 0) {
        if (loud) std::fprintf(stderr, "[rsx] hipGetDeviceCount: %s (count %d)\n", hipGetErrorString(he), count);
        return RSX_ERR_NODEVICE;
    }
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) return RSX_ERR_NODEVICE;
    }
    if (device >= count) return RSX_ERR_NODEVICE;
    rsx_ctx* ctx = new (std::nothrow) rsx_ctx();
    if (!ctx) return RSX_ERR_NOMEM;
    ctx->device = device;
    if (loud) ctx->options |= OPT_VERBOSE;
#ifdef RSX_TUNING  // timing ablations exist in tuning builds only (some give wrong output by design)
    if (const char* dbg = std::getenv("RSX_DEBUG")) ctx->dbg = (uint32_t)std::strtoul(dbg, nullptr, 0);
#endif
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {  // code objects are gfx950-only
            if (loud) std::fprintf(stderr, "[rsx] device %d is %s, not gfx950\n", device, prop.gcnArchName);
            delete ctx;
            return RSX_ERR_NODEVICE;
        }
    }
    *out = ctx;
    return RSX_OK;
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_ctx_destroy(rsx_ctx* ctx) try {
    if (!ctx) return RSX_ERR_ARG;
    {
        DeviceGuard g(ctx->device);
        if (ctx->busy && ctx->last_event) (void)hipEventSynchronize(ctx->last_event);
        if (ctx->status) (void)hipFree(ctx->status);
        if (ctx->aux) (void)hipFree(ctx->aux);
        if (ctx->host_err) (void)hipHostFree(ctx->host_err);
        if (ctx->last_event) (void)hipEventDestroy(ctx->last_event);
        for (void* p : ctx->host_buf)
            if (p) (void)hipFree(p);
        for (void* p : ctx->pinned)
            if (p) (void)hipHostFree(p);
        if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
        for (hipEvent_t e : ctx->copy_event)
            if (e) (void)hipEventDestroy(e);
        if (ctx->part_J) (void)hipFree(ctx->part_J);
        if (ctx->ovf16) (void)hipFree(ctx->ovf16);
        if (ctx->wide_buf) (void)hipFree(ctx->wide_buf);
        if (ctx->any_buf) (void)hipFree(ctx->any_buf);
        if (ctx->shard_q) (void)hipFree(ctx->shard_q);
        if (ctx->shard_out) (void)hipFree(ctx->shard_out);
        if (ctx->shard_hist) (void)hipFree(ctx->shard_hist);
        if (ctx->shard_host) (void)hipHostFree(ctx->shard_host);
        if (ctx->shard_stream) (void)hipStreamDestroy(ctx->shard_stream);
        for (int k = 0; k < RSX_PROF_KINDS; ++k)
            for (auto& e : ctx->prof_pending[k]) ctx->prof_free.push_back(e);
        for (auto& e : ctx->prof_free) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    }
    delete ctx;
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve(rsx_ctx* ctx, size_t n, const rsx_layout* layout) try {
    int rc = check_any(ctx, layout);
    if (rc) return rc;
    RSX_ENTER(nullptr);
    if (!direct_layout(layout)) return reserve_any(ctx, n, layout, nullptr);
    return ensure_workspace(ctx, n, layout, nullptr);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_ctx_check(rsx_ctx* ctx, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    RSX_ENTER(nullptr);
    RSX_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    if (!ctx->host_err) return RSX_OK;
    if (host_word(ctx, HV_ERROR)) {
        if (ctx->busy) (void)hipEventSynchronize(ctx->last_event);  // nothing of this context may still be running
        host_word(ctx, HV_ERROR) = 0;
        return fail(ctx, RSX_ERR_INTERNAL, "look-back spin gave up, or an atomic rank failed its cross-check (device protocol error)");
    }
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_set_option(rsx_ctx* ctx, int option, uint64_t value) try {
    if (!ctx) return RSX_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto flag = [&](uint32_t bit, bool on) { ctx->options = on ? (ctx->options | bit) : (ctx->options & ~bit); };
    switch (option) {
        case RSX_OPT_TILE_SCHEDULE:
            if (value > 1) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_TILE_SCHEDULE: 0 (roll call) or 1 (tickets)");
            flag(OPT_DYNAMIC_TILES, value == 1);
            return RSX_OK;
        case RSX_OPT_RANKING:
            if (value > 2) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_RANKING: 0 (auto), 1 (ballots) or 2 (LDS atomics)");
            flag(OPT_BALLOT_RANKS, value == 1);
            flag(OPT_ATOMIC_RANKS, value == 2);
            return RSX_OK;
        case RSX_OPT_STATUS_SCOPE:
            if (value > 1) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_STATUS_SCOPE: 0 (auto) or 1 (agent)");
            flag(OPT_AGENT_STATUS, value == 1);
            return RSX_OK;
        case RSX_OPT_XCD_MAJOR:
            if (value > 1) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_XCD_MAJOR: 0 or 1");
            flag(OPT_NO_XCD_MAJOR, value == 0);
            return RSX_OK;
        case RSX_OPT_BYTE_COUNTING:
            if (value > 1) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_BYTE_COUNTING: 0 or 1");
            flag(OPT_GENERAL_BYTES, value == 0);
            return RSX_OK;
        case RSX_OPT_MAX_REGIONS:
            if (value > (uint64_t)MAX_REGIONS) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_MAX_REGIONS: 0 (default) .. 32");
            ctx->max_regions = (uint32_t)value;
            return RSX_OK;
        case RSX_OPT_HOT_LANES:
            if (value < 2 || value > 65) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_HOT_LANES: 2 .. 65");
            ctx->hot_lanes = (uint32_t)value;
            return RSX_OK;
        case RSX_OPT_VERBOSE:
            flag(OPT_VERBOSE, value != 0);
            return RSX_OK;
        case RSX_OPT_RANK_CHECK:
            flag(OPT_RANK_CHECK, value != 0);
            return RSX_OK;
        case RSX_OPT_SMALL_SORT:
            if (value > 1) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_SMALL_SORT: 0 or 1");
            flag(OPT_NO_SMALL_SORT, value == 0);
            return RSX_OK;
        case RSX_OPT_WIDE_SORT:
            if (value > 3) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_WIDE_SORT: 0 (off), 1 (auto), 2 (always) or 3 (auto from 2^22 elements on)");
            ctx->wide_mode = (uint32_t)value;
            ctx->wide_skip = 0;  // setting the option forgets an earlier refusal
            if (ctx->host_err) host_word(ctx, HV_WIDE_HINT) = 0;
            return RSX_OK;
        case RSX_OPT_BUCKET_SKIP:
            if (value > 1) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_BUCKET_SKIP: 0 or 1");
            ctx->bucket_no_skip = value == 0 ? 1u : 0u;
            return RSX_OK;
        case RSX_OPT_BUCKET_GROUP:
            if (value > 1) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_BUCKET_GROUP: 0 or 1");
            ctx->bucket_group = (uint32_t)value;
            return RSX_OK;
        case RSX_OPT_BUCKET_DIRECT:
            if (value > 1) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_BUCKET_DIRECT: 0 or 1");
            ctx->bucket_direct = (uint32_t)value;
            return RSX_OK;
        case RSX_OPT_HOST_CHUNK:
            if (value < 4096 || value > (uint64_t)HOST_CHUNK || value % 4096)
                return fail(ctx, RSX_ERR_ARG, "RSX_OPT_HOST_CHUNK: a multiple of 4096 in 4096 .. 32 MiB");
            ctx->host_chunk = (size_t)value;
            return RSX_OK;
        case RSX_OPT_MID_SORT:
            if (value > 3) return fail(ctx, RSX_ERR_ARG, "RSX_OPT_MID_SORT: 0 (off), 1 (forecast), 2 (always split) or 3 (always LSD passes)");
            flag(OPT_NO_MID_SORT, value == 0);
            ctx->mid_force = value >= 2 ? (uint32_t)value - 1u : 0u;
            return RSX_OK;
        default:
            return fail(ctx, RSX_ERR_ARG, "unknown option");
    }
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_ctx_get_info(rsx_ctx* ctx, int what, uint64_t* out) try {
    if (!ctx || !out) return RSX_ERR_ARG;
    RSX_ENTER(nullptr);
    if (what == RSX_INFO_RANK_ATOMIC || what == RSX_INFO_L2_LOCAL) {
        int rc = ensure_aux(ctx, nullptr);  // runs the self-tests on first use
        if (rc) return rc;
    }
    switch (what) {
        case RSX_INFO_RANK_ATOMIC: *out = ctx->rank_atomic ? 1 : 0; return RSX_OK;
        case RSX_INFO_L2_LOCAL: *out = ctx->l2_local ? 1 : 0; return RSX_OK;
        case RSX_INFO_NUM_CU: *out = (uint64_t)ctx->num_cu; return RSX_OK;
        case RSX_INFO_DEVICE: *out = (uint64_t)ctx->device; return RSX_OK;
        case RSX_INFO_LAST_PASSES: {
            switch (ctx->last_path) {
                case PATH_SEGMENTS: case PATH_TOPK: case PATH_UNIQUE: case PATH_REDUCE:  // bits 0-7 are the kernels launched
                    *out = (uint64_t)(ctx->last_sort_passes & 0xFFu) | (uint64_t)ctx->last_path << 24;
                    return RSX_OK;
                case PATH_SEARCH:  // bits 0-7 the kernels launched after any sort, bit 8 the needles were sorted first
                case PATH_SETOP:   // bits 0-7 the kernels launched
                case PATH_JOIN:    // bits 0-7 the kernels launched
                case PATH_MERGE:   // bits 0-7 the kernels launched, bit 8 the wide-value route
                case PATH_SCAN:    // bits 0-7 the kernels launched after any sort, bit 8 RSX_SCAN_RUNS
                    *out = (uint64_t)(ctx->last_sort_passes & 0x1FFu) | (uint64_t)ctx->last_path << 24;
                    return RSX_OK;
                case PATH_SELECT: {  // bits 0-7 the kernels launched, bits 8-11 what the device's plan says of the compaction
                    uint32_t compacted = 0;
                    if (ctx->last_sort_passes && ctx->any_buf) {
                        if (ctx->busy) RSX_HIP(hipEventSynchronize(ctx->last_event));
                        RSX_HIP(hipMemcpy(&compacted, ctx->any_buf + offsetof(SelectState, compacted), sizeof compacted, hipMemcpyDeviceToHost));
                    }
                    *out = (uint64_t)(ctx->last_sort_passes & 0xFFu) | (uint64_t)(compacted & 0xFu) << 8 | (uint64_t)ctx->last_path << 24;
                    return RSX_OK;
                }
                case PATH_BIN:      // bits 0-7 the kernels launched; the path takes bit 28, a bin count has no route
                case PATH_COMPACT:  // the same: bits 0-7 the kernels launched, the path in bits 24-28
                case PATH_MSPLIT:   // the same
                case PATH_BINRED:   // the same
                    *out = (uint64_t)(ctx->last_sort_passes & 0xFFu) | (uint64_t)ctx->last_path << 24;
                    return RSX_OK;
                default: break;
            }
            *out = (uint64_t)ctx->last_path << 24 | (uint64_t)ctx->last_route << 28;
            if (!ctx->aux || ctx->last_sort_passes == 0) return RSX_OK;
            if (ctx->busy) RSX_HIP(hipEventSynchronize(ctx->last_event));
            uint64_t stat = 0, placed = 0;
            uint32_t path = ctx->last_path, passes = ctx->last_sort_passes;
            if (path == PATH_WIDE && ctx->wide_buf) {  // both sequences were enqueued: the device's verdict says which one ran
                uint32_t verdict = 0;
                RSX_HIP(hipMemcpy(&verdict, reinterpret_cast<char*>(ctx->wide_buf) + WIDE_PLAN_OFFSET, sizeof verdict, hipMemcpyDeviceToHost));
                if ((verdict & VERDICT_PATH_MASK) == VERDICT_HYBRID) passes = 2;
                else path = PATH_LSD;
            }
            for (uint32_t p = 0; p < passes && p < (uint32_t)MAX_PASSES; ++p) {
                uint32_t mode = 0;  // the roll call's verdict word: 1 static, 3 static + placement verified, 2 / 0 tickets
                RSX_HIP(hipMemcpy(&mode, reinterpret_cast<uint32_t*>(cb_of(ctx, ctx->cb_last) + CB_TICKETS) + (size_t)p * TICKET_WORDS + ROLL_MODE,
                                  sizeof mode, hipMemcpyDeviceToHost));
                stat += (mode == 1u || mode == 3u) ? 1u : 0u;
                placed += mode == 3u ? 1u : 0u;
            }
            *out = (uint64_t)passes | (stat << 8) | (placed << 16) | ((uint64_t)path << 24) | ((uint64_t)ctx->last_route << 28);
            return RSX_OK;
        }
        case RSX_INFO_LAST_PAIRS: *out = (uint64_t)ctx->last_pairs; return RSX_OK;
        case RSX_INFO_LAST_LEX: *out = (uint64_t)ctx->last_lex; return RSX_OK;
        case RSX_INFO_LAST_DIRECT: {
            *out = ~(uint64_t)0;
            if (ctx->last_path != PATH_WIDE || !ctx->last_direct || !ctx->wide_buf) return RSX_OK;
            if (ctx->busy) RSX_HIP(hipEventSynchronize(ctx->last_event));
            uint32_t verdict = 0, left = 0;  // (both sequences were enqueued: a hybrid the device refused ran no direct kernel)
            RSX_HIP(hipMemcpy(&verdict, ctx->wide_buf + WIDE_PLAN_OFFSET, sizeof verdict, hipMemcpyDeviceToHost));
            if ((verdict & VERDICT_PATH_MASK) != VERDICT_HYBRID) return RSX_OK;
            RSX_HIP(hipMemcpy(&left, ctx->wide_buf + WIDE_LEFT_OFFSET, sizeof left, hipMemcpyDeviceToHost));
            *out = (uint64_t)left;
            return RSX_OK;
        }
        default: return fail(ctx, RSX_ERR_ARG, "unknown info id");
    }
} catch (...) {
    return RSX_ERR_HIP;
}

// Diagnostic counters of the sweep kernel (RSX_TUNING builds, RSX_DEBUG & 0x100); not part of include/rsx.h.
int rsx_debug_counters(rsx_ctx* ctx, unsigned long long* out128, int reset) try {
    if (!ctx || !out128 || !ctx->aux) return RSX_ERR_ARG;
    RSX_ENTER(nullptr);
    RSX_HIP(hipDeviceSynchronize());
    RSX_HIP(hipMemcpy(out128, ctx->aux + OFF_DBG, 1024, hipMemcpyDeviceToHost));  // caller passes 128 u64
    if (reset) RSX_HIP(hipMemset(ctx->aux + OFF_DBG, 0, 1024));
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_profile(rsx_ctx* ctx, int enable) try {
    if (!ctx) return RSX_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (enable) {
        for (int k = 0; k < RSX_PROF_KINDS; ++k) {
            for (auto& e : ctx->prof_pending[k]) ctx->prof_free.push_back(e);
            ctx->prof_pending[k].clear();
            ctx->prof_ms[k] = 0;
            ctx->prof_n[k] = 0;
        }
    }
    ctx->prof = enable != 0;
    return RSX_OK;
} catch (...) {
    return RSX_ERR_NOMEM;
}

// Durations (ms) of the sweep launches read by rsx_ctx_profile_read so far, in launch order (diagnostics;
// not part of include/rsx.h).  Returns how many were written; clears the list.
int rsx_debug_sweep_times(rsx_ctx* ctx, float* out, int max) try {
    if (!ctx || !out) return RSX_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    int n = 0;
    for (float t : ctx->prof_each) {
        if (n >= max) break;
        out[n++] = t;
    }
    ctx->prof_each.clear();
    return n;
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_ctx_profile_read(rsx_ctx* ctx, double* ms, uint64_t* launches) try {
    if (!ctx || !ms || !launches) return RSX_ERR_ARG;
    RSX_ENTER(nullptr);
    for (int k = 0; k < RSX_PROF_KINDS; ++k) {
        for (auto& e : ctx->prof_pending[k]) {
            RSX_HIP(hipEventSynchronize(e.second));
            float t = 0;
            RSX_HIP(hipEventElapsedTime(&t, e.first, e.second));
            ctx->prof_ms[k] += t;
            ctx->prof_n[k] += 1;
            if (k == RSX_PROF_SWEEP && ctx->prof_each.size() < 4096) ctx->prof_each.push_back(t);
            ctx->prof_free.push_back(e);
        }
        ctx->prof_pending[k].clear();
        ms[k] = ctx->prof_ms[k];
        launches[k] = ctx->prof_n[k];
    }
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_sort_device(rsx_ctx* ctx, void* d_data, void* d_tmp, size_t n, const rsx_layout* L, void* stream) try {
    int rc = check_any(ctx, L);
    if (rc) return rc;
    if (n <= 1) return RSX_OK;  // reference panics on n == 0 (mod.rs:66-70,92); nothing to compare
    if (!d_data || !d_tmp) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (direct_layout(L)) {  // (the other layouts are read and written at any alignment)
        const uint32_t al = elem_align(L->elem_bytes);
        if (!aligned(d_data, al) || !aligned(d_tmp, al)) return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    }
    RSX_ENTER(stream);
    return sort_any_locked(ctx, d_data, d_tmp, n, L, held.st);
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_pairs(rsx_ctx* ctx, size_t n, uint32_t key_bytes, uint32_t value_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED) || value_bytes > RSX_MAX_ELEM_BYTES) return fail(ctx, RSX_ERR_ARG, "invalid key or value width");
    RSX_ENTER(nullptr);
    int rc = reserve_joined(ctx, pairs_plan(n, key_bytes, value_bytes).j, nullptr);
    // an argsort with 8-byte indices joins 4-byte positions while n < 2^32: another element size
    if (!rc && value_bytes == 8 && (uint64_t)n < (1ull << 32)) rc = reserve_joined(ctx, pairs_plan(n, key_bytes, 4).j, nullptr);
    // the segmented calls keep values without a fused kernel behind four-byte positions, whatever their width
    if (!rc && !value_width_fused(value_bytes)) rc = ensure_any(ctx, proxy_plan(n, key_bytes, value_bytes).j.ws.bytes, nullptr);
    return rc;
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_sort_pairs_device(rsx_ctx* ctx, void* d_keys, void* d_values, size_t n, uint32_t key_bytes, uint32_t key_kind, uint32_t value_bytes,
                          int order, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    if (value_bytes > RSX_MAX_ELEM_BYTES) return fail(ctx, RSX_ERR_ARG, "value wider than RSX_MAX_ELEM_BYTES");
    uint32_t desc = 0;
    if (int rc = order_desc(ctx, order, &desc)) return rc;
    if ((d_values == nullptr) != (value_bytes == 0) && (n > 0 || d_values != nullptr)) return fail(ctx, RSX_ERR_ARG, "d_values and value_bytes disagree");
    if (n == 0) return RSX_OK;
    if (!d_keys) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!aligned(d_keys, key_bytes) || (value_bytes && !aligned(d_values, value_align(value_bytes)))) return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    if (n == 1) return RSX_OK;
    RSX_ENTER(stream);
    return pairs_locked(ctx, d_keys, d_values, nullptr, n, key_bytes, key_kind, value_bytes, 0, desc, held.st);
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_argsort_device(rsx_ctx* ctx, const void* d_keys, void* d_index, size_t n, uint32_t key_bytes, uint32_t key_kind, uint32_t index_bytes,
                       int order, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    if (int rc = check_index_bytes(ctx, index_bytes)) return rc;
    uint32_t desc = 0;
    if (int rc = order_desc(ctx, order, &desc)) return rc;
    if (n == 0) return RSX_OK;
    if (!d_keys || !d_index) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!aligned(d_keys, key_bytes) || !aligned(d_index, index_bytes)) return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (n == 1) {  // the one position
        RSX_HIP(hipMemsetAsync(d_index, 0, index_bytes, st));
        return RSX_OK;
    }
    return pairs_locked(ctx, const_cast<void*>(d_keys), nullptr, d_index, n, key_bytes, key_kind, 0, index_bytes, desc, st);
} catch (...) {
    return RSX_ERR_HIP;
}

// Shared body of rsx_sort_segments_device (d_offsets) and rsx_sort_rows_device (d_offsets == nullptr, nseg rows of row_len).
namespace {
// Rows above what a workgroup holds in LDS (cap, the largest class): the whole-array call, row by row (the context's
// workspace as for any sort).  Only where every CU has a row of its own and the rows are short enough for one workgroup's
// passes through memory to beat a launch sequence per row does the through-memory class take them (measured, DESIGN
// section 5: 4681 rows of 28673 u32 12 ms against 121 ms; the two meet at some 10 x cap elements per row).
bool rows_one_by_one(const rsx_ctx* ctx, size_t nseg, uint64_t row_len, uint64_t cap) {
    return row_len > cap && !(nseg >= (size_t)ctx->num_cu && row_len <= 4 * cap);
}
int sort_segments_common(rsx_ctx* ctx, void* d_data, void* d_tmp, size_t n, const rsx_layout* L, const uint64_t* d_offsets, size_t nseg,
                         uint64_t row_len, uint64_t max_len, void* stream) {
    int rc = check_common(ctx, L);
    if (rc) return rc;
    if (nseg == 0 || (!d_offsets && row_len <= 1)) return RSX_OK;
    if (!d_data || !d_tmp) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    const uint32_t al = elem_align(L->elem_bytes);
    if (!aligned(d_data, al) || !aligned(d_tmp, al) || !aligned(d_offsets, 8)) return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    const uint64_t cap = segment_cap((int)L->elem_bytes, RSX_SEG_CLASSES - 1);
    if (!d_offsets && rows_one_by_one(ctx, nseg, row_len, cap)) {
        for (size_t i = 0; i < nseg; ++i) {
            const size_t off = i * (size_t)row_len * L->elem_bytes;
            rc = sort_device_locked(ctx, static_cast<char*>(d_data) + off, static_cast<char*>(d_tmp) + off, (size_t)row_len, L, st);
            if (rc) return rc;
        }
        return RSX_OK;
    }
    rc = pending_error(ctx);
    if (rc) return rc;
    rc = ensure_aux(ctx, st);  // (the error word and the ranking self-test: a context's first call, never a captured one)
    if (rc) return rc;
    Enqueue enq(ctx, st);
    uint32_t launched = 0;
    rc = launchers_for(L->elem_bytes)->segment_sort(ctx, d_data, d_tmp, n, L, d_offsets, nseg, row_len, max_len, &launched, st);
    note_path(ctx, PATH_SEGMENTS, launched);
    return rc;
}
}  // namespace

int rsx_sort_segments_device(rsx_ctx* ctx, void* d_data, void* d_tmp, size_t n, const rsx_layout* L, const uint64_t* d_offsets, size_t nseg,
                             uint64_t max_seg_len, void* stream) try {
    if (ctx && nseg != 0 && !d_offsets) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    return sort_segments_common(ctx, d_data, d_tmp, n, L, d_offsets, nseg, 0, max_seg_len, stream);
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_sort_rows_device(rsx_ctx* ctx, void* d_data, void* d_tmp, size_t rows, size_t row_len, const rsx_layout* L, void* stream) try {
    if (ctx && rows != 0 && row_len > SIZE_MAX / rows) return fail(ctx, RSX_ERR_ARG, "rows * row_len overflows");
    if (ctx && L && L->elem_bytes != 0 && rows != 0 && rows * row_len > SIZE_MAX / L->elem_bytes) return fail(ctx, RSX_ERR_ARG, "rows * row_len overflows");
    return sort_segments_common(ctx, d_data, d_tmp, rows * row_len, L, nullptr, rows, row_len, 0, stream);
} catch (...) {
    return RSX_ERR_HIP;
}

// ---- many segments of separate key and value columns (include/rsx.h) ----
// Shared body of rsx_sort_segments_pairs_device / rsx_argsort_segments_device (d_offsets) and their row forms (d_offsets ==
// nullptr, nseg rows of row_len).  d_index != nullptr: argsort.
namespace {

int segments_pairs_common(rsx_ctx* ctx, void* d_keys, void* d_values, void* d_index, bool argsort, size_t n, uint32_t kb, uint32_t kind, uint32_t vb,
                          uint32_t ib, int order, const uint64_t* d_offsets, bool rows, size_t nseg, uint64_t row_len, uint64_t max_len, void* stream) {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(kb, kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    int rc = argsort ? check_index_bytes(ctx, ib) : RSX_OK;
    if (rc) return rc;
    if (!argsort && vb > RSX_MAX_ELEM_BYTES) return fail(ctx, RSX_ERR_ARG, "value wider than RSX_MAX_ELEM_BYTES");
    uint32_t desc = 0;
    rc = order_desc(ctx, order, &desc);
    if (rc) return rc;
    if (!argsort && (d_values == nullptr) != (vb == 0)) return fail(ctx, RSX_ERR_ARG, "d_values and value_bytes disagree");
    if (nseg == 0 || n == 0 || (rows && row_len == 0)) return RSX_OK;
    if (rows && row_len == 1 && !argsort) return RSX_OK;
    if (!rows && !d_offsets) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!d_keys || (argsort && !d_index)) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!aligned(d_keys, kb) || (argsort && !aligned(d_index, ib)) || (vb && !aligned(d_values, value_align(vb))) || !aligned(d_offsets, 8))
        return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (rows && row_len == 1) {  // argsort: every row's one position
        RSX_HIP(hipMemsetAsync(d_index, 0, n * (size_t)ib, st));
        return RSX_OK;
    }
    const bool wide = !argsort && !value_width_fused(vb);  // route B: positions and a gather
    const uint32_t es = segment_pairs_elem(kb, vb, argsort);
    if (es == 0 || !launchers_for(es)) return fail(ctx, RSX_ERR_INTERNAL, "no joined element for these widths");
    if (wide && (uint64_t)n >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more pairs with values too wide to join");
    if (rows && rows_one_by_one(ctx, nseg, row_len, segment_cap((int)es, RSX_SEG_CLASSES - 1))) {
        for (size_t i = 0; i < nseg; ++i) {
            const size_t off = i * (size_t)row_len;
            char* k = static_cast<char*>(d_keys) + off * kb;
            if (argsort) rc = pairs_locked(ctx, k, nullptr, static_cast<char*>(d_index) + off * ib, (size_t)row_len, kb, kind, 0, ib, desc, st);
            else rc = pairs_locked(ctx, k, vb ? static_cast<char*>(d_values) + off * vb : nullptr, nullptr, (size_t)row_len, kb, kind, vb, 0, desc, st);
            if (rc) return rc;
        }
        return RSX_OK;
    }
    rc = pending_error(ctx);
    if (rc) return rc;
    const bool mem = segment_pairs_mem(es, d_offsets, row_len, max_len);
    // either way two arrays of n elements of es bytes; route B keeps the copy of the values behind them
    const PairsPlan P = wide ? proxy_plan(n, kb, vb) : pairs_plan(n, kb, argsort ? 4u : vb);
    if (wide) {
        rc = ensure_aux(ctx, st);
        if (!rc) rc = ensure_any(ctx, P.j.ws.bytes, st);
    } else if (mem) {
        rc = reserve_joined(ctx, P.j, st);
    } else {
        rc = ensure_aux(ctx, st);  // (the error word and the ranking self-test: a context's first call, never a captured one)
    }
    if (rc) return rc;
    Enqueue enq(ctx, st);
    char* w0 = (wide || mem) ? ctx->any_buf : nullptr;
    char* w1 = w0 ? w0 + P.j.half : nullptr;
    SegPairsCall c{};
    c.keys = d_keys;
    c.values = argsort ? d_index : wide ? static_cast<void*>(w0) : d_values;
    c.w0 = w0;
    c.w1 = w1;
    c.n = n;
    c.kb = kb;
    c.vb = (argsort || wide) ? 4u : vb;
    c.kind = kind;
    c.desc = desc;
    c.mode = argsort ? SEGP_LOCAL : wide ? SEGP_GLOBAL : SEGP_VALUES;
    c.ib = ib;
    c.offsets = d_offsets;
    c.nseg = nseg;
    c.row_len = row_len;
    c.max_len = max_len;
    char* cp = nullptr;
    if (wide) {  // every element's own position first: what no segment covers, and what a bad one holds, stays where it is
        cp = w0 + P.copy_off;
        rc = launch_pairs_join(ctx, d_keys, nullptr, w0, n, kb, 4, true, kind, desc, st);
        if (rc) return rc;
        RSX_HIP(hipMemcpyAsync(cp, d_values, n * (size_t)vb, hipMemcpyDeviceToDevice, st));
    }
    uint32_t launched = 0;
    rc = launchers_for(es)->segment_pairs(ctx, c, &launched, st);
    if (rc) return rc;
    if (wide) {
        rc = launch_gather(ctx, cp, d_values, vb, w0, es, pairs_value_offset(kb, 4), n, st);
        if (rc) return rc;
    }
    note_path(ctx, PATH_SEGMENTS, launched);
    ctx->last_pairs = (wide ? 4u : 3u) | es << 8;
    return RSX_OK;
}
bool rows_overflow(size_t rows, size_t row_len, uint32_t widest) {
    if (rows == 0 || row_len == 0) return false;
    if (row_len > SIZE_MAX / rows) return true;
    return widest != 0 && rows * row_len > SIZE_MAX / widest;
}
}  // namespace

int rsx_sort_segments_pairs_device(rsx_ctx* ctx, void* d_keys, void* d_values, size_t n, uint32_t key_bytes, uint32_t key_kind, uint32_t value_bytes,
                                   int order, const uint64_t* d_offsets, size_t nseg, uint64_t max_seg_len, void* stream) try {
    return segments_pairs_common(ctx, d_keys, d_values, nullptr, false, n, key_bytes, key_kind, value_bytes, 0, order, d_offsets, false, nseg, 0,
                                 max_seg_len, stream);
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_argsort_segments_device(rsx_ctx* ctx, const void* d_keys, void* d_index, size_t n, uint32_t key_bytes, uint32_t key_kind, uint32_t index_bytes,
                                int order, const uint64_t* d_offsets, size_t nseg, uint64_t max_seg_len, void* stream) try {
    return segments_pairs_common(ctx, const_cast<void*>(d_keys), nullptr, d_index, true, n, key_bytes, key_kind, 0, index_bytes, order, d_offsets, false,
                                 nseg, 0, max_seg_len, stream);
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_sort_rows_pairs_device(rsx_ctx* ctx, void* d_keys, void* d_values, size_t rows, size_t row_len, uint32_t key_bytes, uint32_t key_kind,
                               uint32_t value_bytes, int order, void* stream) try {
    if (ctx && rows_overflow(rows, row_len, key_bytes > value_bytes ? key_bytes : value_bytes)) return fail(ctx, RSX_ERR_ARG, "rows * row_len overflows");
    return segments_pairs_common(ctx, d_keys, d_values, nullptr, false, rows * row_len, key_bytes, key_kind, value_bytes, 0, order, nullptr, true, rows,
                                 row_len, 0, stream);
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_argsort_rows_device(rsx_ctx* ctx, const void* d_keys, void* d_index, size_t rows, size_t row_len, uint32_t key_bytes, uint32_t key_kind,
                            uint32_t index_bytes, int order, void* stream) try {
    if (ctx && rows_overflow(rows, row_len, key_bytes > 8 ? key_bytes : 8)) return fail(ctx, RSX_ERR_ARG, "rows * row_len overflows");
    return segments_pairs_common(ctx, const_cast<void*>(d_keys), nullptr, d_index, true, rows * row_len, key_bytes, key_kind, 0, index_bytes, order,
                                 nullptr, true, rows, row_len, 0, stream);
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_segment_pairs_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t* caps) {
    if (!caps || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED) || value_bytes > RSX_MAX_ELEM_BYTES) return RSX_ERR_ARG;
    const uint32_t es = segment_pairs_elem(key_bytes, value_bytes, false);
    if (es == 0) return RSX_ERR_UNSUPPORTED;
    for (int c = 0; c < RSX_SEG_CLASSES; ++c) caps[c] = segment_cap((int)es, c);
    return RSX_OK;
}

// ---- the first k of every row (rsx_topk_kernels.hpp, include/rsx.h) ----
namespace {
// the checks rsx_topk_rows_device and rsx_ctx_reserve_topk share; *es: the joined (key, u32 position) element
int topk_shape(rsx_ctx* ctx, size_t rows, size_t row_len, size_t k, uint32_t kb, uint32_t* es) {
    if (k > row_len) return fail(ctx, RSX_ERR_ARG, "k above row_len");
    if (rows_overflow(rows, row_len, kb > 8 ? kb : 8)) return fail(ctx, RSX_ERR_ARG, "rows * row_len overflows");
    *es = pairs_elem_bytes(kb, 4);
    if (*es == 0 || !launchers_for(*es)) return fail(ctx, RSX_ERR_INTERNAL, "no joined element for this key width");
    if (rows == 0 || k == 0) return RSX_OK;
    if ((uint64_t)row_len >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "rows of 2^32 or more keys");
    if ((uint64_t)row_len > segment_cap((int)*es, RSX_SEG_CLASSES - 1) && (uint64_t)k > topk_max_k(*es))
        return fail(ctx, RSX_ERR_UNSUPPORTED, "k above rsx_topk_caps' max_k for rows longer than the largest LDS class");
    return RSX_OK;
}
}  // namespace

int rsx_topk_rows_device(rsx_ctx* ctx, const void* d_keys, void* d_out_keys, void* d_out_index, size_t rows, size_t row_len, size_t k,
                         uint32_t key_bytes, uint32_t key_kind, uint32_t index_bytes, int order, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    int rc = check_index_bytes(ctx, index_bytes);
    if (rc) return rc;
    uint32_t desc = 0;
    rc = order_desc(ctx, order, &desc);
    if (rc) return rc;
    uint32_t es = 0;
    rc = topk_shape(ctx, rows, row_len, k, key_bytes, &es);
    if (rc) return rc;
    if (rows == 0 || k == 0) return RSX_OK;  // (empty outputs: no pointer is looked at)
    if (!d_out_keys && !d_out_index) return fail(ctx, RSX_ERR_ARG, "both output pointers are null");
    if (!d_keys) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!aligned(d_keys, key_bytes) || !aligned(d_out_keys, key_bytes) || !aligned(d_out_index, index_bytes))
        return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    rc = pending_error(ctx);
    if (rc) return rc;
    rc = ensure_aux(ctx, st);  // (the error word and the ranking self-test: a context's first call, never a captured one)
    const size_t half = topk_workspace_half(es, rows, row_len, k);
    if (!rc && half) rc = ensure_any(ctx, 2 * half, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);
    TopkCall c{};
    c.keys = d_keys;
    c.out_keys = d_out_keys;
    c.out_index = d_out_index;
    c.w0 = half ? ctx->any_buf : nullptr;
    c.w1 = half ? ctx->any_buf + half : nullptr;
    c.rows = rows;
    c.row_len = row_len;
    c.k = k;
    c.kb = key_bytes;
    c.kind = key_kind;
    c.desc = desc;
    c.ib = index_bytes;
    uint32_t launched = 0;
    rc = launchers_for(es)->topk(ctx, c, &launched, st);
    if (rc) return rc;
    note_path(ctx, PATH_TOPK, launched);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_topk(rsx_ctx* ctx, size_t rows, size_t row_len, size_t k, uint32_t key_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return fail(ctx, RSX_ERR_ARG, "invalid key width");
    uint32_t es = 0;
    int rc = topk_shape(ctx, rows, row_len, k, key_bytes, &es);
    if (rc) return rc;
    return reserve_any_entry(ctx, (rows == 0 || k == 0) ? 0 : 2 * topk_workspace_half(es, rows, row_len, k));
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_topk_caps(uint32_t key_bytes, uint32_t* caps, uint32_t* max_k) {
    if (!caps || !max_k || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return RSX_ERR_ARG;
    const uint32_t es = pairs_elem_bytes(key_bytes, 4);
    if (es == 0) return RSX_ERR_UNSUPPORTED;
    for (int c = 0; c < RSX_SEG_CLASSES; ++c) caps[c] = segment_cap((int)es, c);
    *max_k = topk_max_k(es);
    return RSX_OK;
}

// ---- groups of equal keys (rsx_unique_kernels.hpp, include/rsx.h) ----
namespace {
// The workspace of one rsx_unique_device call: the two arrays of joined elements and, behind them, the per-tile arrays
// of the run kernels.
struct UniquePlan {
    JoinedPlan j;
    size_t heads_off;  // tile_heads [tiles] u32
    size_t base_off;   // tile_base [tiles] u64
};
UniquePlan unique_plan(size_t n, uint32_t kb, bool pos) {
    UniquePlan P{joined_plan(n, kb, pos ? 4u : 0u), 0, 0};
    const uint32_t tile = unique_tile_elems(kb, pos);
    const size_t tiles = (n + tile - 1) / tile;
    P.heads_off = P.j.ws.take(tiles * sizeof(uint32_t));
    P.base_off = P.j.ws.take(tiles * sizeof(uint64_t));
    return P;
}
bool unique_size_ok(size_t n) { return (uint64_t)n < (1ull << 32); }
// rsx_unique_device and rsx_reduce_by_key_device on no keys: no group, so two memsets and no kernel
int no_group(rsx_ctx* ctx, uint32_t path, uint64_t* d_out_num, uint64_t* d_out_offsets, hipStream_t st) {
    RSX_HIP(hipMemsetAsync(d_out_num, 0, sizeof(uint64_t), st));
    if (d_out_offsets) RSX_HIP(hipMemsetAsync(d_out_offsets, 0, sizeof(uint64_t), st));
    note_path(ctx, path, 0);
    return RSX_OK;
}
}  // namespace

int rsx_unique_device(rsx_ctx* ctx, const void* d_keys, size_t n, uint32_t key_bytes, uint32_t key_kind, int order, void* d_out_keys,
                      uint64_t* d_out_offsets, void* d_out_perm, void* d_out_inverse, uint32_t index_bytes, uint64_t* d_out_num,
                      void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    uint32_t desc = 0;
    if (int rc = order_desc(ctx, order, &desc)) return rc;
    if (!d_out_num) return fail(ctx, RSX_ERR_ARG, "d_out_num is null");
    const bool pos = d_out_perm != nullptr || d_out_inverse != nullptr;
    int rc = pos ? check_index_bytes(ctx, index_bytes) : RSX_OK;
    if (rc) return rc;
    if (n > 0 && !d_keys) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!aligned(d_keys, key_bytes) || !aligned(d_out_keys, key_bytes) || !aligned(d_out_offsets, 8) || !aligned(d_out_num, 8) ||
        (pos && (!aligned(d_out_perm, index_bytes) || !aligned(d_out_inverse, index_bytes))))
        return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    if (!unique_size_ok(n)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (n == 0) return no_group(ctx, PATH_UNIQUE, d_out_num, d_out_offsets, st);
    const UniquePlan P = unique_plan(n, key_bytes, pos);
    if (P.j.inner.elem_bytes == 0 || !launchers_for(P.j.inner.elem_bytes)) return fail(ctx, RSX_ERR_INTERNAL, "no joined element for this key width");
    rc = pending_error(ctx);
    if (rc) return rc;
    rc = reserve_joined(ctx, P.j, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* w0 = nullptr;
    // the join of rsx_argsort_device (mapped key, u32 position), or of keys alone in descending order (the mapped key)
    rc = joined_sort(ctx, P.j, d_keys, nullptr, pos, key_kind, desc, st, &w0);
    if (rc) return rc;
    UniqueCall c{};
    c.elems = w0;
    c.tile_heads = reinterpret_cast<uint32_t*>(w0 + P.heads_off);
    c.tile_base = reinterpret_cast<uint64_t*>(w0 + P.base_off);
    c.n = n;
    c.kb = key_bytes;
    c.kind = key_kind;
    c.desc = desc;
    c.pos = pos;
    c.ib = index_bytes;
    c.out_keys = d_out_keys;
    c.out_offsets = d_out_offsets;
    c.out_perm = d_out_perm;
    c.out_inverse = d_out_inverse;
    c.out_num = d_out_num;
    uint32_t launched = 0;
    rc = launch_unique(ctx, c, &launched, st);
    if (rc) return rc;
    note_path(ctx, PATH_UNIQUE, launched);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_unique(rsx_ctx* ctx, size_t n, uint32_t key_bytes, int with_positions) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return fail(ctx, RSX_ERR_ARG, "invalid key width");
    if (!unique_size_ok(n)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys");
    return reserve_joined_entry(ctx, unique_plan(n, key_bytes, with_positions != 0).j);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_unique_caps(uint32_t key_bytes, int with_positions, uint32_t* tile, uint32_t* scan_span) {
    if (!tile || !scan_span || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return RSX_ERR_ARG;
    *tile = unique_tile_elems(key_bytes, with_positions != 0);
    *scan_span = unique_scan_span();
    return RSX_OK;
}

// ---- bounds of many needles in a sorted key array (rsx_search_kernels.hpp, include/rsx.h) ----
int rsx_search_sorted_device(rsx_ctx* ctx, const void* d_sorted, size_t n, const uint64_t* d_sorted_num, const void* d_needles, size_t m,
                             uint32_t key_bytes, uint32_t key_kind, int order, void* d_out_lower, void* d_out_upper, uint32_t index_bytes,
                             uint32_t flags, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    uint32_t desc = 0;
    int rc = order_desc(ctx, order, &desc);
    if (!rc) rc = check_index_bytes(ctx, index_bytes);
    if (rc) return rc;
    if (flags & ~(uint32_t)RSX_SEARCH_PRESORT) return fail(ctx, RSX_ERR_ARG, "unknown flag bits");
    if (index_bytes == 4 && (uint64_t)n >= (1ull << 32)) return fail(ctx, RSX_ERR_ARG, "2^32 or more sorted keys need 8-byte indices");
    const bool presort = (flags & RSX_SEARCH_PRESORT) != 0;
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (m == 0) {  // nothing asked: no pointer is looked at
        note_path(ctx, PATH_SEARCH, 0);
        return RSX_OK;
    }
    if (!d_out_lower && !d_out_upper) return fail(ctx, RSX_ERR_ARG, "d_out_lower and d_out_upper are both null");
    if (!d_needles || (n > 0 && !d_sorted)) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!aligned(d_sorted, key_bytes) || !aligned(d_needles, key_bytes) || !aligned(d_sorted_num, 8) || !aligned(d_out_lower, index_bytes) ||
        !aligned(d_out_upper, index_bytes))
        return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    if (presort && (uint64_t)m >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more needles to sort first");
    if (!tiles_fit(m, search_tile_elems(key_bytes))) return fail(ctx, RSX_ERR_UNSUPPORTED, "too many needles for one launch");
    if (n == 0) {  // an empty haystack: every count is zero
        if (d_out_lower) RSX_HIP(hipMemsetAsync(d_out_lower, 0, m * (size_t)index_bytes, st));
        if (d_out_upper) RSX_HIP(hipMemsetAsync(d_out_upper, 0, m * (size_t)index_bytes, st));
        note_path(ctx, PATH_SEARCH, 0);
        return RSX_OK;
    }
    rc = pending_error(ctx);
    if (rc) return rc;
    SearchCall c{};
    c.sorted = d_sorted;
    c.n = n;
    c.sorted_num = d_sorted_num;
    c.needles = d_needles;
    c.m = m;
    c.kb = key_bytes;
    c.kind = key_kind;
    c.desc = desc;
    c.pos = presort;
    c.ib = index_bytes;
    c.out_lower = d_out_lower;
    c.out_upper = d_out_upper;
    uint32_t launched = 0;
    if (!presort) {  // the needles as given: one launch, no workspace
        rc = ensure_aux(ctx, st);
        if (rc) return rc;
        Enqueue enq(ctx, st);
        rc = launch_search(ctx, c, &launched, st);
        if (rc) return rc;
        note_path(ctx, PATH_SEARCH, launched);
        return RSX_OK;
    }
    // the presort route: the m needles as joined (mapped key, u32 position) elements, sorted
    const JoinedPlan P = joined_plan(m, key_bytes, 4);
    if (P.inner.elem_bytes == 0 || !launchers_for(P.inner.elem_bytes)) return fail(ctx, RSX_ERR_INTERNAL, "no joined element for this key width");
    rc = reserve_joined(ctx, P, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* w0 = nullptr;
    rc = joined_sort(ctx, P, d_needles, nullptr, true, key_kind, desc, st, &w0);
    if (rc) return rc;
    c.needles = w0;
    rc = launch_search(ctx, c, &launched, st);
    if (rc) return rc;
    note_path(ctx, PATH_SEARCH, launched | 0x100u);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_search(rsx_ctx* ctx, size_t m, uint32_t key_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return fail(ctx, RSX_ERR_ARG, "invalid key width");
    if ((uint64_t)m >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more needles to sort first");
    return reserve_joined_entry(ctx, joined_plan(m, key_bytes, 4));
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_search_caps(uint32_t key_bytes, int with_positions, uint32_t* tile, uint32_t* window) {
    (void)with_positions;  // both routes run one tile shape
    if (!tile || !window || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return RSX_ERR_ARG;
    *tile = search_tile_elems(key_bytes);
    *window = search_window_elems(key_bytes);
    return RSX_OK;
}

// ---- order statistics of an unsorted key array (rsx_select_kernels.hpp, include/rsx.h) ----
namespace {
// The workspace of one rsx_select_device call: the state and the bins (zeroed together before level 0), the candidate
// buffer and the per-tile counts of the index launches.
struct SelectPlan {
    size_t bins_off;   // [SELECT_MAX_RANKS][SELECT_BINS] u64, right behind the state
    size_t cand_off;   // cand_cap mapped keys
    size_t tiles_off;  // [SELECT_MAX_RANKS][tiles] u32
    uint64_t cand_cap, tiles;
    Carve ws;
};
SelectPlan select_plan(size_t n, uint32_t kb) {
    SelectPlan P{};
    P.ws.take(sizeof(SelectState));
    P.bins_off = P.ws.take((size_t)SELECT_MAX_RANKS * SELECT_BINS * sizeof(uint64_t));
    P.cand_cap = (uint64_t)n / SELECT_CAND_DIV + SELECT_CAND_FLOOR;
    P.cand_off = P.ws.take((size_t)P.cand_cap * kb);
    P.tiles = ((uint64_t)n + SELECT_TILE - 1) / SELECT_TILE;
    P.tiles_off = P.ws.take((size_t)SELECT_MAX_RANKS * P.tiles * sizeof(uint32_t));
    return P;
}
// level l of a key of kb bytes: SELECT_BITS bits from the top down, the last level what is left
SelectLevel select_level(uint32_t kb, uint32_t l) {
    const uint32_t top = 8 * kb - SELECT_BITS * l;
    const uint32_t width = top < SELECT_BITS ? top : SELECT_BITS;
    return SelectLevel{l, top - width, width, top == width ? 1u : 0u};
}
uint32_t select_levels(uint32_t kb) { return (8 * kb + SELECT_BITS - 1) / SELECT_BITS; }

extern "C++" template <int KB>
int select_launches(rsx_ctx* ctx, const SelectPlan& P, const void* d_keys, size_t n, uint32_t kind, uint32_t desc, const SelectRanks& ranks,
                    uint32_t nranks, void* d_out_keys, void* d_out_index, uint32_t ib, uint32_t* launched, hipStream_t st) {
    char* w = ctx->any_buf;
    SelectState* state = reinterpret_cast<SelectState*>(w);
    unsigned long long* bins = reinterpret_cast<unsigned long long*>(w + P.bins_off);
    void* cand = w + P.cand_off;
    uint32_t* tile_count = reinterpret_cast<uint32_t*>(w + P.tiles_off);
    const uint32_t stream = (uint64_t)n * KB >= (uint64_t)RSX_COUNT16_NT_BYTES ? 1u : 0u;  // as rsx_count16top_kernel takes the hint
    uint64_t shares = ((uint64_t)n + SELECT_SHARE - 1) / SELECT_SHARE;
    const uint64_t count_groups = std::min<uint64_t>(shares, (uint64_t)ctx->num_cu * 2);
    const uint64_t compact_groups = std::min<uint64_t>(shares, (uint64_t)ctx->num_cu * 8);
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    // (a kernel, not a memset node: rsx_zero16_kernel)
    hipLaunchKernelGGL(rsx_zero16_kernel, dim3(64), dim3(256), 0, st, reinterpret_cast<uint4*>(w),
                       (uint64_t)((P.bins_off + (size_t)SELECT_MAX_RANKS * SELECT_BINS * sizeof(uint64_t)) / 16));
    RSX_HIP(hipGetLastError());
    ++*launched;
    const uint32_t levels = select_levels(KB);
    for (uint32_t l = 0; l < levels; ++l) {
        const SelectLevel lv = select_level(KB, l);
        hipLaunchKernelGGL(rsx_select_count_kernel<KB>, dim3((uint32_t)count_groups), dim3(SELECT_COUNT_WG), 0, st, d_keys, (uint64_t)n,
                           static_cast<const void*>(cand), static_cast<const SelectState*>(state), bins, P.cand_cap, lv, kind, desc, stream);
        RSX_HIP(hipGetLastError());
        hipLaunchKernelGGL(rsx_select_pick_kernel, dim3(1), dim3(1024), 0, st, state, bins, ranks, nranks, lv, P.cand_cap);
        RSX_HIP(hipGetLastError());
        *launched += 2;
        if (lv.last) break;
        hipLaunchKernelGGL(rsx_select_compact_kernel<KB>, dim3((uint32_t)compact_groups), dim3(256), 0, st, d_keys, (uint64_t)n, cand, P.cand_cap,
                           state, lv, kind, desc, stream);
        RSX_HIP(hipGetLastError());
        ++*launched;
    }
    if (d_out_index) {
        hipLaunchKernelGGL(rsx_select_tile_kernel<KB>, dim3((uint32_t)P.tiles), dim3(256), 0, st, d_keys, (uint64_t)n,
                           static_cast<const SelectState*>(state), tile_count, P.tiles, nranks, kind, desc, stream);
        RSX_HIP(hipGetLastError());
        hipLaunchKernelGGL(rsx_select_scan_kernel, dim3(nranks), dim3(1024), 0, st, state, static_cast<const uint32_t*>(tile_count), P.tiles);
        RSX_HIP(hipGetLastError());
        hipLaunchKernelGGL(rsx_select_find_kernel<KB>, dim3(nranks), dim3(256), 0, st, d_keys, (uint64_t)n, static_cast<const SelectState*>(state),
                           d_out_keys, d_out_index, ib, kind, desc);
        RSX_HIP(hipGetLastError());
        *launched += 3;
    } else {
        hipLaunchKernelGGL(rsx_select_write_kernel<KB>, dim3(1), dim3(64), 0, st, static_cast<const SelectState*>(state), d_out_keys, nranks, kind,
                           desc);
        RSX_HIP(hipGetLastError());
        ++*launched;
    }
    return RSX_OK;
}
}  // namespace

int rsx_select_device(rsx_ctx* ctx, const void* d_keys, size_t n, uint32_t key_bytes, uint32_t key_kind, const uint64_t* ranks, uint32_t nranks,
                      void* d_out_keys, void* d_out_index, uint32_t index_bytes, int order, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    uint32_t desc = 0;
    int rc = order_desc(ctx, order, &desc);
    if (rc) return rc;
    if (nranks > SELECT_MAX_RANKS) return fail(ctx, RSX_ERR_ARG, "more ranks than rsx_select_caps reports");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (nranks == 0) {  // nothing asked: no pointer is looked at
        note_path(ctx, PATH_SELECT, 0);
        return RSX_OK;
    }
    if (!d_out_keys && !d_out_index) return fail(ctx, RSX_ERR_ARG, "d_out_keys and d_out_index are both null");
    if (d_out_index) {
        rc = check_index_bytes(ctx, index_bytes);
        if (rc) return rc;
    }
    if (!ranks || !d_keys) return fail(ctx, RSX_ERR_ARG, "null pointer");
    SelectRanks r{};
    for (uint32_t q = 0; q < nranks; ++q) {
        if (ranks[q] >= (uint64_t)n) return fail(ctx, RSX_ERR_ARG, "rank out of range");
        r.r[q] = ranks[q];
    }
    if (!aligned(d_keys, key_bytes) || !aligned(d_out_keys, key_bytes) || (d_out_index && !aligned(d_out_index, index_bytes)))
        return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    if (d_out_index && index_bytes == 4 && (uint64_t)n >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys need 8-byte indices");
    if (d_out_index && !tiles_fit(n, SELECT_TILE)) return fail(ctx, RSX_ERR_UNSUPPORTED, "too many keys for one launch of the index kernels");
    rc = pending_error(ctx);
    if (rc) return rc;
    const SelectPlan P = select_plan(n, key_bytes);
    rc = ensure_aux(ctx, st);
    if (!rc) rc = ensure_any(ctx, P.ws.bytes, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace belongs to this call from the first launch on
    uint32_t launched = 0;
    for_key_width(key_bytes, [&](auto kb) {
        rc = select_launches<decltype(kb)::value>(ctx, P, d_keys, n, key_kind, desc, r, nranks, d_out_keys, d_out_index, index_bytes, &launched, st);
    });
    if (rc) return rc;
    note_path(ctx, PATH_SELECT, launched);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_select(rsx_ctx* ctx, size_t n, uint32_t key_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return fail(ctx, RSX_ERR_ARG, "invalid key width");
    return reserve_any_entry(ctx, select_plan(n, key_bytes).ws.bytes);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_select_caps(uint32_t key_bytes, uint32_t* max_ranks, uint32_t* digit_bits, uint32_t* tile, uint32_t* cand_div, uint32_t* cand_floor) {
    if (!max_ranks || !digit_bits || !tile || !cand_div || !cand_floor || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return RSX_ERR_ARG;
    *max_ranks = SELECT_MAX_RANKS;
    *digit_bits = SELECT_BITS;
    *tile = SELECT_TILE;
    *cand_div = SELECT_CAND_DIV;
    *cand_floor = SELECT_CAND_FLOOR;
    return RSX_OK;
}

// ---- keys per bin of an unsorted key array (rsx_bin_kernels.hpp, include/rsx.h) ----
namespace {
struct BinCall {
    const void* keys;
    uint64_t n;
    const uint64_t* num;
    const void* edges;
    uint32_t m, mode, kind, desc, cb;
    void* counts;
};
extern "C++" template <int KB>
int bin_launch(rsx_ctx* ctx, const BinCall& c, hipStream_t st) {
    const uint32_t stream = c.n * KB >= (uint64_t)RSX_COUNT16_NT_BYTES ? 1u : 0u;  // as rsx_count16top_kernel takes the hint
    const uint64_t shares = (c.n + SELECT_SHARE - 1) / SELECT_SHARE;
    const uint32_t groups = c.m == 0 ? 1u : (uint32_t)std::min<uint64_t>(shares, (uint64_t)ctx->num_cu * 2);
    if (c.mode == RSX_BIN_INDEX) {
        if constexpr (KB <= 8) {
            if (c.m <= BIN_INDEX_WINDOWS * BIN_INDEX_LDS)
                hipLaunchKernelGGL((rsx_bin_index_kernel<KB, true>), dim3(groups), dim3(BIN_WG), 0, st, c.keys, c.n, c.num, c.m, c.counts, c.cb, c.kind,
                                   stream);
            else
                hipLaunchKernelGGL((rsx_bin_index_kernel<KB, false>), dim3(groups), dim3(BIN_WG), 0, st, c.keys, c.n, c.num, c.m, c.counts, c.cb, c.kind,
                                   stream);
        } else {
            return fail(ctx, RSX_ERR_INTERNAL, "no index form for this key width");
        }
    } else if (c.mode == RSX_BIN_UPPER) {
        hipLaunchKernelGGL((rsx_bin_edge_kernel<KB, true>), dim3(groups), dim3(BIN_WG), 0, st, c.keys, c.n, c.num, c.edges, c.m, c.counts, c.cb, c.kind,
                           c.desc, stream);
    } else {
        hipLaunchKernelGGL((rsx_bin_edge_kernel<KB, false>), dim3(groups), dim3(BIN_WG), 0, st, c.keys, c.n, c.num, c.edges, c.m, c.counts, c.cb, c.kind,
                           c.desc, stream);
    }
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}
}  // namespace

int rsx_bin_count_device(rsx_ctx* ctx, const void* d_keys, size_t n, const uint64_t* d_num, uint32_t key_bytes, uint32_t key_kind, const void* d_edges,
                         uint32_t m, uint32_t mode, int order, void* d_counts, uint32_t count_bytes, uint32_t flags, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (mode != RSX_BIN_UPPER && mode != RSX_BIN_LOWER && mode != RSX_BIN_INDEX) return fail(ctx, RSX_ERR_ARG, "invalid mode");
    if (flags & ~(uint32_t)RSX_BIN_ACCUMULATE) return fail(ctx, RSX_ERR_ARG, "unknown flag bits");
    if (count_bytes != 4 && count_bytes != 8) return fail(ctx, RSX_ERR_ARG, "count_bytes must be 4 or 8");
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    uint32_t desc = 0;
    int rc = order_desc(ctx, order, &desc);
    if (rc) return rc;
    if (mode == RSX_BIN_INDEX) {
        if (desc || d_edges) return fail(ctx, RSX_ERR_ARG, "the index mode takes no edges and no order");
        if (key_bytes == 16 || key_kind == RSX_KEY_FLOAT) return fail(ctx, RSX_ERR_UNSUPPORTED, "the index mode takes integer keys of 1, 2, 4 or 8 bytes");
    } else if (m > bin_max_edges(key_bytes)) {
        return fail(ctx, RSX_ERR_UNSUPPORTED, "more edges than rsx_bin_caps reports");
    }
    if (m == UINT32_MAX) return fail(ctx, RSX_ERR_ARG, "m + 1 bins do not fit 32 bits");
    if (count_bytes == 4 && (uint64_t)n >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys need 8-byte counts");
    if (!d_counts || (n > 0 && !d_keys) || (mode != RSX_BIN_INDEX && m > 0 && !d_edges)) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!aligned(d_counts, count_bytes) || !aligned(d_keys, key_bytes) || !aligned(d_edges, key_bytes) || !aligned(d_num, 8))
        return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    rc = pending_error(ctx);
    if (rc) return rc;
    // No workspace of the context is touched: nothing to make and nothing to order against its other calls.
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    uint32_t launched = 0;
    if (!(flags & RSX_BIN_ACCUMULATE)) {
        const uint32_t bins = m + 1;
        hipLaunchKernelGGL(rsx_bin_zero_kernel, dim3(std::min<uint32_t>((bins + 255u) / 256u, 1024u)), dim3(256), 0, st, d_counts, bins, count_bytes);
        RSX_HIP(hipGetLastError());
        ++launched;
    }
    if (n > 0) {
        const BinCall c{d_keys, (uint64_t)n, d_num, d_edges, m, mode, key_kind, desc, count_bytes, d_counts};
        for_key_width(key_bytes, [&](auto kb) { rc = bin_launch<decltype(kb)::value>(ctx, c, st); });
        if (rc) return rc;
        ++launched;
    }
    note_path(ctx, PATH_BIN, launched);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_bin_caps(uint32_t key_bytes, uint32_t* max_edges, uint32_t* max_index_bins_lds, uint32_t* share) {
    if (!max_edges || !max_index_bins_lds || !share || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return RSX_ERR_ARG;
    *max_edges = bin_max_edges(key_bytes);
    *max_index_bins_lds = BIN_INDEX_LDS;
    *share = SELECT_SHARE;
    return RSX_OK;
}

// ---- stable merge of two sorted key arrays (rsx_merge_kernels.hpp, include/rsx.h) ----
namespace {
// The workspace of one rsx_merge_device call: nothing on the fused route; n u64 source positions for values the kernel
// does not move itself.
struct MergePlan {
    bool wide;
    Carve ws;
    size_t pos_off;
};
MergePlan merge_plan(size_t n, uint32_t vb) {
    MergePlan P{};
    P.wide = !value_width_fused(vb);
    if (P.wide) P.pos_off = P.ws.take(n * sizeof(uint64_t));
    return P;
}
// [p, p + bytes) and [q, q + qbytes) share a byte (an absent or empty range shares none)
bool ranges_overlap(const void* p, uint64_t bytes, const void* q, uint64_t qbytes) {
    if (!p || !q || bytes == 0 || qbytes == 0) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + qbytes && b < a + bytes;
}
// The calls on two sorted arrays are not in place: no output may share a byte with an input or with another output.
struct ByteRange {
    const void* p;
    uint64_t bytes;
};
int check_disjoint(rsx_ctx* ctx, std::initializer_list<ByteRange> in, std::initializer_list<ByteRange> out) {
    for (const ByteRange* o = out.begin(); o != out.end(); ++o) {
        for (const ByteRange& i : in)
            if (ranges_overlap(o->p, o->bytes, i.p, i.bytes)) return fail(ctx, RSX_ERR_ARG, "an output overlaps an input");
        for (const ByteRange* p = o + 1; p != out.end(); ++p)
            if (ranges_overlap(o->p, o->bytes, p->p, p->bytes)) return fail(ctx, RSX_ERR_ARG, "two outputs overlap");
    }
    return RSX_OK;
}
// The checks rsx_merge_device and rsx_setop_device share, of na + nb >= 1 keys, their values and the three outputs.
// need_b_values false: b's values are not asked for, and not looked at beyond their agreement with value_bytes.
int check_merge_args(rsx_ctx* ctx, const void* d_a_keys, const void* d_a_values, size_t na, const void* d_b_keys, const void* d_b_values, size_t nb,
                     bool need_b_values, uint32_t key_bytes, uint32_t value_bytes, const void* d_out_keys, const void* d_out_values,
                     const void* d_out_index, uint32_t index_bytes) {
    if (d_out_index) {
        if (int rc = check_index_bytes(ctx, index_bytes)) return rc;
        if (index_bytes == 4 && (uint64_t)na + (uint64_t)nb > (1ull << 32)) return fail(ctx, RSX_ERR_ARG, "more than 2^32 keys need 8-byte indices");
    }
    if (!d_out_keys && !d_out_values && !d_out_index) return fail(ctx, RSX_ERR_ARG, "d_out_keys, d_out_values and d_out_index are all null");
    if (value_bytes == 0 && (d_a_values || d_b_values || d_out_values)) return fail(ctx, RSX_ERR_ARG, "value pointers and value_bytes disagree");
    if ((na > 0 && !d_a_keys) || (nb > 0 && !d_b_keys)) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!need_b_values) d_b_values = nullptr;
    if (value_bytes != 0 && ((na > 0 && !d_a_values) || (need_b_values && nb > 0 && !d_b_values)))
        return fail(ctx, RSX_ERR_ARG, "values are given on one side only");
    const uint32_t va = value_bytes ? value_align(value_bytes) : 1u, ia = d_out_index ? index_bytes : 1u;
    if (!aligned(d_a_keys, key_bytes) || !aligned(d_b_keys, key_bytes) || !aligned(d_out_keys, key_bytes) || !aligned(d_a_values, va) ||
        !aligned(d_b_values, va) || !aligned(d_out_values, va) || !aligned(d_out_index, ia))
        return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    return RSX_OK;
}
}  // namespace

int rsx_merge_device(rsx_ctx* ctx, const void* d_a_keys, const void* d_a_values, size_t na, const void* d_b_keys, const void* d_b_values, size_t nb,
                     uint32_t key_bytes, uint32_t key_kind, uint32_t value_bytes, int order, void* d_out_keys, void* d_out_values, void* d_out_index,
                     uint32_t index_bytes, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    if (value_bytes > RSX_MAX_ELEM_BYTES) return fail(ctx, RSX_ERR_ARG, "value wider than RSX_MAX_ELEM_BYTES");
    uint32_t desc = 0;
    if (int rc = order_desc(ctx, order, &desc)) return rc;
    const uint64_t n = (uint64_t)na + (uint64_t)nb;
    if (n < (uint64_t)na) return fail(ctx, RSX_ERR_UNSUPPORTED, "too many keys for one launch");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (n == 0) {  // nothing asked: no pointer is looked at
        note_path(ctx, PATH_MERGE, 0);
        return RSX_OK;
    }
    int rc = check_merge_args(ctx, d_a_keys, d_a_values, na, d_b_keys, d_b_values, nb, true, key_bytes, value_bytes, d_out_keys, d_out_values,
                              d_out_index, index_bytes);
    if (rc) return rc;
    if (!tiles_fit(n, merge_tile_elems(key_bytes, value_bytes))) return fail(ctx, RSX_ERR_UNSUPPORTED, "too many keys for one launch");
    rc = check_disjoint(ctx,
                        {{d_a_keys, (uint64_t)na * key_bytes}, {d_b_keys, (uint64_t)nb * key_bytes}, {d_a_values, (uint64_t)na * value_bytes},
                         {d_b_values, (uint64_t)nb * value_bytes}},
                        {{d_out_keys, n * key_bytes}, {d_out_values, n * value_bytes}, {d_out_index, n * (d_out_index ? index_bytes : 0u)}});
    if (rc) return rc;
    rc = pending_error(ctx);
    if (rc) return rc;
    MergeCall c{};
    c.a_keys = d_a_keys;
    c.a_values = d_a_values;
    c.na = na;
    c.b_keys = d_b_keys;
    c.b_values = d_b_values;
    c.nb = nb;
    c.kb = key_bytes;
    c.kind = key_kind;
    c.desc = desc;
    c.vb = value_bytes;
    c.ib = index_bytes;
    c.out_keys = d_out_keys;
    c.out_values = d_out_values;
    c.out_index = d_out_index;
    uint32_t launched = 0;
    const MergePlan P = merge_plan((size_t)n, d_out_values ? value_bytes : 0u);
    rc = ensure_aux(ctx, st);
    if (rc) return rc;
    if (!P.wide) {  // one launch, no workspace
        Enqueue enq(ctx, st);
        rc = launch_merge(ctx, c, &launched, st);
        if (rc) return rc;
        note_path(ctx, PATH_MERGE, launched);
        return RSX_OK;
    }
    // the wide-value route: keys and u64 source positions from the same kernel, then the two-source row gather
    rc = ensure_any(ctx, P.ws.bytes, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace array belongs to this call from the first launch on
    uint64_t* pos = reinterpret_cast<uint64_t*>(ctx->any_buf + P.pos_off);
    MergeCall k = c;
    k.out_values = nullptr;
    k.out_index = pos;
    k.ib = 8;
    rc = launch_merge(ctx, k, &launched, st);
    if (rc) return rc;
    rc = launch_merge_gather(ctx, c, pos, d_out_values, d_out_index, st);
    if (rc) return rc;
    note_path(ctx, PATH_MERGE, (launched + 1u) | 0x100u);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_merge(rsx_ctx* ctx, size_t n_total, uint32_t key_bytes, uint32_t value_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED) || value_bytes > RSX_MAX_ELEM_BYTES) return fail(ctx, RSX_ERR_ARG, "invalid key or value width");
    if (!tiles_fit(n_total, merge_tile_elems(key_bytes, value_bytes))) return fail(ctx, RSX_ERR_UNSUPPORTED, "too many keys for one launch");
    return reserve_any_entry(ctx, merge_plan(n_total, value_bytes).ws.bytes);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_merge_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t* tile) {
    if (!tile || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED) || value_bytes > RSX_MAX_ELEM_BYTES) return RSX_ERR_ARG;
    *tile = merge_tile_elems(key_bytes, value_bytes);
    return RSX_OK;
}

// ---- set operations on two sorted key arrays (rsx_setop_kernels.hpp, include/rsx.h) ----
namespace {
// The workspace of one rsx_setop_device call, per tile of the merge of up to n keys: the count, the base, what the count
// launch saves for the write launch; and the scan's sum.
struct SetopPlan {
    Carve ws;
    size_t count_off;  // tile_count [tiles] u32
    size_t base_off;   // tile_base [tiles] u64
    size_t save_off;   // tile_save [tiles][setop_save_words()] u64
    size_t num_off;    // one u64
};
SetopPlan setop_plan(size_t n, uint32_t kb) {
    SetopPlan P{};
    const uint32_t tile = setop_tile_elems(kb);
    const size_t tiles = (n + tile - 1) / tile;
    P.count_off = P.ws.take(tiles * sizeof(uint32_t));
    P.base_off = P.ws.take(tiles * sizeof(uint64_t));
    P.save_off = P.ws.take(tiles * setop_save_words() * sizeof(uint64_t));
    P.num_off = P.ws.take(sizeof(uint64_t));
    return P;
}
// rows the caller provides in every output
uint64_t setop_cap(uint32_t op, uint64_t na, uint64_t nb) {
    switch (op) {
        case RSX_SETOP_INTERSECTION: return na < nb ? na : nb;
        case RSX_SETOP_DIFFERENCE: return na;
        default: return na + nb;
    }
}
}  // namespace

int rsx_setop_device(rsx_ctx* ctx, uint32_t op, const void* d_a_keys, const void* d_a_values, size_t na, const uint64_t* d_a_num, const void* d_b_keys,
                     const void* d_b_values, size_t nb, const uint64_t* d_b_num, uint32_t key_bytes, uint32_t key_kind, uint32_t value_bytes, int order,
                     void* d_out_keys, void* d_out_values, void* d_out_index, uint32_t index_bytes, uint64_t* d_out_num, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (op > RSX_SETOP_SYMMETRIC_DIFFERENCE) return fail(ctx, RSX_ERR_ARG, "invalid set operation");
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    if (value_bytes > RSX_MAX_ELEM_BYTES) return fail(ctx, RSX_ERR_ARG, "value wider than RSX_MAX_ELEM_BYTES");
    if (!value_width_fused(value_bytes)) return fail(ctx, RSX_ERR_UNSUPPORTED, "values of 1, 2, 4, 8 or 16 bytes only (ask for d_out_index and gather)");
    uint32_t desc = 0;
    if (int rc = order_desc(ctx, order, &desc)) return rc;
    if (!d_out_num) return fail(ctx, RSX_ERR_ARG, "d_out_num is null");
    if (!aligned(d_out_num, 8) || !aligned(d_a_num, 8) || !aligned(d_b_num, 8)) return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    const uint64_t n = (uint64_t)na + (uint64_t)nb;
    if (n < (uint64_t)na) return fail(ctx, RSX_ERR_UNSUPPORTED, "too many keys for one launch");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (n == 0) return no_group(ctx, PATH_SETOP, d_out_num, nullptr, st);  // nothing kept: no other pointer is looked at
    const bool emits_b = op == RSX_SETOP_UNION || op == RSX_SETOP_SYMMETRIC_DIFFERENCE;
    int rc = check_merge_args(ctx, d_a_keys, d_a_values, na, d_b_keys, d_b_values, nb, emits_b, key_bytes, value_bytes, d_out_keys, d_out_values,
                              d_out_index, index_bytes);
    if (rc) return rc;
    if (!emits_b) d_b_values = nullptr;  // not looked at
    if (!tiles_fit(n, setop_tile_elems(key_bytes))) return fail(ctx, RSX_ERR_UNSUPPORTED, "too many keys for one launch");
    const uint64_t cap = setop_cap(op, na, nb);
    rc = check_disjoint(ctx,
                        {{d_a_keys, (uint64_t)na * key_bytes}, {d_b_keys, (uint64_t)nb * key_bytes}, {d_a_values, (uint64_t)na * value_bytes},
                         {d_b_values, (uint64_t)nb * value_bytes}, {d_a_num, 8}, {d_b_num, 8}},
                        {{d_out_keys, cap * key_bytes}, {d_out_values, cap * value_bytes}, {d_out_index, cap * (d_out_index ? index_bytes : 0u)},
                         {d_out_num, 8}});
    if (rc) return rc;
    rc = pending_error(ctx);
    if (rc) return rc;
    const SetopPlan P = setop_plan((size_t)n, key_bytes);
    rc = ensure_aux(ctx, st);
    if (rc) return rc;
    rc = ensure_any(ctx, P.ws.bytes, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* w = reinterpret_cast<char*>(ctx->any_buf);
    SetopCall c{};
    c.a_keys = d_a_keys;
    c.a_values = d_out_values ? d_a_values : nullptr;
    c.na = na;
    c.a_num = d_a_num;
    c.b_keys = d_b_keys;
    c.b_values = d_out_values ? d_b_values : nullptr;
    c.nb = nb;
    c.b_num = d_b_num;
    c.op = op;
    c.kb = key_bytes;
    c.kind = key_kind;
    c.desc = desc;
    c.vb = value_bytes;
    c.ib = index_bytes;
    c.tile_count = reinterpret_cast<uint32_t*>(w + P.count_off);
    c.tile_base = reinterpret_cast<uint64_t*>(w + P.base_off);
    c.tile_save = reinterpret_cast<uint64_t*>(w + P.save_off);
    c.raw_num = reinterpret_cast<uint64_t*>(w + P.num_off);
    c.cap = (size_t)cap;
    c.out_keys = d_out_keys;
    c.out_values = d_out_values;
    c.out_index = d_out_index;
    c.out_num = d_out_num;
    uint32_t launched = 0;
    rc = launch_setop(ctx, c, &launched, st);
    if (rc) return rc;
    note_path(ctx, PATH_SETOP, launched);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_setop(rsx_ctx* ctx, size_t n_total, uint32_t key_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return fail(ctx, RSX_ERR_ARG, "invalid key width");
    if (!tiles_fit(n_total, setop_tile_elems(key_bytes))) return fail(ctx, RSX_ERR_UNSUPPORTED, "too many keys for one launch");
    return reserve_any_entry(ctx, setop_plan(n_total, key_bytes).ws.bytes);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_setop_caps(uint32_t key_bytes, uint32_t* tile) {
    if (!tile || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return RSX_ERR_ARG;
    *tile = setop_tile_elems(key_bytes);
    return RSX_OK;
}

// ---- rows that pass a predicate, in input order (rsx_compact_kernels.hpp, include/rsx.h) ----
namespace {
// The workspace of one rsx_compact_device call: per tile its kept rows and those in front of it; n u32 positions when the
// values have no typed kernel and the caller's own index cannot serve.
struct CompactPlan {
    Carve ws;
    bool wide;         // the values ride behind positions and a row gather
    uint32_t kvb;      // the value width of the kernels: 0 on that route
    size_t count_off;  // tile_count [tiles] u32
    size_t base_off;   // tile_base [tiles] u64
    size_t pos_off;    // wide: pos [n] u32
};
CompactPlan compact_plan(size_t n, uint32_t kb, uint32_t vb) {
    CompactPlan P{};
    P.wide = !value_width_fused(vb);
    P.kvb = P.wide ? 0u : vb;
    const uint32_t tile = compact_tile_elems(kb, P.kvb);
    const size_t tiles = (n + tile - 1) / tile;
    P.count_off = P.ws.take(tiles * sizeof(uint32_t));
    P.base_off = P.ws.take(tiles * sizeof(uint64_t));
    if (P.wide) P.pos_off = P.ws.take(n * sizeof(uint32_t));
    return P;
}
// Every check of rsx_compact_device that needs neither the context nor the device: 0, or the code with *what set.
int compact_check(const void* d_keys, size_t n, const uint64_t* d_num, uint32_t key_bytes, uint32_t key_kind, int order, const uint8_t* d_flags,
                  const void* d_lo, const void* d_hi, const void* d_values, uint32_t value_bytes, uint32_t flags, const void* d_out_keys,
                  const void* d_out_values, const void* d_out_index, uint32_t index_bytes, const uint64_t* d_out_num, const char** what) {
    const bool keyed = d_lo || d_hi || d_out_keys;
    *what = "invalid key width or kind";
    if (keyed && !key_widths_ok(key_bytes, key_kind)) return RSX_ERR_ARG;
    *what = "invalid order";
    if (order != RSX_ORDER_ASCENDING && order != RSX_ORDER_DESCENDING) return RSX_ERR_ARG;
    *what = "unknown flag bits";
    if (flags & ~(uint32_t)(RSX_COMPACT_INVERT | RSX_COMPACT_PARTITION)) return RSX_ERR_ARG;
    *what = "value wider than RSX_MAX_ELEM_BYTES";
    if (value_bytes > RSX_MAX_ELEM_BYTES) return RSX_ERR_ARG;
    *what = "index_bytes must be 4 or 8";
    if (d_out_index && index_bytes != 4 && index_bytes != 8) return RSX_ERR_ARG;
    *what = "d_out_num is null";
    if (!d_out_num) return RSX_ERR_ARG;
    *what = "value pointers and value_bytes disagree";
    if ((value_bytes == 0 && (d_values || d_out_values)) || (d_out_values && !d_values)) return RSX_ERR_ARG;
    *what = "null device pointer";
    if (n > 0 && keyed && !d_keys) return RSX_ERR_ARG;  // (values without d_values: refused above)
    *what = "device pointer misaligned";
    const uint32_t ka = keyed ? key_bytes : 1u, va = value_bytes ? value_align(value_bytes) : 1u, ia = d_out_index ? index_bytes : 1u;
    if (!aligned(d_keys, ka) || !aligned(d_lo, ka) || !aligned(d_hi, ka) || !aligned(d_out_keys, ka) || !aligned(d_values, va) ||
        !aligned(d_out_values, va) || !aligned(d_out_index, ia) || !aligned(d_num, 8) || !aligned(d_out_num, 8))
        return RSX_ERR_ARG;
    *what = "an output pointer equals an input pointer";
    const void* in[] = {d_keys, d_flags, d_lo, d_hi, d_values, d_num};
    const void* out[] = {d_out_keys, d_out_values, d_out_index, d_out_num};
    for (const void* o : out)
        for (const void* i : in)
            if (o && o == i) return RSX_ERR_ARG;
    *what = "2^32 or more rows";  // (the last check: what is wrong with the arguments themselves comes first)
    if ((uint64_t)n >= (1ull << 32)) return RSX_ERR_UNSUPPORTED;
    *what = "";
    return RSX_OK;
}
}  // namespace

int rsx_compact_device(rsx_ctx* ctx, const void* d_keys, size_t n, const uint64_t* d_num, uint32_t key_bytes, uint32_t key_kind, int order,
                       const uint8_t* d_flags, const void* d_lo, const void* d_hi, const void* d_values, uint32_t value_bytes, uint32_t flags,
                       void* d_out_keys, void* d_out_values, void* d_out_index, uint32_t index_bytes, uint64_t* d_out_num, void* stream) try {
    // the argument checks come first and need no context: a caller's mistake has the same answer with and without one
    const char* what = "";
    int rc = compact_check(d_keys, n, d_num, key_bytes, key_kind, order, d_flags, d_lo, d_hi, d_values, value_bytes, flags, d_out_keys, d_out_values,
                           d_out_index, index_bytes, d_out_num, &what);
    if (rc) return fail(ctx, rc, what);
    if (!ctx) return RSX_ERR_ARG;
    const uint32_t desc = order == RSX_ORDER_DESCENDING ? 1u : 0u;
    const bool keyed = d_lo || d_hi || d_out_keys;
    const uint32_t kb = keyed ? key_bytes : 0u;
    if (!d_out_values) value_bytes = 0;  // the values are not looked at
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (n == 0) return no_group(ctx, PATH_COMPACT, d_out_num, nullptr, st);
    const uint32_t ib = d_out_index ? index_bytes : 0u;
    rc = check_disjoint(ctx,
                        {{d_keys, (uint64_t)n * kb}, {d_flags, (uint64_t)n}, {d_lo, kb}, {d_hi, kb}, {d_values, (uint64_t)n * value_bytes}, {d_num, 8}},
                        {{d_out_keys, (uint64_t)n * kb}, {d_out_values, (uint64_t)n * value_bytes}, {d_out_index, (uint64_t)n * ib}, {d_out_num, 8}});
    if (rc) return rc;
    rc = pending_error(ctx);
    if (rc) return rc;
    const CompactPlan P = compact_plan(n, kb, value_bytes);
    // the positions of the wide route: the index the caller asked for when there is one, else n u32 in the workspace
    const bool ws_pos = P.wide && !d_out_index;
    const size_t need = P.wide && !ws_pos ? P.pos_off : P.ws.bytes;  // (without them: the arrays in front of them)
    rc = ensure_aux(ctx, st);
    if (rc) return rc;
    rc = ensure_any(ctx, need, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* w = reinterpret_cast<char*>(ctx->any_buf);
    CompactCall c{};
    c.keys = kb ? d_keys : nullptr;
    c.flags = d_flags;
    c.lo = d_lo;
    c.hi = d_hi;
    c.values = d_values;
    c.n = n;
    c.num = d_num;
    c.kb = kb;
    c.kind = key_kind;
    c.desc = desc;
    c.vb = P.kvb;
    c.ib = ws_pos ? 4u : (ib ? ib : 4u);
    c.mode = flags;
    c.tile_count = reinterpret_cast<uint32_t*>(w + P.count_off);
    c.tile_base = reinterpret_cast<uint64_t*>(w + P.base_off);
    c.out_keys = d_out_keys;
    c.out_values = P.wide ? nullptr : d_out_values;
    c.out_index = ws_pos ? static_cast<void*>(w + P.pos_off) : d_out_index;
    c.out_num = d_out_num;
    uint32_t launched = 0;
    rc = launch_compact(ctx, c, &launched, st);
    if (rc) return rc;
    if (P.wide) {
        rc = launch_compact_gather(ctx, c, c.out_index, c.ib, value_bytes, d_out_values, st);
        if (rc) return rc;
        ++launched;
    }
    note_path(ctx, PATH_COMPACT, launched);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_compact(rsx_ctx* ctx, size_t n, uint32_t key_bytes, uint32_t value_bytes, uint32_t index_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    if ((key_bytes != 0 && !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) || value_bytes > RSX_MAX_ELEM_BYTES ||
        (index_bytes != 0 && index_bytes != 4 && index_bytes != 8))
        return fail(ctx, RSX_ERR_ARG, "invalid key, value or index width");
    if ((uint64_t)n >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more rows");
    // enough whichever of these columns a call leaves out: a narrower row only widens the tile, so there are fewer of them
    return reserve_any_entry(ctx, compact_plan(n, key_bytes, value_bytes).ws.bytes);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_compact_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t index_bytes, uint32_t* tile, uint32_t* scan_span) {
    if (!tile || !scan_span || (key_bytes != 0 && !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) || value_bytes > RSX_MAX_ELEM_BYTES ||
        (index_bytes != 0 && index_bytes != 4 && index_bytes != 8))
        return RSX_ERR_ARG;
    *tile = compact_tile_elems(key_bytes, value_width_fused(value_bytes) ? value_bytes : 0u);
    *scan_span = unique_scan_span();
    return RSX_OK;
}

// ---- rows regrouped by bin, in input order inside each bin (rsx_msplit_kernels.hpp, include/rsx.h) ----
namespace {
// The workspace of one rsx_multisplit_device call: the count matrix, one column per workgroup; the bins' totals; n u32
// positions when the values have no typed kernel and the caller's own index cannot serve.
struct MsplitPlan {
    Carve ws;
    bool wide;         // the values ride behind positions and a row gather
    uint32_t kvb;      // the value width of the write kernel: 0 on that route
    uint32_t groups;   // workgroups of the count and the write launch
    size_t cnt_off;    // cnt [(m + 1) * groups] u32
    size_t tot_off;    // tot [m + 1] u32
    size_t pos_off;    // wide: pos [n] u32
};
MsplitPlan msplit_plan(const rsx_ctx* ctx, size_t n, uint32_t m, uint32_t vb) {
    MsplitPlan P{};
    P.wide = !value_width_fused(vb);
    P.kvb = P.wide ? 0u : vb;
    const uint64_t shares = ((uint64_t)n + SELECT_SHARE - 1) / SELECT_SHARE;
    P.groups = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(shares, (uint64_t)ctx->num_cu * 2));
    P.cnt_off = P.ws.take((size_t)(m + 1) * P.groups * sizeof(uint32_t));
    P.tot_off = P.ws.take((size_t)(m + 1) * sizeof(uint32_t));
    if (P.wide) P.pos_off = P.ws.take(n * sizeof(uint32_t));
    return P;
}
struct MsplitCall {
    const void* keys;
    const void* values;
    uint64_t n;
    const uint64_t* num;
    const void* edges;
    uint32_t m, mode, kind, desc, vb, ib, groups;
    uint32_t* cnt;
    uint32_t* tot;
    void* out_keys;
    void* out_values;
    void* out_index;
    uint64_t* out_offsets;
};
extern "C++" template <int KB, int MODE>
void msplit_typed(const MsplitCall& c, bool write, hipStream_t st) {
    const uint32_t stream = c.n * KB >= (uint64_t)RSX_COUNT16_NT_BYTES && !write ? 1u : 0u;  // (a write launch reads the keys again)
    const uint32_t bins = c.m + 1;
    hipLaunchKernelGGL((rsx_msplit_count_kernel<KB, MODE>), dim3(c.groups), dim3(BIN_WG), 0, st, c.keys, c.n, c.num, c.edges, c.m, c.cnt, c.kind, c.desc,
                       stream);
    hipLaunchKernelGGL(rsx_msplit_scan_kernel, dim3((bins + MSPLIT_WAVES - 1) / MSPLIT_WAVES), dim3(MSPLIT_WG), 0, st, c.cnt, bins, c.groups, c.tot);
    hipLaunchKernelGGL(rsx_msplit_offsets_kernel, dim3(1), dim3(MSPLIT_OFFSETS_WG), 0, st, c.tot, bins, c.out_offsets);
    if (!write) return;
    for_value_index_width(c.vb, 0u, [&](auto vb, auto) {
        hipLaunchKernelGGL((rsx_msplit_write_kernel<KB, decltype(vb)::value, MODE>), dim3(c.groups), dim3(MSPLIT_WG), 0, st, c.keys,
                           static_cast<const uint8_t*>(c.values), c.n, c.num, c.edges, c.m, c.cnt, c.out_offsets, c.kind, c.desc,
                           static_cast<uint8_t*>(c.out_keys), static_cast<uint8_t*>(c.out_values), static_cast<uint8_t*>(c.out_index), c.ib);
    });
}
extern "C++" template <int KB>
int msplit_launch(rsx_ctx* ctx, const MsplitCall& c, bool write, hipStream_t st) {
    if (c.mode == RSX_BIN_INDEX) {
        if constexpr (KB <= 8) msplit_typed<KB, MSPLIT_INDEX>(c, write, st);
        else return fail(ctx, RSX_ERR_INTERNAL, "no index form for this key width");
    } else if (c.mode == RSX_BIN_UPPER) {
        msplit_typed<KB, MSPLIT_UPPER>(c, write, st);
    } else {
        msplit_typed<KB, MSPLIT_LOWER>(c, write, st);
    }
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}
// Every check of rsx_multisplit_device that needs neither the context nor the device: 0, or the code with *what set.
int msplit_check(const void* d_keys, size_t n, const uint64_t* d_num, uint32_t key_bytes, uint32_t key_kind, const void* d_edges, uint32_t m,
                 uint32_t mode, int order, const void* d_values, uint32_t value_bytes, const void* d_out_keys, const void* d_out_values,
                 const void* d_out_index, uint32_t index_bytes, const uint64_t* d_out_offsets, const char** what) {
    *what = "invalid mode";
    if (mode != RSX_BIN_UPPER && mode != RSX_BIN_LOWER && mode != RSX_BIN_INDEX) return RSX_ERR_ARG;
    *what = "invalid key width or kind";
    if (!key_widths_ok(key_bytes, key_kind)) return RSX_ERR_ARG;
    *what = "invalid order";
    if (order != RSX_ORDER_ASCENDING && order != RSX_ORDER_DESCENDING) return RSX_ERR_ARG;
    *what = "the index mode takes no edges and no order";
    if (mode == RSX_BIN_INDEX && (order != RSX_ORDER_ASCENDING || d_edges)) return RSX_ERR_ARG;
    *what = "value wider than RSX_MAX_ELEM_BYTES";
    if (value_bytes > RSX_MAX_ELEM_BYTES) return RSX_ERR_ARG;
    *what = "index_bytes must be 4 or 8";
    if (d_out_index && index_bytes != 4 && index_bytes != 8) return RSX_ERR_ARG;
    *what = "d_out_offsets is null";
    if (!d_out_offsets) return RSX_ERR_ARG;
    *what = "value pointers and value_bytes disagree";
    if ((value_bytes == 0 && (d_values || d_out_values)) || (d_out_values && !d_values)) return RSX_ERR_ARG;
    *what = "null device pointer";
    if ((n > 0 && !d_keys) || (mode != RSX_BIN_INDEX && m > 0 && !d_edges)) return RSX_ERR_ARG;
    *what = "device pointer misaligned";
    const uint32_t va = value_bytes ? value_align(value_bytes) : 1u, ia = d_out_index ? index_bytes : 1u;
    if (!aligned(d_keys, key_bytes) || !aligned(d_edges, key_bytes) || !aligned(d_out_keys, key_bytes) || !aligned(d_values, va) ||
        !aligned(d_out_values, va) || !aligned(d_out_index, ia) || !aligned(d_num, 8) || !aligned(d_out_offsets, 8))
        return RSX_ERR_ARG;
    *what = "an output overlaps an input or another output";
    const uint64_t rows = (uint64_t)n;
    const bool edged = mode != RSX_BIN_INDEX;
    const ByteRange in[] = {{d_keys, rows * key_bytes}, {d_values, rows * value_bytes}, {d_num, 8}, {edged ? d_edges : nullptr, (uint64_t)m * key_bytes}};
    const ByteRange out[] = {{d_out_keys, rows * key_bytes}, {d_out_values, rows * value_bytes}, {d_out_index, rows * ia}, {d_out_offsets, ((uint64_t)m + 2) * 8}};
    for (const ByteRange* o = out; o != out + 4; ++o) {
        for (const ByteRange& i : in)
            if (ranges_overlap(o->p, o->bytes, i.p, i.bytes)) return RSX_ERR_ARG;
        for (const ByteRange* p = o + 1; p != out + 4; ++p)
            if (ranges_overlap(o->p, o->bytes, p->p, p->bytes)) return RSX_ERR_ARG;
    }
    *what = "2^32 or more rows";  // (what is wrong with the arguments themselves comes first)
    if (rows >= (1ull << 32)) return RSX_ERR_UNSUPPORTED;
    *what = "the index mode takes integer keys of 1, 2, 4 or 8 bytes";
    if (mode == RSX_BIN_INDEX && (key_bytes == 16 || key_kind == RSX_KEY_FLOAT)) return RSX_ERR_UNSUPPORTED;
    *what = "more edges or bins than rsx_multisplit_caps reports";
    if (m > MSPLIT_MAX_EDGES) return RSX_ERR_UNSUPPORTED;
    *what = "";
    return RSX_OK;
}
}  // namespace

int rsx_multisplit_device(rsx_ctx* ctx, const void* d_keys, size_t n, const uint64_t* d_num, uint32_t key_bytes, uint32_t key_kind, const void* d_edges,
                          uint32_t m, uint32_t mode, int order, const void* d_values, uint32_t value_bytes, void* d_out_keys, void* d_out_values,
                          void* d_out_index, uint32_t index_bytes, uint64_t* d_out_offsets, void* stream) try {
    // the argument checks come first and need no context: a caller's mistake has the same answer with and without one
    const char* what = "";
    int rc = msplit_check(d_keys, n, d_num, key_bytes, key_kind, d_edges, m, mode, order, d_values, value_bytes, d_out_keys, d_out_values, d_out_index,
                          index_bytes, d_out_offsets, &what);
    if (rc) return fail(ctx, rc, what);
    if (!ctx) return RSX_ERR_ARG;
    const uint32_t desc = order == RSX_ORDER_DESCENDING ? 1u : 0u;
    if (!d_out_values) value_bytes = 0;  // the values are not looked at
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    rc = pending_error(ctx);
    if (rc) return rc;
    const MsplitPlan P = msplit_plan(ctx, n, m, value_bytes);
    // the positions of the wide route: the index the caller asked for when there is one, else n u32 in the workspace
    const bool ws_pos = P.wide && !d_out_index;
    const size_t need = P.wide && !ws_pos ? P.pos_off : P.ws.bytes;  // (without them: the arrays in front of them)
    rc = ensure_aux(ctx, st);
    if (rc) return rc;
    rc = ensure_any(ctx, need, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* w = reinterpret_cast<char*>(ctx->any_buf);
    MsplitCall c{};
    c.keys = d_keys;
    c.values = d_values;
    c.n = n;
    c.num = d_num;
    c.edges = d_edges;
    c.m = m;
    c.mode = mode;
    c.kind = key_kind;
    c.desc = desc;
    c.vb = P.kvb;
    c.ib = ws_pos ? 4u : (d_out_index ? index_bytes : 4u);
    c.groups = P.groups;
    c.cnt = reinterpret_cast<uint32_t*>(w + P.cnt_off);
    c.tot = reinterpret_cast<uint32_t*>(w + P.tot_off);
    c.out_keys = d_out_keys;
    c.out_values = P.wide ? nullptr : d_out_values;
    c.out_index = ws_pos ? static_cast<void*>(w + P.pos_off) : d_out_index;
    c.out_offsets = d_out_offsets;
    const bool write = n > 0 && (c.out_keys || c.out_values || c.out_index);
    uint32_t launched = write ? 4u : 3u;
    {
        LaunchTimer lt(ctx, RSX_PROF_SCAN, st);  // (count, scan, write: the phases of one scan, timed as one)
        for_key_width(key_bytes, [&](auto kb) { rc = msplit_launch<decltype(kb)::value>(ctx, c, write, st); });
        if (rc) return rc;
    }
    if (P.wide && n > 0) {  // the compact call's row gather, over the first N rows
        CompactCall g{};
        g.values = d_values;
        g.n = n;
        g.num = d_num;
        g.mode = RSX_COMPACT_PARTITION;
        rc = launch_compact_gather(ctx, g, c.out_index, c.ib, value_bytes, d_out_values, st);
        if (rc) return rc;
        ++launched;
    }
    note_path(ctx, PATH_MSPLIT, launched);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_multisplit(rsx_ctx* ctx, size_t n, uint32_t m, uint32_t key_bytes, uint32_t value_bytes, uint32_t index_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED) || value_bytes > RSX_MAX_ELEM_BYTES || (index_bytes != 0 && index_bytes != 4 && index_bytes != 8))
        return fail(ctx, RSX_ERR_ARG, "invalid key, value or index width");
    if ((uint64_t)n >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more rows");
    if (m > MSPLIT_MAX_EDGES) return fail(ctx, RSX_ERR_UNSUPPORTED, "more edges or bins than rsx_multisplit_caps reports");
    // enough with and without an index output: the positions of the wide route are counted in either way
    return reserve_any_entry(ctx, msplit_plan(ctx, n, m, value_bytes).ws.bytes);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_multisplit_caps(uint32_t key_bytes, uint32_t* max_edges, uint32_t* max_index_bins, uint32_t* tile, uint32_t* share) {
    if (!max_edges || !max_index_bins || !tile || !share || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return RSX_ERR_ARG;
    *max_edges = MSPLIT_MAX_EDGES;
    *max_index_bins = MSPLIT_MAX_EDGES;
    *tile = MSPLIT_TILE;
    *share = SELECT_SHARE;
    return RSX_OK;
}

// ---- sort-merge join of two sorted key arrays (rsx_join_kernels.hpp, include/rsx.h) ----
namespace {
// The workspace of one rsx_join_device call: per key of a its lower bound in b and the rows in front of it in its count
// tile; per count tile its rows and (one word more) the rows in front of it.
struct JoinPlan {
    Carve ws;
    size_t lo_off;     // ws_lo [na] u32
    size_t local_off;  // ws_local [na] u64
    size_t total_off;  // tile_total [tiles] u64
    size_t base_off;   // tile_base [tiles + 1] u64
};
JoinPlan join_plan(size_t na) {
    JoinPlan P{};
    const uint32_t tile = join_tile_elems();
    const size_t tiles = (na + tile - 1) / tile;
    P.lo_off = P.ws.take(na * sizeof(uint32_t));
    P.local_off = P.ws.take(na * sizeof(uint64_t));
    P.total_off = P.ws.take(tiles * sizeof(uint64_t));
    P.base_off = P.ws.take((tiles + 1) * sizeof(uint64_t));
    return P;
}
// the most rows a join of na and nb keys (each below 2^32: no overflow) can have
uint64_t join_bound(uint32_t how, uint64_t na, uint64_t nb) {
    switch (how) {
        case RSX_JOIN_INNER: return na * nb;
        case RSX_JOIN_LEFT: return na * (nb ? nb : 1u);
        default: return na;
    }
}
// rows * width bytes at p for ranges_overlap; a product that does not fit ends with the address space
uint64_t join_bytes(const void* p, uint64_t rows, uint32_t width) {
    const uint64_t room = ~(uint64_t)0 - reinterpret_cast<uintptr_t>(p);
    return rows > room / width ? room : rows * width;
}
}  // namespace

int rsx_join_device(rsx_ctx* ctx, uint32_t how, const void* d_a_keys, size_t na, const uint64_t* d_a_num, const void* d_a_index, const void* d_b_keys,
                    size_t nb, const uint64_t* d_b_num, const void* d_b_index, uint32_t key_bytes, uint32_t key_kind, int order, void* d_out_a,
                    void* d_out_b, uint32_t index_bytes, size_t capacity, uint64_t* d_out_num, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (how > RSX_JOIN_ANTI) return fail(ctx, RSX_ERR_ARG, "invalid kind of join");
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    uint32_t desc = 0;
    if (int rc = order_desc(ctx, order, &desc)) return rc;
    if (int rc = check_index_bytes(ctx, index_bytes)) return rc;
    if (!d_out_num) return fail(ctx, RSX_ERR_ARG, "d_out_num is null");
    if (!aligned(d_out_num, 8) || !aligned(d_a_num, 8) || !aligned(d_b_num, 8)) return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    if ((uint64_t)na >= (1ull << 32) || (uint64_t)nb >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys on one side");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (na == 0) return no_group(ctx, PATH_JOIN, d_out_num, nullptr, st);  // no row: no other pointer is looked at
    const bool pairs = how == RSX_JOIN_INNER || how == RSX_JOIN_LEFT;
    if (!pairs && (d_out_b || d_b_index)) return fail(ctx, RSX_ERR_ARG, "a semi or anti join has no right-hand output: d_out_b and d_b_index must be null");
    const bool count_only = !d_out_a && !d_out_b && capacity == 0;
    if (!count_only && (!d_out_a || (pairs && !d_out_b))) return fail(ctx, RSX_ERR_ARG, "null output (only the count-only form, both outputs null and capacity 0, has none)");
    if (!d_a_keys || (nb > 0 && !d_b_keys)) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!aligned(d_a_keys, key_bytes) || !aligned(d_b_keys, key_bytes) || !aligned(d_a_index, index_bytes) || !aligned(d_b_index, index_bytes) ||
        !aligned(d_out_a, index_bytes) || !aligned(d_out_b, index_bytes))
        return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    const uint64_t bound = join_bound(how, na, nb);
    const uint64_t rows = (uint64_t)capacity < bound ? (uint64_t)capacity : bound;  // the rows the call may write
    const uint64_t per = join_rows();
    const uint64_t groups = rows / per + (rows % per ? 1u : 0u);
    if (groups > (1ull << 31)) return fail(ctx, RSX_ERR_UNSUPPORTED, "too many rows for one launch: lower the capacity");
    int rc = check_disjoint(ctx,
                            {{d_a_keys, (uint64_t)na * key_bytes}, {d_b_keys, (uint64_t)nb * key_bytes}, {d_a_index, (uint64_t)na * index_bytes},
                             {d_b_index, (uint64_t)nb * index_bytes}, {d_a_num, 8}, {d_b_num, 8}},
                            {{d_out_a, join_bytes(d_out_a, rows, index_bytes)}, {d_out_b, join_bytes(d_out_b, rows, index_bytes)}, {d_out_num, 8}});
    if (rc) return rc;
    rc = pending_error(ctx);
    if (rc) return rc;
    const JoinPlan P = join_plan(na);
    rc = ensure_aux(ctx, st);
    if (rc) return rc;
    rc = ensure_any(ctx, P.ws.bytes, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* w = reinterpret_cast<char*>(ctx->any_buf);
    JoinCall c{};
    c.how = how;
    c.a_keys = d_a_keys;
    c.na = na;
    c.a_num = d_a_num;
    c.a_index = d_a_index;
    c.b_keys = d_b_keys;
    c.nb = nb;
    c.b_num = d_b_num;
    c.b_index = d_b_index;
    c.kb = key_bytes;
    c.kind = key_kind;
    c.desc = desc;
    c.ib = index_bytes;
    c.ws_lo = reinterpret_cast<uint32_t*>(w + P.lo_off);
    c.ws_local = reinterpret_cast<uint64_t*>(w + P.local_off);
    c.tile_total = reinterpret_cast<uint64_t*>(w + P.total_off);
    c.tile_base = reinterpret_cast<uint64_t*>(w + P.base_off);
    c.write = !count_only;
    c.write_groups = groups ? groups : 1u;  // (no row can be written: one workgroup that reads the count and leaves)
    c.out_a = d_out_a;
    c.out_b = d_out_b;
    c.capacity = (size_t)rows;
    c.out_num = d_out_num;
    uint32_t launched = 0;
    rc = launch_join(ctx, c, &launched, st);
    if (rc) return rc;
    note_path(ctx, PATH_JOIN, launched);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_join(rsx_ctx* ctx, size_t na, uint32_t key_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return fail(ctx, RSX_ERR_ARG, "invalid key width");
    if ((uint64_t)na >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys on one side");
    return reserve_any_entry(ctx, join_plan(na).ws.bytes);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_join_caps(uint32_t key_bytes, uint32_t* tile, uint32_t* window, uint32_t* rows) {
    if (!tile || !window || !rows || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return RSX_ERR_ARG;
    *tile = join_tile_elems();
    *window = search_window_elems(key_bytes);
    *rows = join_rows();
    return RSX_OK;
}

// ---- reduce by key (rsx_reduce_kernels.hpp, include/rsx.h) ----
namespace {
// The workspace of one rsx_reduce_by_key_device call: the two arrays of joined (mapped key, value) elements and, behind
// them, the four per-tile arrays of the run kernels.
struct ReducePlan {
    JoinedPlan j;
    size_t heads_off;  // tile_heads [tiles] u32
    size_t base_off;   // tile_base [tiles] u64
    size_t tail_off;   // tile_tail [tiles] u64
    size_t carry_off;  // tile_carry [tiles] u64
};
ReducePlan reduce_plan(size_t n, uint32_t kb, uint32_t vb) {
    ReducePlan P{joined_plan(n, kb, vb), 0, 0, 0, 0};
    const uint32_t tile = reduce_tile_elems(kb, vb);
    const size_t tiles = (n + tile - 1) / tile;
    P.heads_off = P.j.ws.take(tiles * sizeof(uint32_t));
    P.base_off = P.j.ws.take(tiles * sizeof(uint64_t));
    P.tail_off = P.j.ws.take(tiles * sizeof(uint64_t));
    P.carry_off = P.j.ws.take(tiles * sizeof(uint64_t));
    return P;
}
bool reduce_value_ok(uint32_t vb, uint32_t vkind) {
    return (vb == 4 || vb == 8) && (vkind == RSX_KEY_UNSIGNED || vkind == RSX_KEY_SIGNED || vkind == RSX_KEY_FLOAT);
}
}  // namespace

int rsx_reduce_by_key_device(rsx_ctx* ctx, const void* d_keys, const void* d_values, size_t n, uint32_t key_bytes, uint32_t key_kind,
                             uint32_t value_bytes, uint32_t value_kind, int op, int order, void* d_out_keys, void* d_out_values,
                             uint64_t* d_out_offsets, uint64_t* d_out_num, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    if (!reduce_value_ok(value_bytes, value_kind)) return fail(ctx, RSX_ERR_ARG, "invalid value width or kind");
    if (op != RSX_REDUCE_SUM && op != RSX_REDUCE_MIN && op != RSX_REDUCE_MAX) return fail(ctx, RSX_ERR_ARG, "invalid operator");
    uint32_t desc = 0;
    if (int rc = order_desc(ctx, order, &desc)) return rc;
    if (!d_out_num) return fail(ctx, RSX_ERR_ARG, "d_out_num is null");
    if (!d_out_keys && !d_out_values) return fail(ctx, RSX_ERR_ARG, "d_out_keys and d_out_values are both null");
    if (n > 0 && (!d_keys || !d_values)) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!aligned(d_keys, key_bytes) || !aligned(d_out_keys, key_bytes) || !aligned(d_values, value_bytes) || !aligned(d_out_values, value_bytes) ||
        !aligned(d_out_offsets, 8) || !aligned(d_out_num, 8))
        return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    if (!unique_size_ok(n)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (n == 0) return no_group(ctx, PATH_REDUCE, d_out_num, d_out_offsets, st);
    const ReducePlan P = reduce_plan(n, key_bytes, value_bytes);
    if (P.j.inner.elem_bytes == 0 || !launchers_for(P.j.inner.elem_bytes)) return fail(ctx, RSX_ERR_INTERNAL, "no joined element for this key and value");
    int rc = pending_error(ctx);
    if (rc) return rc;
    rc = reserve_joined(ctx, P.j, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* w0 = nullptr;
    // the join of rsx_sort_pairs_device: both inputs are consumed here, before any output is stored
    rc = joined_sort(ctx, P.j, d_keys, d_values, false, key_kind, desc, st, &w0);
    if (rc) return rc;
    ReduceCall c{};
    c.elems = w0;
    c.tile_heads = reinterpret_cast<uint32_t*>(w0 + P.heads_off);
    c.tile_base = reinterpret_cast<uint64_t*>(w0 + P.base_off);
    c.tile_tail = reinterpret_cast<uint64_t*>(w0 + P.tail_off);
    c.tile_carry = reinterpret_cast<uint64_t*>(w0 + P.carry_off);
    c.n = n;
    c.kb = key_bytes;
    c.kind = key_kind;
    c.desc = desc;
    c.vb = value_bytes;
    c.vkind = value_kind;
    c.op = (uint32_t)op;
    c.out_keys = d_out_keys;
    c.out_values = d_out_values;
    c.out_offsets = d_out_offsets;
    c.out_num = d_out_num;
    uint32_t launched = 0;
    rc = launch_reduce(ctx, c, &launched, st);
    if (rc) return rc;
    note_path(ctx, PATH_REDUCE, launched);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_reduce(rsx_ctx* ctx, size_t n, uint32_t key_bytes, uint32_t value_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return fail(ctx, RSX_ERR_ARG, "invalid key width");
    if (!reduce_value_ok(value_bytes, RSX_KEY_UNSIGNED)) return fail(ctx, RSX_ERR_ARG, "invalid value width");
    if (!unique_size_ok(n)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys");
    return reserve_joined_entry(ctx, reduce_plan(n, key_bytes, value_bytes).j);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_reduce_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t* tile, uint32_t* scan_span) {
    if (!tile || !scan_span || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED) || !reduce_value_ok(value_bytes, RSX_KEY_UNSIGNED)) return RSX_ERR_ARG;
    *tile = reduce_tile_elems(key_bytes, value_bytes);
    *scan_span = reduce_scan_span();
    return RSX_OK;
}

// ---- a value column combined per bin (rsx_binred_kernels.hpp, include/rsx.h) ----
namespace {
// The workspace of one rsx_bin_reduce_device call: the matrix of partial values and the matrix of partial counts, one
// column per workgroup.
struct BinredPlan {
    Carve ws;
    uint32_t groups;   // workgroups of the first launch (0: no rows)
    size_t part_off;   // part [(m + 1) * groups] values
    size_t cnt_off;    // cnt  [(m + 1) * groups] u32
};
BinredPlan binred_plan(const rsx_ctx* ctx, size_t n, uint32_t m, uint32_t vb) {
    BinredPlan P{};
    const uint64_t shares = ((uint64_t)n + SELECT_SHARE - 1) / SELECT_SHARE;
    P.groups = (uint32_t)std::min<uint64_t>(shares, (uint64_t)ctx->num_cu * 2);
    P.part_off = P.ws.take((size_t)(m + 1) * std::max(P.groups, 1u) * vb);
    P.cnt_off = P.ws.take((size_t)(m + 1) * std::max(P.groups, 1u) * sizeof(uint32_t));
    return P;
}
uint32_t binred_cap(uint32_t mode, uint32_t kb, uint32_t vb) { return mode == RSX_BIN_INDEX ? binred_max_index(vb) : binred_max_edges(kb, vb); }
struct BinredCall {
    const void* keys;
    const void* values;
    uint64_t n;
    const uint64_t* num;
    const void* edges;
    uint32_t m, mode, kind, desc, op, groups, accumulate, cb;
    uint64_t flip;     // the sign bit of a signed integer value under MIN and MAX, else 0 (rsx_binred_kernels.hpp)
    void* part;
    uint32_t* cnt;
    void* out_values;
    void* out_counts;
};
extern "C++" template <int KB, int VB, bool FLT>
int binred_launch(rsx_ctx* ctx, const BinredCall& c, hipStream_t st) {
    uint32_t* cnt = c.out_counts ? c.cnt : nullptr;
    if (c.groups != 0) {
        const auto part = [&](auto idx) {
            hipLaunchKernelGGL((rsx_binred_part_kernel<KB, VB, FLT, decltype(idx)::value>), dim3(c.groups), dim3(BINRED_WG), 0, st, c.keys, c.values, c.n,
                               c.num, c.edges, c.m, c.mode == RSX_BIN_UPPER ? 1u : 0u, c.kind, c.desc, c.op, c.flip, c.part, cnt);
        };
        if (c.mode == RSX_BIN_INDEX) {
            if constexpr (KB <= 8) part(std::true_type{});
            else return fail(ctx, RSX_ERR_INTERNAL, "no index form for this key width");
        } else {
            part(std::false_type{});
        }
        RSX_HIP(hipGetLastError());
    }
    const uint32_t bins = c.m + 1;
    hipLaunchKernelGGL((rsx_binred_final_kernel<VB, FLT>), dim3((bins + BINRED_WAVES - 1) / BINRED_WAVES), dim3(BINRED_WG), 0, st, c.part, c.cnt, bins,
                       c.groups, c.n, c.num, c.op, c.flip, c.accumulate, c.out_values, c.out_counts, c.cb);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}
extern "C++" template <int KB>
int binred_value(rsx_ctx* ctx, const BinredCall& c, uint32_t vb, uint32_t vkind, hipStream_t st) {
    const auto kind = [&](auto w) -> int {
        constexpr int VB = decltype(w)::value;
        return vkind == RSX_KEY_FLOAT ? binred_launch<KB, VB, true>(ctx, c, st) : binred_launch<KB, VB, false>(ctx, c, st);
    };
    return vb == 8 ? kind(Width<8>{}) : kind(Width<4>{});
}
// Every check of rsx_bin_reduce_device that needs neither the context nor the device: 0, or the code with *what set.
int binred_check(const void* d_keys, const void* d_values, size_t n, const uint64_t* d_num, uint32_t key_bytes, uint32_t key_kind, const void* d_edges,
                 uint32_t m, uint32_t mode, int order, uint32_t value_bytes, uint32_t value_kind, int op, const void* d_out_values,
                 const void* d_out_counts, uint32_t count_bytes, uint32_t flags, const char** what) {
    *what = "invalid mode";
    if (mode != RSX_BIN_UPPER && mode != RSX_BIN_LOWER && mode != RSX_BIN_INDEX) return RSX_ERR_ARG;
    *what = "unknown flag bits";
    if (flags & ~(uint32_t)RSX_BIN_ACCUMULATE) return RSX_ERR_ARG;
    *what = "invalid key width or kind";
    if (!key_widths_ok(key_bytes, key_kind)) return RSX_ERR_ARG;
    *what = "invalid value width or kind";
    if (!reduce_value_ok(value_bytes, value_kind)) return RSX_ERR_ARG;
    *what = "invalid operator";
    if (op != RSX_REDUCE_SUM && op != RSX_REDUCE_MIN && op != RSX_REDUCE_MAX) return RSX_ERR_ARG;
    *what = "invalid order";
    if (order != RSX_ORDER_ASCENDING && order != RSX_ORDER_DESCENDING) return RSX_ERR_ARG;
    *what = "the index mode takes no edges and no order";
    if (mode == RSX_BIN_INDEX && (order != RSX_ORDER_ASCENDING || d_edges)) return RSX_ERR_ARG;
    *what = "count_bytes must be 4 or 8";
    if (d_out_counts && count_bytes != 4 && count_bytes != 8) return RSX_ERR_ARG;
    *what = "d_out_values is null";
    if (!d_out_values) return RSX_ERR_ARG;
    *what = "null device pointer";
    if ((n > 0 && !d_values) || (n > 0 && m > 0 && !d_keys) || (mode != RSX_BIN_INDEX && m > 0 && !d_edges)) return RSX_ERR_ARG;
    *what = "device pointer misaligned";
    const uint32_t ca = d_out_counts ? count_bytes : 1u;
    if (!aligned(d_keys, key_bytes) || !aligned(d_edges, key_bytes) || !aligned(d_values, value_bytes) || !aligned(d_out_values, value_bytes) ||
        !aligned(d_out_counts, ca) || !aligned(d_num, 8))
        return RSX_ERR_ARG;
    *what = "an output overlaps an input or the other output";
    const uint64_t rows = (uint64_t)n, bins = (uint64_t)m + 1;
    const bool edged = mode != RSX_BIN_INDEX;
    const ByteRange in[] = {{d_keys, rows * key_bytes}, {d_values, rows * value_bytes}, {d_num, 8}, {edged ? d_edges : nullptr, (uint64_t)m * key_bytes}};
    const ByteRange out[] = {{d_out_values, bins * value_bytes}, {d_out_counts, bins * ca}};
    for (const ByteRange& o : out)
        for (const ByteRange& i : in)
            if (ranges_overlap(o.p, o.bytes, i.p, i.bytes)) return RSX_ERR_ARG;
    if (ranges_overlap(out[0].p, out[0].bytes, out[1].p, out[1].bytes)) return RSX_ERR_ARG;
    *what = "2^32 or more rows";  // (what is wrong with the arguments themselves comes first)
    if (rows >= (1ull << 32)) return RSX_ERR_UNSUPPORTED;
    *what = "the index mode takes integer keys of 1, 2, 4 or 8 bytes";
    if (mode == RSX_BIN_INDEX && (key_bytes == 16 || key_kind == RSX_KEY_FLOAT)) return RSX_ERR_UNSUPPORTED;
    *what = "more edges or bins than rsx_bin_reduce_caps reports";
    if (m > binred_cap(mode, key_bytes, value_bytes)) return RSX_ERR_UNSUPPORTED;
    *what = "";
    return RSX_OK;
}
}  // namespace

int rsx_bin_reduce_device(rsx_ctx* ctx, const void* d_keys, const void* d_values, size_t n, const uint64_t* d_num, uint32_t key_bytes, uint32_t key_kind,
                          const void* d_edges, uint32_t m, uint32_t mode, int order, uint32_t value_bytes, uint32_t value_kind, int op,
                          void* d_out_values, void* d_out_counts, uint32_t count_bytes, uint32_t flags, void* stream) try {
    // the argument checks come first and need no context: a caller's mistake has the same answer with and without one
    const char* what = "";
    int rc = binred_check(d_keys, d_values, n, d_num, key_bytes, key_kind, d_edges, m, mode, order, value_bytes, value_kind, op, d_out_values,
                          d_out_counts, count_bytes, flags, &what);
    if (rc) return fail(ctx, rc, what);
    if (!ctx) return RSX_ERR_ARG;
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    rc = pending_error(ctx);
    if (rc) return rc;
    const bool accumulate = (flags & RSX_BIN_ACCUMULATE) != 0;
    if (n == 0 && accumulate) {  // nothing to add: the outputs stay as they are
        note_path(ctx, PATH_BINRED, 0);
        return RSX_OK;
    }
    const BinredPlan P = binred_plan(ctx, n, m, value_bytes);
    rc = ensure_aux(ctx, st);
    if (rc) return rc;
    rc = ensure_any(ctx, P.ws.bytes, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* w = reinterpret_cast<char*>(ctx->any_buf);
    BinredCall c{};
    c.keys = d_keys;
    c.values = d_values;
    c.n = n;
    c.num = d_num;
    c.edges = d_edges;
    c.m = m;
    c.mode = mode;
    c.kind = key_kind;
    c.desc = order == RSX_ORDER_DESCENDING ? 1u : 0u;
    c.op = (uint32_t)op;
    c.flip = value_kind == RSX_KEY_SIGNED && op != RSX_REDUCE_SUM ? 1ull << (8 * value_bytes - 1) : 0ull;
    c.groups = P.groups;
    c.accumulate = accumulate ? 1u : 0u;
    c.cb = count_bytes;
    c.part = w + P.part_off;
    c.cnt = reinterpret_cast<uint32_t*>(w + P.cnt_off);
    c.out_values = d_out_values;
    c.out_counts = d_out_counts;
    {
        LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
        for_key_width(key_bytes, [&](auto kb) { rc = binred_value<decltype(kb)::value>(ctx, c, value_bytes, value_kind, st); });
        if (rc) return rc;
    }
    note_path(ctx, PATH_BINRED, P.groups != 0 ? 2u : 1u);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_bin_reduce(rsx_ctx* ctx, size_t n, uint32_t m, uint32_t key_bytes, uint32_t value_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED) || !reduce_value_ok(value_bytes, RSX_KEY_UNSIGNED))
        return fail(ctx, RSX_ERR_ARG, "invalid key or value width");
    if ((uint64_t)n >= (1ull << 32)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more rows");
    // (the index mode's cap is the larger one: a reserve does not know the mode)
    if (m > binred_max_index(value_bytes)) return fail(ctx, RSX_ERR_UNSUPPORTED, "more edges or bins than rsx_bin_reduce_caps reports");
    return reserve_any_entry(ctx, binred_plan(ctx, n, m, value_bytes).ws.bytes);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_bin_reduce_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t* max_edges, uint32_t* max_index_bins, uint32_t* tile, uint32_t* share) {
    if (!max_edges || !max_index_bins || !tile || !share || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED) || !reduce_value_ok(value_bytes, RSX_KEY_UNSIGNED))
        return RSX_ERR_ARG;
    *max_edges = binred_max_edges(key_bytes, value_bytes);
    *max_index_bins = binred_max_index(value_bytes);
    *tile = binred_tile((int)key_bytes, (int)value_bytes);
    *share = SELECT_SHARE;
    return RSX_OK;
}

// ---- scan by key (rsx_scan_kernels.hpp, include/rsx.h) ----
namespace {
// The workspace of one rsx_scan_by_key_device call: for the grouped form the two arrays of joined (mapped key, u32
// position) elements and the column of gathered values; the four per-tile arrays; one word for the number of groups.
struct ScanPlan {
    JoinedPlan j;       // RSX_SCAN_RUNS: only its ws, nothing is joined
    size_t column_off;  // values [n] in sorted order (grouped form)
    size_t heads_off;   // tile_heads [tiles] u32
    size_t base_off;    // tile_base [tiles] u64
    size_t tail_off;    // tile_tail [tiles] u64
    size_t carry_off;   // tile_carry [tiles] u64
    size_t num_off;     // one u64
};
ScanPlan scan_plan(size_t n, uint32_t kb, uint32_t vb, bool runs) {
    ScanPlan P{};
    if (!runs) {
        P.j = joined_plan(n, kb, 4);
        P.column_off = P.j.ws.take(n * (size_t)vb);
    }
    const uint32_t tile = scan_tile_elems(kb, runs);
    const size_t tiles = (n + tile - 1) / tile;
    P.heads_off = P.j.ws.take(tiles * sizeof(uint32_t));
    P.base_off = P.j.ws.take(tiles * sizeof(uint64_t));
    P.tail_off = P.j.ws.take(tiles * sizeof(uint64_t));
    P.carry_off = P.j.ws.take(tiles * sizeof(uint64_t));
    P.num_off = P.j.ws.take(sizeof(uint64_t));
    return P;
}
constexpr uint32_t SCAN_FLAGS = RSX_SCAN_EXCLUSIVE | RSX_SCAN_RUNS;
}  // namespace

int rsx_scan_by_key_device(rsx_ctx* ctx, const void* d_keys, const void* d_values, size_t n, uint32_t key_bytes, uint32_t key_kind,
                           uint32_t value_bytes, uint32_t value_kind, int op, uint32_t flags, uint64_t first, void* d_out, uint64_t* d_out_num,
                           void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, key_kind)) return fail(ctx, RSX_ERR_ARG, "invalid key width or kind");
    if (!reduce_value_ok(value_bytes, value_kind)) return fail(ctx, RSX_ERR_ARG, "invalid value width or kind");
    if (op != RSX_REDUCE_SUM && op != RSX_REDUCE_MIN && op != RSX_REDUCE_MAX) return fail(ctx, RSX_ERR_ARG, "invalid operator");
    if (flags & ~SCAN_FLAGS) return fail(ctx, RSX_ERR_ARG, "unknown flag bits");
    if (!d_values && (op != RSX_REDUCE_SUM || value_kind == RSX_KEY_FLOAT))
        return fail(ctx, RSX_ERR_ARG, "the count form (d_values NULL) takes RSX_REDUCE_SUM and an integer value kind");
    if (n > 0 && (!d_keys || !d_out)) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!aligned(d_keys, key_bytes) || !aligned(d_values, value_bytes) || !aligned(d_out, value_bytes) || !aligned(d_out_num, 8))
        return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    if (!unique_size_ok(n)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys");
    // (d_out may be d_values; the key in front of a thread's rows is read while other threads store)
    if (int rc = check_disjoint(ctx, {{d_keys, (uint64_t)n * key_bytes}}, {{d_out, (uint64_t)n * value_bytes}, {d_out_num, d_out_num ? 8u : 0u}})) return rc;
    const bool runs = (flags & RSX_SCAN_RUNS) != 0;
    const uint32_t runs_bit = runs ? 0x100u : 0u;
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (n == 0) {  // no group: one memset and no kernel
        if (d_out_num) RSX_HIP(hipMemsetAsync(d_out_num, 0, sizeof(uint64_t), st));
        note_path(ctx, PATH_SCAN, runs_bit);
        return RSX_OK;
    }
    const ScanPlan P = scan_plan(n, key_bytes, d_values ? value_bytes : 0u, runs);
    if (!runs && (P.j.inner.elem_bytes == 0 || !launchers_for(P.j.inner.elem_bytes)))
        return fail(ctx, RSX_ERR_INTERNAL, "no joined element for this key width");
    int rc = pending_error(ctx);
    if (rc) return rc;
    if (runs) {
        rc = ensure_aux(ctx, st);
        if (rc) return rc;
        rc = ensure_any(ctx, P.j.ws.bytes, st);
    } else {
        rc = reserve_joined(ctx, P.j, st);
    }
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* w0 = ctx->any_buf;
    if (!runs) {
        // the join of rsx_argsort_device: ascending (mapped key, u32 position), so every group in input order
        rc = joined_sort(ctx, P.j, d_keys, nullptr, true, key_kind, 0, st, &w0);
        if (rc) return rc;
    }
    ScanCall c{};
    c.runs = runs;
    c.keys = runs ? d_keys : static_cast<const void*>(w0);
    c.values = d_values;
    c.column = (!runs && d_values) ? w0 + P.column_off : nullptr;
    c.tile_heads = reinterpret_cast<uint32_t*>(w0 + P.heads_off);
    c.tile_base = reinterpret_cast<uint64_t*>(w0 + P.base_off);
    c.tile_tail = reinterpret_cast<uint64_t*>(w0 + P.tail_off);
    c.tile_carry = reinterpret_cast<uint64_t*>(w0 + P.carry_off);
    c.n = n;
    c.kb = key_bytes;
    c.vb = value_bytes;
    c.vkind = value_kind;
    c.op = (uint32_t)op;
    c.exclusive = (flags & RSX_SCAN_EXCLUSIVE) != 0;
    c.first = first;
    c.out = d_out;
    c.out_num = d_out_num ? d_out_num : reinterpret_cast<uint64_t*>(w0 + P.num_off);
    uint32_t launched = 0;
    rc = launch_scan_by_key(ctx, c, &launched, st);
    if (rc) return rc;
    note_path(ctx, PATH_SCAN, launched | runs_bit);
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_ctx_reserve_scan_by_key(rsx_ctx* ctx, size_t n, uint32_t key_bytes, uint32_t value_bytes, uint32_t flags) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!key_widths_ok(key_bytes, RSX_KEY_UNSIGNED)) return fail(ctx, RSX_ERR_ARG, "invalid key width");
    if (!reduce_value_ok(value_bytes, RSX_KEY_UNSIGNED)) return fail(ctx, RSX_ERR_ARG, "invalid value width");
    if (flags & ~SCAN_FLAGS) return fail(ctx, RSX_ERR_ARG, "unknown flag bits");
    if (!unique_size_ok(n)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys");
    const bool runs = (flags & RSX_SCAN_RUNS) != 0;
    const ScanPlan P = scan_plan(n, key_bytes, value_bytes, runs);
    return runs ? reserve_any_entry(ctx, P.j.ws.bytes) : reserve_joined_entry(ctx, P.j);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_scan_by_key_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t flags, uint32_t* tile, uint32_t* scan_span) {
    if (!tile || !scan_span || !key_widths_ok(key_bytes, RSX_KEY_UNSIGNED) || !reduce_value_ok(value_bytes, RSX_KEY_UNSIGNED) || (flags & ~SCAN_FLAGS))
        return RSX_ERR_ARG;
    *tile = scan_tile_elems(key_bytes, (flags & RSX_SCAN_RUNS) != 0);
    *scan_span = reduce_scan_span();
    return RSX_OK;
}

// ---- several key columns (rsx_lex_kernels.hpp, include/rsx.h) ----
namespace {
// One round of the plan: the columns [first, last) make a compound key of k used bytes inside w, joined with a u32
// position into elements of es bytes.
struct LexRound {
    uint32_t first, last, k, w, es;
};
struct LexPlan {
    uint32_t rounds;
    LexRound r[RSX_LEX_MAX_COLUMNS];
    uint32_t max_es;  // the widest round's element
    uint32_t max_kb;  // the widest column
};
// RSX_OK, or why the columns are refused (the pointers are not looked at)
int lex_columns_status(const rsx_key_column* cols, uint32_t ncols) {
    if (!cols || ncols == 0 || ncols > RSX_LEX_MAX_COLUMNS) return RSX_ERR_ARG;
    for (uint32_t j = 0; j < ncols; ++j)
        if (cols[j].reserved != 0) return RSX_ERR_ARG;
    for (uint32_t j = 0; j < ncols; ++j)
        if (!key_widths_ok(cols[j].key_bytes, cols[j].key_kind)) return RSX_ERR_UNSUPPORTED;
    return RSX_OK;
}
// From the last column to the first: whole columns join the current round while its key bytes stay <= 16.
LexPlan lex_plan(const rsx_key_column* cols, uint32_t ncols) {
    LexPlan P{};
    auto close = [&](uint32_t first, uint32_t last, uint32_t k) {
        uint32_t w = 1;
        while (w < k) w *= 2;
        const uint32_t es = pairs_elem_bytes(w, 4);
        P.r[P.rounds++] = LexRound{first, last, k, w, es};
        if (es > P.max_es) P.max_es = es;
    };
    uint32_t last = ncols, k = 0;
    for (uint32_t j = ncols; j-- > 0;) {
        const uint32_t kb = cols[j].key_bytes;
        if (kb > P.max_kb) P.max_kb = kb;
        if (k + kb > 16) {
            close(j + 1, last, k);
            last = j + 1;
            k = 0;
        }
        k += kb;
    }
    close(0, last, k);
    return P;
}
// the two element arrays of the widest round and, behind them, `stage` bytes per key of staging (rsx_sort_columns_device)
struct LexSpace {
    size_t half;       // the second array's offset
    size_t stage_off;
    size_t bytes;
};
LexSpace lex_space(size_t n, const LexPlan& P, uint32_t stage) {
    Carve ws{};
    ws.take(n * (size_t)P.max_es);
    LexSpace S{};
    S.half = ws.take(n * (size_t)P.max_es);
    S.stage_off = ws.take(n * (size_t)stage);
    S.bytes = ws.bytes;
    return S;
}
int reserve_lex_one(rsx_ctx* ctx, size_t n, const LexPlan& P, const LexSpace& S, hipStream_t st) {
    for (uint32_t r = 0; r < P.rounds; ++r) {
        const rsx_layout L{P.r[r].es, 0, P.r[r].w, RSX_KEY_UNSIGNED};
        int rc = ensure_workspace(ctx, n, &L, st);
        if (rc) return rc;
    }
    return ensure_any(ctx, S.bytes, st);
}
// The rounds of the plan on n >= 2 keys: join, sort, and the next round reads the columns through this one's positions.
// *sorted receives the last round's sorted elements (in the workspace), *es / *voff their size and position offset.
// Caller holds ctx->mu, has set the device, checked the arguments and reserved the workspace under its Enqueue.
int lex_rounds_locked(rsx_ctx* ctx, const rsx_key_column* cols, const LexPlan& P, const LexSpace& S, size_t n, char** sorted, uint32_t* es,
                      uint32_t* voff, hipStream_t st) {
    char* w[2] = {ctx->any_buf, ctx->any_buf + S.half};
    const char* prev = nullptr;
    uint32_t prev_es = 0, prev_voff = 0;
    for (uint32_t r = 0; r < P.rounds; ++r) {
        const LexRound& R = P.r[r];
        char* cur = w[r & 1];
        LexJoinCall c{};
        uint32_t off = 0;
        for (uint32_t j = R.last; j-- > R.first;) {  // the round's last column in the lowest bytes
            c.col[c.ncols++] = LexJoinCol{cols[j].d_keys, cols[j].key_bytes, cols[j].key_kind, cols[j].descending ? 1u : 0u, off};
            off += cols[j].key_bytes;
        }
        c.w = R.w;
        c.prev = prev;
        c.prev_es = prev_es;
        c.prev_voff = prev_voff;
        c.elems = cur;
        c.n = n;
        int rc = launch_lex_join(ctx, c, st);
        if (rc) return rc;
        const rsx_layout L{R.es, 0, R.w, RSX_KEY_UNSIGNED};
        rc = sort_device_locked(ctx, cur, w[(r & 1) ^ 1], n, &L, st);
        if (rc) return rc;
        prev = cur;
        prev_es = R.es;
        prev_voff = pairs_value_offset(R.w, 4);
    }
    *sorted = const_cast<char*>(prev);
    *es = prev_es;
    *voff = prev_voff;
    ctx->last_lex = P.rounds | prev_es << 8;
    return RSX_OK;
}
// the checks both calls share, once the columns themselves passed lex_columns_status
int lex_check_pointers(rsx_ctx* ctx, const rsx_key_column* cols, uint32_t ncols) {
    for (uint32_t j = 0; j < ncols; ++j) {
        if (!cols[j].d_keys) return fail(ctx, RSX_ERR_ARG, "null device pointer");
        if (!aligned(cols[j].d_keys, cols[j].key_bytes)) return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    }
    return RSX_OK;
}
int lex_fail_columns(rsx_ctx* ctx, int rc) {
    return fail(ctx, rc, rc == RSX_ERR_UNSUPPORTED ? "a column's key width or kind has no kernels" : "invalid key columns");
}
}  // namespace

int rsx_lex_plan(const rsx_key_column* cols, uint32_t ncols, uint32_t* rounds, uint32_t* first_col, uint32_t* key_bytes, uint32_t* elem_bytes) {
    if (!rounds || !first_col || !key_bytes || !elem_bytes) return RSX_ERR_ARG;
    const int rc = lex_columns_status(cols, ncols);
    if (rc) return rc;
    const LexPlan P = lex_plan(cols, ncols);
    *rounds = P.rounds;
    for (uint32_t r = 0; r < P.rounds; ++r) {
        first_col[r] = P.r[r].first;
        key_bytes[r] = P.r[r].k;
        elem_bytes[r] = P.r[r].es;
    }
    return RSX_OK;
}

int rsx_ctx_reserve_lex(rsx_ctx* ctx, size_t n, const rsx_key_column* cols, uint32_t ncols, uint32_t value_bytes) try {
    if (!ctx) return RSX_ERR_ARG;
    int rc = lex_columns_status(cols, ncols);
    if (rc) return lex_fail_columns(ctx, rc);
    if (value_bytes > RSX_MAX_ELEM_BYTES) return fail(ctx, RSX_ERR_ARG, "value wider than RSX_MAX_ELEM_BYTES");
    if (!unique_size_ok(n)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys");
    RSX_ENTER(nullptr);
    const LexPlan P = lex_plan(cols, ncols);
    return reserve_lex_one(ctx, n, P, lex_space(n, P, std::max(P.max_kb, value_bytes)), nullptr);
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_lexsort_device(rsx_ctx* ctx, const rsx_key_column* cols, uint32_t ncols, void* d_index, size_t n, uint32_t index_bytes,
                       void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    int rc = lex_columns_status(cols, ncols);
    if (rc) return lex_fail_columns(ctx, rc);
    rc = check_index_bytes(ctx, index_bytes);
    if (rc) return rc;
    if (!unique_size_ok(n)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys");
    if (n == 0) return RSX_OK;
    if (!d_index) return fail(ctx, RSX_ERR_ARG, "null device pointer");
    if (!aligned(d_index, index_bytes)) return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    rc = lex_check_pointers(ctx, cols, ncols);
    if (rc) return rc;
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (n == 1) {  // the one position
        RSX_HIP(hipMemsetAsync(d_index, 0, index_bytes, st));
        return RSX_OK;
    }
    const LexPlan P = lex_plan(cols, ncols);
    const LexSpace S = lex_space(n, P, 0);
    rc = pending_error(ctx);
    if (rc) return rc;
    rc = reserve_lex_one(ctx, n, P, S, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* sorted = nullptr;
    uint32_t es = 0, voff = 0;
    rc = lex_rounds_locked(ctx, cols, P, S, n, &sorted, &es, &voff, st);
    if (rc) return rc;
    // the split of rsx_argsort_device: the position alone, widened to the caller's index type
    return launch_pairs_split(ctx, sorted, nullptr, d_index, n, P.r[P.rounds - 1].w, 4, 2, index_bytes, RSX_KEY_UNSIGNED, 0, st);
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_sort_columns_device(rsx_ctx* ctx, const rsx_key_column* cols, uint32_t ncols, void* d_values, uint32_t value_bytes, size_t n,
                            void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    int rc = lex_columns_status(cols, ncols);
    if (rc) return lex_fail_columns(ctx, rc);
    if (value_bytes > RSX_MAX_ELEM_BYTES) return fail(ctx, RSX_ERR_ARG, "value wider than RSX_MAX_ELEM_BYTES");
    if ((d_values == nullptr) != (value_bytes == 0) && (n > 0 || d_values != nullptr)) return fail(ctx, RSX_ERR_ARG, "d_values and value_bytes disagree");
    if (!unique_size_ok(n)) return fail(ctx, RSX_ERR_UNSUPPORTED, "2^32 or more keys");
    if (n == 0) return RSX_OK;
    rc = lex_check_pointers(ctx, cols, ncols);
    if (rc) return rc;
    if (value_bytes && !aligned(d_values, value_align(value_bytes))) return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
    if (n == 1) return RSX_OK;
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    const LexPlan P = lex_plan(cols, ncols);
    const LexSpace S = lex_space(n, P, std::max(P.max_kb, value_bytes));
    rc = pending_error(ctx);
    if (rc) return rc;
    rc = reserve_lex_one(ctx, n, P, S, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);  // the workspace arrays belong to this call from the first launch on
    char* sorted = nullptr;
    uint32_t es = 0, voff = 0;
    rc = lex_rounds_locked(ctx, cols, P, S, n, &sorted, &es, &voff, st);
    if (rc) return rc;
    // every column, then the values: a copy into the staging area, gathered back through the sorted positions.  The
    // rounds above have read every column for the last time; stream order keeps each copy in front of its gather.
    char* stage = ctx->any_buf + S.stage_off;
    for (uint32_t j = 0; j < ncols; ++j) {
        void* col = const_cast<void*>(cols[j].d_keys);
        RSX_HIP(hipMemcpyAsync(stage, col, n * (size_t)cols[j].key_bytes, hipMemcpyDeviceToDevice, st));
        rc = launch_gather(ctx, stage, col, cols[j].key_bytes, sorted, es, voff, n, st);
        if (rc) return rc;
    }
    if (value_bytes) {
        RSX_HIP(hipMemcpyAsync(stage, d_values, n * (size_t)value_bytes, hipMemcpyDeviceToDevice, st));
        rc = launch_gather(ctx, stage, d_values, value_bytes, sorted, es, voff, n, st);
        if (rc) return rc;
    }
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_segment_caps(const rsx_layout* L, uint32_t* caps) {
    if (!caps || !layout_ok(L)) return RSX_ERR_ARG;
    if (!size_supported(L->elem_bytes)) return RSX_ERR_UNSUPPORTED;
    for (int c = 0; c < RSX_SEG_CLASSES; ++c) caps[c] = segment_cap((int)L->elem_bytes, c);
    return RSX_OK;
}

// Host drop-in.  The slice is pageable memory; a pageable hipMemcpy is staged by the runtime through
// one bounce buffer by one thread (measured 27 GB/s each way on the 4 GB rung of the reference's
// ladder).  Here the copy is a pipeline of HOST_CHUNK pieces over a ring of pinned buffers: worker
// threads fill (drain) the pinned chunks with memcpy while the DMA engine moves the previous ones,
// H2D and D2H each on its own stream; the count kernel of pass 0 cannot start before the last
// chunk, so the sort itself is not overlapped (8 ms of ~150).
namespace {
void par_memcpy(char* dst, const char* src, size_t bytes, int threads) {
    if (bytes < (4u << 20) || threads <= 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> th;
    // bytes / threads rounded UP before it is rounded to 4096: rounded down, threads * per falls short of bytes by
    // bytes % threads whenever the quotient is a multiple of 4096 (4 MiB + 4 bytes over 8 threads lost its last 4)
    const size_t per = (((bytes + threads - 1) / threads) + 4095) & ~(size_t)4095;
    for (int t = 0; t < threads; ++t) {
        const size_t off = (size_t)t * per;
        if (off >= bytes) break;
        const size_t len = bytes - off < per ? bytes - off : per;
        th.emplace_back([=] { std::memcpy(dst + off, src + off, len); });
    }
    for (auto& x : th) x.join();
}

int host_pipeline(rsx_ctx* ctx, char* host, char* dev, size_t bytes, bool to_device) {
    for (int i = 0; i < HOST_RING; ++i) {
        if (!ctx->pinned[i]) RSX_HIP(hipHostMalloc(&ctx->pinned[i], HOST_CHUNK, hipHostMallocDefault));
        if (!ctx->copy_event[i]) RSX_HIP(hipEventCreateWithFlags(&ctx->copy_event[i], hipEventDisableTiming));
    }
    if (!ctx->copy_stream) RSX_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    hipStream_t cs = ctx->copy_stream;
    const int threads = (int)std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency() / 2));
    const size_t chunk = ctx->host_chunk;
    const size_t chunks = (bytes + chunk - 1) / chunk;
    if (to_device) {
        for (size_t c = 0; c < chunks; ++c) {
            const int slot = (int)(c % HOST_RING);
            const size_t off = c * chunk, len = std::min(chunk, bytes - off);
            if (c >= (size_t)HOST_RING) RSX_HIP(hipEventSynchronize(ctx->copy_event[slot]));  // slot's DMA done
            par_memcpy(static_cast<char*>(ctx->pinned[slot]), host + off, len, threads);
            RSX_HIP(hipMemcpyAsync(dev + off, ctx->pinned[slot], len, hipMemcpyHostToDevice, cs));
            RSX_HIP(hipEventRecord(ctx->copy_event[slot], cs));
        }
        RSX_HIP(hipStreamSynchronize(cs));
    } else {
        // DMA runs HOST_RING chunks ahead of the draining memcpy
        for (size_t c = 0; c < chunks + HOST_RING; ++c) {
            if (c >= (size_t)HOST_RING) {  // drain chunk c - HOST_RING
                const size_t k = c - HOST_RING;
                const int slot = (int)(k % HOST_RING);
                const size_t off = k * chunk, len = std::min(chunk, bytes - off);
                RSX_HIP(hipEventSynchronize(ctx->copy_event[slot]));
                par_memcpy(host + off, static_cast<const char*>(ctx->pinned[slot]), len, threads);
            }
            if (c < chunks) {
                const int slot = (int)(c % HOST_RING);
                const size_t off = c * chunk, len = std::min(chunk, bytes - off);
                RSX_HIP(hipMemcpyAsync(ctx->pinned[slot], dev + off, len, hipMemcpyDeviceToHost, cs));
                RSX_HIP(hipEventRecord(ctx->copy_event[slot], cs));
            }
        }
    }
    return RSX_OK;
}
}  // namespace

int rsx_sort_host(rsx_ctx* ctx, void* data, size_t n, const rsx_layout* L) try {
    int rc = check_any(ctx, L);
    if (rc) return rc;
    if (n <= 1) return RSX_OK;
    if (!data) return fail(ctx, RSX_ERR_ARG, "null host pointer");
    const size_t bytes = n * (size_t)L->elem_bytes;
    RSX_ENTER(nullptr);  // one lock across copy-in, sort and copy-out: the staging buffers are the context's
    if (bytes > ctx->host_bytes) {
        if (ctx->busy) RSX_HIP(hipEventSynchronize(ctx->last_event));
        for (void*& p : ctx->host_buf) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        ctx->host_bytes = 0;
        for (void*& p : ctx->host_buf) {
            hipError_t e = hipMalloc(&p, bytes);
            if (e != hipSuccess) return fail(ctx, RSX_ERR_NOMEM, "staging hipMalloc", e);
        }
        ctx->host_bytes = bytes;
    }
    if (ctx->busy) RSX_HIP(hipEventSynchronize(ctx->last_event));  // an earlier device sort may still use the workspace
    rc = host_pipeline(ctx, static_cast<char*>(data), static_cast<char*>(ctx->host_buf[0]), bytes, true);
    if (rc) return rc;
    hipStream_t st = ctx->copy_stream;
    rc = sort_any_locked(ctx, ctx->host_buf[0], ctx->host_buf[1], n, L, st);
    if (rc) return rc;
    RSX_HIP(hipStreamSynchronize(st));
    rc = pending_error(ctx);
    if (rc) {
        host_word(ctx, HV_ERROR) = 0;
        return fail(ctx, RSX_ERR_INTERNAL, "look-back spin gave up (device protocol error)");
    }
    return host_pipeline(ctx, static_cast<char*>(data), static_cast<char*>(ctx->host_buf[0]), bytes, false);
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_histogram_device(rsx_ctx* ctx, const void* d_src, size_t n, const rsx_layout* L, uint32_t digit,
                         uint64_t* d_hist, void* stream) try {
    int rc = check_common(ctx, L);
    if (rc) return rc;
    if (digit >= L->key_bytes || !d_hist) return fail(ctx, RSX_ERR_ARG, "bad digit / null histogram");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (n == 0) {
        RSX_HIP(hipMemsetAsync(d_hist, 0, RADIX * sizeof(uint64_t), st));
        return RSX_OK;
    }
    if (!d_src || !aligned(d_src, elem_align(L->elem_bytes))) return fail(ctx, RSX_ERR_ARG, "bad source pointer");
    rc = ensure_workspace(ctx, n, L, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);
    const RegionGeom geom = make_geom(ctx, n, L->elem_bytes);
    SortRun run;
    rc = begin_control(ctx, run, st, geom, false);
    if (rc) return rc;
    rc = launchers_for(L->elem_bytes)->hist(ctx, run, d_src, geom, L, digit, J_of(ctx, run, 0), nullptr, false, st);
    if (rc) return rc;
    rc = launch_totals(ctx, geom, J_of(ctx, run, 0), d_hist, st);  // column sums -> d_hist
    if (rc == RSX_OK) end_control(ctx);
    return rc;
} catch (...) {
    return RSX_ERR_HIP;
}

namespace {
int partition_locked(rsx_ctx* ctx, const void* d_src, void* d_dst, size_t n, const rsx_layout* L, uint32_t digit,
                     uint64_t* d_hist, hipStream_t st) {
    int rc = pending_error(ctx);
    if (rc) return rc;
    rc = ensure_workspace(ctx, n, L, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);
    const RegionGeom geom = make_geom(ctx, n, L->elem_bytes);
    const EsLaunchers& K = *launchers_for(L->elem_bytes);
    SortRun run;
    rc = begin_control(ctx, run, st, geom, false);
    if (rc) return rc;
    rc = K.hist(ctx, run, d_src, geom, L, digit, J_of(ctx, run, 0), nullptr, true, st);
    if (rc) return rc;
    if (d_hist) {
        rc = launch_totals(ctx, geom, J_of(ctx, run, 0), d_hist, st);
        if (rc) return rc;
    }
    rc = K.sweep(ctx, run, SweepPass{0, true, 0}, d_src, d_dst, geom, L, digit, J_of(ctx, run, 0), nullptr, nullptr, 3, st);  // a lone pass maps and unmaps
    if (rc == RSX_OK) end_control(ctx);
    return rc;
}
}  // namespace

int rsx_partition_device(rsx_ctx* ctx, const void* d_src, void* d_dst, size_t n, const rsx_layout* L,
                         uint32_t digit, uint64_t* d_hist, void* stream) try {
    int rc = check_common(ctx, L);
    if (rc) return rc;
    if (digit >= L->key_bytes) return fail(ctx, RSX_ERR_ARG, "bad digit");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (n == 0) {
        if (d_hist) RSX_HIP(hipMemsetAsync(d_hist, 0, RADIX * sizeof(uint64_t), st));
        return RSX_OK;
    }
    const uint32_t al = elem_align(L->elem_bytes);
    if (!d_src || !d_dst || !aligned(d_src, al) || !aligned(d_dst, al))
        return fail(ctx, RSX_ERR_ARG, "bad device pointer");
    return partition_locked(ctx, d_src, d_dst, n, L, digit, d_hist, st);
} catch (...) {
    return RSX_ERR_HIP;
}

namespace {
inline uint64_t sub_start(uint64_t n, uint32_t nsub, uint32_t k) { return (uint64_t)(((unsigned __int128)n * k) / nsub); }
}  // namespace

int rsx_partition_count_device(rsx_ctx* ctx, const void* d_src, size_t n, const rsx_layout* L, uint32_t digit,
                               uint32_t nsub, uint64_t* d_hist, void* stream) try {
    int rc = check_common(ctx, L);
    if (rc) return rc;
    if (digit >= L->key_bytes) return fail(ctx, RSX_ERR_ARG, "bad digit");
    if (nsub == 0 || nsub > PART_MAX_SUB || !d_hist) return fail(ctx, RSX_ERR_ARG, "1..16 sub-ranges, non-null histogram");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    if (n && (!d_src || !aligned(d_src, elem_align(L->elem_bytes)))) return fail(ctx, RSX_ERR_ARG, "bad source pointer");
    rc = ensure_aux(ctx, st);
    if (rc) return rc;
    if (!ctx->part_J) {
        if (capturing(st)) return fail(ctx, RSX_ERR_WORKSPACE, "sub-range count matrices not allocated before stream capture");
        RSX_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->part_J), (size_t)PART_MAX_SUB * J_BYTES));
    }
    Enqueue enq(ctx, st);
    RSX_HIP(hipMemsetAsync(ctx->part_J, 0, (size_t)nsub * J_BYTES, st));
    const EsLaunchers& K = *launchers_for(L->elem_bytes);
    SortRun run;  // no control block, nothing to clean: the counts go to matrices of their own
    for (uint32_t k = 0; k < nsub; ++k) {
        const uint64_t beg = sub_start(n, nsub, k), nk = sub_start(n, nsub, k + 1) - beg;
        if (nk == 0) {
            RSX_HIP(hipMemsetAsync(d_hist + (size_t)k * RADIX, 0, RADIX * sizeof(uint64_t), st));
            continue;
        }
        const RegionGeom geom = make_geom(ctx, nk, L->elem_bytes);
        unsigned long long* Jk = ctx->part_J + (size_t)k * (J_BYTES / sizeof(unsigned long long));
        rc = K.hist(ctx, run, static_cast<const char*>(d_src) + beg * L->elem_bytes, geom, L, digit, Jk, nullptr, false, st);
        if (rc) return rc;
        rc = launch_totals(ctx, geom, Jk, d_hist + (size_t)k * RADIX, st);
        if (rc) return rc;
    }
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_partition_scatter_device(rsx_ctx* ctx, const void* d_src, void* d_dst, size_t n, const rsx_layout* L,
                                 uint32_t digit, uint32_t nsub, uint32_t k, void* stream) try {
    int rc = check_common(ctx, L);
    if (rc) return rc;
    if (digit >= L->key_bytes) return fail(ctx, RSX_ERR_ARG, "bad digit");
    if (nsub == 0 || nsub > PART_MAX_SUB || k >= nsub) return fail(ctx, RSX_ERR_ARG, "bad sub-range");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    const uint64_t beg = sub_start(n, nsub, k), nk = sub_start(n, nsub, k + 1) - beg;
    if (nk == 0) return RSX_OK;
    const uint32_t al = elem_align(L->elem_bytes);
    if (!d_src || !d_dst || !aligned(d_src, al) || !aligned(d_dst, al)) return fail(ctx, RSX_ERR_ARG, "bad device pointer");
    if (!ctx->part_J) return fail(ctx, RSX_ERR_ARG, "rsx_partition_count_device has not run on this context");
    rc = pending_error(ctx);
    if (rc) return rc;
    rc = ensure_workspace(ctx, nk, L, st);
    if (rc) return rc;
    Enqueue enq(ctx, st);
    const RegionGeom geom = make_geom(ctx, nk, L->elem_bytes);
    // what the count kernel of a whole sort clears on its way: this pass's control words and status words
    RSX_HIP(hipMemsetAsync(part_tickets_of(ctx), 0, TICKET_WORDS * sizeof(uint32_t), st));
    RSX_HIP(hipMemsetAsync(ctx->status, 0, status_bytes_for(ctx, nk, L->elem_bytes), st));
    SortRun run;
    run.tickets_override = part_tickets_of(ctx);  // outside the alternating control blocks
    const size_t off = beg * (size_t)L->elem_bytes;
    return launchers_for(L->elem_bytes)->sweep(ctx, run, SweepPass{0, true, 0}, static_cast<const char*>(d_src) + off, static_cast<char*>(d_dst) + off, geom, L,
                                               digit, ctx->part_J + (size_t)k * (J_BYTES / sizeof(unsigned long long)), nullptr, nullptr, 3, st);
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_splitter_count_device(rsx_ctx* ctx, const void* d_data, size_t n, const rsx_layout* L, const uint64_t* d_ranges,
                              const uint64_t* d_prefix, uint32_t nb, uint32_t digit, uint64_t* d_less, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!layout_ok(L)) return fail(ctx, RSX_ERR_ARG, "invalid rsx_layout");
    if (nb == 0) return RSX_OK;
    if (digit >= L->key_bytes || !d_ranges || !d_prefix || !d_less || (n && !d_data)) return fail(ctx, RSX_ERR_ARG, "bad digit / null pointer");
    RSX_ENTER(nullptr);
    hipLaunchKernelGGL(rsx_splitter_count_kernel, dim3(nb), dim3(RADIX), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(d_data), (uint64_t)n, L->elem_bytes, L->key_offset, L->key_bytes, L->key_kind,
                       d_ranges, d_prefix, digit, d_less);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_splitter_pick_device(rsx_ctx* ctx, const uint64_t* d_total, const uint64_t* d_rank, uint64_t* d_prefix, uint32_t nb,
                             uint32_t digit, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (nb == 0) return RSX_OK;
    if (digit >= 16 || !d_total || !d_rank || !d_prefix) return fail(ctx, RSX_ERR_ARG, "bad digit / null pointer");
    RSX_ENTER(nullptr);
    hipLaunchKernelGGL(rsx_splitter_pick_kernel, dim3(nb), dim3(RADIX), 0, static_cast<hipStream_t>(stream), d_total, d_rank,
                       d_prefix, digit);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_segmented_copy_device(rsx_ctx* ctx, const void* d_src, void* d_dst, uint32_t elem_bytes,
                              const uint64_t* d_src_off, const uint64_t* d_dst_off, const uint64_t* d_len,
                              uint32_t nseg, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (nseg == 0) return RSX_OK;
    if (!d_src || !d_dst || !d_src_off || !d_dst_off || !d_len) return fail(ctx, RSX_ERR_ARG, "null pointer");
    if (!size_supported(elem_bytes)) return fail(ctx, RSX_ERR_UNSUPPORTED, "element size has no device kernel");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    return launchers_for(elem_bytes)->segcopy(ctx, d_src, d_dst, d_src_off, d_dst_off, d_len, nseg, st);
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_bounds_device(rsx_ctx* ctx, const void* d_sorted, size_t n, const rsx_layout* L, const uint64_t* d_queries,
                      uint32_t nq, uint64_t* d_out, void* stream) {
    return rsx_bounds_ranges_device(ctx, d_sorted, n, L, d_queries, nullptr, nq, d_out, stream);
}

int rsx_bounds_ranges_device(rsx_ctx* ctx, const void* d_sorted, size_t n, const rsx_layout* L, const uint64_t* d_queries,
                             const uint64_t* d_ranges, uint32_t nq, uint64_t* d_out, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!layout_ok(L)) return fail(ctx, RSX_ERR_ARG, "invalid rsx_layout");
    if (nq == 0) return RSX_OK;
    if (!d_queries || !d_out || (n && !d_sorted)) return fail(ctx, RSX_ERR_ARG, "null pointer");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    hipLaunchKernelGGL(rsx_bounds_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, static_cast<const uint8_t*>(d_sorted),
                       (uint64_t)n, L->elem_bytes, L->key_offset, L->key_bytes, L->key_kind, d_queries, nq, d_out,
                       d_ranges);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

// ---- multi-GPU, one process ---------------------------------------------------------------------
// The G slices are "chunks" in the sense of mod.rs:66-70; the result is what the reference would
// produce on their concatenation.  Two schedules, both moving every element across devices ONCE:
//
//  exchange first (default): (1) every device makes one stable partition pass of its slice by the
//    MOST significant digit (count + scatter of mod.rs:90-168 for that digit) and reports the 256
//    counts; (2) the host lays the G x 256 counts out in global order: a slice boundary that falls
//    between two buckets needs nothing more; for a boundary inside bucket v, every device sorts
//    its piece of bucket v (a small local sort) and the exact cut is found as in the other
//    schedule, inside those pieces only; (3) each device pushes, per owner, ONE contiguous range of
//    its partitioned slice over xGMI, ordered by source slice at the receiver; (4) ONE local sort.
//    Work per element: 1 + D passes (plus the boundary buckets: 1/256 of the data per boundary for
//    spread-out keys; all of it when one top digit holds everything -- then this schedule costs
//    what the other does).
//  sort first: (1) every device sorts its slice; (2) the G-1 boundaries are located exactly by a
//    256-way search per digit, counted by binary search in every sorted slice; (3) exchange;
//    (4) a second stable local sort merges the G sorted runs.  2 D passes per element.
//
// Stability in both: equal keys stay in (source slice, local index) order through the exchange --
// ties on a boundary key are dealt out in slice order -- and the final local sort is stable.
namespace {

struct Shard {
    rsx_ctx* c;
    char* data;
    char* tmp;
    size_t n;
};

std::mutex g_peer_mu;
bool g_peer_on[64][64];

int shard_prepare(rsx_ctx* ctx0, rsx_ctx* ctx) {
    DeviceGuard dg(ctx->device);
    if (!dg.ok) return fail(ctx0, RSX_ERR_NODEVICE, "hipSetDevice failed");
    hipError_t e = hipSuccess;
    if (!ctx->shard_stream) e = hipStreamCreateWithFlags(&ctx->shard_stream, hipStreamNonBlocking);
    const size_t qbytes = (size_t)64 * RADIX * 4 * sizeof(uint64_t);  // queries: (lo, hi) + (begin, end)
    if (e == hipSuccess && !ctx->shard_q) e = hipMalloc(reinterpret_cast<void**>(&ctx->shard_q), qbytes);
    if (e == hipSuccess && !ctx->shard_out) e = hipMalloc(reinterpret_cast<void**>(&ctx->shard_out), qbytes / 2);
    if (e == hipSuccess && !ctx->shard_hist) e = hipMalloc(reinterpret_cast<void**>(&ctx->shard_hist), RADIX * sizeof(uint64_t));
    if (e == hipSuccess && !ctx->shard_host) e = hipHostMalloc(reinterpret_cast<void**>(&ctx->shard_host), qbytes / 2 + RADIX * sizeof(uint64_t), hipHostMallocDefault);
    if (e != hipSuccess) return fail(ctx0, RSX_ERR_NOMEM, "multi-GPU scratch allocation", e);
    return RSX_OK;
}

void enable_peer(int from, int to) {  // direct xGMI writes where the topology allows; the copies work either way
    if (from == to || from >= 64 || to >= 64) return;
    std::lock_guard<std::mutex> lk(g_peer_mu);
    if (g_peer_on[from][to]) return;
    g_peer_on[from][to] = true;
    DeviceGuard dg(from);
    if (hipDeviceEnablePeerAccess(to, 0) != hipSuccess) (void)hipGetLastError();
}

int sync_all(rsx_ctx* ctx, const std::vector<Shard>& sh) {
    for (const Shard& s : sh) {
        DeviceGuard dg(s.c->device);
        RSX_HIP(hipStreamSynchronize(s.c->shard_stream));
    }
    for (size_t g = 0; g < sh.size(); ++g) {
        std::lock_guard<std::mutex> lk(sh[g].c->mu);
        int rc = pending_error(sh[g].c);
        if (rc) {
            host_word(sh[g].c, HV_ERROR) = 0;
            return fail(ctx, RSX_ERR_INTERNAL, "look-back spin gave up on one of the slices");
        }
    }
    return RSX_OK;
}

// local sort of `n` elements at `data` (scratch `tmp`) on the slice's own stream, not synchronised
int sort_async(rsx_ctx* ctx0, rsx_ctx* c, void* data, void* tmp, size_t n, const rsx_layout* L) {
    if (n <= 1) return RSX_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    int rc = sort_device_locked(c, data, tmp, n, L, c->shard_stream);
    if (rc && c != ctx0) return fail(ctx0, rc, c->err.c_str());
    return rc;
}

struct Range {
    uint64_t beg, end;
};

// Exact cuts inside sorted ranges.  For boundary b, slice g holds a range rng[b][g] of its buffer
// buf[g] that is sorted by mapped key; the digits above `top_digit` of the boundary key are known
// (pre_lo/pre_hi[b]).  rank[b] elements of the union of the ranges lie below the cut in the global
// order (key, slice, index).  cut[b][g] = how many of rng[b][g]'s elements lie below it.
// Digit by digit from `top_digit` down: 256 candidate keys per boundary, counted by binary search
// in every range (rsx_bounds_kernel), all devices at once, one host round trip per digit.
int find_cuts(rsx_ctx* ctx, const std::vector<Shard>& sh, const std::vector<char*>& buf, const rsx_layout* L,
              const std::vector<std::vector<Range>>& rng, const std::vector<uint64_t>& rank, int top_digit,
              std::vector<uint64_t> pre_lo, std::vector<uint64_t> pre_hi, std::vector<std::vector<uint64_t>>& cut) {
    const uint32_t G = (uint32_t)sh.size();
    const uint32_t nb = (uint32_t)rank.size();
    cut.assign(nb, std::vector<uint64_t>(G, 0));
    if (nb == 0) return RSX_OK;
    if (nb > 64) return fail(ctx, RSX_ERR_ARG, "more than 64 boundaries");
    std::vector<uint64_t> q((size_t)nb * RADIX * 4);
    auto ask = [&](uint32_t per) -> int {  // `per` candidates per boundary are in q; answers land in shard_host
        const uint32_t nq = nb * per;
        for (uint32_t g = 0; g < G; ++g) {
            rsx_ctx* c = sh[g].c;
            std::lock_guard<std::mutex> lk(c->mu);
            DeviceGuard dg(c->device);
            // queries: nq x (lo, hi), then nq x (begin, end) -- the ranges differ per slice
            std::vector<uint64_t>& stage = c->shard_stage;
            stage.resize((size_t)nq * 4);
            for (uint32_t i = 0; i < nq; ++i) {
                stage[2 * i] = q[2 * i];
                stage[2 * i + 1] = q[2 * i + 1];
                stage[(size_t)2 * nq + 2 * i] = rng[i / per][g].beg;
                stage[(size_t)2 * nq + 2 * i + 1] = rng[i / per][g].end;
            }
            RSX_HIP(hipMemcpyAsync(c->shard_q, stage.data(), (size_t)nq * 4 * sizeof(uint64_t), hipMemcpyHostToDevice, c->shard_stream));
            hipLaunchKernelGGL(rsx_bounds_kernel, dim3((nq + 255) / 256), dim3(256), 0, c->shard_stream,
                               reinterpret_cast<const uint8_t*>(buf[g]), (uint64_t)sh[g].n, L->elem_bytes, L->key_offset,
                               L->key_bytes, L->key_kind, c->shard_q, nq, c->shard_out, c->shard_q + (size_t)2 * nq);
            RSX_HIP(hipGetLastError());
            RSX_HIP(hipMemcpyAsync(c->shard_host, c->shard_out, (size_t)nq * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->shard_stream));
        }
        for (uint32_t g = 0; g < G; ++g) {
            DeviceGuard dg(sh[g].c->device);
            RSX_HIP(hipStreamSynchronize(sh[g].c->shard_stream));
        }
        return RSX_OK;
    };
    for (int digit = top_digit; digit >= 0; --digit) {
        for (uint32_t b = 0; b < nb; ++b)
            for (uint32_t j = 0; j < RADIX; ++j) {
                uint64_t lo = pre_lo[b], hi = pre_hi[b];
                if (digit < 8) lo |= (uint64_t)j << (8 * digit);
                else hi |= (uint64_t)j << (8 * (digit - 8));
                q[2 * ((size_t)b * RADIX + j)] = lo;
                q[2 * ((size_t)b * RADIX + j) + 1] = hi;
            }
        int rc = ask(RADIX);
        if (rc) return rc;
        for (uint32_t b = 0; b < nb; ++b) {
            uint32_t pick = 0;  // largest candidate whose global "less" count does not exceed the rank
            for (uint32_t j = 0; j < RADIX; ++j) {
                uint64_t less = 0;
                for (uint32_t g = 0; g < G; ++g) less += sh[g].c->shard_host[(size_t)b * RADIX + j];
                if (less <= rank[b]) pick = j;  // monotone in j
            }
            if (digit < 8) pre_lo[b] |= (uint64_t)pick << (8 * digit);
            else pre_hi[b] |= (uint64_t)pick << (8 * (digit - 8));
        }
    }
    for (uint32_t b = 0; b < nb; ++b) {
        q[2 * b] = pre_lo[b];
        q[2 * b + 1] = pre_hi[b];
    }
    int rc = ask(1);
    if (rc) return rc;
    for (uint32_t b = 0; b < nb; ++b) {
        uint64_t less_total = 0;
        for (uint32_t g = 0; g < G; ++g) less_total += sh[g].c->shard_host[b];
        if (less_total > rank[b]) return fail(ctx, RSX_ERR_INTERNAL, "splitter search inconsistent");
        uint64_t need = rank[b] - less_total;  // elements equal to the boundary key that go below the cut
        for (uint32_t g = 0; g < G; ++g) {      // ties: lower slice first (stability)
            const uint64_t less = sh[g].c->shard_host[b], eq = sh[g].c->shard_host[nb + b] - less;
            const uint64_t take = need < eq ? need : eq;
            cut[b][g] = less + take;
            need -= take;
        }
        if (need != 0) return fail(ctx, RSX_ERR_INTERNAL, "splitter search inconsistent");
    }
    return RSX_OK;
}

// split[g][h] .. split[g][h+1] of src[g] goes to owner h, behind the ranges of the slices before g
int exchange(rsx_ctx* ctx, const std::vector<Shard>& sh, const std::vector<char*>& src, const std::vector<char*>& dst,
             const std::vector<std::vector<uint64_t>>& split, size_t es) {
    const uint32_t G = (uint32_t)sh.size();
    for (uint32_t h = 0; h < G; ++h) {
        uint64_t got = 0;
        for (uint32_t g = 0; g < G; ++g) {
            if (split[g][h + 1] < split[g][h]) return fail(ctx, RSX_ERR_INTERNAL, "splitters not monotone");
            got += split[g][h + 1] - split[g][h];
        }
        if (got != sh[h].n) return fail(ctx, RSX_ERR_INTERNAL, "exchange plan does not fill a slice");
    }
    for (uint32_t g = 0; g < G; ++g) {
        DeviceGuard dg(sh[g].c->device);
        for (uint32_t k = 0; k < G; ++k) {
            const uint32_t h = (g + k) % G;  // start with myself, then round the ring: spreads the links
            const uint64_t cnt = split[g][h + 1] - split[g][h];
            if (cnt == 0) continue;
            uint64_t at = 0;
            for (uint32_t p = 0; p < g; ++p) at += split[p][h + 1] - split[p][h];
            const char* s = src[g] + split[g][h] * es;
            char* d = dst[h] + at * es;
            if (sh[h].c->device == sh[g].c->device) {
                RSX_HIP(hipMemcpyAsync(d, s, cnt * es, hipMemcpyDeviceToDevice, sh[g].c->shard_stream));
            } else {
                enable_peer(sh[g].c->device, sh[h].c->device);
                RSX_HIP(hipMemcpyPeerAsync(d, sh[h].c->device, s, sh[g].c->device, cnt * es, sh[g].c->shard_stream));
            }
        }
    }
    return sync_all(ctx, sh);
}

}  // namespace

int rsx_sort_sharded_ex(rsx_ctx* const* ctxs, uint32_t ndev, void* const* d_slices, void* const* d_tmps,
                        const size_t* n_per_dev, const rsx_layout* L, int schedule) try {
    if (!ctxs || ndev == 0 || !ctxs[0]) return RSX_ERR_ARG;
    rsx_ctx* ctx = ctxs[0];  // carries the error text
    if (!d_slices || !d_tmps || !n_per_dev) return fail(ctx, RSX_ERR_ARG, "null table");
    if (schedule != RSX_SHARD_EXCHANGE_FIRST && schedule != RSX_SHARD_SORT_FIRST) return fail(ctx, RSX_ERR_ARG, "unknown schedule");
    const uint32_t G = ndev;
    if (G > 64) return fail(ctx, RSX_ERR_ARG, "more than 64 slices");
    std::vector<Shard> sh(G);
    const uint32_t al = L ? elem_align(L->elem_bytes) : 1;
    for (uint32_t g = 0; g < G; ++g) {
        if (!ctxs[g]) return fail(ctx, RSX_ERR_ARG, "null context in table");
        int rc = check_common(ctxs[g], L);
        if (rc) return rc == RSX_ERR_ARG ? fail(ctx, rc, "invalid rsx_layout") : fail(ctx, rc, "element size has no device kernel");
        if (n_per_dev[g] && (!d_slices[g] || !d_tmps[g])) return fail(ctx, RSX_ERR_ARG, "null device pointer");
        if (n_per_dev[g] && (!aligned(d_slices[g], al) || !aligned(d_tmps[g], al))) return fail(ctx, RSX_ERR_ARG, "device pointer misaligned");
        for (uint32_t h = 0; h < g; ++h)
            if (ctxs[h] == ctxs[g]) return fail(ctx, RSX_ERR_ARG, "one context per slice");
        sh[g] = Shard{ctxs[g], static_cast<char*>(d_slices[g]), static_cast<char*>(d_tmps[g]), n_per_dev[g]};
    }
    const size_t es = L->elem_bytes;
    const uint32_t D = L->key_bytes;
    for (uint32_t g = 0; g < G; ++g) {
        int rc = shard_prepare(ctx, ctxs[g]);
        if (rc) return rc;
    }
    std::vector<char*> slices(G), tmps(G);
    for (uint32_t g = 0; g < G; ++g) {
        slices[g] = sh[g].data;
        tmps[g] = sh[g].tmp;
    }
    auto sort_all = [&]() -> int {
        for (uint32_t g = 0; g < G; ++g) {
            int rc = sort_async(ctx, sh[g].c, sh[g].data, sh[g].tmp, sh[g].n, L);
            if (rc) return rc;
        }
        return sync_all(ctx, sh);
    };
    if (G == 1) return sort_all();

    std::vector<uint64_t> bounds(G + 1, 0);
    for (uint32_t g = 0; g < G; ++g) bounds[g + 1] = bounds[g] + sh[g].n;
    const uint32_t nb = G - 1;
    std::vector<std::vector<uint64_t>> split(G, std::vector<uint64_t>(G + 1, 0));
    for (uint32_t g = 0; g < G; ++g) split[g][G] = sh[g].n;
    std::vector<std::vector<uint64_t>> cut;

    if (schedule == RSX_SHARD_SORT_FIRST) {
        int rc = sort_all();
        if (rc) return rc;
        std::vector<std::vector<Range>> rng(nb, std::vector<Range>(G));
        std::vector<uint64_t> rank(nb);
        for (uint32_t b = 0; b < nb; ++b) {
            rank[b] = bounds[b + 1];
            for (uint32_t g = 0; g < G; ++g) rng[b][g] = Range{0, sh[g].n};
        }
        rc = find_cuts(ctx, sh, slices, L, rng, rank, (int)D - 1, std::vector<uint64_t>(nb, 0), std::vector<uint64_t>(nb, 0), cut);
        if (rc) return rc;
        for (uint32_t b = 0; b < nb; ++b)
            for (uint32_t g = 0; g < G; ++g) split[g][b + 1] = cut[b][g];
        rc = exchange(ctx, sh, slices, tmps, split, es);
        if (rc) return rc;
        for (uint32_t g = 0; g < G; ++g) {  // back into the slices (an even number of passes ends where it starts)
            if (sh[g].n == 0) continue;
            DeviceGuard dg(sh[g].c->device);
            RSX_HIP(hipMemcpyAsync(sh[g].data, sh[g].tmp, sh[g].n * es, hipMemcpyDeviceToDevice, sh[g].c->shard_stream));
        }
        return sort_all();
    }

    // ---- exchange first ----
    // (1) one stable partition pass by the most significant digit, slice -> tmp, with its 256 counts
    const uint32_t top = D - 1;
    for (uint32_t g = 0; g < G; ++g) {
        rsx_ctx* c = sh[g].c;
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceGuard dg(c->device);
        uint64_t* hh = c->shard_host + (size_t)64 * RADIX * 2;  // pinned: this slice's 256 counts
        if (sh[g].n == 0) {
            std::memset(hh, 0, RADIX * sizeof(uint64_t));
            continue;
        }
        int rc = partition_locked(c, sh[g].data, sh[g].tmp, sh[g].n, L, top, c->shard_hist, c->shard_stream);
        if (rc) return c != ctx ? fail(ctx, rc, c->err.c_str()) : rc;
        RSX_HIP(hipMemcpyAsync(hh, c->shard_hist, RADIX * sizeof(uint64_t), hipMemcpyDeviceToHost, c->shard_stream));
    }
    int rc = sync_all(ctx, sh);
    if (rc) return rc;
    // (2) global layout of the buckets; which boundaries fall inside one
    std::vector<std::vector<uint64_t>> lstart(G, std::vector<uint64_t>(RADIX + 1, 0));
    std::vector<uint64_t> gstart(RADIX + 1, 0);
    for (uint32_t v = 0; v < RADIX; ++v) {
        uint64_t tot = 0;
        for (uint32_t g = 0; g < G; ++g) {
            const uint64_t c = sh[g].c->shard_host[(size_t)64 * RADIX * 2 + v];
            lstart[g][v + 1] = lstart[g][v] + c;
            tot += c;
        }
        gstart[v + 1] = gstart[v] + tot;
    }
    for (uint32_t g = 0; g < G; ++g)
        if (lstart[g][RADIX] != sh[g].n) return fail(ctx, RSX_ERR_INTERNAL, "digit counts do not add up to the slice");
    std::vector<uint32_t> inside;       // boundaries that fall strictly inside a bucket
    std::vector<uint32_t> bucket_of(nb, RADIX);
    bool sorted_bucket[RADIX] = {false};
    for (uint32_t b = 0; b < nb; ++b) {
        const uint64_t T = bounds[b + 1];
        uint32_t v = 0;
        while (v < RADIX && gstart[v + 1] <= T) ++v;  // first bucket that ends above T
        bucket_of[b] = v;
        if (v == RADIX || gstart[v] == T) {
            for (uint32_t g = 0; g < G; ++g) split[g][b + 1] = v == RADIX ? sh[g].n : lstart[g][v];
            continue;
        }
        inside.push_back(b);
        if (!sorted_bucket[v]) {  // every device sorts its piece of this bucket: tmp piece in place, slice piece as scratch
            sorted_bucket[v] = true;
            for (uint32_t g = 0; g < G; ++g) {
                const uint64_t off = lstart[g][v] * es;
                rc = sort_async(ctx, sh[g].c, sh[g].tmp + off, sh[g].data + off, lstart[g][v + 1] - lstart[g][v], L);
                if (rc) return rc;
            }
        }
    }
    if (!inside.empty()) {
        rc = sync_all(ctx, sh);
        if (rc) return rc;
        const uint32_t ni = (uint32_t)inside.size();
        std::vector<std::vector<Range>> rng(ni, std::vector<Range>(G));
        std::vector<uint64_t> rank(ni), pre_lo(ni, 0), pre_hi(ni, 0);
        for (uint32_t i = 0; i < ni; ++i) {
            const uint32_t b = inside[i], v = bucket_of[b];
            rank[i] = bounds[b + 1] - gstart[v];
            if (top < 8) pre_lo[i] = (uint64_t)v << (8 * top);
            else pre_hi[i] = (uint64_t)v << (8 * (top - 8));
            for (uint32_t g = 0; g < G; ++g) rng[i][g] = Range{lstart[g][v], lstart[g][v + 1]};
        }
        rc = find_cuts(ctx, sh, tmps, L, rng, rank, (int)top - 1, pre_lo, pre_hi, cut);
        if (rc) return rc;
        for (uint32_t i = 0; i < ni; ++i)
            for (uint32_t g = 0; g < G; ++g) split[g][inside[i] + 1] = lstart[g][bucket_of[inside[i]]] + cut[i][g];
    }
    // (3) the exchange, straight into the slices (their old contents live on in the tmps); (4) one local sort
    rc = exchange(ctx, sh, tmps, slices, split, es);
    if (rc) return rc;
    return sort_all();
} catch (...) {
    return RSX_ERR_NOMEM;
}

int rsx_sort_sharded(rsx_ctx* const* ctxs, uint32_t ndev, void* const* d_slices, void* const* d_tmps,
                     const size_t* n_per_dev, const rsx_layout* L) {
    return rsx_sort_sharded_ex(ctxs, ndev, d_slices, d_tmps, n_per_dev, L, RSX_SHARD_EXCHANGE_FIRST);
}

int rsx_generate_device(rsx_ctx* ctx, void* d_data, size_t n, const rsx_layout* L, int gen, uint64_t seed,
                        double param, uint64_t index_base, void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!layout_ok(L, true)) return fail(ctx, RSX_ERR_ARG, "invalid rsx_layout");
    if (L->elem_bytes > RSX_MAX_ELEM_BYTES) return fail(ctx, RSX_ERR_UNSUPPORTED, "element larger than RSX_MAX_ELEM_BYTES");
    if (n == 0) return RSX_OK;
    if (!d_data) return fail(ctx, RSX_ERR_ARG, "null pointer");
    const uint32_t payload_zero = (gen & RSX_GEN_PAYLOAD_ZERO) ? 1u : 0u;
    gen &= ~RSX_GEN_PAYLOAD_ZERO;
    if (gen < RSX_GEN_UNIFORM || gen > RSX_GEN_GEOMETRIC) return fail(ctx, RSX_ERR_ARG, "unknown generator");
    uint64_t iparam = 0;
    if (gen == RSX_GEN_STEP) {
        if (!(param >= 1.0)) return fail(ctx, RSX_ERR_ARG, "step generator needs param >= 1");
        iparam = (uint64_t)param;
    } else if (gen == RSX_GEN_CONSTANT) {
        iparam = (uint64_t)param;
    } else if (gen == RSX_GEN_GEOMETRIC) {
        if (!(param > 0.0 && param < 1.0)) return fail(ctx, RSX_ERR_ARG, "geometric generator needs 0 < param < 1");
        // -log2(1 - p) as 32.32 fixed point (made on the host, once: the kernel divides by it)
        const double c = -std::log2(1.0 - param) * 4294967296.0;
        iparam = c < 1.0 ? 1ull : c >= 18446744073709551615.0 ? ~0ull : (uint64_t)c;
    } else if (gen == RSX_GEN_ZIPF) {
        if (!(param > 0.0)) return fail(ctx, RSX_ERR_ARG, "Zipf generator needs param > 0");
    }
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    uint64_t blocks = (n + 255) / 256;
    const uint64_t cap = (uint64_t)ctx->num_cu * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(rsx_generate_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, static_cast<uint8_t*>(d_data),
                       (uint64_t)n, L->elem_bytes, L->key_offset, L->key_bytes, gen, seed, param, iparam, index_base,
                       payload_zero);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

int rsx_verify_device(rsx_ctx* ctx, const void* d_data, size_t n, const rsx_layout* L, uint64_t* d_out,
                      void* stream) try {
    if (!ctx) return RSX_ERR_ARG;
    if (!layout_ok(L, true)) return fail(ctx, RSX_ERR_ARG, "invalid rsx_layout");
    if (L->elem_bytes > RSX_MAX_ELEM_BYTES) return fail(ctx, RSX_ERR_UNSUPPORTED, "element larger than RSX_MAX_ELEM_BYTES");
    if (!d_out) return fail(ctx, RSX_ERR_ARG, "null pointer");
    RSX_ENTER(stream);
    const hipStream_t st = held.st;
    RSX_HIP(hipMemsetAsync(d_out, 0, 3 * sizeof(uint64_t), st));
    if (n == 0) return RSX_OK;
    if (!d_data) return fail(ctx, RSX_ERR_ARG, "null pointer");
    uint64_t blocks = (n + 255) / 256;
    const uint64_t cap = (uint64_t)ctx->num_cu * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(rsx_verify_kernel, dim3((uint32_t)blocks), dim3(256), 0, st,
                       static_cast<const uint8_t*>(d_data), (uint64_t)n, L->elem_bytes, L->key_offset, L->key_bytes,
                       L->key_kind, d_out);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
} catch (...) {
    return RSX_ERR_HIP;
}

}  // extern "C"
