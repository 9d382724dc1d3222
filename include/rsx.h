/*
 * rsx.h -- C-ABI of the MI355X-native LSD radix sort (librsx.so).
 *
 * This is the drop-in boundary for the hot path of jgrodzki/radix_sort:
 *     impl<T: RadixDigits> RadixSort<T> for [T] { fn radix_sort(&mut self) }
 *         reference src/radix_sort/mod.rs:18-20,61-176
 *     trait RadixDigits { const NUMBER_OF_DIGITS: u8; fn get_digit(&self, u8) -> u8 }
 *         reference src/radix_sort/radix_digits.rs:1-5 (+ impls :7-136)
 * The reference has no FFI layer of its own (pure Rust, bin crate); these are
 * the entry points a Rust `extern "C"` block would bind so that the body of
 * `radix_sort()` becomes one call (binding shown in INTEGRATION.md).
 *
 * Plain pointers and sizes only; no C++/torch types.  Every function returns
 * an `int` status (0 = RSX_OK, negative = error) and never unwinds.
 */
#ifndef RSX_H
#define RSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSX_VERSION 200 /* 0.2.0 */

/* status codes */
enum {
    RSX_OK = 0,
    RSX_ERR_ARG = -1,         /* bad pointer / size / layout */
    RSX_ERR_UNSUPPORTED = -2, /* element size or key width without a device kernel */
    RSX_ERR_HIP = -3,         /* a HIP runtime call failed; see rsx_last_error */
    RSX_ERR_NOMEM = -4,       /* device workspace allocation failed */
    RSX_ERR_NODEVICE = -5,    /* no gfx950-class device / wrong device */
    RSX_ERR_WORKSPACE = -6,   /* the call would have to allocate while its stream is being captured:
                                 rsx_ctx_reserve first */
    RSX_ERR_INTERNAL = -7     /* a bounded device-side wait gave up (protocol error); results invalid */
};

/* How a key is mapped to its order-preserving unsigned form before digits are
 * taken; restates radix_digits.rs. */
enum {
    RSX_KEY_UNSIGNED = 0, /* u8,u16,u32,u64,u128,usize      radix_digits.rs:7-53   */
    RSX_KEY_SIGNED = 1,   /* i8..i128,isize: x ^ MIN        radix_digits.rs:55-101 */
    RSX_KEY_FLOAT = 2     /* f32,f64: b ^= (b>>31)|MIN      radix_digits.rs:103-124 */
};

/* Element descriptor: what `T: RadixDigits` means to the device.
 *   elem_bytes  size_of::<T>(), 1 .. RSX_MAX_ELEM_BYTES
 *   key_offset  byte offset of the key inside the element (0 for primitives;
 *               offset_of!((K,U), 0) for tuples, radix_digits.rs:126-136);
 *               key_offset + key_bytes <= elem_bytes
 *   key_bytes   T::NUMBER_OF_DIGITS (8-bit digits, LSB first): 1 .. 16 for
 *               RSX_KEY_UNSIGNED / RSX_KEY_SIGNED (a signed key of k bytes is the
 *               k-byte two's-complement integer), 4 or 8 for RSX_KEY_FLOAT
 *   key_kind    RSX_KEY_*
 * Elements are moved bitwise (mod.rs:133-140 uses copy_nonoverlapping), so any
 * payload -- padding included -- is carried unchanged.
 *
 * Any layout.  Element sizes 1,2,4,8,12,16,24,32 with key widths 1,2,4,8,16 have
 * sort kernels of their own ("direct" layouts; d_data and d_tmp aligned to the
 * element's natural alignment: 1, 2, 4 for 4 and 12 bytes, 8 for 8 and 24, 16
 * for 16 and 32).  rsx_sort_device, rsx_sort_host and rsx_ctx_reserve take every
 * other layout above too and hand it to those kernels through a CANONICAL key:
 * the key moved to offset 0 and widened to the next of 1,2,4,8,16 bytes (zero-
 * or sign-extended).  The route (RSX_INFO_LAST_PASSES bits 28-29):
 *   1 packed re-layout, when the canonical key plus the other elem_bytes -
 *     key_bytes bytes fit 16: the elements are re-laid out into a workspace array
 *     of n*s' bytes (s' that sum rounded up to 4, 8, 12 or 16), sorted there
 *     with a second array of n*s' bytes as ping-pong, and restored into d_data;
 *     d_tmp is not used;
 *   2 key-index proxy, for larger elements: (canonical key, u32 position)
 *     proxies of p = 8 (keys up to 4 bytes), 16 (up to 8) or 32 bytes are
 *     sorted in two workspace arrays of n*p bytes, and d_data[i] =
 *     d_tmp[proxy[i].position] after the elements were copied into d_tmp; n must
 *     be below 2^32 (RSX_ERR_UNSUPPORTED otherwise).
 * The workspace of a route is the context's (2*n*s' or 2*n*p bytes, each array
 * rounded up to 256 bytes, beside the direct sort's own), made on first use or by
 * rsx_ctx_reserve(n, layout); such layouts need only 1-byte alignment of d_data
 * and d_tmp, may overwrite d_tmp, and leave every byte outside the n elements
 * as it was.  Results are bit-exact with the stable sort by mapped key.  Of the
 * other entry points, histogram, partition*, sort_segments / sort_rows and
 * sort_sharded* take direct layouts only (RSX_ERR_UNSUPPORTED otherwise);
 * bounds* and splitter* read the key where it lies, so they take elements of any
 * size (no alignment asked) whose key is 1, 2, 4, 8 or 16 bytes wide, and refuse
 * other key widths with RSX_ERR_ARG; rsx_generate_device and rsx_verify_device
 * take any layout of up to RSX_MAX_ELEM_BYTES (RSX_ERR_UNSUPPORTED above, as for
 * the sorts). */
#define RSX_MAX_ELEM_BYTES 32768u
typedef struct rsx_layout {
    uint32_t elem_bytes;
    uint32_t key_offset;
    uint32_t key_bytes;
    uint32_t key_kind;
} rsx_layout;

/* Owns the device workspace of its sorts.  Any number of threads may call into one context (calls
 * are serialised by a mutex) and its calls may name different streams: work enqueued on a stream
 * other than the context's previous one first waits, on the device, for that previous work (the
 * workspace belongs to one sort at a time).  Use one context per stream to run sorts concurrently. */
typedef struct rsx_ctx rsx_ctx;

/* -- context ------------------------------------------------------------- */
/* Binds a context to HIP device `device` (-1 = current device). */
int rsx_ctx_create(int device, rsx_ctx **out);
int rsx_ctx_destroy(rsx_ctx *ctx);
/* Pre-allocates the internal workspace for sorts of up to `n` elements of
 * `layout` so that rsx_sort_device performs no allocation (stream-capture
 * safe).  Replaces the reference's per-call temp-buffer allocation + page
 * touch (mod.rs:71-82) for everything except the caller-owned ping-pong
 * buffer. */
int rsx_ctx_reserve(rsx_ctx *ctx, size_t n, const rsx_layout *layout);
/* Synchronises `stream` and reports RSX_ERR_INTERNAL if any kernel of this
 * context flagged a device-side protocol error since the last check (the
 * reference panics on worker failure, mod.rs:106; across a C ABI that becomes
 * a status), then clears the condition.  The error word is host-visible, so a
 * pending error also fails the NEXT rsx_sort_device / rsx_partition_device on
 * the context without any synchronisation; callers of the stream-ordered entry
 * points should still call this at their own sync point -- it is the only way
 * to learn that the sort just enqueued went wrong.  rsx_sort_host and
 * rsx_sort_sharded check by themselves. */
int rsx_ctx_check(rsx_ctx *ctx, void *stream);
/* Alternative code paths of the sweep kernel; every one gives the same bytes (they exist as
 * fall-backs that the library selects itself when a device self-test fails, and are exposed so
 * that callers and tests can force them).  RSX_OPT_HOST_CHUNK is the one option of the host path. */
enum {
    RSX_OPT_TILE_SCHEDULE = 1, /* 0 (default): static tile assignment behind a start-up roll call, tickets if
                                  it fails; 1: ticketed tiles always */
    RSX_OPT_RANKING = 2,       /* 0 (default): ranks from returned LDS atomics where the device's ordering
                                  self-test passed and the tile is not skewed, wave ballots otherwise;
                                  1: ballots only; 2: LDS atomics whatever the skew */
    RSX_OPT_STATUS_SCOPE = 3,  /* 0 (default): look-back status words of a verified single-XCD chain stay in
                                  that XCD's L2; 1: agent-scope stores everywhere */
    RSX_OPT_XCD_MAJOR = 4,     /* 1 (default): workgroups numbered XCD-major; 0: by blockIdx */
    RSX_OPT_BYTE_COUNTING = 5, /* 1 (default): u8/i8 arrays, and u16/i16 arrays of at least 2^23 elements, by counting
                                  (the element is its key: the histogram is the sorted array); 0: through the general passes */
    RSX_OPT_MAX_REGIONS = 6,   /* 0 (default: 8 or 16 by element size) .. 32 look-back chains per pass */
    RSX_OPT_HOT_LANES = 7,     /* 2..65 (default 16): lanes sharing a digit that mark a tile as skewed */
    RSX_OPT_VERBOSE = 8,       /* 1: launch geometry and self-test verdicts on stderr (also env RSX_VERBOSE=1) */
    RSX_OPT_RANK_CHECK = 9,    /* 1: in every tile, one round of LDS-atomic ranks is cross-checked against the
                                  ballot-derived ranks (the property rsx_lds_order_kernel tests on an idle device,
                                  here under the real sweeps' LDS contention); a mismatch makes rsx_ctx_check fail */
    RSX_OPT_SMALL_SORT = 10,   /* 1 (default): arrays of at most one tile (14336 4-byte, 7168 8-byte, 2560 16-byte
                                  elements ...) are sorted by ONE launch of one workgroup; 0: by the general path */
    RSX_OPT_MID_SORT = 11      /* middle-size arrays (up to 2^22 4-byte, 2^21 8-byte, 2^20 16-byte elements): when their most
                                  significant digit spreads them over its 256 buckets, one sweep makes the buckets and one
                                  workgroup per bucket sorts it in LDS (two trips through memory instead of D).  1 (default):
                                  the host forecasts from what the context's previous middle-size sort reported; an input
                                  that is skewed after all is still sorted correctly (an oversized bucket goes through
                                  memory), then the context keeps to LSD passes for its next sorts.  0: LSD passes always,
                                  top digit not even counted.  2: always split.  3: always LSD passes. */,
    RSX_OPT_WIDE_SORT = 12,    /* large arrays of 8-byte (and wider) keys: count the top 16 bits of the key, two sweeps for
                                  those two digits, then every 16-bit bucket sorted by its remaining digits in LDS.
                                  0: never; 1 (default): by key width and size (8- and 16-byte keys above the middle sizes, 4-byte keys in
                                  8-byte elements from 1 GiB, in wider ones from 2 GiB), when the count says every bucket
                                  fits (a handful of larger ones is tolerated, unless 32768 elements of one lie so close
                                  together in the input that one count workgroup meets them all: padding, a pre-sorted
                                  block -- then, as after any refusal, the LSD passes run and RSX_INFO_LAST_PASSES
                                  reports path 0); 2: always (any array of 65536+ such elements, buckets that do not fit go through
                                  memory); 3: as 1 without the size floor (above the middle sizes) */
    RSX_OPT_BUCKET_SKIP = 13,  /* the LDS passes of the bucket kernels: 1 (default) start at the digit that leaves them the
                                  bits an array of that size is, as a rule, told apart by (2 log2 m - 6 of its variable
                                  bits: three passes for a 16-bit bucket of 2^30 u64 keys) and put right the neighbours
                                  that still agree, by the digits skipped; 0: every pass */
    RSX_OPT_BUCKET_GROUP = 14, /* the hybrid on arrays whose 16-bit buckets are small (8-byte and wider keys): 1 (default)
                                  a workgroup sorts a group of consecutive buckets as one array; 0: bucket by bucket */
    RSX_OPT_BUCKET_DIRECT = 15,/* the hybrid's buckets of key-only elements of 8 and 16 bytes (the key is the whole element:
                                  u64, i64, f64, u128 -- equal elements are the same bytes): 1 (default) one unstable
                                  counting pass in LDS and an exact rank among neighbours, buckets of few distinct keys
                                  left to the stable passes; 0: the stable passes always.  Same bytes either way.
                                  No effect where groups of small buckets are on offer (RSX_OPT_BUCKET_GROUP: arrays up to
                                  about 2^26 8-byte / 2^25 16-byte elements): those sorts keep to the stable passes. */
    RSX_OPT_HOST_CHUNK = 16    /* rsx_sort_host: the bytes of one piece of its copy pipeline, a multiple of 4096 in
                                  4096 .. 33554432 (32 MiB, the default; anything else is RSX_ERR_ARG and leaves the value
                                  as it was).  The four pinned buffers of the ring keep their 32 MiB whatever the value:
                                  a smaller one only shortens the pieces.  Same bytes at every value; exposed so that
                                  tests reach the ring's slot reuse, the short last piece and the drain of the copy
                                  back with arrays of a few KB instead of hundreds of MB. */
};
int rsx_ctx_set_option(rsx_ctx *ctx, int option, uint64_t value);
enum {
    RSX_INFO_RANK_ATOMIC = 1, /* 1 if the LDS atomic ordering self-test passed on this device */
    RSX_INFO_L2_LOCAL = 2,    /* 1 if the same-XCD hand-off self-test passed on this device */
    RSX_INFO_NUM_CU = 3,
    RSX_INFO_DEVICE = 4,
    RSX_INFO_LAST_PASSES = 5, /* which tile schedule the passes of the context's LAST sort ran with (waits for it):
                                 bits 0-7 sweep passes launched (0: one-launch or counting path), bits 8-15 of them
                                 with static tiles (the roll call succeeded), bits 16-23 of them with the XCD
                                 placement verified (status words of single-XCD chains stay in L2), bits 24-27 the
                                 path: 0 general passes, 1 one-launch sort of at most one tile, 2 middle-size bucket
                                 split, 3 one-byte counting, 4 two-byte counting, 5 wide-key hybrid (two sweeps + the
                                 16-bit buckets in LDS; a hybrid the device refused reports 0 and its D passes),
                                 6 segmented sort (rsx_sort_segments_device, rsx_sort_rows_device: bits 0-7 are then
                                 the kernels launched, one per size class, and bits 8-23 are 0),
                                 7 top-k (rsx_topk_rows_device: bits 0-7 are then the kernels launched, one per round
                                 of the selection, and bits 8-23 are 0),
                                 8 groups of equal keys (rsx_unique_device: bits 0-7 are then the kernels launched
                                 after the sort of the joined elements, and bits 8-23 are 0),
                                 9 reduce by key (rsx_reduce_by_key_device: bits 0-7 and 8-23 as for path 8),
                                 10 search (rsx_search_sorted_device: bits 0-7 are then the kernels launched after
                                 any sort of the needles, bit 8 is set when they were sorted first, bits 9-23 are 0),
                                 11 merge (rsx_merge_device: bits 0-7 are then the kernels launched, bit 8 is set on the
                                 wide-value route, bits 9-23 are 0),
                                 12 set operation (rsx_setop_device: bits 0-7 are then the kernels launched, bits 8-23
                                 are 0),
                                 13 join (rsx_join_device: bits 0-7 are then the kernels launched -- 0, 2 for the
                                 count-only form, 3 otherwise -- and bits 8-23 are 0),
                                 14 scan by key (rsx_scan_by_key_device: bits 0-7 are then the kernels launched after
                                 any sort, bit 8 is set under RSX_SCAN_RUNS, bits 9-23 are 0),
                                 15 order statistics (rsx_select_device: bits 0-7 are then the kernels launched, bits
                                 8-11 are 0 when the candidates were never compacted, else 1 + the level after which
                                 they were -- read from the device, so this waits for the call --, bits 12-23 are 0),
                                 16 keys per bin (rsx_bin_count_device: the four bits are full, so this path is the
                                 value of bits 24-28, bits 24-27 zero and bit 28 set; bits 0-7 are then the kernels
                                 launched, every other bit is 0 -- a bin count has no route),
                                 17 rows that pass a predicate (rsx_compact_device: reported like 16, bits 24 and 28
                                 set; bits 0-7 are the kernels launched),
                                 18 rows regrouped by bin (rsx_multisplit_device: reported like 16, bits 25 and 28
                                 set; bits 0-7 are the kernels launched),
                                 19 a value column combined per bin (rsx_bin_reduce_device: reported like 16, bits
                                 24, 25 and 28 set; bits 0-7 are the kernels launched),
                                 bits 28-29 the route of a layout without kernels of its own: 0 direct, 1 packed
                                 re-layout, 2 key-index proxy (bits 0-27 then describe the sort of the re-laid-out
                                 elements / of the proxies) */
    RSX_INFO_LAST_PAIRS = 6,  /* how the context's last rsx_sort_pairs_device / rsx_argsort_device call ran: 0 none yet,
                                 1 joined elements, 2 proxies and gather; bits 8-15 the size of the joined element (of
                                 the proxy).  RSX_INFO_LAST_PASSES describes the inner sort of those elements.
                                 The segmented key / value calls report 3, fused per segment (the joined elements exist
                                 in registers and LDS only), or 4, fused per segment on (key, position) proxies followed
                                 by a gather of the values; bits 8-15 as above, RSX_INFO_LAST_PASSES path 6. */
    RSX_INFO_LAST_DIRECT = 7, /* the context's last sort (waits for it): ~0 if it did not enqueue the direct bucket kernel
                                 (RSX_OPT_BUCKET_DIRECT) or the device refused the hybrid, else the number of buckets
                                 that kernel left to the stable passes -- 0 when it sorted every bucket */
    RSX_INFO_LAST_LEX = 8     /* the context's last rsx_lexsort_device / rsx_sort_columns_device call that sorted (n >= 2;
                                 0 none yet): bits 0-7 the rounds it ran, bits 8-15 the bytes of the joined element of
                                 its last round.  RSX_INFO_LAST_PASSES describes the inner sort of that round. */
};
int rsx_ctx_get_info(rsx_ctx *ctx, int what, uint64_t *out);
/* Per-launch timing with HIP events on the launch stream (measurement only).
 * rsx_ctx_profile(ctx, 1) clears the counters and makes every later kernel
 * launch of this context record a start/stop event pair around itself;
 * rsx_ctx_profile(ctx, 0) stops recording.  rsx_ctx_profile_read waits for the
 * recorded events and returns, per kernel kind, the summed duration in
 * milliseconds and the number of launches (arrays of RSX_PROF_KINDS). */
enum { RSX_PROF_HIST = 0, RSX_PROF_SCAN = 1, RSX_PROF_SWEEP = 2, RSX_PROF_OTHER = 3, RSX_PROF_KINDS = 4 };
int rsx_ctx_profile(rsx_ctx *ctx, int enable);
int rsx_ctx_profile_read(rsx_ctx *ctx, double *ms, uint64_t *launches);
/* Last error text for this context (never NULL). */
const char *rsx_last_error(const rsx_ctx *ctx);
const char *rsx_strerror(int status);
int rsx_version(void);

/* -- the sort ------------------------------------------------------------ */
/* In-place ascending stable sort of `n` elements resident in device memory:
 * the device-side body of `<[T]>::radix_sort` (mod.rs:62-175).  `d_tmp` is the
 * ping-pong buffer (the reference's `temp`, mod.rs:71-83), n*elem_bytes bytes,
 * caller-owned.  All work is enqueued on `stream` (a hipStream_t, NULL =
 * default stream); the call does not synchronise the device.  On return the
 * result is (stream-ordered) in `d_data`, as after mod.rs:170-174. */
int rsx_sort_device(rsx_ctx *ctx, void *d_data, void *d_tmp, size_t n, const rsx_layout *layout,
                    void *stream);

/* Literal drop-in for `&mut [T]` in host memory: H2D, rsx_sort_device, D2H,
 * blocking (mod.rs:62 is blocking too).  The copies run as a pipeline over a ring of
 * pinned chunks (the slice itself is pageable).  PCIe-bound; not the measured path. */
int rsx_sort_host(rsx_ctx *ctx, void *data, size_t n, const rsx_layout *layout);

/* -- many segments of one array ------------------------------------------ */
/* Sorts every segment [d_offsets[i], d_offsets[i+1]) of d_data, i in [0, nseg), independently: ascending, stable,
 * in place, by the mapped key of `layout` -- the bytes rsx_sort_device would leave if called on each segment.
 * d_offsets: nseg + 1 uint64 ON THE DEVICE, in elements, non-decreasing, d_offsets[nseg] <= n.  Elements in front
 * of d_offsets[0] and behind d_offsets[nseg] are not touched.  d_tmp: n * elem_bytes, caller-owned, may be
 * overwritten.  max_seg_len: an upper bound on the segment lengths that the caller vouches for, 0 = unknown.
 * Stream-ordered, no synchronisation, no workspace: once a context has made its first call of any kind (which
 * creates its error word and runs its self-tests, and therefore cannot be a captured one), this call allocates
 * nothing and can be captured into a graph without rsx_ctx_reserve.  Direct layouts only (RSX_ERR_UNSUPPORTED
 * otherwise); nseg == 0 succeeds and launches nothing.
 *
 * Every segment is sorted by ONE workgroup.  Size classes by length: RSX_SEG_CLASSES classes that sort inside LDS
 * (256 and 1024 threads; rsx_segment_caps) and one that sorts through memory (LSD passes between d_data and
 * d_tmp by one workgroup: correct for any length below 2^32, slow for long segments).  The lengths live on the
 * device, so one kernel per class is launched and its workgroups pick their segments from d_offsets themselves;
 * max_seg_len drops the classes that cannot occur (a segment longer than vouched for is left unsorted or
 * sorted, never out of bounds).  RSX_INFO_LAST_PASSES then reports path 6 and, in bits 0-7, the kernels launched.
 *
 * The offsets are not trusted: the host never reads them, and a segment with begin > end, end > n or 2^32 and
 * more elements is left untouched and sets the context's error word (rsx_ctx_check and the next call report
 * RSX_ERR_INTERNAL).  No kernel reads or writes outside the n elements of d_data and d_tmp whatever the offsets
 * hold.  Overlapping segments cannot be detected: the contents of the overlapping segments are then undefined
 * (still a permutation of nothing in particular, still in bounds). */
int rsx_sort_segments_device(rsx_ctx *ctx, void *d_data, void *d_tmp, size_t n, const rsx_layout *layout,
                             const uint64_t *d_offsets, size_t nseg, uint64_t max_seg_len, void *stream);
/* The same for `rows` segments of `row_len` elements each, back to back (a contiguous 2-D array sorted along its
 * last dimension): no offsets array, and the host knows the length, so exactly the launches needed are made (one).
 * d_tmp: rows * row_len * elem_bytes.  rows == 0 and row_len <= 1 succeed and launch nothing; rows * row_len
 * overflowing is RSX_ERR_ARG.  A row_len above the largest LDS class is sorted by one rsx_sort_device per row on
 * its sub-range (with that sort's rules: under capture rsx_ctx_reserve(row_len, layout) first, RSX_ERR_WORKSPACE
 * otherwise; RSX_INFO_LAST_PASSES then describes the last row's sort) -- unless there are at least as many rows
 * as the device has CUs and row_len is at most four times that class: then one launch of the through-memory
 * class takes them (path 6).  Per-row sorts are efficient once rows have millions of elements; rows between the
 * LDS capacity and the middle sizes stay slow either way (a launch sequence, or one workgroup's passes through
 * memory, per row). */
int rsx_sort_rows_device(rsx_ctx *ctx, void *d_data, void *d_tmp, size_t rows, size_t row_len,
                         const rsx_layout *layout, void *stream);
/* Host-only, needs no device: caps[c] = the longest segment that size class c sorts inside LDS for this layout
 * (ascending; RSX_SEG_CLASSES entries).  Longer segments go through memory. */
#define RSX_SEG_CLASSES 2
int rsx_segment_caps(const rsx_layout *layout, uint32_t *caps);

/* -- separate key and value arrays ---------------------------------------- */
/* The callers who hold a column of keys and a column of values (or want the permutation) instead of one array of
 * elements.  Order of every call: the STABLE permutation p by mapped key (the radix_digits.rs mapping, as everywhere
 * else: a total order on bit patterns, -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN for floats) -- ascending, or
 * descending = larger mapped key first, equal keys still in input order (torch.sort(stable=True, descending=True)).
 *
 * All three are stream-ordered, do not synchronise and take no caller scratch: the joined elements live in the
 * context's workspace (two arrays of n * s bytes, s the joined element's size, each rounded up to 256 bytes, and on
 * route 2 a copy of the values), made on first use or by rsx_ctx_reserve_pairs; under stream capture without a
 * sufficient reserve they return RSX_ERR_WORKSPACE and enqueue nothing.  Bad widths, kinds, orders or alignments, and
 * null pointers with n > 0: RSX_ERR_ARG.  n of 0 or 1 succeeds without a sort.  No byte outside the n keys / n values /
 * n indices is written.  The route is chosen from the widths alone (RSX_INFO_LAST_PAIRS):
 *   1 joined elements: the mapped key (complemented for descending order) and the value behind it, aligned to the
 *     value's alignment up to 4, fit an element size with sort kernels (1,2,4,8,12,16,24,32, a multiple of the key
 *     width): a join kernel writes the elements, they are sorted as RSX_KEY_UNSIGNED, a split kernel writes the two
 *     columns back.  Keys alone in ascending order are sorted where they lie, the workspace as ping-pong array;
 *   2 proxies and gather, for wider values: (mapped key, u32 position) proxies are sorted, the keys written from them
 *     and the values gathered through the copy; n must be below 2^32 (RSX_ERR_UNSUPPORTED otherwise). */
enum { RSX_ORDER_ASCENDING = 0, RSX_ORDER_DESCENDING = 1 };

/* keys: n keys of key_bytes (1, 2, 4, 8, 16; RSX_KEY_FLOAT: 4 or 8), packed, naturally aligned (16-byte keys: 16).
 * values: n values of value_bytes (1 .. RSX_MAX_ELEM_BYTES) each, packed, moved bitwise, aligned to the largest
 * power of two (at most 16) that divides value_bytes.  d_values == NULL and value_bytes == 0: keys only.
 * Both arrays are sorted in place: keys[i], values[i] = keys_in[p[i]], values_in[p[i]].  Arrays whose base addresses
 * are 16-byte aligned and values of 1, 2, 4, 8 or 16 bytes take the typed join and split kernels; anything else a
 * slower element-by-element form. */
int rsx_sort_pairs_device(rsx_ctx *ctx, void *d_keys, void *d_values, size_t n, uint32_t key_bytes,
                          uint32_t key_kind, uint32_t value_bytes, int order, void *stream);
/* d_keys is only read; d_index receives p as n integers of index_bytes (4 or 8; naturally aligned).  n == 1 writes
 * the one 0.  Positions are joined as u32 while n < 2^32 and as u64 beyond (index_bytes 4 is then
 * RSX_ERR_UNSUPPORTED). */
int rsx_argsort_device(rsx_ctx *ctx, const void *d_keys, void *d_index, size_t n, uint32_t key_bytes,
                       uint32_t key_kind, uint32_t index_bytes, int order, void *stream);
/* Workspace for either call on up to n pairs of these widths, so that the call allocates nothing (stream capture);
 * for rsx_argsort_device pass value_bytes = index_bytes. */
int rsx_ctx_reserve_pairs(rsx_ctx *ctx, size_t n, uint32_t key_bytes, uint32_t value_bytes);

/* -- many segments of separate key and value arrays ------------------------ */
/* The segmented calls and the key / value calls combined: every segment [d_offsets[i], d_offsets[i+1]) (every row of
 * row_len) of the key column gets the stable permutation by mapped key that rsx_sort_pairs_device / rsx_argsort_device
 * would leave on that segment alone, ascending or descending, and the value column (1 .. RSX_MAX_ELEM_BYTES bytes a
 * value; d_values == NULL with value_bytes == 0: keys only, which is how plain keys are sorted in descending order per
 * segment) moves with it.  The argsort forms only read d_keys; d_index[i] receives the position INSIDE its segment,
 * 0 .. len-1, as index_bytes (4 or 8) wide integers: torch.sort(dim=-1).indices.  Key widths, kinds and alignments
 * are those of rsx_sort_pairs_device; the offsets follow the rules of rsx_sort_segments_device (on the device, never
 * read by the host, a bad segment left untouched with the error word set, nothing outside the n keys / values /
 * indices read or written, whatever lies outside [offsets[0], offsets[nseg]) as it was).  Index slots of segments of
 * length 0 are untouched, a segment of length 1 gets its one 0.
 *
 * Routes (RSX_INFO_LAST_PAIRS; RSX_INFO_LAST_PASSES reports path 6 and the kernels launched):
 *   3 fused per segment: values of 0, 1, 2, 4, 8 or 16 bytes, and positions.  One workgroup per segment reads its part
 *     of the two columns, sorts the joined (mapped key, value) elements in LDS and writes the columns back; one launch
 *     per size class of the JOINED element size (rsx_segment_pairs_caps).  The LDS classes touch no workspace and can be
 *     captured once the context has made its first call.  Segments above the largest LDS class are joined into the
 *     context's pairs workspace (the shape of rsx_ctx_reserve_pairs: for the argsort forms pass value_bytes = 4 or 8),
 *     sorted through memory by their workgroup and split back; that class is launched only when such a segment can
 *     occur (max_seg_len unknown or above the cap, row_len above the cap), and under capture without a sufficient
 *     reserve the call then returns RSX_ERR_WORKSPACE and enqueues nothing.
 *   4 wider values: the values are copied into the workspace, the fused kernels sort (key, u32 position in the array),
 *     write the keys in place and the positions into a workspace array, and a gather moves the values.  n must be
 *     below 2^32 (RSX_ERR_UNSUPPORTED otherwise).
 * Rows longer than the largest LDS class follow the rule of rsx_sort_rows_device: at least as many rows as the device
 * has CUs and row_len at most four times that class go through memory in one launch; otherwise rsx_sort_pairs_device /
 * rsx_argsort_device runs once per row on its sub-range (RSX_INFO_LAST_PAIRS then describes the last row's call).
 * Very short rows are the weak spot they are for rsx_sort_rows_device: one workgroup per row. */
int rsx_sort_segments_pairs_device(rsx_ctx *ctx, void *d_keys, void *d_values, size_t n, uint32_t key_bytes,
                                   uint32_t key_kind, uint32_t value_bytes, int order, const uint64_t *d_offsets,
                                   size_t nseg, uint64_t max_seg_len, void *stream);
int rsx_argsort_segments_device(rsx_ctx *ctx, const void *d_keys, void *d_index, size_t n, uint32_t key_bytes,
                                uint32_t key_kind, uint32_t index_bytes, int order, const uint64_t *d_offsets,
                                size_t nseg, uint64_t max_seg_len, void *stream);
int rsx_sort_rows_pairs_device(rsx_ctx *ctx, void *d_keys, void *d_values, size_t rows, size_t row_len,
                               uint32_t key_bytes, uint32_t key_kind, uint32_t value_bytes, int order, void *stream);
int rsx_argsort_rows_device(rsx_ctx *ctx, const void *d_keys, void *d_index, size_t rows, size_t row_len,
                            uint32_t key_bytes, uint32_t key_kind, uint32_t index_bytes, int order, void *stream);
/* Host-only, needs no device: caps[c] = the longest segment that size class c of the calls above sorts inside LDS for
 * these widths (RSX_SEG_CLASSES entries): rsx_segment_caps of the joined element, which for values without a fused
 * kernel -- and for the argsort forms, whatever index_bytes: pass value_bytes = 4 -- is the (key, u32 position) proxy. */
int rsx_segment_pairs_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t *caps);

/* -- the first k of every row --------------------------------------------- */
/* Top-k along the rows of a (rows, row_len) key array without sorting the rows.  One definition: let p_r be the stable
 * permutation of row r that rsx_argsort_rows_device produces in `order` (ascending or descending by mapped key, equal
 * keys in input order, floats by the total order on bit patterns); then, for i in [0, k),
 *     d_out_keys[r*k + i] = d_keys[r*row_len + p_r[i]],    d_out_index[r*k + i] = p_r[i]
 * -- the first k columns of the full sort, byte for byte: sorted output, and ties at the threshold go to the lowest
 * positions.  d_keys is only read.  Key widths, kinds and alignments are those of rsx_argsort_rows_device; index_bytes
 * is 4 or 8; either output pointer may be NULL (that output is not produced), not both.  A flat array is rows == 1.
 * RSX_ERR_ARG: k > row_len, rows * row_len overflowing, bad widths, kinds, orders or alignments, both outputs NULL.
 * rows == 0 or k == 0 succeeds, launches nothing and looks at no pointer.  row_len >= 2^32 is RSX_ERR_UNSUPPORTED.  Stream-ordered, no
 * synchronisation; nothing outside the rows*k output keys and rows*k indices is written.
 *
 * One workgroup selects inside LDS: a most-significant-digit-first radix select over the joined (mapped key, u32
 * position) elements (at most key_bytes counting passes that move nothing), a compaction in position order, and the
 * stable sort of the k chosen elements.  Rows of at most caps[last] elements (rsx_topk_caps) take ONE launch, one
 * workgroup per row, and no workspace: once the context has made its first call of any kind the call can be captured.
 * Longer rows are a tournament: the row is cut into chunks of caps[last], every chunk leaves its min(k, length) best as
 * joined candidates, and the candidates of a row are the row of the next round until it fits one chunk (one launch per
 * round).  That needs k <= max_k (RSX_ERR_UNSUPPORTED otherwise: sort the row) and two workspace arrays of the first
 * round's candidates in the context, made on first use or by rsx_ctx_reserve_topk; under capture without a sufficient
 * reserve the call returns RSX_ERR_WORKSPACE and enqueues nothing.  RSX_INFO_LAST_PASSES reports path 7 and the rounds. */
int rsx_topk_rows_device(rsx_ctx *ctx, const void *d_keys, void *d_out_keys, void *d_out_index, size_t rows,
                         size_t row_len, size_t k, uint32_t key_bytes, uint32_t key_kind, uint32_t index_bytes,
                         int order, void *stream);
/* Workspace (and the context's first-call set-up) for rsx_topk_rows_device of this shape, so that the call allocates
 * nothing.  The argument rules are the call's. */
int rsx_ctx_reserve_topk(rsx_ctx *ctx, size_t rows, size_t row_len, size_t k, uint32_t key_bytes);
/* Host-only, needs no device: caps[c] = the longest row that size class c (256 and 1024 threads) selects inside LDS
 * for this key width (RSX_SEG_CLASSES entries, ascending: the classes of the joined (key, u32 position) element);
 * *max_k = the largest k accepted for rows longer than caps[last] (half of it). */
int rsx_topk_caps(uint32_t key_bytes, uint32_t *caps, uint32_t *max_k);

/* -- groups of equal keys -------------------------------------------------- */
/* What most callers do after a sort: which keys are equal, and where each group starts.  One definition: let p be the
 * stable permutation of the n keys that rsx_argsort_device produces in `order` (ascending or descending by mapped key,
 * equal keys in input order, floats by the total order on bit patterns), s[i] = d_keys[p[i]], and call position i a
 * HEAD when i == 0 or s[i] and s[i-1] differ in any bit (-0.0 and +0.0 are two keys, NaNs of different payloads are
 * different keys; the mapping is a bijection, so this is equality of mapped keys).  With the heads h[0] < ... < h[m-1]
 * and h[m] = n, every output optional through a NULL pointer but d_out_num:
 *     d_out_keys[j]    = s[h[j]], j < m: the distinct keys in order, as raw keys        (n entries of key_bytes)
 *     d_out_offsets[j] = h[j], j <= m: CSR offsets of the groups inside p, uint64; the counts are their differences --
 *                        the d_offsets of every rsx_*_segments* call, made on the device             (n + 1 entries)
 *     d_out_perm[i]    = p[i]: d_out_perm[h[j] .. h[j+1]) are the input positions of group j in input order, the first
 *                        of them its first occurrence                                (n entries of index_bytes)
 *     d_out_inverse[q] = the j with d_keys[q] == d_out_keys[j], for every input position q      (n entries of index_bytes)
 *     d_out_num[0]     = m, uint64
 * Entries of d_out_keys at m and beyond and of d_out_offsets beyond m are not written; nothing outside these arrays
 * and the context's workspace is written; d_keys is only read.  Key widths, kinds and alignments are those of
 * rsx_argsort_device; the outputs are naturally aligned (offsets and num: 8 bytes); index_bytes is 4 or 8 and looked at
 * only when d_out_perm or d_out_inverse is given.  RSX_ERR_ARG: bad widths, kinds, orders or alignments, d_out_num NULL,
 * d_keys NULL with n > 0.  n >= 2^32 is RSX_ERR_UNSUPPORTED.  n == 0 writes d_out_num[0] = 0 and d_out_offsets[0] = 0 with
 * stream-ordered memsets and launches nothing.  Stream-ordered, no synchronisation, no caller scratch: the host never
 * reads m.
 *
 * Two routes, chosen from the pointers alone.  Keys only (d_out_perm and d_out_inverse NULL): the mapped keys,
 * complemented for descending order, are sorted as elements of key_bytes.  With positions: (mapped key, u32 position)
 * elements of 8 bytes (keys of 1, 2 and 4 bytes), 16 (8-byte keys) or 32 (16-byte keys), the join of
 * rsx_argsort_device.  Either way the elements are sorted in the context's pairs workspace and three run kernels follow
 * instead of the split kernel: heads per tile, one workgroup's exclusive sum over the tiles (it writes m and
 * d_out_offsets[m]), and the write of the outputs.  No kernel waits for another workgroup.  d_out_inverse is a scatter by
 * input position, the one uncoalesced stream of the call.  The workspace -- the two element arrays and two per-tile
 * arrays -- is made on first use or by rsx_ctx_reserve_unique; under capture without a sufficient reserve the call
 * returns RSX_ERR_WORKSPACE and enqueues nothing.  RSX_INFO_LAST_PASSES reports path 8 and, in bits 0-7, the kernels
 * launched after the sort; RSX_INFO_LAST_PAIRS route 1 and the joined element's size. */
int rsx_unique_device(rsx_ctx *ctx, const void *d_keys, size_t n, uint32_t key_bytes, uint32_t key_kind, int order,
                      void *d_out_keys, uint64_t *d_out_offsets, void *d_out_perm, void *d_out_inverse,
                      uint32_t index_bytes, uint64_t *d_out_num, void *stream);
/* Workspace (and the context's first-call set-up) for rsx_unique_device on up to n keys of this width by the route
 * with positions (with_positions != 0) or keys only, so that the call allocates nothing (stream capture). */
int rsx_ctx_reserve_unique(rsx_ctx *ctx, size_t n, uint32_t key_bytes, int with_positions);
/* Host-only, needs no device: *tile = the elements one workgroup of the run kernels takes for this key width and
 * route, *scan_span = the tiles one sweep of the scan kernel's loop sums. */
int rsx_unique_caps(uint32_t key_bytes, int with_positions, uint32_t *tile, uint32_t *scan_span);

/* -- reduce by key ----------------------------------------------------------- */
/* What most callers do with a group: combine a column of values over it.  Let p, s, the heads h[0] < ... < h[m-1] and
 * h[m] = n be exactly those of rsx_unique_device for d_keys in `order`, and (+) the operator `op`.  Every output
 * optional through a NULL pointer but d_out_num, and at least one of d_out_keys and d_out_values given:
 *     d_out_keys[j]    = s[h[j]], j < m: the distinct keys in order, as raw keys        (n entries of key_bytes)
 *     d_out_values[j]  = d_values[p[h[j]]] (+) d_values[p[h[j]+1]] (+) ... (+) d_values[p[h[j+1]-1]], j < m: the values of
 *                        group j, taken in input order                                  (n entries of value_bytes)
 *     d_out_offsets[j] = h[j], j <= m: CSR offsets of the groups inside p, uint64               (n + 1 entries)
 *     d_out_num[0]     = m, uint64
 * Entries of d_out_keys and d_out_values at m and beyond and of d_out_offsets beyond m are not written; nothing outside
 * these arrays and the context's workspace is written; d_keys and d_values are only read.
 *
 * Keys: every width and kind of rsx_argsort_device (1, 2, 4, 8, 16 bytes; unsigned, signed, float).  Values: value_bytes
 * 4 or 8, value_kind RSX_KEY_UNSIGNED, RSX_KEY_SIGNED or RSX_KEY_FLOAT (u32, i32, f32, u64, i64, f64).  The operators:
 *     integer RSX_REDUCE_SUM wraps modulo 2^bits; integer MIN and MAX compare by the value's signedness;
 *     float MIN and MAX compare by the total order on bit patterns of the float keys (-NaN lowest, -0.0 below +0.0, +NaN
 *       highest): the result is the bit pattern of one of the group's values, exact and independent of association;
 *     float SUM is IEEE addition in the value's own type.  The association is the kernels': a function of (n, key_bytes,
 *       value_bytes, the group's start h[j] and length) alone -- the run kernels' tiling -- so the same input gives the
 *       same bytes on every call and every context; there are no floating-point atomics.  No zero is ever added: a group
 *       of -0.0 sums to -0.0.  Accuracy is the order-free bound |result - exact| <= g(c-1) * sum|v| for a group of c
 *       values, g(k) = k*u / (1 - k*u), u the unit roundoff of the value type.
 * RSX_ERR_ARG: bad widths, kinds, op, order or alignments (keys and d_out_keys: those of rsx_argsort_device; d_values and
 * d_out_values: value_bytes; offsets and num: 8 bytes), d_out_num NULL, d_keys or d_values NULL with n > 0, d_out_keys and
 * d_out_values both NULL.  n >= 2^32 is RSX_ERR_UNSUPPORTED.  n == 0 writes d_out_num[0] = 0 and d_out_offsets[0] = 0 with
 * stream-ordered memsets and launches nothing.  Stream-ordered, no synchronisation, no caller scratch: the host never
 * reads m.
 *
 * d_out_keys may be d_keys and d_out_values may be d_values: the first kernel of the call joins (mapped key, value)
 * elements of 8, 12, 16 or 32 bytes in the context's workspace -- the join of rsx_sort_pairs_device -- and has consumed
 * both inputs before the first output is stored; stream order guarantees it.  The elements are sorted in the workspace
 * and three run kernels follow: heads and the value of the open tail per tile; one workgroup's scan over the tiles (the
 * heads in front of each tile and the value of the run that is open in front of it; it writes m and d_out_offsets[m]);
 * and the write, in which the LAST element of a run stores the run's value.  No kernel waits for another workgroup.  The
 * workspace -- the two element arrays and four per-tile arrays -- is made on first use or by rsx_ctx_reserve_reduce;
 * under capture without a sufficient reserve the call returns RSX_ERR_WORKSPACE and enqueues nothing.
 * RSX_INFO_LAST_PASSES reports path 9 and, in bits 0-7, the kernels launched after the sort; RSX_INFO_LAST_PAIRS route 1
 * and the joined element's size. */
enum { RSX_REDUCE_SUM = 0, RSX_REDUCE_MIN = 1, RSX_REDUCE_MAX = 2 };
int rsx_reduce_by_key_device(rsx_ctx *ctx, const void *d_keys, const void *d_values, size_t n, uint32_t key_bytes,
                             uint32_t key_kind, uint32_t value_bytes, uint32_t value_kind, int op, int order,
                             void *d_out_keys, void *d_out_values, uint64_t *d_out_offsets, uint64_t *d_out_num,
                             void *stream);
/* Workspace (and the context's first-call set-up) for rsx_reduce_by_key_device on up to n keys of these widths, so that
 * the call allocates nothing (stream capture). */
int rsx_ctx_reserve_reduce(rsx_ctx *ctx, size_t n, uint32_t key_bytes, uint32_t value_bytes);
/* Host-only, needs no device: *tile = the elements one workgroup of the run kernels takes for these widths (256 threads,
 * each a whole number of 16-byte words), *scan_span = the tiles one sweep of the scan kernel's loop takes. */
int rsx_reduce_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t *tile, uint32_t *scan_span);

/* -- scan by key ------------------------------------------------------------- */
/* The other thing callers do with a group: a result for EVERY row -- the running sum, minimum or maximum of a column
 * inside the row's group, or the row's number inside it (groupby().cumsum() / cummax() / cumcount(), row_number() over
 * (partition by ...), inclusive_scan_by_key).
 *
 * Groups.  Two keys are equal when all their bits are equal, the rule of rsx_unique_device (-0.0 and +0.0 are two keys).
 *     default (grouped)  the group of position q is every position with q's key, anywhere in the array;
 *     RSX_SCAN_RUNS      the group of q is the maximal run of CONSECUTIVE positions with q's key: the keys are taken as
 *                        they lie, nothing is sorted, and a key that appears again later starts a new group.
 * Inclusive result.  Let q_1 < q_2 < ... be the positions of q's group that are <= q and (+) the operator `op`
 * (RSX_REDUCE_SUM / MIN / MAX with the operators, value types and order rules of rsx_reduce_by_key_device):
 *     d_out[q] = d_values[q_1] (+) d_values[q_2] (+) ... (+) d_values[q]                (n entries of value_bytes)
 * The result stands at the INPUT position q; the order in which groups are processed is not observable, so the call has
 * no `order` argument.
 * RSX_SCAN_EXCLUSIVE.  d_out[q] is the inclusive result at q's predecessor in its group; the first position of every
 * group receives the low value_bytes bytes of `first`, which is stored, never combined (no identity element is ever
 * added, as everywhere in this library).
 * d_values == NULL, the count form.  Every value is the integer 1 of the stated value type; accepted only with
 * RSX_REDUCE_SUM and an integer value_kind.  Inclusive gives the 1-based rank of q in its group, exclusive with first = 0
 * the 0-based rank (cumcount, row_number).
 * d_out_num (optional) receives the number of groups -- of runs under RSX_SCAN_RUNS -- as uint64: a by-product of the
 * tile scan, never read by the host.
 * Float sums.  The association is fixed by the tiling: a function of (n, the widths, the flags, the group's start and
 * the rank) alone.  The same input gives the same bytes on every call and every context; there are no atomics.
 * Aliasing.  d_out may be d_values (a thread of the write kernel stores only positions whose values it has itself
 * already loaded; in the grouped form the values were gathered into the workspace by the launch before).  d_out must
 * not overlap d_keys.
 *
 * Keys: every width and kind of rsx_argsort_device.  Values: 4 or 8 bytes of kind unsigned, signed or float.  Natural
 * alignment suffices for all four pointers; under RSX_SCAN_RUNS columns that are not 16-byte aligned are loaded and
 * stored element by element and give the same bytes.  RSX_ERR_ARG: bad widths, kinds, op, unknown flag bits or
 * misalignment, d_out or d_keys NULL with n > 0, the count form with a float kind or an op other than RSX_REDUCE_SUM,
 * d_out or d_out_num sharing a byte with d_keys or with each other.
 * n >= 2^32 is RSX_ERR_UNSUPPORTED.  n == 0 writes d_out_num[0] = 0 where given, by a stream-ordered memset, and launches
 * nothing.  Stream-ordered, never synchronised.
 *
 * Three kernels, none of which waits for another workgroup: per tile (rsx_scan_by_key_caps) the heads and the value of
 * the open tail; the tile scan of rsx_reduce_by_key_device; and the write, in which every element stores its result.
 * Under RSX_SCAN_RUNS they read the caller's columns directly (keys and values twice, one write: no element workspace).
 * The grouped form first joins and sorts the (mapped key, u32 position) elements of rsx_argsort_device in the context's
 * workspace; the first kernel gathers d_values[position] into a workspace column and the write scatters d_out[position].
 * The workspace -- the per-tile arrays, one word, and for the grouped form the two element arrays and the value column
 * -- is made on first use or by rsx_ctx_reserve_scan_by_key; under capture without a sufficient reserve the call returns
 * RSX_ERR_WORKSPACE and enqueues nothing.  RSX_INFO_LAST_PASSES reports path 14: bits 0-7 the kernels launched after any
 * sort, bit 8 set under RSX_SCAN_RUNS, bits 9-23 zero (the sort of the grouped form is described as for path 8).
 * RSX_INFO_LAST_PAIRS reports route 1 and the joined element's size for the grouped form and keeps its previous value
 * under RSX_SCAN_RUNS. */
enum { RSX_SCAN_EXCLUSIVE = 1, RSX_SCAN_RUNS = 2 };
int rsx_scan_by_key_device(rsx_ctx *ctx, const void *d_keys, const void *d_values, size_t n, uint32_t key_bytes,
                           uint32_t key_kind, uint32_t value_bytes, uint32_t value_kind, int op, uint32_t flags,
                           uint64_t first, void *d_out, uint64_t *d_out_num, void *stream);
/* Workspace (and the context's first-call set-up) for rsx_scan_by_key_device on up to n keys of these widths with these
 * flags (only RSX_SCAN_RUNS matters), so that the call allocates nothing (stream capture). */
int rsx_ctx_reserve_scan_by_key(rsx_ctx *ctx, size_t n, uint32_t key_bytes, uint32_t value_bytes, uint32_t flags);
/* Host-only, needs no device: *tile = the elements one workgroup of the count and write kernels takes (256 threads; under
 * RSX_SCAN_RUNS each a whole number of 16-byte words of both columns), *scan_span = the tiles one sweep of the scan
 * kernel's loop takes. */
int rsx_scan_by_key_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t flags, uint32_t *tile, uint32_t *scan_span);

/* -- bounds of many needles in a sorted key array ---------------------------- */
/* The other thing callers do with a sorted array: look keys up in it (searchsorted / bucketize, membership, the probe side
 * of a sort-merge join against the keys rsx_unique_device leaves on the device).  Let M be the key mapping of
 * rsx_argsort_device for (key_bytes, key_kind), complemented when `order` is descending (floats by the total order on bit
 * patterns), and N = n, or min(n, *d_sorted_num) when that pointer is given: it is read on the device, so the d_out_num of
 * rsx_unique_device can be passed without a host read.  PRECONDITION: M(d_sorted[j]) is non-decreasing for j < N -- what
 * rsx_sort_device, rsx_sort_pairs_device and rsx_unique_device produce in that `order`.  For every needle i < m:
 *     d_out_lower[i] = #{ j < N : M(d_sorted[j]) <  M(d_needles[i]) }
 *     d_out_upper[i] = #{ j < N : M(d_sorted[j]) <= M(d_needles[i]) }
 * so d_sorted[lower[i] .. upper[i]) are exactly the keys equal to needle i in every bit.  Either output may be NULL, not
 * both.  Indices are index_bytes (4 or 8) wide; with 4, n >= 2^32 is RSX_ERR_ARG.  Key widths, kinds and alignments are
 * those of rsx_argsort_device (1, 2, 4, 8, 16 bytes); the outputs are aligned to index_bytes, d_sorted_num to 8.  The inputs
 * are only read; nothing outside the m-entry outputs and the context's workspace is written.  If the precondition does not
 * hold, every output is still in [0, N] and no byte outside the arrays is read; nothing else is promised.  m == 0 launches
 * nothing and looks at no pointer.  N == 0 gives zeros (n == 0: stream-ordered memsets, no kernel).  Stream-ordered, no
 * synchronisation; the host reads nothing.  RSX_ERR_ARG: bad widths, kinds, order, index_bytes or alignments, NULL inputs
 * with n or m > 0, both outputs NULL, unknown flag bits.
 *
 * One kernel, one workgroup per tile of `tile` consecutive needles (rsx_search_caps): it reduces the smallest and largest
 * mapped key of the tile, finds lo = lower(smallest) and hi = upper(largest) in the whole haystack by a cooperative 64-ary
 * search (one wave each, a probe per lane and round), and, when hi - lo <= `window`, stages the mapped keys of
 * d_sorted[lo .. hi) in LDS, where every needle does its two binary searches; otherwise every needle searches [lo, hi) in
 * global memory.  Every answer of the tile lies in [lo, hi] whatever the order of the needles: their order decides how
 * narrow the window is, never the result.  No workgroup waits for another one, there are no atomics.  Weak spot: a run of
 * equal keys in d_sorted longer than `window` sends its tiles to the global searches even when the needles are ordered.
 *
 * The route is the caller's choice.  flags == 0, the needles as given: the streaming merge when the needles are ordered
 * or clustered, a binary search per needle when they are scattered; no workspace, so the call can be captured once the
 * context has made its first call.  RSX_SEARCH_PRESORT: the needles are joined with their positions (the join of
 * rsx_argsort_device) and sorted in the context's pairs workspace, the same kernel reads the sorted elements and stores
 * at out[position]; m >= 2^32 is RSX_ERR_UNSUPPORTED; the workspace is made on first use or by rsx_ctx_reserve_search, and
 * under capture without a sufficient reserve the call returns RSX_ERR_WORKSPACE and enqueues nothing.
 * RSX_INFO_LAST_PASSES reports path 10. */
enum { RSX_SEARCH_PRESORT = 1 };
int rsx_search_sorted_device(rsx_ctx *ctx, const void *d_sorted, size_t n, const uint64_t *d_sorted_num,
                             const void *d_needles, size_t m, uint32_t key_bytes, uint32_t key_kind, int order,
                             void *d_out_lower, void *d_out_upper, uint32_t index_bytes, uint32_t flags, void *stream);
/* Workspace (and the context's first-call set-up) of the RSX_SEARCH_PRESORT route for up to m needles of this width, so
 * that the call allocates nothing (stream capture). */
int rsx_ctx_reserve_search(rsx_ctx *ctx, size_t m, uint32_t key_bytes);
/* Host-only, needs no device: *tile = the needles one workgroup takes, *window = the most haystack keys it stages in LDS
 * (window >= 2 * tile; window * key_bytes leaves more than two workgroups per CU).  Both routes run the same shape. */
int rsx_search_caps(uint32_t key_bytes, int with_positions, uint32_t *tile, uint32_t *window);

/* -- stable merge of two sorted key arrays ------------------------------------ */
/* Combining two arrays the sorting calls left on the device (append a sorted batch to a sorted index, fold the keys of two
 * rsx_unique_device results together) in one read and one write of every byte, where concatenating and sorting again
 * moves every byte several times.  Let M be the key mapping of rsx_argsort_device for (key_bytes, key_kind), complemented
 * when `order` is descending (floats by the total order on bit patterns: -NaN first, -0.0 before +0.0, +NaN last), and
 * n = na + nb.  PRECONDITION: M(d_a_keys[i]) is non-decreasing and M(d_b_keys[j]) is non-decreasing -- what every sorting
 * call of the library leaves in that `order`.  Let c = a ++ b and p the stable permutation that sorts c by M, exactly
 * rsx_argsort_device of the concatenation: equal keys of a come before equal keys of b, and equal keys inside one array
 * keep their order.  Then, for t < n:
 *     d_out_keys[t]   = c[p[t]]                          as raw key bytes
 *     d_out_values[t] = (a_values ++ b_values)[p[t]]     moved bitwise
 *     d_out_index[t]  = p[t]                             index_bytes wide: below na a position in a, else p[t] - na in b
 * Each output is optional through a NULL pointer; at least one must be given.  The inputs are only read; nothing outside
 * the n-entry outputs and the context's workspace is written.  Key widths, kinds and alignments are those of
 * rsx_argsort_device (1, 2, 4, 8, 16 bytes); value_bytes is 0 .. RSX_MAX_ELEM_BYTES with the value alignment of
 * rsx_sort_pairs_device, and value_bytes == 0 goes with all three value pointers NULL; index_bytes is 4 or 8 and is looked
 * at only when d_out_index is given.  RSX_ERR_ARG: bad widths, kinds, order, index_bytes or alignments; a NULL input with
 * a nonzero count; values given on one side only; all outputs NULL; index_bytes == 4 with n > 2^32; an output range that
 * overlaps an input range or another output (the merge is not in place; checked on the host from the pointers and byte
 * lengths).  RSX_ERR_UNSUPPORTED: n of 2^31 tiles or more.  n == 0 launches nothing and looks at no pointer; na == 0 or
 * nb == 0 is a copy through the same kernel.  Stream-ordered, no synchronisation; the host reads nothing.
 * If the precondition does not hold, every read stays inside the two inputs, every write inside the outputs and every
 * d_out_index[t] is below n; nothing else is promised, and the output need not be a permutation.
 *
 * One kernel, one workgroup per tile of `tile` consecutive OUTPUT positions (rsx_merge_caps): two of its waves find the
 * tile's two cuts on the merge path by the cooperative 64-ary search of rsx_search_sorted_device, the mapped keys of the
 * two input ranges between the cuts go to LDS, every thread merges its share there, and keys, values and positions are
 * stored as contiguous ranges.  No workgroup waits for another one, there are no atomics.  Values of 1, 2, 4, 8 and 16
 * bytes move in that kernel, which needs no workspace: the call can be captured once the context has made its first call.
 * Values of any other width: the kernel writes 8-byte source positions into the context's workspace and a row gather
 * moves the values; the workspace is made on first use or by rsx_ctx_reserve_merge, and under capture without a sufficient
 * reserve the call returns RSX_ERR_WORKSPACE and enqueues nothing.  RSX_INFO_LAST_PASSES reports path 11. */
int rsx_merge_device(rsx_ctx *ctx,
                     const void *d_a_keys, const void *d_a_values, size_t na,
                     const void *d_b_keys, const void *d_b_values, size_t nb,
                     uint32_t key_bytes, uint32_t key_kind, uint32_t value_bytes, int order,
                     void *d_out_keys, void *d_out_values, void *d_out_index, uint32_t index_bytes,
                     void *stream);
/* Workspace (and the context's first-call set-up) of a merge into up to n_total outputs of these widths, so that the call
 * allocates nothing (stream capture). */
int rsx_ctx_reserve_merge(rsx_ctx *ctx, size_t n_total, uint32_t key_bytes, uint32_t value_bytes);
/* Host-only, needs no device: *tile = the output positions one workgroup takes (256 threads; tile * (key_bytes + 2) + 16
 * bytes of LDS at most, which leaves more than two workgroups per CU). */
int rsx_merge_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t *tile);

/* -- set operations on two sorted key arrays ---------------------------------- */
/* Union, intersection, difference and symmetric difference of two sorted key arrays as MULTISETS (the rules of
 * std::set_union and its siblings): which ids are in both, which only in the first, the deduplicated union of two
 * rsx_unique_device results -- in one merge-path pass, where the chain of searches, a mask and a compaction moves the keys
 * several times and reads a count back.  Let M be the key mapping of rsx_argsort_device for (key_bytes, key_kind),
 * complemented when `order` is descending, N_a = na, or min(na, *d_a_num) when that pointer is given (one device word, such
 * as the d_out_num of rsx_unique_device, read on the device), and N_b likewise.  PRECONDITION: a[0 .. N_a) and b[0 .. N_b)
 * are each non-decreasing under M.  For a key k let A_lo(k) = #{ i < N_a : M(a[i]) < M(k) } and B_lo(k) the same count in
 * b.  The rank of a[i] in its run of equal keys is r = i - A_lo(a[i]), that of b[j] is s = j - B_lo(b[j]).
 *     a[i] is MATCHED when B_lo(a[i]) + r < N_b and b[B_lo(a[i]) + r] has the same bit pattern (the key occurs more than r
 *          times in b);
 *     b[j] is MATCHED when A_lo(b[j]) + s < N_a and a[A_lo(b[j]) + s] equals it.
 * The operation keeps
 *     RSX_SETOP_UNION                 every a[i]; the unmatched b[j]
 *     RSX_SETOP_INTERSECTION          the matched a[i]
 *     RSX_SETOP_DIFFERENCE            the unmatched a[i]
 *     RSX_SETOP_SYMMETRIC_DIFFERENCE  the unmatched a[i]; the unmatched b[j]
 * and the output is the kept elements in the order of the stable merge of a ++ b, equal keys of a first (the order of
 * rsx_merge_device): for t < *d_out_num,
 *     d_out_keys[t]    the key, as raw key bytes
 *     d_out_values[t]  the value of that very element, moved bitwise
 *     d_out_index[t]   its position in the concatenation: i for a[i], na + j for b[j] -- the offset is the HOST's na, so
 *                      that index - na always indexes the b array
 *     *d_out_num       the number kept; entries at t >= *d_out_num are not written.
 * The caller provides cap(op) rows in every output it asks for: na + nb for union and symmetric difference, na for
 * difference, min(na, nb) for intersection.  Each of keys, values, index is optional through a NULL pointer, at least one
 * must be given; d_out_num is required and 8-byte aligned (so are d_a_num and d_b_num when given).  Key widths, kinds and
 * alignments are those of rsx_argsort_device (1, 2, 4, 8, 16 bytes); value_bytes is 0, 1, 2, 4, 8 or 16 with the value
 * alignment of rsx_sort_pairs_device, and any other width up to RSX_MAX_ELEM_BYTES returns RSX_ERR_UNSUPPORTED: ask for
 * d_out_index and gather.  value_bytes == 0 goes with all three value pointers NULL; d_b_values is looked at only by the
 * two operations that can emit from b.  index_bytes is 4 or 8 and is looked at only when d_out_index is given.
 * RSX_ERR_ARG: a bad op, widths, kinds, order, index_bytes or alignments; a NULL input with a nonzero count; values missing
 * on a side that can be emitted; all outputs NULL; d_out_num NULL; index_bytes == 4 with na + nb > 2^32; an output range
 * (cap(op) rows, or the word of d_out_num) that overlaps an input range, a count word or another output.
 * RSX_ERR_UNSUPPORTED: na + nb of 2^31 tiles or more.  na + nb == 0 stores *d_out_num = 0, launches no kernel and looks at
 * no other pointer; one empty side goes through the same kernels.  Stream-ordered, no synchronisation; the host reads
 * nothing.  If the precondition does not hold, every read stays inside the two inputs, every write inside cap(op) rows of
 * the outputs, *d_out_num <= cap(op) and every d_out_index[t] is below na + nb; nothing else is promised.
 *
 * Three launches over tiles of `tile` consecutive positions of the MERGE of a and b (rsx_setop_caps): a count launch, a
 * one-workgroup scan, a write launch; no workgroup waits for another one and there are no atomics.  A workgroup finds its
 * tile's two cuts on the merge path and merges in LDS as rsx_merge_device does, and decides every element while it
 * merges, by one probe of the other array at the element's rank.  Workspace, per tile: a 4-byte count, an 8-byte base and
 * 32 bytes the first launch saves for the second; it is made on first use or by rsx_ctx_reserve_setop, and under capture
 * without a sufficient reserve the call returns RSX_ERR_WORKSPACE and enqueues nothing.  RSX_INFO_LAST_PASSES reports
 * path 12. */
enum { RSX_SETOP_UNION = 0, RSX_SETOP_INTERSECTION = 1, RSX_SETOP_DIFFERENCE = 2, RSX_SETOP_SYMMETRIC_DIFFERENCE = 3 };
int rsx_setop_device(rsx_ctx *ctx, uint32_t op,
                     const void *d_a_keys, const void *d_a_values, size_t na, const uint64_t *d_a_num,
                     const void *d_b_keys, const void *d_b_values, size_t nb, const uint64_t *d_b_num,
                     uint32_t key_bytes, uint32_t key_kind, uint32_t value_bytes, int order,
                     void *d_out_keys, void *d_out_values, void *d_out_index, uint32_t index_bytes,
                     uint64_t *d_out_num, void *stream);
/* Workspace (and the context's first-call set-up) of a set operation on up to n_total = na + nb keys of this width, so that
 * the call allocates nothing (stream capture). */
int rsx_ctx_reserve_setop(rsx_ctx *ctx, size_t n_total, uint32_t key_bytes);
/* Host-only, needs no device: *tile = the merge positions one workgroup takes (256 threads; tile * (key_bytes + 2) + 64
 * bytes of LDS at most, which leaves more than two workgroups per CU; tile <= 4096). */
int rsx_setop_caps(uint32_t key_bytes, uint32_t *tile);

/* -- sort-merge join of two sorted key arrays --------------------------------- */
/* Which rows of table A match which rows of table B on a key: the row pairs of the join, in one read of the keys and one
 * write of the pairs, where rsx_search_sorted_device (the probe) leaves the expansion -- counts, their running sum, a
 * repeat and the right-hand positions -- to the caller.  The set operations do not cover it: they keep min(m, n) copies
 * of a key, a join emits m * n pairs.  Let M be the key mapping of rsx_argsort_device for (key_bytes, key_kind),
 * complemented when `order` is descending, N_a = na, or min(na, *d_a_num) when that pointer is given (one device word,
 * read on the device), and N_b likewise.  PRECONDITION: a[0 .. N_a) and b[0 .. N_b) are each non-decreasing under M.
 * For i < N_a let
 *     lo(i) = #{ j < N_b : M(b[j]) <  M(a[i]) }      hi(i) = #{ j < N_b : M(b[j]) <= M(a[i]) }      m(i) = hi(i) - lo(i),
 * the number of keys of b that equal a[i] in every bit.  a[i] contributes c(i) rows, row r of them (0 <= r < c(i)) being
 *     RSX_JOIN_INNER  c(i) = m(i)               (i, lo(i) + r)
 *     RSX_JOIN_LEFT   c(i) = max(m(i), 1)       (i, lo(i) + r), or (i, NONE) when m(i) == 0
 *     RSX_JOIN_SEMI   c(i) = m(i) > 0 ? 1 : 0   (i)
 *     RSX_JOIN_ANTI   c(i) = m(i) == 0 ? 1 : 0  (i)
 * With S(i) = c(0) + ... + c(i - 1) and T = S(N_a), row t = S(i) + r is
 *     d_out_a[t] = A(i)        d_out_b[t] = B(lo(i) + r), or NONE
 * where A(i) = d_a_index ? d_a_index[i] : i and B likewise with d_b_index; NONE has all bits of the index set.  So the rows
 * are ordered by i, then by position in b: the order of the stable sorts.  *d_out_num = T, the FULL number of rows
 * whatever `capacity` is; rows t >= min(T, capacity) are not written.
 *
 * d_a_index / d_b_index are optional arrays of index_bytes-wide words, na / nb entries, moved bitwise: the permutations a
 * caller got from sorting unsorted tables, so that the rows come out as positions in the ORIGINAL tables with no gather
 * afterwards.  Key widths, kinds and alignments are those of rsx_argsort_device (1, 2, 4, 8, 16 bytes); index_bytes is 4
 * or 8; d_out_num is required and 8-byte aligned (so are d_a_num and d_b_num when given).  For SEMI and ANTI d_out_b and
 * d_b_index must be NULL.  d_out_a == NULL && d_out_b == NULL with capacity == 0 is the COUNT-ONLY form: it launches the
 * first two kernels, stores T and writes nothing else, and a caller sizes its outputs from it.  Otherwise d_out_a (and,
 * for INNER and LEFT, d_out_b) is required.
 * RSX_ERR_ARG: a bad how, widths, kinds, order, index_bytes or alignments; a NULL input with a nonzero count; d_out_num
 * NULL; a NULL output outside the count-only form; d_out_b or d_b_index given to SEMI or ANTI; an output range
 * (min(capacity, bound(how)) rows, or the word of d_out_num) that overlaps an input, an index array, a count word or
 * another output.  bound(how) is na * nb for INNER, na * max(nb, 1) for LEFT and na for SEMI and ANTI.
 * RSX_ERR_UNSUPPORTED: na >= 2^32 or nb >= 2^32 (so that T < 2^64 and a position in b fits 32 bits next to NONE); more
 * than 2^31 write workgroups (min(capacity, bound(how)) / rows of rsx_join_caps).  The write grid is sized from
 * min(capacity, bound(how)), so a generous capacity costs only workgroups that read T and leave.
 * na == 0 stores *d_out_num = 0 stream-ordered, launches nothing and looks at no other pointer; nb == 0 goes through the
 * kernels (LEFT and ANTI emit N_a rows).  Stream-ordered, no synchronisation; the host reads nothing.  If the precondition
 * does not hold, every read stays inside the inputs and index arrays, every write inside min(capacity, bound(how)) rows,
 * every d_out_a[t] comes from [0, na) or the index array, every d_out_b[t] from [0, nb), the index array or NONE, and
 * *d_out_num <= bound(how); nothing else is promised.
 *
 * Three launches, no workgroup waits for another one and there are no atomics, so the same input gives the same bytes on
 * every call: a count launch over tiles of `tile` keys of a (the kernel of rsx_search_sorted_device with a's keys as
 * ordered needles, then the rows of every key and their sums inside the tile), a one-workgroup scan of the tiles' sums,
 * and a write launch over tiles of `rows` OUTPUT rows, each row finding its key by a search in the sums -- a workgroup's
 * work is bounded by its rows, not by any key's fan-out.  Workspace: 12 bytes per key of a and 16 per count tile; it is
 * made on first use or by rsx_ctx_reserve_join, and under capture without a sufficient reserve the call returns
 * RSX_ERR_WORKSPACE and enqueues nothing.  RSX_INFO_LAST_PASSES reports path 13. */
enum { RSX_JOIN_INNER = 0, RSX_JOIN_LEFT = 1, RSX_JOIN_SEMI = 2, RSX_JOIN_ANTI = 3 };
int rsx_join_device(rsx_ctx *ctx, uint32_t how,
                    const void *d_a_keys, size_t na, const uint64_t *d_a_num, const void *d_a_index,
                    const void *d_b_keys, size_t nb, const uint64_t *d_b_num, const void *d_b_index,
                    uint32_t key_bytes, uint32_t key_kind, int order,
                    void *d_out_a, void *d_out_b, uint32_t index_bytes, size_t capacity,
                    uint64_t *d_out_num, void *stream);
/* Workspace (and the context's first-call set-up) of a join whose left side has up to na keys of this width, so that the
 * call allocates nothing (stream capture). */
int rsx_ctx_reserve_join(rsx_ctx *ctx, size_t na, uint32_t key_bytes);
/* Host-only, needs no device: *tile = the keys of a one count workgroup takes, *window = the keys of b it stages in LDS at
 * most, *rows = the output rows one write workgroup stores (256 threads each).  Static LDS: the count kernel window *
 * key_bytes + 8 * key_bytes + 160 bytes at most, the write kernel 8 * rows + 32 bytes at most, the scan kernel 32 bytes;
 * every one leaves more than two workgroups per CU. */
int rsx_join_caps(uint32_t key_bytes, uint32_t *tile, uint32_t *window, uint32_t *rows);

/* -- order statistics of an unsorted key array -------------------------------- */
/* The elements at given ranks of the stable sort, without sorting.  With p the permutation rsx_argsort_device produces for
 * these keys in `order` (by mapped key, complemented for descending order; equal keys in input order; floats by the total
 * order on bit patterns), for every q < nranks
 *     d_out_keys[q]  = keys[p[ranks[q]]]     (the raw key bytes)
 *     d_out_index[q] = p[ranks[q]]           (index_bytes 4 or 8; 4 with n >= 2^32: RSX_ERR_UNSUPPORTED)
 * -- column ranks[q] of the full stable sort, byte for byte, the rule of rsx_topk_rows_device.  Key widths, kinds and
 * alignment as rsx_argsort_device; d_keys is only read.  `ranks` is a HOST array, read during the call and handed to the
 * kernels by value (no copy is enqueued, so the call can be captured into a graph); ranks may repeat and come in any
 * order, every one below n, and nranks <= max_ranks of rsx_select_caps.  Either output may be null, not both.
 * nranks == 0 succeeds, launches nothing and looks at no pointer.  Stream-ordered, no synchronisation, the host reads
 * nothing from the device; nothing outside the nranks output keys and nranks indices is written.
 *
 * A counting select: levels of digit_bits bits run over the mapped key from the top.  Each level counts one digit of the
 * keys under the prefixes the ranks have reached (LDS counters per workgroup and per distinct prefix, flushed into
 * global bins with integer atomics: the sums do not depend on the order), then one workgroup picks every rank's bin.
 * Nothing is moved -- except once: as soon as the keys still under some prefix number at most
 * cand_cap(n) = n / cand_div + cand_floor, a gated kernel copies them (keys only, in arbitrary order) into a buffer of
 * that capacity and the later levels count the buffer; if that never happens (all keys equal, heavy skew) every level
 * counts the whole array, which is correct and slower.  The host enqueues every level, the device decides what runs.
 * With d_out_index the wanted occurrence of the value is then found in three launches without atomics over tiles of
 * `tile` keys (count per tile, scan per rank, find inside one tile); no workgroup waits for another.
 * Workspace: the bins, cand_cap(n) keys and 4 * max_ranks bytes per tile; it is made on first use or by
 * rsx_ctx_reserve_select, and under capture without a sufficient reserve the call returns RSX_ERR_WORKSPACE and enqueues
 * nothing.  RSX_INFO_LAST_PASSES reports path 15. */
int rsx_select_device(rsx_ctx *ctx, const void *d_keys, size_t n, uint32_t key_bytes, uint32_t key_kind,
                      const uint64_t *ranks /* HOST array */, uint32_t nranks, void *d_out_keys, void *d_out_index,
                      uint32_t index_bytes, int order, void *stream);
/* Workspace (and the context's first-call set-up) of a select over up to n keys of this width, so that the call
 * allocates nothing (stream capture). */
int rsx_ctx_reserve_select(rsx_ctx *ctx, size_t n, uint32_t key_bytes);
/* Host-only, needs no device: *max_ranks = the ranks one call takes, *digit_bits = the bits of a level, *tile = the keys
 * per workgroup of the index launches, *cand_div and *cand_floor as in cand_cap(n) above.  The count kernel keeps
 * max_ranks * 2^digit_bits four-byte counters in LDS, at most 80 KiB: two workgroups per CU. */
int rsx_select_caps(uint32_t key_bytes, uint32_t *max_ranks, uint32_t *digit_bits, uint32_t *tile,
                    uint32_t *cand_div, uint32_t *cand_floor);

/* -- keys per bin of an unsorted key array ------------------------------------ */
/* How many keys fall between given cut points (a histogram), or have each small integer value (a bincount), in one read
 * of the keys.  (rsx_histogram_device above is something else: the 256-bin digit count of the multi-GPU path.)
 * With N = n, or min(n, *d_num) when d_num is given -- a device word such as the d_out_num of rsx_unique_device, read on
 * the device as sorted_num is in rsx_search_sorted_device -- and M the mapped key of rsx_argsort_device (complemented
 * for descending `order`), d_counts holds m + 1 integers of count_bytes (4 or 8) and
 *     counts[b] = #{ i < N : bin(keys[i]) == b }        for b = 0 .. m
 * with bin(key) one of
 *     RSX_BIN_UPPER   #{ j < m : M(edges[j]) <= M(key) }   bins [e[j-1], e[j]): numpy.histogram, bucketize(right=True)
 *     RSX_BIN_LOWER   #{ j < m : M(edges[j]) <  M(key) }   bins (e[j-1], e[j]]
 *     RSX_BIN_INDEX   no edges: the key's integer value when 0 <= value < m, else m ("outside")
 * Without RSX_BIN_ACCUMULATE in `flags` every one of the m + 1 entries is overwritten; with it the counts are added to
 * what is there.  In the edge modes the result is bincount(upper_or_lower(edges, keys), minlength = m + 1) of
 * rsx_search_sorted_device with the same edges, order and kind: every key width (1, 2, 4, 8, 16) and kind, by the total
 * order on bit patterns -- NaN, +-0 and +-inf are keys and edges like any other.  counts[0] and counts[m] are the two open
 * ends.  The edges (m keys of the keys' width and kind) must be sorted in `order`; otherwise the result is unspecified,
 * but no access goes out of bounds.  Equal edges give empty bins.  m == 0 is legal: one bin holds N.
 * The index mode takes integer keys of 1, 2, 4 or 8 bytes, signed or unsigned (negative keys are outside); float kinds
 * and 16-byte keys return RSX_ERR_UNSUPPORTED; it requires order == 0 and d_edges == NULL (RSX_ERR_ARG otherwise).
 * RSX_ERR_UNSUPPORTED, with nothing enqueued: an edge mode with m > max_edges of rsx_bin_caps; count_bytes == 4 with
 * n >= 2^32.  RSX_ERR_ARG: bad widths, kinds, modes, flags, order or count_bytes; m == 2^32 - 1; d_counts NULL; d_keys NULL
 * with n > 0; d_edges NULL with m > 0 in an edge mode; a pointer not aligned to its element (d_num: 8 bytes).
 * n == 0 or N == 0 still zeroes the counts (unless accumulating) and counts nothing.  d_keys and d_edges are only read.
 *
 * A zeroing kernel (skipped when accumulating) and one counting kernel: a fixed number of persistent workgroups, each
 * streaming one share of at least `share` keys in 16-byte words.  Edge modes: the mapped edges are staged in LDS beside
 * m + 1 four-byte counters, every key is mapped and its bin found by a bound search in LDS, several keys of a thread in
 * step.  Index mode: the same counters without a search, one window of max_index_bins_lds values at a time (a workgroup
 * walks its share once per window; the outside bin is counted beside the last window's values) while
 * m <= 16 * max_index_bins_lds, atomics straight into d_counts above.  A wave whose lanes all hold one bin adds once; the LDS counters are flushed into d_counts with integer
 * atomics (before any could wrap: a workgroup flushes every 2^31 keys), so the counts do not depend on any order.
 * Stream-ordered, no synchronisation, the host reads nothing.  There is no workspace: the call allocates nothing and can
 * be captured with no reserve.  RSX_INFO_LAST_PASSES reports path 16 and, in bits 0-7, the kernels launched. */
#define RSX_BIN_UPPER 0u
#define RSX_BIN_LOWER 1u
#define RSX_BIN_INDEX 2u
#define RSX_BIN_ACCUMULATE 1u  /* flags: add to d_counts instead of overwriting it */
int rsx_bin_count_device(rsx_ctx *ctx, const void *d_keys, size_t n, const uint64_t *d_num, uint32_t key_bytes,
                         uint32_t key_kind, const void *d_edges, uint32_t m, uint32_t mode, int order, void *d_counts,
                         uint32_t count_bytes, uint32_t flags, void *stream);
/* Host-only, needs no device: *max_edges = the most edges an edge mode takes for this key width (the edges and m + 1
 * counters share at most 80 KiB of LDS, two workgroups per CU), *max_index_bins_lds = the values, and with m + 1 <=
 * this all bins, that the index mode counts in LDS in one pass over the keys, *share = the fewest keys worth a workgroup. */
int rsx_bin_caps(uint32_t key_bytes, uint32_t *max_edges, uint32_t *max_index_bins_lds, uint32_t *share);

/* -- rows that pass a predicate, in input order -------------------------------- */
/* keys[mask], masked_select, nonzero and a stable two-way partition with the count left on the device.
 * With N = n, or min(n, *d_num) when d_num is given -- a device word, read on the device exactly as in
 * rsx_bin_count_device -- and M the mapped key of rsx_argsort_device (complemented for descending `order`), row i < N
 * passes when
 *     pred(i) = (d_flags == NULL || d_flags[i] != 0)
 *            && (d_lo == NULL || M(*d_lo) <= M(keys[i]))
 *            && (d_hi == NULL || M(keys[i]) <  M(*d_hi))
 * d_lo and d_hi each point to ONE key of key_bytes on the device -- the output of rsx_select_device, a key of
 * rsx_unique_device, a word the caller wrote --, read by the kernels, never by the host.  The order is the total order on
 * bit patterns: NaN, +-0 and +-inf are keys and bounds like any other.
 *     keep(i) = pred(i) XOR (flags & RSX_COMPACT_INVERT)
 * Let i_0 < ... < i_{m-1} be the kept rows and j_0 < ... < j_{N-m-1} the others.  Every output is optional through NULL
 * except d_out_num:
 *     d_out_keys[t]   = keys[i_t]      t < m   the raw key bytes, untouched
 *     d_out_values[t] = values[i_t]    t < m
 *     d_out_index[t]  = i_t            t < m   integers of index_bytes (4 or 8)
 *     d_out_num[0]    = m
 * With RSX_COMPACT_PARTITION additionally out[m + u] = row j_u for u < N - m in each given output: a stable two-way
 * partition, the rejected rows in input order too (CUB writes them in reverse).  Without it nothing is written at m and
 * beyond, with it nothing at N and beyond; nothing but the outputs and the context's workspace is written, the inputs
 * are only read.
 * d_keys may be NULL when d_lo, d_hi and d_out_keys are all NULL (a pure mask call; with d_out_index alone: nonzero);
 * key_bytes and key_kind are then ignored.  All three predicates may be NULL: every row passes, a bounded copy.  Keys of
 * 1, 2, 4, 8, 16 bytes and every kind.  Values of 1, 2, 4, 8, 16 bytes are moved by the write kernel; any other width up
 * to RSX_MAX_ELEM_BYTES rides behind positions (d_out_index when given, else n u32 in the workspace) and a row gather
 * that stops at the device count.  d_values is looked at only when d_out_values is given.
 * RSX_ERR_ARG: bad widths, kinds, order, flags bits or index_bytes; d_out_num NULL; a needed pointer NULL with n > 0; a
 * pointer not aligned (keys and bounds: key_bytes; values: as in rsx_sort_pairs_device; index: index_bytes; d_num and
 * d_out_num: 8); an output pointer equal to (or overlapping) an input.  RSX_ERR_UNSUPPORTED: n >= 2^32.  These are
 * answered before the context is looked at.  The call is not in place: the tiles of the write launch do not run in order.
 * n == 0 or N == 0 stores d_out_num[0] = 0 and writes nothing else.
 *
 * Three launches, no workgroup waits for another, no atomics -- the same bytes on every call: a count per tile of `tile`
 * rows (rsx_compact_caps) that streams only the columns the predicate needs, one workgroup's scan over the tile counts
 * (`scan_span` tiles per sweep; it writes d_out_num), and the write, which ranks the keep bits inside the workgroup,
 * compacts key, value and source slot in LDS and stores contiguous ranges.  Stream-ordered, no synchronisation, the host
 * reads nothing.  Workspace: 12 bytes per tile, plus n u32 positions on the wide-value route without d_out_index; made on
 * first use or by rsx_ctx_reserve_compact (key_bytes, value_bytes, index_bytes: 0 for a column the calls will not have).
 * Under capture without a sufficient reserve the call returns RSX_ERR_WORKSPACE and enqueues nothing.
 * RSX_INFO_LAST_PASSES reports path 17 and, in bits 0-7, the kernels launched. */
#define RSX_COMPACT_INVERT 1u     /* keep the rows the predicate rejects */
#define RSX_COMPACT_PARTITION 2u  /* write the rejected rows, in input order, behind the kept ones */
int rsx_compact_device(rsx_ctx *ctx, const void *d_keys, size_t n, const uint64_t *d_num, uint32_t key_bytes,
                       uint32_t key_kind, int order, const uint8_t *d_flags, const void *d_lo, const void *d_hi,
                       const void *d_values, uint32_t value_bytes, uint32_t flags, void *d_out_keys, void *d_out_values,
                       void *d_out_index, uint32_t index_bytes, uint64_t *d_out_num, void *stream);
int rsx_ctx_reserve_compact(rsx_ctx *ctx, size_t n, uint32_t key_bytes, uint32_t value_bytes, uint32_t index_bytes);
/* Host-only, needs no device: *tile = the rows one workgroup of the count and write launches takes for these widths (a
 * multiple of 256; a key, a value and a two-byte slot per row stay within 80 KiB of LDS, two workgroups per CU; a value
 * width without a typed kernel counts as none), *scan_span = the tiles one sweep of the scan takes. */
int rsx_compact_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t index_bytes, uint32_t *tile, uint32_t *scan_span);

/* -- rows regrouped by bin, in input order inside each bin ----------------------- */
/* A stable multi-way partition: token -> expert dispatch, the bucketing step of a sample sort, range or hash partitioning
 * of a table.  bin(key) and N are exactly those of rsx_bin_count_device: `mode` is RSX_BIN_UPPER, RSX_BIN_LOWER (m edges of
 * key_bytes on the device, compared as mapped keys in the total order on bit patterns, complemented for descending
 * `order`) or RSX_BIN_INDEX (integer keys, no edges, ascending; bin m is "outside": negative and too-large ids); N = n, or
 * min(n, *d_num) read on the device.  Let p be the ONE permutation of 0 .. N-1 with bin(keys[p[t]]) non-decreasing in t
 * and p increasing among equal bins: the stable argsort of the bins.
 *     d_out_offsets[b] = #{ i < N : bin(keys[i]) < b }    b = 0 .. m + 1: m + 2 uint64, offsets[0] = 0, offsets[m+1] = N;
 *                                                         required, always written; the layout the *_segments calls take
 *     d_out_keys[t]    = keys[p[t]]      t < N   the raw key bytes, untouched
 *     d_out_values[t]  = values[p[t]]    t < N
 *     d_out_index[t]   = p[t]            t < N   integers of index_bytes (4 or 8)
 * Each of the three row outputs is optional through NULL; all NULL: the offsets alone, the exclusive sums of
 * rsx_bin_count_device's counts.  Nothing is written at N and beyond, the inputs are only read, and the call is not in
 * place.  Equal edges give empty bins; m == 0 copies the first N rows and writes {0, N}; n == 0 or N == 0 writes the
 * offsets (all 0) and nothing else.  Edges that are not sorted give an unspecified grouping, but both passes compute the
 * same bin for a key: every one of the N rows is still written exactly once, no access leaves the arrays and
 * offsets[m+1] == N.
 * Keys of 1, 2, 4, 8, 16 bytes and every kind in the edge modes; integer keys of 1 to 8 bytes in the index mode.  Values
 * of 1, 2, 4, 8, 16 bytes are moved by the write kernel; any other width up to RSX_MAX_ELEM_BYTES rides behind positions
 * (d_out_index when given, else n u32 in the workspace) and rsx_compact_device's row gather, bounded by N on the device.
 * d_values is looked at only when d_out_values is given.
 * RSX_ERR_ARG: bad widths, kinds, mode, order or index_bytes; edges or a descending order in the index mode;
 * d_out_offsets NULL; a needed pointer NULL; a pointer not aligned (keys and edges: key_bytes; values: as in
 * rsx_sort_pairs_device; index: index_bytes; d_num and d_out_offsets: 8); an output that overlaps an input or another
 * output.  RSX_ERR_UNSUPPORTED, with nothing enqueued: n >= 2^32; float or 16-byte keys in the index mode; m above
 * max_edges (edge modes) or max_index_bins (index mode) of rsx_multisplit_caps.  All of these are answered before the
 * context is looked at.
 *
 * Four launches over min(ceil(n / share), 2 * CUs) persistent workgroups, each owning one contiguous share of the rows:
 * the bin count's body, flushed by plain stores into the workgroup's column of a workspace matrix; a scan of every bin's
 * row of it; one workgroup that writes the offsets; and the write, which walks the share in tiles of `tile` rows, ranks
 * every row among the rows of its bin in the wave's 64 (a wave match) and in the tile (LDS counters of the wave), and
 * stores key, value and position.  A fifth launch gathers values of a width without a typed kernel; without a row output
 * the write is left out.  No workgroup waits for another and there are no atomics on global memory: the same bytes on
 * every call.  Stream-ordered, no synchronisation, the host reads nothing.  Workspace: 4 (m + 1) bytes per workgroup, plus
 * n u32 positions on the wide-value route without d_out_index; made on first use or by rsx_ctx_reserve_multisplit
 * (value_bytes, index_bytes: 0 for a column the calls will not have).  Under capture without a sufficient reserve the call
 * returns RSX_ERR_WORKSPACE and enqueues nothing.  RSX_INFO_LAST_PASSES reports path 18 and, in bits 0-7, the kernels
 * launched. */
int rsx_multisplit_device(rsx_ctx *ctx, const void *d_keys, size_t n, const uint64_t *d_num, uint32_t key_bytes,
                          uint32_t key_kind, const void *d_edges, uint32_t m, uint32_t mode, int order,
                          const void *d_values, uint32_t value_bytes, void *d_out_keys, void *d_out_values,
                          void *d_out_index, uint32_t index_bytes, uint64_t *d_out_offsets, void *stream);
int rsx_ctx_reserve_multisplit(rsx_ctx *ctx, size_t n, uint32_t m, uint32_t key_bytes, uint32_t value_bytes,
                               uint32_t index_bytes);
/* Host-only, needs no device: *max_edges = the most edges of an edge mode, *max_index_bins = the largest m of the index
 * mode -- what the write kernel's LDS holds beside m + 1 cursors and four waves' m + 1 counters, within 80 KiB so that two
 * workgroups fit a CU --, *tile = the rows of one tile of the write launch, *share = the fewest rows worth a workgroup. */
int rsx_multisplit_caps(uint32_t key_bytes, uint32_t *max_edges, uint32_t *max_index_bins, uint32_t *tile,
                        uint32_t *share);

/* -- a value column combined per bin, nothing sorted ----------------------------- */
/* numpy.histogram(weights=), torch.bincount(weights=), zeros.index_add_(0, ids, w), scatter_reduce over a few hundred
 * labels: per-expert load and score sums, per-class loss sums, sum, min and max of a measure per range of a key.
 * bin(key), N, `mode`, `order`, the edges and the key widths and kinds are exactly those of rsx_bin_count_device and
 * rsx_multisplit_device (RSX_BIN_INDEX: bin m is "outside"); values and operators are those of rsx_reduce_by_key_device:
 * value_bytes 4 or 8, value_kind RSX_KEY_UNSIGNED, RSX_KEY_SIGNED or RSX_KEY_FLOAT; RSX_REDUCE_SUM (integers wrap, floats
 * add by IEEE addition in their own type), RSX_REDUCE_MIN, RSX_REDUCE_MAX (floats by the total order on bit patterns: the
 * result is the bit pattern of one of the bin's values).  For b = 0 .. m
 *     d_out_values[b] = the (+) of values[i] over { i < N : bin(keys[i]) == b }     in the value's type; required
 *     d_out_counts[b] = the size of that set, count_bytes (4 or 8) each             optional through NULL; byte for byte
 *                                                                                   what rsx_bin_count_device writes
 * An empty bin holds the operator's identity: SUM integer 0 or +0.0; MIN the highest value of the order (the integer
 * type's maximum; the float bit pattern 0x7FFF...F, a +NaN); MAX the lowest (the integer type's minimum; 0xFFFF...F).  A
 * float sum starts from +0.0, so a bin of -0.0 values holds +0.0.  The association of a float sum belongs to the kernels,
 * but it is a function of the inputs' contents and sizes and of the grid alone -- never of which wave or workgroup ran
 * first; there are no floating-point atomics: the same input gives the same bytes on every call and every context of one
 * device.  Accuracy is the order-free bound of rsx_reduce_by_key_device: |result - exact| <= g(c - 1) * sum |v| for a
 * bin of c values.
 * With RSX_BIN_ACCUMULATE in `flags` the store becomes out[b] = out[b] (+) r[b], r the result without the flag, and the
 * counts are added likewise; without it every one of the m + 1 entries of each given output is overwritten.  n == 0 or
 * N == 0 still writes the identities -- or, accumulating, leaves the outputs alone.  m == 0 combines all N values into
 * the one bin without reading a key (d_keys may be NULL).  Edges that are not sorted give an unspecified grouping, but no
 * access leaves the arrays and the counts still sum to N.
 * RSX_ERR_ARG: bad widths, kinds, mode, order, operator, flags or count_bytes; edges or a descending order in the index
 * mode; d_out_values NULL; a needed pointer NULL; a pointer not aligned (keys and edges: key_bytes; values: value_bytes;
 * counts: count_bytes; d_num: 8); an output that overlaps an input or the other output.  RSX_ERR_UNSUPPORTED, with
 * nothing enqueued: n >= 2^32; float or 16-byte keys in the index mode; m above max_edges (edge modes) or max_index_bins
 * (index mode) of rsx_bin_reduce_caps.  All of these are answered before the context is looked at.
 *
 * Two launches.  The first runs min(ceil(n / share), 2 * CUs) persistent workgroups, each owning one contiguous share of
 * the rows: mapped edges, one row of m + 1 accumulators per wave and one row of counters in LDS; a wave takes 64
 * consecutive rows per round, finds their bins, and either -- all 64 in one bin -- adds in registers, or matches equal bins
 * (a wave match), combines the matched lanes' values along the peer mask in a fixed order and lets the group's first lane
 * update the wave's own row by a plain read, combine and write; at the end the four rows are combined in wave order and
 * stored into the workgroup's column of a workspace matrix.  The second gives every bin a wave that combines its row of
 * partials in a fixed order, applies the flag and writes the outputs.  No zeroing launch, no workgroup waits for another.
 * Stream-ordered, no synchronisation, the host reads nothing.  Workspace: (value_bytes + 4) (m + 1) bytes per workgroup;
 * made on first use or by rsx_ctx_reserve_bin_reduce.  Under capture without a sufficient reserve the call returns
 * RSX_ERR_WORKSPACE and enqueues nothing.  RSX_INFO_LAST_PASSES reports path 19 and, in bits 0-7, the kernels launched. */
int rsx_bin_reduce_device(rsx_ctx *ctx, const void *d_keys, const void *d_values, size_t n, const uint64_t *d_num,
                          uint32_t key_bytes, uint32_t key_kind, const void *d_edges, uint32_t m, uint32_t mode, int order,
                          uint32_t value_bytes, uint32_t value_kind, int op, void *d_out_values,
                          void *d_out_counts, uint32_t count_bytes, uint32_t flags, void *stream);
int rsx_ctx_reserve_bin_reduce(rsx_ctx *ctx, size_t n, uint32_t m, uint32_t key_bytes, uint32_t value_bytes);
/* Host-only, needs no device: *max_edges = the most edges of an edge mode, *max_index_bins = the largest m of the index
 * mode -- what the first launch's LDS holds beside four waves' m + 1 accumulators of value_bytes and m + 1 counters, within
 * 80 KiB so that two workgroups fit a CU, and at most 2047, the 11 bits of the wave match --, *tile = the rows of one tile
 * of the first launch, *share = the fewest rows worth a workgroup. */
int rsx_bin_reduce_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t *max_edges, uint32_t *max_index_bins,
                        uint32_t *tile, uint32_t *share);

/* -- several key columns ----------------------------------------------------- */
/* Sorting a table by (a, b descending, c): ncols key columns of n keys each, column 0 the MOST significant (the opposite
 * of numpy.lexsort, whose last key is the primary one).  Every column has its own key_bytes (1, 2, 4, 8, 16), key_kind
 * (RSX_KEY_*; float at 4 and 8 bytes only) and direction.  With M(j, i) the mapped key of key i of column j -- the mapping
 * of rsx_argsort_device, complemented when column j is descending -- the result is the ONE permutation p for which the
 * tuples (M(0, p[t]), ..., M(ncols-1, p[t])) are non-decreasing in t and equal tuples have increasing p: stable whatever
 * the directions.  Floats order by bit pattern: -NaN first, +NaN last, -0.0 before +0.0.
 *
 *   rsx_lexsort_device       writes p into d_index as index_bytes-wide integers (4 or 8); the columns are only read.
 *                            n == 0 writes nothing, n == 1 writes 0.
 *   rsx_sort_columns_device  applies p in place to every column and to the n values of value_bytes (0 .. 32768) at
 *                            d_values (NULL with value_bytes 0: the keys alone).  THE COLUMNS ARE WRITTEN by this call; the
 *                            const on rsx_key_column::d_keys is there so that one array of columns serves both calls.
 *                            n <= 1 writes nothing.
 * Columns are aligned to their key_bytes, d_index to index_bytes, d_values as in rsx_sort_pairs_device.  Columns that
 * overlap each other, d_index or d_values are undefined behaviour.  RSX_ERR_ARG: ncols 0 or above RSX_LEX_MAX_COLUMNS,
 * cols NULL, a nonzero `reserved`, index_bytes not 4 or 8, value_bytes above 32768, d_values and value_bytes disagreeing,
 * a NULL or misaligned pointer with n > 0.  RSX_ERR_UNSUPPORTED: a key_bytes or key_kind without kernels, n >= 2^32.
 * Stream-ordered, no synchronisation, the host reads nothing from the device.
 *
 * The plan (rsx_lex_plan, a function of the column widths alone): the columns are walked from the last to the first and
 * whole columns are added to the current round while the round's key bytes K stay <= 16; otherwise the next round begins
 * (a column is never split).  Round 0 holds the least significant columns and runs first; the last round holds column 0.
 * A round's compound key has W bytes, the smallest of 1, 2, 4, 8, 16 with W >= K: the round's most significant column in
 * the highest of the K used bytes, little-endian, the W - K bytes above them zero.  One join kernel per round maps and
 * packs the columns and puts a uint32 position behind the key (the joined element of rsx_argsort_device for key_bytes W:
 * 8, 16 or 32 bytes); from the second round on it reads the columns through the positions of the previous round's sorted
 * elements.  The elements are sorted as unsigned W-byte keys by the kernels every call uses, stable, so that each round
 * keeps the previous one's order among equal keys.  rsx_lexsort_device then writes the positions of the last round's
 * elements; rsx_sort_columns_device copies every column, and the values, into a staging area and gathers it back through
 * those positions, so every input is consumed before it is stored.
 * Workspace: two element arrays of the widest round and, for rsx_sort_columns_device, n * max(widest column,
 * value_bytes) bytes of staging, made on first use or by rsx_ctx_reserve_lex; under capture without a sufficient
 * reserve the calls return RSX_ERR_WORKSPACE and enqueue nothing.  RSX_INFO_LAST_LEX reports the rounds. */
typedef struct rsx_key_column {
    const void *d_keys;   /* n keys of key_bytes */
    uint32_t key_bytes;   /* 1, 2, 4, 8, 16 */
    uint32_t key_kind;    /* RSX_KEY_* */
    uint32_t descending;  /* 0 ascending, anything else descending */
    uint32_t reserved;    /* 0 */
} rsx_key_column;         /* 24 bytes */
#define RSX_LEX_MAX_COLUMNS 16
int rsx_lexsort_device(rsx_ctx *ctx, const rsx_key_column *cols, uint32_t ncols, void *d_index, size_t n,
                       uint32_t index_bytes, void *stream);
int rsx_sort_columns_device(rsx_ctx *ctx, const rsx_key_column *cols, uint32_t ncols, void *d_values,
                            uint32_t value_bytes, size_t n, void *stream);
/* Workspace (and the context's first-call set-up) for either call on up to n keys of these columns (d_keys is not looked
 * at) and, for rsx_sort_columns_device, values of value_bytes, so that the call allocates nothing (stream capture). */
int rsx_ctx_reserve_lex(rsx_ctx *ctx, size_t n, const rsx_key_column *cols, uint32_t ncols, uint32_t value_bytes);
/* Host-only, needs no device; d_keys is not looked at.  *rounds = the number of rounds; for round r (0 runs first),
 * first_col[r] = the round's first (most significant) column -- it holds the columns first_col[r] .. first_col[r-1] - 1,
 * round 0 up to ncols - 1 --, key_bytes[r] = K, the sum of their widths, elem_bytes[r] = the bytes of its joined element.
 * Each array has room for RSX_LEX_MAX_COLUMNS entries. */
int rsx_lex_plan(const rsx_key_column *cols, uint32_t ncols, uint32_t *rounds, uint32_t *first_col,
                 uint32_t *key_bytes, uint32_t *elem_bytes);

/* -- per-pass building blocks (multi-GPU bucket exchange) ---------------- */
/* 256-bin count of digit `digit` (0 = least significant) over `n` elements:
 * the count phase, mod.rs:90-109, with "chunk" = this device's slice.
 * `d_hist` receives 256 uint64 counts (overwritten). */
int rsx_histogram_device(rsx_ctx *ctx, const void *d_src, size_t n, const rsx_layout *layout,
                         uint32_t digit, uint64_t *d_hist, void *stream);
/* One stable LSD pass by `digit`, d_src -> d_dst (count -> scan -> scatter of
 * mod.rs:90-168 for one current_digit_index).  If `d_hist` is non-NULL it
 * receives the 256 uint64 digit counts of the slice. */
int rsx_partition_device(rsx_ctx *ctx, const void *d_src, void *d_dst, size_t n,
                         const rsx_layout *layout, uint32_t digit, uint64_t *d_hist, void *stream);
/* The same pass over `nsub` (1..16) independent position sub-ranges of the slice, in two steps, so that a
 * multi-GPU driver can put the buckets of sub-range 0 on the links while sub-range 1 is still being scattered:
 * sub-range k = elements [n*k/nsub, n*(k+1)/nsub).
 *   rsx_partition_count_device    counts `digit` over every sub-range (count phase, mod.rs:90-109, chunk ==
 *                                 sub-range): d_hist receives nsub x 256 uint64; the context keeps the count
 *                                 matrices for the scatter calls that follow;
 *   rsx_partition_scatter_device  stable partition of sub-range k by `digit` (prefix + scatter, mod.rs:110-168):
 *                                 its elements land in the same position range of d_dst, grouped by digit.
 * Every scatter call of a count call must name the same src, n, layout, digit and nsub. */
int rsx_partition_count_device(rsx_ctx *ctx, const void *d_src, size_t n, const rsx_layout *layout, uint32_t digit,
                               uint32_t nsub, uint64_t *d_hist, void *stream);
int rsx_partition_scatter_device(rsx_ctx *ctx, const void *d_src, void *d_dst, size_t n, const rsx_layout *layout,
                                 uint32_t digit, uint32_t nsub, uint32_t k, void *stream);

/* Segmented device copy: for i in [0, nseg): copy len[i] ELEMENTS of
 * `elem_bytes` from d_src + src_off[i] to d_dst + dst_off[i] (offsets in
 * elements).  Places the received (digit, source-GPU) runs after the
 * all-to-all -- the "digit-major, chunk-minor" order of mod.rs:110-120 with
 * chunk == GPU.  The three tables are device arrays of nseg uint64. */
int rsx_segmented_copy_device(rsx_ctx *ctx, const void *d_src, void *d_dst, uint32_t elem_bytes,
                              const uint64_t *d_src_off, const uint64_t *d_dst_off,
                              const uint64_t *d_len, uint32_t nseg, void *stream);

/* Lower and upper bounds of `nq` 128-bit mapped-key queries in a slice that is
 * already sorted: d_queries holds nq pairs (low 64 bits, high 64 bits) of the
 * mapped key of radix_digits.rs:7-124 (unsigned order == sort order); d_out
 * receives 2*nq uint64: d_out[i] = elements with key < query i, d_out[nq + i] =
 * elements with key <= query i.  The splitter search of a multi-GPU sort asks
 * these of every locally sorted slice (mod.rs:110-120's cursors, by search
 * instead of by scan). */
int rsx_bounds_device(rsx_ctx *ctx, const void *d_sorted, size_t n, const rsx_layout *layout,
                      const uint64_t *d_queries, uint32_t nq, uint64_t *d_out, void *stream);
/* The same with a range per query: query i is answered inside elements [d_ranges[2i], d_ranges[2i+1]) of
 * `d_data` (a range sorted by mapped key; different queries may name different ranges), counts relative
 * to the range's start.  One call then serves all boundaries of the exchange-first schedule, whose
 * sorted pieces are the top-digit buckets the boundaries fall into. */
int rsx_bounds_ranges_device(rsx_ctx *ctx, const void *d_data, size_t n, const rsx_layout *layout,
                             const uint64_t *d_queries, const uint64_t *d_ranges, uint32_t nq, uint64_t *d_out,
                             void *stream);

/* One digit of the splitter search with the key prefix kept on the device (no host round trip per digit): for
 * boundary b (0 .. nb-1), d_ranges[2b], d_ranges[2b+1] name a range of `d_data` sorted by mapped key and
 * d_prefix[2b], d_prefix[2b+1] hold the low / high 64 bits of the mapped key with the digits above `digit` fixed and
 * the rest zero.  rsx_splitter_count_device writes d_less[b*256 + j] = elements of range b with key below
 * prefix_b | j << 8*digit; the caller sums d_less over the ranks (an all-reduce on the device); then
 * rsx_splitter_pick_device ORs into prefix_b the largest j whose summed count does not exceed d_rank[b].  After digit
 * 0, rsx_bounds_ranges_device with d_queries = d_prefix gives the final (less, less-or-equal) counts. */
int rsx_splitter_count_device(rsx_ctx *ctx, const void *d_data, size_t n, const rsx_layout *layout,
                              const uint64_t *d_ranges, const uint64_t *d_prefix, uint32_t nb, uint32_t digit,
                              uint64_t *d_less, void *stream);
int rsx_splitter_pick_device(rsx_ctx *ctx, const uint64_t *d_total, const uint64_t *d_rank, uint64_t *d_prefix,
                             uint32_t nb, uint32_t digit, void *stream);

/* -- multi-GPU from one process ------------------------------------------- */
/* Sorts the concatenation slice 0 | slice 1 | ... | slice ndev-1 as ONE array,
 * stably and in place: slice g keeps its length n_per_dev[g] and ends up
 * holding elements [sum(n_per_dev[..g]), +n_per_dev[g]) of the sorted whole --
 * bit-identical to rsx_sort_device on the concatenation.  "Chunk per thread"
 * of mod.rs:66-70,90-168 becomes "slice per GPU".  ctxs[g] is bound to the
 * device that holds d_slices[g] and d_tmps[g] (scratch of the same size as the
 * slice); one context per slice, several may share a device.  Blocking; uses
 * one private stream per slice; data crosses devices once (peer copies over
 * xGMI).  Errors are reported on ctxs[0]. */
int rsx_sort_sharded(rsx_ctx *const *ctxs, uint32_t ndev, void *const *d_slices, void *const *d_tmps,
                     const size_t *n_per_dev, const rsx_layout *layout);
/* The same with the schedule named.  Both move every element across devices once and give the
 * same bytes:
 *   RSX_SHARD_EXCHANGE_FIRST (what rsx_sort_sharded runs): one stable partition pass by the most
 *     significant digit per slice, the G x 256 counts laid out globally (mod.rs:110-120 with chunk ==
 *     slice), boundary buckets sorted locally and cut exactly, exchange, ONE local sort;
 *   RSX_SHARD_SORT_FIRST: local sort, exact splitters by search in the sorted slices, exchange,
 *     second local sort. */
enum { RSX_SHARD_EXCHANGE_FIRST = 0, RSX_SHARD_SORT_FIRST = 1 };
int rsx_sort_sharded_ex(rsx_ctx *const *ctxs, uint32_t ndev, void *const *d_slices, void *const *d_tmps,
                        const size_t *n_per_dev, const rsx_layout *layout, int schedule);

/* -- harness helpers (input generation / verification on device) --------- */
enum {
    RSX_GEN_UNIFORM = 0, /* key = splitmix64(seed, i) truncated        (distr.rs:40-52 KeyUniform shape) */
    RSX_GEN_ZIPF = 1,    /* key ~ Zipf-shaped over [0, 2^bits - 1), exponent s = param: floor(2^(u bits)) - 1
                            for s = 1                                   (distr.rs:54-76,108-130)         */
    RSX_GEN_STEP = 2,    /* key uniform over `param` equally spaced values (distr.rs:78-106,132-160)    */
    RSX_GEN_SORTED = 3,  /* key = i (already sorted)                                                   */
    RSX_GEN_REVERSED = 4,/* key = n-1-i                                                                */
    RSX_GEN_CONSTANT = 5,/* key = param                                                                */
    RSX_GEN_GEOMETRIC = 6,/* key ~ Geometric(p = param): failures before the first success (distr.rs:3-38 MyExp) */
    RSX_GEN_PAYLOAD_ZERO = 0x100 /* OR into `gen`: payload bytes are 0, the reference's `(key, 0)` pairs
                                    (distr.rs:22-26,42-52), instead of the element's index */
};
/* Fills `n` elements: key field generated as above -- counter-based (splitmix64 of seed and
 * index) and in integer arithmetic throughout, so the same (seed, index) gives the same key on
 * any device and in the CPU restatement (tests/test_generators.py compares them byte for byte);
 * the one exception is RSX_GEN_ZIPF with param != 1, which uses the device's double-precision
 * pow.  The reference draws from rand_distr with an unseeded thread_rng: these are its
 * distributions' shapes, not its streams.  Every payload byte outside the key holds the low
 * bytes of the element's global index `index_base + i` (reveals instability) unless
 * RSX_GEN_PAYLOAD_ZERO is set. */
int rsx_generate_device(rsx_ctx *ctx, void *d_data, size_t n, const rsx_layout *layout, int gen,
                        uint64_t seed, double param, uint64_t index_base, void *stream);
/* Order check + order-independent checksum, on device:
 *   out[0] = number of adjacent pairs (i, i+1) with mapped_key[i] > mapped_key[i+1]
 *   out[1] = sum over elements of hash(element bytes) mod 2^64 (multiset checksum);
 *            hash: h = 0x243F6A8885A308D3, then for each of the elem_bytes bytes b in
 *            order h = splitmix64(h ^ b)  (the SplitMix64 output step: h += 0x9E3779B97F4A7C15,
 *            h = (h ^ h >> 30) * 0xBF58476D1CE4E5B9, h = (h ^ h >> 27) * 0x94D049BB133111EB, h ^ h >> 31)
 *   out[2] = number of adjacent equal-key pairs whose payload index decreases: the first 8
 *            bytes outside the key, read little-endian (stability violations; meaningful for
 *            rsx_generate_device payloads; 0 for elements that are all key)
 * `d_out` is 3 uint64 on the device (overwritten by every call, not accumulated); n == 0 writes
 * three zeros and does not look at d_data.  tests/test_gpu_verify.py holds all three words
 * against a numpy restatement. */
int rsx_verify_device(rsx_ctx *ctx, const void *d_data, size_t n, const rsx_layout *layout,
                      uint64_t *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RSX_H */
