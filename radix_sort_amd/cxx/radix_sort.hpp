// radix_sort.hpp -- C++ host mirror of the reference's operator interface over the
// C-ABI of include/rsx.h (the reference is compiled Rust; no Rust toolchain exists in
// the build image, so the host side above the C-ABI is C++ here and the Rust shim a
// maintainer would add is given as text in INTEGRATION.md / rust/).
//
// Reference interface (src/radix_sort/radix_digits.rs:1-5, src/radix_sort/mod.rs:18-20):
//     pub trait RadixDigits { const NUMBER_OF_DIGITS: u8; fn get_digit(&self, index: u8) -> u8; }
//     pub trait RadixSort<T: RadixDigits> { fn radix_sort(&mut self); }      impl for [T]
// Mirror:
//     rsx::RadixDigits<T>::NUMBER_OF_DIGITS / ::get_digit(const T&, index) / ::layout()
//     rsx::radix_sort(T* data, size_t n)            // host slice, in place, blocking (mod.rs:62)
//     rsx::radix_sort(std::vector<T>& v)
//     rsx::radix_sort_device(T* d_data, T* d_tmp, size_t n, hipStream_t)   // device-resident
//     rsx::radix_sort_pairs(K* d_keys, V* d_values, size_t n, bool descending, hipStream_t)   // separate columns
//     rsx::radix_argsort(const K* d_keys, I* d_index, size_t n, bool descending, hipStream_t)
//     rsx::unique(const K* d_keys, size_t n, K* keys, uint64_t* offsets, I* perm, I* inverse, uint64_t* num, bool descending, hipStream_t)
//     rsx::reduce_by_key(const K* d_keys, const V* d_values, size_t n, int op, K* keys, V* values, uint64_t* offsets, uint64_t* num, bool descending, hipStream_t)
//     rsx::scan_by_key(const K* d_keys, const V* d_values, size_t n, int op, V* d_out, bool exclusive, V first, bool runs, uint64_t* num, hipStream_t)
//     rsx::search_sorted(const K* d_sorted, size_t n, const K* d_needles, size_t m, I* lower, I* upper, bool descending, const uint64_t* d_sorted_num, bool presort, hipStream_t)
//     rsx::merge(const K* d_a_keys, size_t na, const K* d_b_keys, size_t nb, K* d_out_keys, bool descending, hipStream_t)   // two sorted arrays
//     rsx::merge_pairs(const K* d_a_keys, const V* d_a_values, size_t na, const K* d_b_keys, const V* d_b_values, size_t nb, K* keys, V* values[, I* index], bool descending, hipStream_t)
//     rsx::set_op(int op, const K* d_a_keys, size_t na, const K* d_b_keys, size_t nb, K* d_out_keys, uint64_t* d_out_num[, I* index], bool descending, const uint64_t* d_a_num, const uint64_t* d_b_num, hipStream_t)   // RSX_SETOP_*
//     rsx::set_op_pairs(int op, const K* d_a_keys, const V* d_a_values, size_t na, const K* d_b_keys, const V* d_b_values, size_t nb, K* keys, V* values, uint64_t* d_out_num, bool descending, const uint64_t* d_a_num, const uint64_t* d_b_num, hipStream_t)
//     rsx::join(int how, const K* d_a_keys, size_t na, const K* d_b_keys, size_t nb, I* d_out_a, I* d_out_b, size_t capacity, uint64_t* d_out_num, bool descending, const uint64_t* d_a_num, const uint64_t* d_b_num, const I* d_a_index, const I* d_b_index, hipStream_t)   // RSX_JOIN_*
//     rsx::join_count(int how, const K* d_a_keys, size_t na, const K* d_b_keys, size_t nb, uint64_t* d_out_num, bool descending, const uint64_t* d_a_num, const uint64_t* d_b_num, hipStream_t)
//     rsx::select(const K* d_keys, size_t n, const uint64_t* ranks /* host */, uint32_t nranks, K* d_out_keys, I* d_out_index, bool descending, hipStream_t)   // order statistics, no sort
//     rsx::bin_count(const K* d_keys, size_t n, const K* d_edges, uint32_t m, uint32_t mode, C* d_counts, bool descending, bool accumulate, const uint64_t* d_num, hipStream_t)   // RSX_BIN_*: histogram, bincount
//     rsx::compact(const K* d_keys, size_t n, const uint8_t* d_flags, const K* d_lo, const K* d_hi, const V* d_values, K* d_out_keys, V* d_out_values, I* d_out_index, uint64_t* d_out_num, uint32_t flags, bool descending, const uint64_t* d_num, hipStream_t)   // RSX_COMPACT_*: select-if, partition, nonzero
//     rsx::multisplit(const K* d_keys, size_t n, const K* d_edges, uint32_t m, uint32_t mode, const V* d_values, K* d_out_keys, V* d_out_values, I* d_out_index, uint64_t* d_out_offsets, bool descending, const uint64_t* d_num, hipStream_t)   // RSX_BIN_*: stable multi-way partition, CSR offsets
//     rsx::bin_reduce(const K* d_keys, const V* d_values, size_t n, const K* d_edges, uint32_t m, uint32_t mode, int op, V* d_out_values, C* d_out_counts, bool descending, bool accumulate, const uint64_t* d_num, hipStream_t)   // RSX_BIN_* x RSX_REDUCE_*: weighted histogram, bincount(weights=)
//     rsx::lexsort({rsx::key_column(d_a), rsx::key_column(d_b, true)}, I* d_index, size_t n, hipStream_t)   // several key columns
//     rsx::sort_columns({rsx::key_column(d_a), rsx::key_column(d_b, true)}, V* d_values, size_t n, hipStream_t)
// Errors: the reference panics (mod.rs:68,106); here std::runtime_error is thrown.
// Empty and one-element slices return immediately (the reference panics on an empty
// slice -- chunks(0), mod.rs:66-70,92 -- there is no output to differ from).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rsx.h"

namespace rsx {

// ---- key model (radix_digits.rs) ----------------------------------------------------
// Specialise for user types: provide layout() (and get_digit for host use).  A specialisation may name any element
// size and any key_bytes from 1 to 16 (RSX_KEY_UNSIGNED / RSX_KEY_SIGNED; 4 or 8 for RSX_KEY_FLOAT), e.g. a packed
// 6-byte record with a 48-bit key: layouts without kernels of their own are sorted through a canonical key
// (include/rsx.h, "Any layout").
template <typename T, typename Enable = void>
struct RadixDigits;

namespace detail {
template <typename T>
constexpr uint32_t kind_of() {
    return std::is_floating_point<T>::value ? RSX_KEY_FLOAT : std::is_signed<T>::value ? RSX_KEY_SIGNED : RSX_KEY_UNSIGNED;
}
inline uint8_t digit_of(const unsigned char* key, uint32_t key_bytes, uint32_t kind, uint8_t index) {
    const uint32_t top = key_bytes - 1;
    uint8_t b = key[index];  // little-endian: byte `index` == (x >> 8*index) as u8
    if (kind == RSX_KEY_SIGNED) {
        if (index == top) b ^= 0x80;  // (x ^ MIN) >> ...   radix_digits.rs:55-101
    } else if (kind == RSX_KEY_FLOAT) {
        if (key[top] & 0x80) b ^= 0xFF;  // b ^= (b >> 31) | MIN   radix_digits.rs:103-124
        else if (index == top) b ^= 0x80;
    }
    return b;
}
}  // namespace detail

// u8..u64, i8..i64, f32, f64 (radix_digits.rs:7-38,47-85,95-124; usize/isize are the 64-bit ones)
template <typename T>
struct RadixDigits<T, typename std::enable_if<std::is_arithmetic<T>::value && !std::is_same<T, bool>::value &&
                                              sizeof(T) <= 8>::type> {
    static constexpr uint8_t NUMBER_OF_DIGITS = sizeof(T);
    static rsx_layout layout() { return rsx_layout{sizeof(T), 0, sizeof(T), detail::kind_of<T>()}; }
    static uint8_t get_digit(const T& x, uint8_t index) {
        unsigned char raw[sizeof(T)];
        std::memcpy(raw, &x, sizeof(T));
        return detail::digit_of(raw, sizeof(T), detail::kind_of<T>(), index);
    }
};

#if defined(__SIZEOF_INT128__)
// u128 / i128 (radix_digits.rs:39-45,87-93)
template <>
struct RadixDigits<unsigned __int128> {
    static constexpr uint8_t NUMBER_OF_DIGITS = 16;
    static rsx_layout layout() { return rsx_layout{16, 0, 16, RSX_KEY_UNSIGNED}; }
    static uint8_t get_digit(const unsigned __int128& x, uint8_t index) { return (uint8_t)(x >> (8 * index)); }
};
template <>
struct RadixDigits<__int128> {
    static constexpr uint8_t NUMBER_OF_DIGITS = 16;
    static rsx_layout layout() { return rsx_layout{16, 0, 16, RSX_KEY_SIGNED}; }
    static uint8_t get_digit(const __int128& x, uint8_t index) {
        unsigned char raw[16];
        std::memcpy(raw, &x, 16);
        return detail::digit_of(raw, 16, RSX_KEY_SIGNED, index);
    }
};
#endif

// (K, U): key `.first`, opaque payload carried along (radix_digits.rs:126-136).  The key offset
// is taken from the actual object layout, as the Rust shim must do with offset_of!.
template <typename K, typename U>
struct RadixDigits<std::pair<K, U>> {
    static constexpr uint8_t NUMBER_OF_DIGITS = RadixDigits<K>::NUMBER_OF_DIGITS;
    static rsx_layout layout() {
        // elements are moved bitwise (mod.rs:133-140 uses copy_nonoverlapping); std::pair itself is never
        // "trivially copyable" (user-provided assignment), so the requirement is put on its members
        static_assert(std::is_trivially_copyable<K>::value && std::is_trivially_copyable<U>::value,
                      "radix_sort moves elements bitwise: key and payload must be trivially copyable");
        const std::pair<K, U>* p = nullptr;
        const uint32_t off = (uint32_t)(reinterpret_cast<const char*>(&p->first) - reinterpret_cast<const char*>(p));
        rsx_layout k = RadixDigits<K>::layout();
        return rsx_layout{(uint32_t)sizeof(std::pair<K, U>), off + k.key_offset, k.key_bytes, k.key_kind};
    }
    static uint8_t get_digit(const std::pair<K, U>& x, uint8_t index) { return RadixDigits<K>::get_digit(x.first, index); }
};

// ---- the sort (mod.rs:18-20,61-176) -------------------------------------------------
class Context {
public:
    explicit Context(int device = -1) {
        const int rc = rsx_ctx_create(device, &ctx_);
        if (rc != RSX_OK) throw std::runtime_error(std::string("rsx_ctx_create: ") + rsx_strerror(rc));
    }
    ~Context() {
        if (ctx_) rsx_ctx_destroy(ctx_);
    }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    rsx_ctx* get() const { return ctx_; }
    void check(int rc, const char* what) const {
        if (rc != RSX_OK)
            throw std::runtime_error(std::string(what) + ": " + rsx_strerror(rc) + " (" + rsx_last_error(ctx_) + ")");
    }
    // rsx_ctx_check: synchronises `stream` and throws if a kernel of this context gave up a device-side
    // wait.  The stream-ordered radix_sort_device cannot report that by itself (the reference's analogue
    // is the worker panic of mod.rs:106): call this where you synchronise.
    void synchronize_and_check(void* stream = nullptr) const { check(rsx_ctx_check(ctx_, stream), "rsx_ctx_check"); }
    // rsx_ctx_set_option: force one of the bit-exact alternative kernel paths (RSX_OPT_*)
    void set_option(int option, uint64_t value) const { check(rsx_ctx_set_option(ctx_, option, value), "rsx_ctx_set_option"); }

private:
    rsx_ctx* ctx_ = nullptr;
};

inline Context& default_context() {
    static Context c(-1);
    return c;
}

// `<[T]>::radix_sort(&mut self)`: in place on a host slice, blocking.
template <typename T>
void radix_sort(T* data, size_t n, Context& ctx = default_context()) {
    const rsx_layout L = RadixDigits<T>::layout();
    ctx.check(rsx_sort_host(ctx.get(), data, n, &L), "rsx_sort_host");
}
template <typename T>
void radix_sort(std::vector<T>& v, Context& ctx = default_context()) {
    radix_sort(v.data(), v.size(), ctx);
}
// Device-resident form: `d_tmp` is the reference's `temp` (mod.rs:71-83); stream-ordered, not synchronised.
// A device-side failure surfaces at ctx.synchronize_and_check(stream) (or at the next sort on the context).
template <typename T>
void radix_sort_device(T* d_data, T* d_tmp, size_t n, void* stream = nullptr, Context& ctx = default_context()) {
    const rsx_layout L = RadixDigits<T>::layout();
    ctx.check(rsx_sort_device(ctx.get(), d_data, d_tmp, n, &L, stream), "rsx_sort_device");
}

// Many segments of one device array in one call (rsx_sort_segments_device): segment i is elements
// [d_offsets[i], d_offsets[i+1]) -- nseg + 1 offsets ON THE DEVICE -- sorted on its own, stably, in place.
// T needs a layout with kernels of its own (sizes 1, 2, 4, 8, 12, 16, 24, 32).  max_seg_len: an upper bound on the
// segment lengths if the caller has one (0: unknown).  Stream-ordered; bad offsets surface at synchronize_and_check.
template <typename T>
void radix_sort_segments(T* d_data, T* d_tmp, size_t n, const uint64_t* d_offsets, size_t nseg, void* stream = nullptr,
                         uint64_t max_seg_len = 0, Context& ctx = default_context()) {
    const rsx_layout L = RadixDigits<T>::layout();
    ctx.check(rsx_sort_segments_device(ctx.get(), d_data, d_tmp, n, &L, d_offsets, nseg, max_seg_len, stream), "rsx_sort_segments_device");
}
// ... and of a contiguous rows x row_len array along its last dimension (rsx_sort_rows_device).
template <typename T>
void radix_sort_rows(T* d_data, T* d_tmp, size_t rows, size_t row_len, void* stream = nullptr, Context& ctx = default_context()) {
    const rsx_layout L = RadixDigits<T>::layout();
    ctx.check(rsx_sort_rows_device(ctx.get(), d_data, d_tmp, rows, row_len, &L, stream), "rsx_sort_rows_device");
}

// Separate key and value arrays on the device (rsx_sort_pairs_device): both sorted in place by key, stably, ascending
// or descending (larger mapped key first, equal keys in input order).  K: a type with a RadixDigits whose element IS
// its key (the primitives); V: any trivially copyable type, moved bitwise.  Stream-ordered; the joined elements live
// in the context's workspace (rsx_ctx_reserve_pairs before a stream capture).
template <typename K, typename V>
void radix_sort_pairs(K* d_keys, V* d_values, size_t n, bool descending = false, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_trivially_copyable<V>::value, "values are moved bitwise");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("radix_sort_pairs: the key type must be its own key");
    ctx.check(rsx_sort_pairs_device(ctx.get(), d_keys, d_values, n, L.key_bytes, L.key_kind, (uint32_t)sizeof(V),
                                    descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, stream), "rsx_sort_pairs_device");
}
// ... keys alone
template <typename K>
void radix_sort_keys(K* d_keys, size_t n, bool descending = false, void* stream = nullptr, Context& ctx = default_context()) {
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("radix_sort_keys: the key type must be its own key");
    ctx.check(rsx_sort_pairs_device(ctx.get(), d_keys, nullptr, n, L.key_bytes, L.key_kind, 0,
                                    descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, stream), "rsx_sort_pairs_device");
}
// The stable sorting permutation of d_keys (rsx_argsort_device) as uint32_t / int32_t or uint64_t / int64_t indices;
// the keys are only read.
template <typename K, typename I>
void radix_argsort(const K* d_keys, I* d_index, size_t n, bool descending = false, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 4- or 8-byte integers");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("radix_argsort: the key type must be its own key");
    ctx.check(rsx_argsort_device(ctx.get(), d_keys, d_index, n, L.key_bytes, L.key_kind, (uint32_t)sizeof(I),
                                 descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, stream), "rsx_argsort_device");
}

// The groups of equal keys of that permutation (rsx_unique_device): d_out_keys[j], j < m, the distinct keys in order;
// d_out_offsets[j], j <= m, where group j starts in the sorted order (n + 1 entries; the d_offsets of the segmented
// calls below); d_out_perm the permutation itself; d_out_inverse[q] the group of input position q; *d_out_num = m.
// Every output but d_out_num may be nullptr; without perm and inverse the keys are sorted alone.  The keys are only
// read.  Stream-ordered, never synchronised (rsx_ctx_reserve_unique before a stream capture).
template <typename K, typename I = uint64_t>
void unique(const K* d_keys, size_t n, K* d_out_keys, uint64_t* d_out_offsets, I* d_out_perm, I* d_out_inverse, uint64_t* d_out_num,
            bool descending = false, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 4- or 8-byte integers");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("unique: the key type must be its own key");
    ctx.check(rsx_unique_device(ctx.get(), d_keys, n, L.key_bytes, L.key_kind, descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING,
                                d_out_keys, d_out_offsets, d_out_perm, d_out_inverse, (uint32_t)sizeof(I), d_out_num, stream),
              "rsx_unique_device");
}
// ... keys alone: the distinct keys, the offsets (their differences are the counts) and their number
template <typename K>
void unique_keys(const K* d_keys, size_t n, K* d_out_keys, uint64_t* d_out_offsets, uint64_t* d_out_num, bool descending = false,
                 void* stream = nullptr, Context& ctx = default_context()) {
    unique<K, uint64_t>(d_keys, n, d_out_keys, d_out_offsets, nullptr, nullptr, d_out_num, descending, stream, ctx);
}

// One value per group of those keys (rsx_reduce_by_key_device): d_out_values[j], j < m, the sum (RSX_REDUCE_SUM), minimum
// or maximum of the values whose key is d_out_keys[j], taken in input order; d_out_offsets and d_out_num as in unique.
// V: uint32_t, int32_t, float, uint64_t, int64_t or double.  Integer sums wrap; float minima and maxima follow the total
// order on bit patterns; a float sum is added in an order fixed by n and the group's place alone (no atomics: the same
// input gives the same bits on every call).  d_out_offsets, and one of d_out_keys and d_out_values, may be nullptr;
// d_out_keys may be d_keys and d_out_values may be d_values.  Stream-ordered, never synchronised (rsx_ctx_reserve_reduce
// before a stream capture).
template <typename K, typename V>
void reduce_by_key(const K* d_keys, const V* d_values, size_t n, int op, K* d_out_keys, V* d_out_values, uint64_t* d_out_offsets,
                   uint64_t* d_out_num, bool descending = false, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_arithmetic<V>::value && !std::is_same<V, bool>::value && (sizeof(V) == 4 || sizeof(V) == 8),
                  "values are 4- or 8-byte integers or floats");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("reduce_by_key: the key type must be its own key");
    const uint32_t vkind = std::is_floating_point<V>::value ? RSX_KEY_FLOAT : std::is_signed<V>::value ? RSX_KEY_SIGNED : RSX_KEY_UNSIGNED;
    ctx.check(rsx_reduce_by_key_device(ctx.get(), d_keys, d_values, n, L.key_bytes, L.key_kind, (uint32_t)sizeof(V), vkind, op,
                                       descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, d_out_keys, d_out_values, d_out_offsets,
                                       d_out_num, stream),
              "rsx_reduce_by_key_device");
}

// One result per ROW (rsx_scan_by_key_device): d_out[q] the running sum (RSX_REDUCE_SUM), minimum or maximum of the values
// of q's group up to and including q -- the group being every row with q's key or, with runs, the run of consecutive
// rows with it (nothing is sorted then).  exclusive: the result of q's predecessor in the group, and `first`, stored and
// never combined, at a group's first row.  d_values == nullptr is the count form: every value is V(1) (V an integer, op
// RSX_REDUCE_SUM), the results are 1-based ranks, or exclusive with first = 0 the 0-based ones.  d_out_num (optional)
// receives the number of groups.  V and the operators as in reduce_by_key; d_out may be d_values and must not overlap
// d_keys.  Stream-ordered, never synchronised (rsx_ctx_reserve_scan_by_key before a stream capture).
template <typename K, typename V>
void scan_by_key(const K* d_keys, const V* d_values, size_t n, int op, V* d_out, bool exclusive = false, V first = V(), bool runs = false,
                 uint64_t* d_out_num = nullptr, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_arithmetic<V>::value && !std::is_same<V, bool>::value && (sizeof(V) == 4 || sizeof(V) == 8),
                  "values are 4- or 8-byte integers or floats");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("scan_by_key: the key type must be its own key");
    const uint32_t vkind = std::is_floating_point<V>::value ? RSX_KEY_FLOAT : std::is_signed<V>::value ? RSX_KEY_SIGNED : RSX_KEY_UNSIGNED;
    uint64_t bits = 0;
    std::memcpy(&bits, &first, sizeof(V));  // (little-endian: the low sizeof(V) bytes)
    ctx.check(rsx_scan_by_key_device(ctx.get(), d_keys, d_values, n, L.key_bytes, L.key_kind, (uint32_t)sizeof(V), vkind, op,
                                     (exclusive ? (uint32_t)RSX_SCAN_EXCLUSIVE : 0u) | (runs ? (uint32_t)RSX_SCAN_RUNS : 0u), bits, d_out, d_out_num,
                                     stream),
              "rsx_scan_by_key_device");
}

// Where m needles fall in n keys sorted in that order (rsx_search_sorted_device): d_out_lower[i] the number of the sorted
// keys that order before needle i, d_out_upper[i] the number that do not order behind it, so that
// d_sorted[lower[i] .. upper[i]) are the keys equal to it in every bit.  Either output may be nullptr.  d_sorted_num, when
// given, is one device word (the d_out_num of unique): only the first min(n, *d_sorted_num) keys count.  presort: sort the
// needles first (RSX_SEARCH_PRESORT; rsx_ctx_reserve_search before a stream capture) instead of taking them as given,
// which is the streaming merge for ordered needles.  Both arrays are only read.  Stream-ordered, never synchronised.
template <typename K, typename I = uint64_t>
void search_sorted(const K* d_sorted, size_t n, const K* d_needles, size_t m, I* d_out_lower, I* d_out_upper, bool descending = false,
                   const uint64_t* d_sorted_num = nullptr, bool presort = false, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 4- or 8-byte integers");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("search_sorted: the key type must be its own key");
    ctx.check(rsx_search_sorted_device(ctx.get(), d_sorted, n, d_sorted_num, d_needles, m, L.key_bytes, L.key_kind,
                                       descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, d_out_lower, d_out_upper, (uint32_t)sizeof(I),
                                       presort ? (uint32_t)RSX_SEARCH_PRESORT : 0u, stream),
              "rsx_search_sorted_device");
}

// The stable merge of two key arrays that are each sorted in that order (rsx_merge_device): d_out_keys receives the
// na + nb keys of the stable sort of a ++ b, equal keys of a in front of equal keys of b.  merge_pairs moves the values
// with their keys (V: any trivially copyable type; 1, 2, 4, 8 and 16 bytes move in the merge kernel, any other width through
// the context's workspace: rsx_ctx_reserve_merge before a stream capture); its overload with d_out_index also stores the
// position of every output in a ++ b (below na a position in a, else that minus na a position in b).  Any output may be
// nullptr, not all; the inputs are only read and no output may overlap them.  Stream-ordered, never synchronised.
template <typename K, typename V, typename I>
void merge_pairs(const K* d_a_keys, const V* d_a_values, size_t na, const K* d_b_keys, const V* d_b_values, size_t nb, K* d_out_keys,
                 V* d_out_values, I* d_out_index, bool descending = false, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_trivially_copyable<V>::value, "values are moved bitwise");
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 4- or 8-byte integers");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("merge: the key type must be its own key");
    ctx.check(rsx_merge_device(ctx.get(), d_a_keys, d_a_values, na, d_b_keys, d_b_values, nb, L.key_bytes, L.key_kind, (uint32_t)sizeof(V),
                               descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, d_out_keys, d_out_values, d_out_index, (uint32_t)sizeof(I),
                               stream),
              "rsx_merge_device");
}
template <typename K, typename V>
void merge_pairs(const K* d_a_keys, const V* d_a_values, size_t na, const K* d_b_keys, const V* d_b_values, size_t nb, K* d_out_keys,
                 V* d_out_values, bool descending = false, void* stream = nullptr, Context& ctx = default_context()) {
    merge_pairs(d_a_keys, d_a_values, na, d_b_keys, d_b_values, nb, d_out_keys, d_out_values, static_cast<uint64_t*>(nullptr), descending, stream, ctx);
}
template <typename K>
void merge(const K* d_a_keys, size_t na, const K* d_b_keys, size_t nb, K* d_out_keys, bool descending = false, void* stream = nullptr,
           Context& ctx = default_context()) {
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("merge: the key type must be its own key");
    ctx.check(rsx_merge_device(ctx.get(), d_a_keys, nullptr, na, d_b_keys, nullptr, nb, L.key_bytes, L.key_kind, 0u,
                               descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, d_out_keys, nullptr, nullptr, 8u, stream),
              "rsx_merge_device");
}

// A set operation on two key arrays that are each sorted in that order, as multisets (rsx_setop_device; op: RSX_SETOP_UNION,
// _INTERSECTION, _DIFFERENCE, _SYMMETRIC_DIFFERENCE): the kept keys in merge order into d_out_keys, equal keys of a first, and
// their number into the device word d_out_num.  Every output holds na + nb rows (union, symmetric difference), na
// (difference) or min(na, nb) (intersection); rows from *d_out_num on are not written.  d_out_index: the position of every
// kept key in a ++ b (below na a position in a, else that minus na a position in b).  d_a_num / d_b_num, when given, are
// device words such as the d_out_num of unique: only the first min(na, *d_a_num) keys of a count.  set_op_pairs moves the
// values with their keys (V of 1, 2, 4, 8 or 16 bytes; d_b_values may be nullptr for intersection and difference).  The
// inputs are only read and no output may overlap them; rsx_ctx_reserve_setop before a stream capture.  Stream-ordered,
// never synchronised.
template <typename K, typename I>
void set_op(int op, const K* d_a_keys, size_t na, const K* d_b_keys, size_t nb, K* d_out_keys, uint64_t* d_out_num, I* d_out_index,
            bool descending = false, const uint64_t* d_a_num = nullptr, const uint64_t* d_b_num = nullptr, void* stream = nullptr,
            Context& ctx = default_context()) {
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 4- or 8-byte integers");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("set_op: the key type must be its own key");
    ctx.check(rsx_setop_device(ctx.get(), (uint32_t)op, d_a_keys, nullptr, na, d_a_num, d_b_keys, nullptr, nb, d_b_num, L.key_bytes, L.key_kind, 0u,
                               descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, d_out_keys, nullptr, d_out_index, (uint32_t)sizeof(I),
                               d_out_num, stream),
              "rsx_setop_device");
}
template <typename K>
void set_op(int op, const K* d_a_keys, size_t na, const K* d_b_keys, size_t nb, K* d_out_keys, uint64_t* d_out_num, bool descending = false,
            const uint64_t* d_a_num = nullptr, const uint64_t* d_b_num = nullptr, void* stream = nullptr, Context& ctx = default_context()) {
    set_op(op, d_a_keys, na, d_b_keys, nb, d_out_keys, d_out_num, static_cast<uint64_t*>(nullptr), descending, d_a_num, d_b_num, stream, ctx);
}
template <typename K, typename V>
void set_op_pairs(int op, const K* d_a_keys, const V* d_a_values, size_t na, const K* d_b_keys, const V* d_b_values, size_t nb, K* d_out_keys,
                  V* d_out_values, uint64_t* d_out_num, bool descending = false, const uint64_t* d_a_num = nullptr,
                  const uint64_t* d_b_num = nullptr, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_trivially_copyable<V>::value, "values are moved bitwise");
    static_assert(sizeof(V) == 1 || sizeof(V) == 2 || sizeof(V) == 4 || sizeof(V) == 8 || sizeof(V) == 16,
                  "values of 1, 2, 4, 8 or 16 bytes move with their keys; for other widths ask set_op for the index and gather");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("set_op_pairs: the key type must be its own key");
    ctx.check(rsx_setop_device(ctx.get(), (uint32_t)op, d_a_keys, d_a_values, na, d_a_num, d_b_keys, d_b_values, nb, d_b_num, L.key_bytes,
                               L.key_kind, (uint32_t)sizeof(V), descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, d_out_keys,
                               d_out_values, nullptr, 8u, d_out_num, stream),
              "rsx_setop_device");
}

// The join of two key arrays that are each sorted in that order (rsx_join_device; how: RSX_JOIN_INNER, _LEFT, _SEMI, _ANTI):
// row t is a pair of positions (d_out_a[t], d_out_b[t]) of equal keys, ordered by position in a, then in b; a left join
// writes all ones into d_out_b for a key of a without a match; semi and anti joins take d_out_b == nullptr.  The FULL number
// of rows goes into the device word d_out_num whatever `capacity` (the rows of d_out_a / d_out_b) is, and rows from
// min(*d_out_num, capacity) on are not written.  d_a_num / d_b_num, when given, are device words such as the d_out_num of
// unique: only the first min(na, *d_a_num) keys of a count.  d_a_index / d_b_index, when given, hold one word per key that
// is written in place of the position (the permutations of two argsorts: rows of the unsorted tables).  join_count stores
// the number of rows alone, for a caller that sizes its outputs from it.  Fewer than 2^32 keys on each side; the inputs are
// only read and no output may overlap them; rsx_ctx_reserve_join before a stream capture.  Stream-ordered, never
// synchronised.
template <typename K, typename I>
void join(int how, const K* d_a_keys, size_t na, const K* d_b_keys, size_t nb, I* d_out_a, I* d_out_b, size_t capacity, uint64_t* d_out_num,
          bool descending = false, const uint64_t* d_a_num = nullptr, const uint64_t* d_b_num = nullptr, const I* d_a_index = nullptr,
          const I* d_b_index = nullptr, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 4- or 8-byte integers");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("join: the key type must be its own key");
    ctx.check(rsx_join_device(ctx.get(), (uint32_t)how, d_a_keys, na, d_a_num, d_a_index, d_b_keys, nb, d_b_num, d_b_index, L.key_bytes, L.key_kind,
                              descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, d_out_a, d_out_b, (uint32_t)sizeof(I), capacity, d_out_num,
                              stream),
              "rsx_join_device");
}
template <typename K>
void join_count(int how, const K* d_a_keys, size_t na, const K* d_b_keys, size_t nb, uint64_t* d_out_num, bool descending = false,
                const uint64_t* d_a_num = nullptr, const uint64_t* d_b_num = nullptr, void* stream = nullptr, Context& ctx = default_context()) {
    join<K, uint64_t>(how, d_a_keys, na, d_b_keys, nb, nullptr, nullptr, 0, d_out_num, descending, d_a_num, d_b_num, nullptr, nullptr, stream, ctx);
}

// Order statistics of an UNSORTED key array (rsx_select_device): for every q < nranks, d_out_keys[q] and d_out_index[q]
// receive the key at position ranks[q] of the stable sort in that order and its input position -- column ranks[q] of
// radix_argsort, without the sort.  `ranks` is a HOST array of at most select_caps<K>().max_ranks ranks below n, read
// during the call; either output may be nullptr, not both.  d_keys is only read; rsx_ctx_reserve_select before a stream
// capture.  Stream-ordered, never synchronised.
struct SelectCaps {
    uint32_t max_ranks, digit_bits, tile, cand_div, cand_floor;
};
template <typename K>
SelectCaps select_caps() {
    SelectCaps c{};
    const rsx_layout L = RadixDigits<K>::layout();
    if (rsx_select_caps(L.key_bytes, &c.max_ranks, &c.digit_bits, &c.tile, &c.cand_div, &c.cand_floor) != RSX_OK)
        throw std::invalid_argument("select_caps: no select for this key width");
    return c;
}
template <typename K, typename I = uint64_t>
void select(const K* d_keys, size_t n, const uint64_t* ranks, uint32_t nranks, K* d_out_keys, I* d_out_index, bool descending = false,
            void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 4- or 8-byte integers");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("select: the key type must be its own key");
    ctx.check(rsx_select_device(ctx.get(), d_keys, n, L.key_bytes, L.key_kind, ranks, nranks, d_out_keys, d_out_index, (uint32_t)sizeof(I),
                                descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, stream),
              "rsx_select_device");
}

// Keys per bin of an UNSORTED key array (rsx_bin_count_device): d_counts[b], b = 0 .. m, receives (accumulate: is
// increased by) the number of the first n -- or min(n, *d_num) -- keys whose bin is b.  mode RSX_BIN_UPPER / RSX_BIN_LOWER:
// the bin is the number of the m edges, sorted in that order, that are <= / < the key (bins closed on the left / on the
// right; d_counts[0] and d_counts[m] are the two open ends); RSX_BIN_INDEX: integer keys, the bin is the key's value when
// it is in 0 .. m - 1, else m, and d_edges is nullptr.  At most bin_caps<K>().max_edges edges.  The keys and edges are
// only read; there is no workspace, so the call can be captured as it is.  Stream-ordered, never synchronised.
struct BinCaps {
    uint32_t max_edges, max_index_bins_lds, share;
};
template <typename K>
BinCaps bin_caps() {
    BinCaps c{};
    const rsx_layout L = RadixDigits<K>::layout();
    if (rsx_bin_caps(L.key_bytes, &c.max_edges, &c.max_index_bins_lds, &c.share) != RSX_OK)
        throw std::invalid_argument("bin_caps: no bin count for this key width");
    return c;
}
template <typename K, typename C = uint64_t>
void bin_count(const K* d_keys, size_t n, const K* d_edges, uint32_t m, uint32_t mode, C* d_counts, bool descending = false,
               bool accumulate = false, const uint64_t* d_num = nullptr, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_integral<C>::value && (sizeof(C) == 4 || sizeof(C) == 8), "counts are 4- or 8-byte integers");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("bin_count: the key type must be its own key");
    ctx.check(rsx_bin_count_device(ctx.get(), d_keys, n, d_num, L.key_bytes, L.key_kind, d_edges, m, mode,
                                   descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, d_counts, (uint32_t)sizeof(C),
                                   accumulate ? RSX_BIN_ACCUMULATE : 0u, stream),
              "rsx_bin_count_device");
}

// Rows that pass a predicate, in input order (rsx_compact_device): row i of the first n -- or min(n, *d_num) -- passes when
// d_flags[i] != 0 (d_flags given) and *d_lo <= d_keys[i] < *d_hi in the sort's order (each bound given; ONE key on the
// device each); flags RSX_COMPACT_INVERT keeps the others.  The kept keys, values and input positions go to the outputs
// that are not nullptr, their number to *d_out_num; RSX_COMPACT_PARTITION writes the remaining rows behind them, in input
// order too.  d_keys may be nullptr when neither a bound nor d_out_keys is given (K is then any key type, say uint8_t).
// Not in place.  Stream-ordered, never synchronised; Context::reserve is not enough for a capture: rsx_ctx_reserve_compact.
struct CompactCaps {
    uint32_t tile, scan_span;
};
template <typename K, typename V = uint32_t, typename I = uint64_t>
CompactCaps compact_caps(bool with_values = false, bool with_index = false) {
    CompactCaps c{};
    const rsx_layout L = RadixDigits<K>::layout();
    if (rsx_compact_caps(L.key_bytes, with_values ? (uint32_t)sizeof(V) : 0u, with_index ? (uint32_t)sizeof(I) : 0u, &c.tile, &c.scan_span) != RSX_OK)
        throw std::invalid_argument("compact_caps: no compaction for these widths");
    return c;
}
template <typename K, typename V = uint32_t, typename I = uint64_t>
void compact(const K* d_keys, size_t n, const uint8_t* d_flags, const K* d_lo, const K* d_hi, const V* d_values, K* d_out_keys,
             V* d_out_values, I* d_out_index, uint64_t* d_out_num, uint32_t flags = 0, bool descending = false,
             const uint64_t* d_num = nullptr, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 4- or 8-byte integers");
    static_assert(std::is_trivially_copyable<V>::value, "values are moved bitwise");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("compact: the key type must be its own key");
    ctx.check(rsx_compact_device(ctx.get(), d_keys, n, d_num, L.key_bytes, L.key_kind, descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING,
                                 d_flags, d_lo, d_hi, d_values, d_out_values ? (uint32_t)sizeof(V) : 0u, flags, d_out_keys, d_out_values,
                                 d_out_index, (uint32_t)sizeof(I), d_out_num, stream),
              "rsx_compact_device");
}

// Rows regrouped by bin (rsx_multisplit_device): the first n -- or min(n, *d_num) -- rows moved into the bin of their key,
// in input order inside each bin; mode and the m edges as in bin_count (RSX_BIN_INDEX: d_edges nullptr, the last bin holds
// the ids outside 0 .. m - 1).  Keys, values and input positions go to the outputs that are not nullptr; d_out_offsets
// receives the m + 2 offsets of the bins, offsets[m + 1] the number of rows.  At most multisplit_caps<K>().max_edges
// edges (index mode: max_index_bins).  Not in place.  Stream-ordered, never synchronised; Context::reserve is not enough
// for a capture: rsx_ctx_reserve_multisplit.
struct MultisplitCaps {
    uint32_t max_edges, max_index_bins, tile, share;
};
template <typename K>
MultisplitCaps multisplit_caps() {
    MultisplitCaps c{};
    const rsx_layout L = RadixDigits<K>::layout();
    if (rsx_multisplit_caps(L.key_bytes, &c.max_edges, &c.max_index_bins, &c.tile, &c.share) != RSX_OK)
        throw std::invalid_argument("multisplit_caps: no partition for this key width");
    return c;
}
template <typename K, typename V = uint32_t, typename I = uint64_t>
void multisplit(const K* d_keys, size_t n, const K* d_edges, uint32_t m, uint32_t mode, const V* d_values, K* d_out_keys, V* d_out_values,
                I* d_out_index, uint64_t* d_out_offsets, bool descending = false, const uint64_t* d_num = nullptr, void* stream = nullptr,
                Context& ctx = default_context()) {
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 4- or 8-byte integers");
    static_assert(std::is_trivially_copyable<V>::value, "values are moved bitwise");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("multisplit: the key type must be its own key");
    ctx.check(rsx_multisplit_device(ctx.get(), d_keys, n, d_num, L.key_bytes, L.key_kind, d_edges, m, mode,
                                    descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, d_out_values ? d_values : nullptr,
                                    d_out_values ? (uint32_t)sizeof(V) : 0u, d_out_keys, d_out_values, d_out_index, (uint32_t)sizeof(I), d_out_offsets, stream),
              "rsx_multisplit_device");
}

// A value column combined per bin, nothing sorted (rsx_bin_reduce_device): d_out_values[b], b = 0 .. m, the sum
// (RSX_REDUCE_SUM), minimum or maximum of the values of the first n -- or min(n, *d_num) -- rows whose key's bin is b; mode
// and the m edges as in bin_count (RSX_BIN_INDEX: d_edges nullptr, the last bin holds the ids outside 0 .. m - 1); V and the
// operators as in reduce_by_key.  An empty bin holds the operator's identity (0 / +0.0; the highest / lowest value of the
// order).  d_out_counts (may be nullptr) receives the bins' sizes, what bin_count writes.  accumulate: combined onto /
// added to what the outputs hold.  No atomics on floats: the same input gives the same bits on every call.  At most
// bin_reduce_caps<K, V>().max_edges edges (index mode: max_index_bins).  Stream-ordered, never synchronised;
// Context::reserve is not enough for a capture: rsx_ctx_reserve_bin_reduce.
struct BinReduceCaps {
    uint32_t max_edges, max_index_bins, tile, share;
};
template <typename K, typename V>
BinReduceCaps bin_reduce_caps() {
    BinReduceCaps c{};
    const rsx_layout L = RadixDigits<K>::layout();
    if (rsx_bin_reduce_caps(L.key_bytes, (uint32_t)sizeof(V), &c.max_edges, &c.max_index_bins, &c.tile, &c.share) != RSX_OK)
        throw std::invalid_argument("bin_reduce_caps: no per-bin reduction for these key and value widths");
    return c;
}
template <typename K, typename V, typename C = uint64_t>
void bin_reduce(const K* d_keys, const V* d_values, size_t n, const K* d_edges, uint32_t m, uint32_t mode, int op, V* d_out_values,
                C* d_out_counts = nullptr, bool descending = false, bool accumulate = false, const uint64_t* d_num = nullptr,
                void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_arithmetic<V>::value && !std::is_same<V, bool>::value && (sizeof(V) == 4 || sizeof(V) == 8),
                  "values are 4- or 8-byte integers or floats");
    static_assert(std::is_integral<C>::value && (sizeof(C) == 4 || sizeof(C) == 8), "counts are 4- or 8-byte integers");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("bin_reduce: the key type must be its own key");
    const uint32_t vkind = std::is_floating_point<V>::value ? RSX_KEY_FLOAT : std::is_signed<V>::value ? RSX_KEY_SIGNED : RSX_KEY_UNSIGNED;
    ctx.check(rsx_bin_reduce_device(ctx.get(), d_keys, d_values, n, d_num, L.key_bytes, L.key_kind, d_edges, m, mode,
                                    descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, (uint32_t)sizeof(V), vkind, op, d_out_values,
                                    d_out_counts, (uint32_t)sizeof(C), accumulate ? RSX_BIN_ACCUMULATE : 0u, stream),
              "rsx_bin_reduce_device");
}

// Several key columns (rsx_lexsort_device, rsx_sort_columns_device): rows sorted by (column 0, column 1, ...), column 0
// the MOST significant, every column with its own type and direction; rows equal in every column keep their input order.
// key_column describes one column of n keys on the device; at most RSX_LEX_MAX_COLUMNS of them.
template <typename K>
rsx_key_column key_column(const K* d_keys, bool descending = false) {
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("key_column: the key type must be its own key");
    return rsx_key_column{d_keys, L.key_bytes, L.key_kind, descending ? 1u : 0u, 0u};
}
// d_index[t] = the row that stands at place t (I: 4 or 8 bytes); the columns are only read.
template <typename I>
void lexsort(const std::vector<rsx_key_column>& columns, I* d_index, size_t n, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 32- or 64-bit integers");
    ctx.check(rsx_lexsort_device(ctx.get(), columns.data(), (uint32_t)columns.size(), d_index, n, (uint32_t)sizeof(I), stream), "rsx_lexsort_device");
}
// That permutation applied in place to every column -- THE COLUMNS ARE WRITTEN -- and to the n values (nullptr: the
// columns alone).  Stream-ordered, never synchronised (rsx_ctx_reserve_lex before a stream capture).
template <typename V>
void sort_columns(const std::vector<rsx_key_column>& columns, V* d_values, size_t n, void* stream = nullptr, Context& ctx = default_context()) {
    static_assert(std::is_trivially_copyable<V>::value, "values are moved bitwise");
    ctx.check(rsx_sort_columns_device(ctx.get(), columns.data(), (uint32_t)columns.size(), d_values, d_values ? (uint32_t)sizeof(V) : 0u, n, stream),
              "rsx_sort_columns_device");
}
inline void sort_columns(const std::vector<rsx_key_column>& columns, size_t n, void* stream = nullptr, Context& ctx = default_context()) {
    ctx.check(rsx_sort_columns_device(ctx.get(), columns.data(), (uint32_t)columns.size(), nullptr, 0u, n, stream), "rsx_sort_columns_device");
}

// The segmented forms of the three calls above (rsx_sort_segments_pairs_device, rsx_argsort_segments_device and their
// row forms): every segment [d_offsets[i], d_offsets[i+1]) -- nseg + 1 offsets ON THE DEVICE -- or every row of row_len
// keys gets the stable permutation by key on its own; d_values == nullptr sorts the keys alone.  Values of 1, 2, 4, 8 or
// 16 bytes are sorted with their keys inside LDS, one workgroup per segment; the indices of the argsort forms are
// positions INSIDE the segment (torch.sort(dim=-1).indices).  Stream-ordered; bad offsets surface at
// synchronize_and_check.  Segments above rsx_segment_pairs_caps use the context's workspace (rsx_ctx_reserve_pairs).
template <typename K, typename V>
void radix_sort_segments_pairs(K* d_keys, V* d_values, size_t n, const uint64_t* d_offsets, size_t nseg, bool descending = false,
                               void* stream = nullptr, uint64_t max_seg_len = 0, Context& ctx = default_context()) {
    static_assert(std::is_trivially_copyable<V>::value, "values are moved bitwise");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("radix_sort_segments_pairs: the key type must be its own key");
    ctx.check(rsx_sort_segments_pairs_device(ctx.get(), d_keys, d_values, n, L.key_bytes, L.key_kind, d_values ? (uint32_t)sizeof(V) : 0u,
                                             descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, d_offsets, nseg, max_seg_len, stream),
              "rsx_sort_segments_pairs_device");
}
template <typename K, typename I>
void radix_argsort_segments(const K* d_keys, I* d_index, size_t n, const uint64_t* d_offsets, size_t nseg, bool descending = false,
                            void* stream = nullptr, uint64_t max_seg_len = 0, Context& ctx = default_context()) {
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 4- or 8-byte integers");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("radix_argsort_segments: the key type must be its own key");
    ctx.check(rsx_argsort_segments_device(ctx.get(), d_keys, d_index, n, L.key_bytes, L.key_kind, (uint32_t)sizeof(I),
                                          descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, d_offsets, nseg, max_seg_len, stream),
              "rsx_argsort_segments_device");
}
template <typename K, typename V>
void radix_sort_rows_pairs(K* d_keys, V* d_values, size_t rows, size_t row_len, bool descending = false, void* stream = nullptr,
                           Context& ctx = default_context()) {
    static_assert(std::is_trivially_copyable<V>::value, "values are moved bitwise");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("radix_sort_rows_pairs: the key type must be its own key");
    ctx.check(rsx_sort_rows_pairs_device(ctx.get(), d_keys, d_values, rows, row_len, L.key_bytes, L.key_kind, d_values ? (uint32_t)sizeof(V) : 0u,
                                         descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, stream), "rsx_sort_rows_pairs_device");
}
template <typename K, typename I>
void radix_argsort_rows(const K* d_keys, I* d_index, size_t rows, size_t row_len, bool descending = false, void* stream = nullptr,
                        Context& ctx = default_context()) {
    static_assert(std::is_integral<I>::value && (sizeof(I) == 4 || sizeof(I) == 8), "indices are 4- or 8-byte integers");
    const rsx_layout L = RadixDigits<K>::layout();
    if (L.key_offset != 0 || L.key_bytes != L.elem_bytes) throw std::invalid_argument("radix_argsort_rows: the key type must be its own key");
    ctx.check(rsx_argsort_rows_device(ctx.get(), d_keys, d_index, rows, row_len, L.key_bytes, L.key_kind, (uint32_t)sizeof(I),
                                      descending ? RSX_ORDER_DESCENDING : RSX_ORDER_ASCENDING, stream), "rsx_argsort_rows_device");
}

// Multi-GPU, one process: slice g lives on the device of ctxs[g]; the concatenation of the slices
// is sorted as one array (slice = the reference's "chunk", mod.rs:66-70).  Blocking.
template <typename T>
void radix_sort_sharded(const std::vector<Context*>& ctxs, const std::vector<T*>& d_slices,
                        const std::vector<T*>& d_tmps, const std::vector<size_t>& n_per_dev) {
    if (ctxs.empty() || ctxs.size() != d_slices.size() || ctxs.size() != d_tmps.size() || ctxs.size() != n_per_dev.size())
        throw std::invalid_argument("radix_sort_sharded: one context, slice, tmp and length per device");
    const rsx_layout L = RadixDigits<T>::layout();
    std::vector<rsx_ctx*> h;
    std::vector<void*> s, t;
    for (size_t g = 0; g < ctxs.size(); ++g) {
        h.push_back(ctxs[g]->get());
        s.push_back(d_slices[g]);
        t.push_back(d_tmps[g]);
    }
    ctxs[0]->check(rsx_sort_sharded(h.data(), (uint32_t)h.size(), s.data(), t.data(), n_per_dev.data(), &L),
                   "rsx_sort_sharded");
}

}  // namespace rsx
