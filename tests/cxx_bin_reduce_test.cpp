// Compile-only check of rsx::bin_reduce and rsx::bin_reduce_caps (radix_sort_amd/cxx/radix_sort.hpp): the wrappers
// instantiate for uint32_t, int64_t, float and double keys in the edge modes and for integer keys in the index mode, with
// every value type, with and without counts of both widths.  tests/test_cxx_bin_reduce.py compiles this file; nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

void instantiate(const uint32_t* u, const int64_t* s, const float* f, const double* d, const int32_t* i32, const uint64_t* u64, uint32_t* ou,
                 int64_t* os, float* of, double* od, int32_t* oi32, uint64_t* ou64, uint32_t* c32, uint64_t* c64, const uint64_t* num, void* stream,
                 rsx::Context& ctx) {
    rsx::bin_reduce(u, f, 100, u + 100, 7, RSX_BIN_UPPER, RSX_REDUCE_SUM, of);  // a weighted histogram
    rsx::bin_reduce(u, f, 100, u + 100, 7, RSX_BIN_LOWER, RSX_REDUCE_MAX, of, c32, true, true, num, stream, ctx);
    rsx::bin_reduce(s, d, 100, static_cast<const int64_t*>(nullptr), 64, RSX_BIN_INDEX, RSX_REDUCE_SUM, od, c64);  // per-expert score sums and load
    rsx::bin_reduce(f, i32, 100, f + 100, 3, RSX_BIN_UPPER, RSX_REDUCE_MIN, oi32, c64, false, false, num);
    rsx::bin_reduce(d, u64, 100, d + 100, 0, RSX_BIN_UPPER, RSX_REDUCE_SUM, ou64);
    rsx::bin_reduce(u, u, 100, static_cast<const uint32_t*>(nullptr), 8, RSX_BIN_INDEX, RSX_REDUCE_MAX, ou, c32, false, true);
    rsx::bin_reduce(s, s, 100, s + 100, 5, RSX_BIN_LOWER, RSX_REDUCE_MIN, os);
    const rsx::BinReduceCaps c = rsx::bin_reduce_caps<uint32_t, float>();
    (void)(c.max_edges + c.max_index_bins + c.tile + c.share);
    (void)rsx::bin_reduce_caps<int64_t, double>();
    (void)rsx::bin_reduce_caps<float, int32_t>();
    (void)rsx::bin_reduce_caps<double, uint64_t>();
}
