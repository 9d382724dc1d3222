// Compile-only check of rsx::bin_count and rsx::bin_caps (radix_sort_amd/cxx/radix_sort.hpp): the wrappers instantiate for
// uint32_t, int64_t, float and double keys in the edge modes and for integer keys in the index mode, with both count
// widths.  tests/test_cxx_bin.py compiles this file; nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

void instantiate(const uint32_t* u, const int64_t* s, const float* f, const double* d, uint32_t* c32, uint64_t* c64, int64_t* i64,
                 const uint64_t* num, void* stream, rsx::Context& ctx) {
    rsx::bin_count(u, 100, u, 7, RSX_BIN_UPPER, c64);
    rsx::bin_count(u, 100, u, 7, RSX_BIN_LOWER, c32, true, true, num, stream, ctx);
    rsx::bin_count(s, 100, s, 0, RSX_BIN_UPPER, i64, false, false, num, stream);
    rsx::bin_count(f, 100, f, 64, RSX_BIN_UPPER, c64, true);
    rsx::bin_count(d, 100, d, 3, RSX_BIN_LOWER, c32);
    rsx::bin_count(u, 100, static_cast<const uint32_t*>(nullptr), 4096, RSX_BIN_INDEX, c64);
    rsx::bin_count(s, 100, static_cast<const int64_t*>(nullptr), 1u << 20, RSX_BIN_INDEX, c32, false, true);
    const rsx::BinCaps c = rsx::bin_caps<uint32_t>();
    (void)(c.max_edges + c.max_index_bins_lds + c.share);
    (void)rsx::bin_caps<int64_t>();
    (void)rsx::bin_caps<float>();
    (void)rsx::bin_caps<double>();
}
