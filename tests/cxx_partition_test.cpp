// Compile-only check of rsx::multisplit and rsx::multisplit_caps (radix_sort_amd/cxx/radix_sort.hpp): the wrappers instantiate
// for uint32_t, int64_t, float and double keys, with and without values, with both index widths, in the edge modes and the
// index mode, with offsets alone.  tests/test_cxx_partition.py compiles this file; nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

struct Wide {
    uint32_t w[3];
};

void instantiate(const uint32_t* u, const int64_t* s, const float* f, const double* d, uint32_t* ou, int64_t* os, float* of, double* od,
                 const Wide* wide, Wide* owide, uint32_t* i32, uint64_t* i64, uint64_t* offsets, const uint64_t* num, void* stream,
                 rsx::Context& ctx) {
    rsx::multisplit<uint32_t, uint32_t, uint64_t>(u, 100, u + 100, 7, RSX_BIN_UPPER, nullptr, ou, nullptr, nullptr, offsets);
    rsx::multisplit(u, 100, u + 100, 7, RSX_BIN_LOWER, u, ou, ou + 100, i64, offsets, true, num, stream, ctx);
    rsx::multisplit<int64_t, double, uint32_t>(s, 100, nullptr, 64, RSX_BIN_INDEX, d, os, od, i32, offsets);  // expert dispatch
    rsx::multisplit<float, Wide, uint64_t>(f, 100, f + 100, 3, RSX_BIN_UPPER, wide, of, owide, nullptr, offsets, false, num);
    rsx::multisplit<double, uint32_t, uint64_t>(d, 100, d + 100, 0, RSX_BIN_UPPER, nullptr, nullptr, nullptr, i64, offsets);
    rsx::multisplit<uint32_t, uint32_t, uint32_t>(u, 100, nullptr, 8, RSX_BIN_INDEX, nullptr, nullptr, nullptr, nullptr, offsets);  // offsets only
    const rsx::MultisplitCaps c = rsx::multisplit_caps<uint32_t>();
    (void)(c.max_edges + c.max_index_bins + c.tile + c.share);
    (void)rsx::multisplit_caps<int64_t>();
    (void)rsx::multisplit_caps<float>();
    (void)rsx::multisplit_caps<double>();
}
