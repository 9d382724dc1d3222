// Compile-only check of rsx::compact and rsx::compact_caps (radix_sort_amd/cxx/radix_sort.hpp): the wrappers instantiate for
// uint32_t, int64_t, float and double keys, with and without values, with both index widths, as a pure mask call and as a
// partition.  tests/test_cxx_compact.py compiles this file; nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

struct Wide {
    uint32_t w[3];
};

void instantiate(const uint32_t* u, const int64_t* s, const float* f, const double* d, const uint8_t* mask, uint32_t* ou, int64_t* os, float* of,
                 double* od, const Wide* wide, Wide* owide, uint32_t* i32, uint64_t* i64, uint64_t* m, const uint64_t* num, void* stream,
                 rsx::Context& ctx) {
    rsx::compact<uint32_t, uint32_t, uint64_t>(u, 100, mask, nullptr, nullptr, nullptr, ou, nullptr, nullptr, m);
    rsx::compact(u, 100, mask, u + 1, u + 2, u, ou, ou + 100, i64, m, RSX_COMPACT_PARTITION, true, num, stream, ctx);
    rsx::compact<int64_t, double, uint32_t>(s, 100, nullptr, s, nullptr, d, os, od, i32, m, RSX_COMPACT_INVERT);
    rsx::compact<float, Wide, uint64_t>(f, 100, nullptr, nullptr, f, wide, of, owide, nullptr, m, 0u, false, num);
    rsx::compact<double, uint32_t, uint64_t>(d, 100, mask, d, d + 1, nullptr, od, nullptr, i64, m);
    rsx::compact<uint8_t, uint32_t, uint32_t>(nullptr, 100, mask, nullptr, nullptr, nullptr, nullptr, nullptr, i32, m);  // nonzero
    const rsx::CompactCaps c = rsx::compact_caps<uint32_t>();
    (void)(c.tile + c.scan_span);
    (void)rsx::compact_caps<int64_t, double, uint32_t>(true, true);
    (void)rsx::compact_caps<float, Wide>(true);
    (void)rsx::compact_caps<double>(false, true);
}
