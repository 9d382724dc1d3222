// Compile-only check of rsx::merge and rsx::merge_pairs (radix_sort_amd/cxx/radix_sort.hpp): the wrappers instantiate for
// uint32_t keys with uint64_t values (with and without the index output, both index widths) and for double keys alone.
// tests/test_cxx_merge.py compiles this file; nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

void instantiate(const uint32_t* ak, const uint64_t* av, const uint32_t* bk, const uint64_t* bv, uint32_t* ok, uint64_t* ov, uint32_t* i32,
                 int64_t* i64, const double* ad, const double* bd, double* od, void* stream, rsx::Context& ctx) {
    rsx::merge_pairs(ak, av, 100, bk, bv, 10, ok, ov);
    rsx::merge_pairs(ak, av, 100, bk, bv, 10, ok, ov, true, stream, ctx);
    rsx::merge_pairs(ak, av, 100, bk, bv, 10, ok, ov, i32, false, stream, ctx);
    rsx::merge_pairs(ak, av, 100, bk, bv, 10, static_cast<uint32_t*>(nullptr), ov, i64, true);
    rsx::merge(ad, 100, bd, 10, od);
    rsx::merge(ad, 100, bd, 10, od, true, stream, ctx);
}
