// Compile-only check of rsx::unique (radix_sort_amd/cxx/radix_sort.hpp): the wrapper instantiates for an integer and a
// float key type and both index widths.  tests/test_cxx_unique.py compiles this file; nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

void instantiate(const uint32_t* k32, const double* k64, uint32_t* o32, double* o64, uint64_t* offsets, uint32_t* i32, int64_t* i64,
                 uint64_t* num, void* stream, rsx::Context& ctx) {
    rsx::unique(k32, 100, o32, offsets, i32, i32, num, false, stream, ctx);
    rsx::unique(k64, 100, o64, offsets, i64, static_cast<int64_t*>(nullptr), num, true, stream, ctx);
    rsx::unique_keys(k64, 100, o64, offsets, num);
}
