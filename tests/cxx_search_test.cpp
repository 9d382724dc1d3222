// Compile-only check of rsx::search_sorted (radix_sort_amd/cxx/radix_sort.hpp): the wrapper instantiates for an integer
// and a float key type, both index widths, one output alone and the presort route.  tests/test_cxx_search.py compiles this
// file; nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

void instantiate(const uint32_t* s32, const uint32_t* n32, const double* s64, const double* n64, uint32_t* i32, int64_t* i64,
                 const uint64_t* num, void* stream, rsx::Context& ctx) {
    rsx::search_sorted(s32, 100, n32, 10, i32, i32, false, num, false, stream, ctx);
    rsx::search_sorted(s64, 100, n64, 10, i64, static_cast<int64_t*>(nullptr), true, nullptr, true, stream, ctx);
    rsx::search_sorted(s64, 100, n64, 10, static_cast<uint64_t*>(nullptr), reinterpret_cast<uint64_t*>(i64));
}
