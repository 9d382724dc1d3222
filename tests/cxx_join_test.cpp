// Compile-only check of rsx::join and rsx::join_count (radix_sort_amd/cxx/radix_sort.hpp): the wrappers instantiate for
// uint32_t keys with both index widths (with and without device counts and index arrays), for double keys, and for the
// semi join without a right-hand output.  tests/test_cxx_join.py compiles this file; nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

void instantiate(const uint32_t* ak, const uint32_t* bk, const double* ad, const double* bd, uint32_t* l32, uint32_t* r32, int64_t* l64, int64_t* r64,
                 const uint32_t* pa32, const uint32_t* pb32, const int64_t* pa64, const int64_t* pb64, uint64_t* num, const uint64_t* an,
                 const uint64_t* bn, void* stream, rsx::Context& ctx) {
    rsx::join(RSX_JOIN_INNER, ak, 100, bk, 10, l32, r32, 1000, num);
    rsx::join(RSX_JOIN_LEFT, ak, 100, bk, 10, l64, r64, 1000, num, true, an, bn, pa64, pb64, stream, ctx);
    rsx::join(RSX_JOIN_INNER, ak, 100, bk, 10, l32, r32, 50, num, false, an, bn, pa32, pb32);
    rsx::join(RSX_JOIN_SEMI, ad, 100, bd, 10, l64, static_cast<int64_t*>(nullptr), 100, num);
    rsx::join(RSX_JOIN_ANTI, ad, 100, bd, 10, l32, static_cast<uint32_t*>(nullptr), 100, num, true, an, bn, pa32);
    rsx::join_count(RSX_JOIN_INNER, ak, 100, bk, 10, num);
    rsx::join_count(RSX_JOIN_LEFT, ad, 100, bd, 10, num, true, an, bn, stream, ctx);
}
