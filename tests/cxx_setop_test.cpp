// Compile-only check of rsx::set_op and rsx::set_op_pairs (radix_sort_amd/cxx/radix_sort.hpp): the wrappers instantiate for
// uint32_t keys with uint64_t values (with and without device counts, and without b's values) and for double keys alone
// (with and without the index output, both index widths).  tests/test_cxx_setop.py compiles this file; nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

void instantiate(const uint32_t* ak, const uint64_t* av, const uint32_t* bk, const uint64_t* bv, uint32_t* ok, uint64_t* ov, uint32_t* i32,
                 int64_t* i64, const double* ad, const double* bd, double* od, uint64_t* num, const uint64_t* an, const uint64_t* bn,
                 void* stream, rsx::Context& ctx) {
    rsx::set_op_pairs(RSX_SETOP_UNION, ak, av, 100, bk, bv, 10, ok, ov, num);
    rsx::set_op_pairs(RSX_SETOP_SYMMETRIC_DIFFERENCE, ak, av, 100, bk, bv, 10, ok, ov, num, true, an, bn, stream, ctx);
    rsx::set_op_pairs(RSX_SETOP_INTERSECTION, ak, av, 100, bk, static_cast<const uint64_t*>(nullptr), 10, ok, ov, num, false, an);
    rsx::set_op(RSX_SETOP_DIFFERENCE, ad, 100, bd, 10, od, num);
    rsx::set_op(RSX_SETOP_UNION, ad, 100, bd, 10, od, num, true, an, bn, stream, ctx);
    rsx::set_op(RSX_SETOP_INTERSECTION, ad, 100, bd, 10, od, num, i32);
    rsx::set_op(RSX_SETOP_INTERSECTION, ad, 100, bd, 10, static_cast<double*>(nullptr), num, i64, true, an, bn, stream, ctx);
    rsx::set_op(RSX_SETOP_UNION, ak, 100, bk, 10, ok, num, i64, false);
}
