// Compile-only check of rsx::reduce_by_key (radix_sort_amd/cxx/radix_sort.hpp): the wrapper instantiates for integer and
// float keys and for signed, unsigned and float values of both widths.  tests/test_cxx_reduce.py compiles this file;
// nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

void instantiate(const uint32_t* k32, const double* k64, uint32_t* o32, double* o64, const float* vf, float* of, const int64_t* vi, int64_t* oi,
                 const uint32_t* vu, uint32_t* ou, const double* vd, double* od, uint64_t* offsets, uint64_t* num, void* stream,
                 rsx::Context& ctx) {
    rsx::reduce_by_key(k32, vf, 100, RSX_REDUCE_SUM, o32, of, offsets, num, false, stream, ctx);
    rsx::reduce_by_key(k64, vi, 100, RSX_REDUCE_MIN, o64, oi, static_cast<uint64_t*>(nullptr), num, true, stream, ctx);
    rsx::reduce_by_key(k32, vu, 100, RSX_REDUCE_MAX, static_cast<uint32_t*>(nullptr), ou, offsets, num);
    rsx::reduce_by_key(k64, vd, 100, RSX_REDUCE_SUM, o64, od, offsets, num);
}
