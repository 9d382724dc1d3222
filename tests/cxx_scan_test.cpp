// Compile-only check of rsx::scan_by_key (radix_sort_amd/cxx/radix_sort.hpp): the wrapper instantiates for integer and
// float keys, for signed, unsigned and float values of both widths, for the count form and with every default argument.
// tests/test_cxx_scan.py compiles this file; nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

#include <limits>

void instantiate(const uint32_t* k32, const double* k64, const float* vf, float* of, const int64_t* vi, int64_t* oi, const uint32_t* vu, uint32_t* ou,
                 const double* vd, double* od, uint64_t* num, void* stream, rsx::Context& ctx) {
    rsx::scan_by_key(k32, vf, 100, RSX_REDUCE_SUM, of);
    rsx::scan_by_key(k64, vi, 100, RSX_REDUCE_MIN, oi, true, std::numeric_limits<int64_t>::max(), false, num, stream, ctx);
    rsx::scan_by_key(k32, vu, 100, RSX_REDUCE_MAX, ou, true, uint32_t(0), true);
    rsx::scan_by_key(k64, vd, 100, RSX_REDUCE_SUM, od, false, 0.0, true, num);
    rsx::scan_by_key(k32, static_cast<const int64_t*>(nullptr), 100, RSX_REDUCE_SUM, oi, true, int64_t(0), false, num, stream, ctx);  // ranks
}
