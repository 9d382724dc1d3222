// Compile-only check of rsx::select and rsx::select_caps (radix_sort_amd/cxx/radix_sort.hpp): the wrappers instantiate for
// uint32_t, int64_t, float and double keys, with both index widths and with either output omitted.
// tests/test_cxx_select.py compiles this file; nothing runs it.
#include "../radix_sort_amd/cxx/radix_sort.hpp"

void instantiate(const uint32_t* u, const int64_t* s, const float* f, const double* d, uint32_t* ou, int64_t* os, float* of, double* od, uint32_t* i32,
                 uint64_t* u64, int64_t* i64, void* stream, rsx::Context& ctx) {
    const uint64_t ranks[3] = {0, 99, 50};
    rsx::select(u, 100, ranks, 3, ou, u64);
    rsx::select(u, 100, ranks, 3, ou, i32, true, stream, ctx);
    rsx::select(s, 100, ranks, 3, os, i64, false, stream);
    rsx::select(f, 100, ranks, 1, of, static_cast<uint64_t*>(nullptr));
    rsx::select(d, 100, ranks, 2, static_cast<double*>(nullptr), i32, true);
    const rsx::SelectCaps c = rsx::select_caps<uint32_t>();
    (void)(c.max_ranks + c.digit_bits + c.tile + c.cand_div + c.cand_floor);
    (void)rsx::select_caps<int64_t>();
    (void)rsx::select_caps<float>();
    (void)rsx::select_caps<double>();
}
