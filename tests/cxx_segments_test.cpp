// The C++ host mirror (radix_sort_amd/cxx/radix_sort.hpp) on the segmented sort: rsx::radix_sort_segments over ragged
// segments of std::pair<uint64_t, uint64_t> and rsx::radix_sort_rows over rows of float, each compared with
// std::stable_sort by mapped key per segment.  Run by tests/test_segments_host.py.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "../radix_sort_amd/cxx/radix_sort.hpp"

#define HIP_OK(call)                                                      \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) {                                           \
            std::printf("%s: %s\n", #call, hipGetErrorString(e_));        \
            return 2;                                                     \
        }                                                                 \
    } while (0)

static uint32_t float_key(float f) {  // radix_digits.rs:103-124
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}

int main() {
    int bad = 0;
    std::mt19937_64 rng(7);
    rsx::Context ctx;
    {
        using P = std::pair<uint64_t, uint64_t>;
        const size_t lens[] = {0, 1, 2, 63, 64, 65, 1000, 5000, 20000};
        std::vector<uint64_t> offs{3};  // three elements in front of the first segment
        for (int i = 0; i < 500; ++i) offs.push_back(offs.back() + lens[rng() % 9]);
        const size_t nseg = offs.size() - 1, n = offs.back() + 4;  // ... and four behind the last
        std::vector<P> v(n);
        for (size_t i = 0; i < n; ++i) v[i] = P(rng() % 300, i);  // many ties: stability shows
        std::vector<P> exp = v;
        for (size_t s = 0; s < nseg; ++s)
            std::stable_sort(exp.begin() + offs[s], exp.begin() + offs[s + 1], [](const P& a, const P& b) { return a.first < b.first; });
        P *d = nullptr, *t = nullptr;
        uint64_t* o = nullptr;
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&d), n * sizeof(P)));
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&t), n * sizeof(P)));
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&o), offs.size() * sizeof(uint64_t)));
        HIP_OK(hipMemcpy(d, v.data(), n * sizeof(P), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(o, offs.data(), offs.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        rsx::radix_sort_segments(d, t, n, o, nseg, nullptr, 0, ctx);
        ctx.synchronize_and_check();
        HIP_OK(hipMemcpy(v.data(), d, n * sizeof(P), hipMemcpyDeviceToHost));
        const bool ok = std::memcmp(v.data(), exp.data(), n * sizeof(P)) == 0;
        std::printf("segments of pair<u64,u64>: nseg=%zu n=%zu %s\n", nseg, n, ok ? "ok" : "MISMATCH");
        bad += !ok;
        HIP_OK(hipFree(d));
        HIP_OK(hipFree(t));
        HIP_OK(hipFree(o));
    }
    {
        const size_t rows = 777, len = 333, n = rows * len;
        std::vector<float> v(n);
        for (auto& x : v) {
            const uint32_t b = (uint32_t)rng();  // every bit pattern: NaNs, infinities, both zeros
            std::memcpy(&x, &b, 4);
        }
        std::vector<float> exp = v;
        for (size_t r = 0; r < rows; ++r)
            std::stable_sort(exp.begin() + r * len, exp.begin() + (r + 1) * len, [](float a, float b) { return float_key(a) < float_key(b); });
        float *d = nullptr, *t = nullptr;
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&d), n * sizeof(float)));
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&t), n * sizeof(float)));
        HIP_OK(hipMemcpy(d, v.data(), n * sizeof(float), hipMemcpyHostToDevice));
        rsx::radix_sort_rows(d, t, rows, len, nullptr, ctx);
        ctx.synchronize_and_check();
        HIP_OK(hipMemcpy(v.data(), d, n * sizeof(float), hipMemcpyDeviceToHost));
        const bool ok = std::memcmp(v.data(), exp.data(), n * sizeof(float)) == 0;
        std::printf("rows of float: %zu x %zu %s\n", rows, len, ok ? "ok" : "MISMATCH");
        bad += !ok;
        HIP_OK(hipFree(d));
        HIP_OK(hipFree(t));
    }
    if (!bad) std::printf("ALL OK\n");
    return bad ? 1 : 0;
}
