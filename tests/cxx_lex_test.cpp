// rsx::lexsort and rsx::sort_columns of the C++ host mirror (radix_sort_amd/cxx/radix_sort.hpp) on the GPU: three columns
// (int64, int64 descending, int32) of 20011 rows -- two rounds of the plan -- against std::stable_sort of the row numbers
// in this program.  tests/test_cxx_lex.py compiles it (CPU) and runs it (GPU); prints ALL OK and returns 0 on success.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <numeric>
#include <random>

#include "../radix_sort_amd/cxx/radix_sort.hpp"

#define HIP_OK(call)                                                                   \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            std::printf("%s: %s\n", #call, hipGetErrorString(e_));                     \
            return 2;                                                                  \
        }                                                                              \
    } while (0)

template <typename T>
static int upload(const std::vector<T>& h, T** d) {
    HIP_OK(hipMalloc(reinterpret_cast<void**>(d), h.size() * sizeof(T)));
    HIP_OK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
template <typename T>
static int download(std::vector<T>& h, const T* d) {
    HIP_OK(hipMemcpy(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

int main() {
    const size_t n = 20011;
    std::mt19937_64 rng(7);
    std::vector<int64_t> a(n), b(n);
    std::vector<int32_t> c(n);
    std::vector<uint16_t> v(n);
    for (size_t i = 0; i < n; ++i) {  // few values per column, both signs: rows tie in every column
        a[i] = (int64_t)((rng() % 5) * 0x4000000000000000ull);  // 0, 2^62, -2^63, -2^62, 0
        b[i] = (int64_t)(rng() % 7) - 3;
        c[i] = (rng() % 3 == 0) ? INT32_MIN : (int32_t)(rng() % 4) - 1;
        v[i] = (uint16_t)i;
    }
    std::vector<uint32_t> want(n);
    std::iota(want.begin(), want.end(), 0u);
    std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) {
        if (a[x] != a[y]) return a[x] < a[y];
        if (b[x] != b[y]) return b[x] > b[y];  // descending
        return c[x] < c[y];
    });

    int64_t *da = nullptr, *db = nullptr;
    int32_t* dc = nullptr;
    uint16_t* dv = nullptr;
    int32_t* di32 = nullptr;
    int64_t* di64 = nullptr;
    if (upload(a, &da) || upload(b, &db) || upload(c, &dc) || upload(v, &dv)) return 2;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&di32), n * sizeof(int32_t)));
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&di64), n * sizeof(int64_t)));
    int bad = 0;
    try {
        rsx::Context ctx;
        const std::vector<rsx_key_column> cols = {rsx::key_column(da), rsx::key_column(db, true), rsx::key_column(dc)};
        rsx::lexsort(cols, di32, n, nullptr, ctx);
        rsx::lexsort(cols, di64, n, nullptr, ctx);
        ctx.synchronize_and_check();
        uint64_t info = 0;
        ctx.check(rsx_ctx_get_info(ctx.get(), RSX_INFO_LAST_LEX, &info), "rsx_ctx_get_info");
        if (info != (2u | 16u << 8)) {
            std::printf("RSX_INFO_LAST_LEX = 0x%llx, expected two rounds and a 16-byte last element\n", (unsigned long long)info);
            ++bad;
        }
        std::vector<int32_t> p32(n);
        std::vector<int64_t> p64(n);
        if (download(p32, di32) || download(p64, di64)) return 2;
        for (size_t i = 0; i < n; ++i)
            if ((uint32_t)p32[i] != want[i] || (uint64_t)p64[i] != want[i]) {
                if (bad++ < 5) std::printf("lexsort: place %zu holds %d / %lld, expected %u\n", i, p32[i], (long long)p64[i], want[i]);
            }
        rsx::sort_columns(cols, dv, n, nullptr, ctx);
        ctx.synchronize_and_check();
        std::vector<int64_t> sa(n), sb(n);
        std::vector<int32_t> sc(n);
        std::vector<uint16_t> sv(n);
        if (download(sa, da) || download(sb, db) || download(sc, dc) || download(sv, dv)) return 2;
        for (size_t i = 0; i < n; ++i)
            if (sa[i] != a[want[i]] || sb[i] != b[want[i]] || sc[i] != c[want[i]] || sv[i] != v[want[i]]) {
                if (bad++ < 5) std::printf("sort_columns: row %zu differs\n", i);
            }
        rsx::sort_columns(cols, n, nullptr, ctx);  // sorted rows stay as they are
        ctx.synchronize_and_check();
        if (download(sa, da)) return 2;
        for (size_t i = 0; i < n; ++i)
            if (sa[i] != a[want[i]]) {
                if (bad++ < 5) std::printf("sort_columns without values: row %zu differs\n", i);
            }
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    (void)hipFree(da);
    (void)hipFree(db);
    (void)hipFree(dc);
    (void)hipFree(dv);
    (void)hipFree(di32);
    (void)hipFree(di64);
    if (bad) {
        std::printf("%d mismatches\n", bad);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
