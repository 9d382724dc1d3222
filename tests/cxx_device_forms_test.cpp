// The device-resident templates of the C++ host mirror (radix_sort_amd/cxx/radix_sort.hpp) on the GPU: radix_sort_device,
// radix_sort_pairs, radix_sort_keys, radix_argsort, the four segment / row forms with values and indices, and
// radix_sort_sharded -- each instantiated, run, and compared with std::stable_sort in this program.  Keys come from few
// values, so stability decides; floats include +-0.0, +-inf and both NaNs and order by their mapped bit pattern.
// tests/test_cxx_device_forms.py compiles it (CPU) and runs it (GPU); prints ALL OK and returns 0 on success.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>

#include "../radix_sort_amd/cxx/radix_sort.hpp"

static void hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

static std::vector<void*> g_allocs;

template <typename T>
static T* device_array(size_t n) {
    void* p = nullptr;
    hip_ok(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)), "hipMalloc");
    g_allocs.push_back(p);
    return static_cast<T*>(p);
}
template <typename T>
static T* upload(const std::vector<T>& h) {
    T* d = device_array<T>(h.size());
    if (!h.empty()) hip_ok(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy to the device");
    return d;
}
template <typename T>
static std::vector<T> download(const T* d, size_t n) {
    std::vector<T> h(n);
    if (n) hip_ok(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy to the host");
    return h;
}

// the order-preserving unsigned form of a key (radix_digits.rs): the sort order of every call
static uint32_t mapped(float x) {
    uint32_t b;
    std::memcpy(&b, &x, sizeof b);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static uint64_t mapped(double x) {
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    return (b >> 63) ? ~b : (b | (uint64_t(1) << 63));
}
static uint32_t mapped(int32_t x) { return (uint32_t)x ^ 0x80000000u; }
static uint64_t mapped(int64_t x) { return (uint64_t)x ^ (uint64_t(1) << 63); }
static uint32_t mapped(uint32_t x) { return x; }
static uint64_t mapped(uint64_t x) { return x; }

// positions begin .. end-1 in the order the stable sort by mapped key leaves them (descending: larger key first, equal
// keys still in input order)
template <typename K>
static std::vector<uint32_t> stable_perm(const std::vector<K>& keys, size_t begin, size_t end, bool descending) {
    std::vector<uint32_t> p(end - begin);
    std::iota(p.begin(), p.end(), (uint32_t)begin);
    std::stable_sort(p.begin(), p.end(), [&](uint32_t a, uint32_t b) {
        return descending ? mapped(keys[a]) > mapped(keys[b]) : mapped(keys[a]) < mapped(keys[b]);
    });
    return p;
}

template <typename T>
static bool same_bits(const T& a, const T& b) {
    return std::memcmp(&a, &b, sizeof(T)) == 0;
}

static int g_bad = 0;
static void report(const char* what, size_t mismatches) {
    std::printf("%-44s %s\n", what, mismatches ? "MISMATCH" : "ok");
    if (mismatches) {
        std::printf("    %zu places differ\n", mismatches);
        ++g_bad;
    }
}
// got[i] must be src[perm[i]], bit for bit
template <typename T>
static size_t gathered_mismatches(const std::vector<T>& got, const std::vector<T>& src, const std::vector<uint32_t>& perm, size_t at = 0) {
    size_t bad = 0;
    for (size_t i = 0; i < perm.size(); ++i) bad += !same_bits(got[at + i], src[perm[i]]);
    return bad;
}

template <typename T>
static size_t changed(const std::vector<T>& got, const std::vector<T>& src) {
    size_t bad = 0;
    for (size_t i = 0; i < src.size(); ++i) bad += !same_bits(got[i], src[i]);
    return bad;
}

struct Rec12 {  // a 12-byte value, moved bitwise
    uint32_t a, b, c;
};
static_assert(sizeof(Rec12) == 12, "Rec12 is 12 bytes");

static std::vector<float> float_keys(size_t n, std::mt19937_64& rng) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float vals[] = {0.0f, -0.0f, inf, -inf, nan, -nan, 1.5f, -1.5f, 3.0f, -2.25f, 1e-40f, -1e-40f};
    std::vector<float> k(n);
    for (auto& x : k) x = vals[rng() % (sizeof vals / sizeof vals[0])];
    return k;
}
static std::vector<double> double_keys(size_t n, std::mt19937_64& rng) {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double vals[] = {0.0, -0.0, inf, -inf, nan, -nan, 1.5, -1.5, 3.0, -2.25, 1e-310, -1e-310, 7e300};
    std::vector<double> k(n);
    for (auto& x : k) x = vals[rng() % (sizeof vals / sizeof vals[0])];
    return k;
}
static std::vector<int32_t> int32_keys(size_t n, std::mt19937_64& rng) {
    std::vector<int32_t> k(n);
    for (auto& x : k) x = (rng() % 9 == 0) ? std::numeric_limits<int32_t>::min() : (int32_t)(rng() % 11) * 0x0C000000 - 0x30000000;
    return k;
}

static void flat_forms(rsx::Context& ctx) {
    const size_t n = 200003;
    std::mt19937_64 rng(11);
    {  // radix_sort_device<uint64_t>: 97 values, one in every byte of the key
        std::vector<uint64_t> h(n);
        for (auto& x : h) x = (rng() % 97) * 0x0102040810204081ull;
        uint64_t *d = upload(h), *tmp = device_array<uint64_t>(n);
        rsx::radix_sort_device(d, tmp, n, nullptr, ctx);
        ctx.synchronize_and_check();
        report("radix_sort_device<uint64_t>", gathered_mismatches(download(d, n), h, stable_perm(h, 0, n, false)));
    }
    {  // radix_sort_device<std::pair<uint32_t, uint32_t>>: the key is .first, .second is the position
        typedef std::pair<uint32_t, uint32_t> P;
        std::vector<P> h(n);
        std::vector<uint32_t> keys(n);
        for (size_t i = 0; i < n; ++i) h[i] = P(keys[i] = (uint32_t)(rng() % 61) << 26 | (uint32_t)(rng() % 3), (uint32_t)i);
        P *d = upload(h), *tmp = device_array<P>(n);
        rsx::radix_sort_device(d, tmp, n, nullptr, ctx);
        ctx.synchronize_and_check();
        report("radix_sort_device<pair<u32,u32>>", gathered_mismatches(download(d, n), h, stable_perm(keys, 0, n, false)));
    }
    {  // radix_sort_pairs<float, uint64_t>, ascending
        std::vector<float> k = float_keys(n, rng);
        std::vector<uint64_t> v(n);
        for (size_t i = 0; i < n; ++i) v[i] = (uint64_t)i << 20 | 0xABCDE;
        float* dk = upload(k);
        uint64_t* dv = upload(v);
        rsx::radix_sort_pairs(dk, dv, n, false, nullptr, ctx);
        ctx.synchronize_and_check();
        const std::vector<uint32_t> p = stable_perm(k, 0, n, false);
        report("radix_sort_pairs<float, uint64_t>", gathered_mismatches(download(dk, n), k, p) + gathered_mismatches(download(dv, n), v, p));
    }
    {  // radix_sort_pairs<int64_t, 12-byte struct>, descending
        std::vector<int64_t> k(n);
        for (auto& x : k) x = (int64_t)((rng() % 7) * 0x2000000000000001ull - 0x6000000000000000ull + (rng() % 2));
        std::vector<Rec12> v(n);
        for (size_t i = 0; i < n; ++i) v[i] = Rec12{(uint32_t)i, ~(uint32_t)i, (uint32_t)i * 2654435761u};
        int64_t* dk = upload(k);
        Rec12* dv = upload(v);
        rsx::radix_sort_pairs(dk, dv, n, true, nullptr, ctx);
        ctx.synchronize_and_check();
        const std::vector<uint32_t> p = stable_perm(k, 0, n, true);
        report("radix_sort_pairs<int64_t, Rec12> descending", gathered_mismatches(download(dk, n), k, p) + gathered_mismatches(download(dv, n), v, p));
    }
    {  // radix_sort_keys<double>, both orders
        const std::vector<double> k = double_keys(n, rng);
        for (int desc = 0; desc < 2; ++desc) {
            double* dk = upload(k);
            rsx::radix_sort_keys(dk, n, desc != 0, nullptr, ctx);
            ctx.synchronize_and_check();
            report(desc ? "radix_sort_keys<double> descending" : "radix_sort_keys<double>",
                   gathered_mismatches(download(dk, n), k, stable_perm(k, 0, n, desc != 0)));
        }
    }
    {  // radix_argsort<int32_t, uint32_t> and <uint64_t, int64_t>: the keys are only read
        const std::vector<int32_t> k = int32_keys(n, rng);
        int32_t* dk = upload(k);
        uint32_t* di = device_array<uint32_t>(n);
        rsx::radix_argsort(dk, di, n, false, nullptr, ctx);
        ctx.synchronize_and_check();
        const std::vector<uint32_t> p = stable_perm(k, 0, n, false), got = download(di, n);
        size_t bad = changed(download(dk, n), k);
        for (size_t i = 0; i < n; ++i) bad += got[i] != p[i];
        report("radix_argsort<int32_t, uint32_t>", bad);
    }
    {
        std::vector<uint64_t> k(n);
        for (auto& x : k) x = (rng() % 5) << 62 | (rng() % 13);
        uint64_t* dk = upload(k);
        int64_t* di = device_array<int64_t>(n);
        rsx::radix_argsort(dk, di, n, true, nullptr, ctx);
        ctx.synchronize_and_check();
        const std::vector<uint32_t> p = stable_perm(k, 0, n, true);
        const std::vector<int64_t> got = download(di, n);
        size_t bad = 0;
        for (size_t i = 0; i < n; ++i) bad += got[i] != (int64_t)p[i];
        report("radix_argsort<uint64_t, int64_t> descending", bad);
    }
    {  // a key type that is not its own key
        bool thrown = false;
        try {
            rsx::radix_sort_pairs<std::pair<uint32_t, uint32_t>, uint32_t>(nullptr, nullptr, 0, false, nullptr, ctx);
        } catch (const std::invalid_argument&) {
            thrown = true;
        }
        report("radix_sort_pairs<pair, ...> throws", thrown ? 0 : 1);
    }
}

// the four segmented forms over `offsets` (nseg + 1, in elements, inside an array of n): i32 keys with u32 values
// ascending, f32 keys with int64_t indices descending; rows == 0: ragged segments, else rows of row_len
static void segment_forms(rsx::Context& ctx, const std::vector<uint64_t>& offsets, size_t n, size_t rows, size_t row_len) {
    std::mt19937_64 rng(23 + rows);
    const size_t nseg = offsets.size() - 1;
    uint64_t* d_off = upload(offsets);
    char label[96];
    {
        const std::vector<int32_t> k = int32_keys(n, rng);
        std::vector<uint32_t> v(n);
        for (size_t i = 0; i < n; ++i) v[i] = (uint32_t)i ^ 0x55AA0000u;
        int32_t* dk = upload(k);
        uint32_t* dv = upload(v);
        if (rows) rsx::radix_sort_rows_pairs(dk, dv, rows, row_len, false, nullptr, ctx);
        else rsx::radix_sort_segments_pairs(dk, dv, n, d_off, nseg, false, nullptr, 0, ctx);
        ctx.synchronize_and_check();
        const std::vector<int32_t> gk = download(dk, n);
        const std::vector<uint32_t> gv = download(dv, n);
        size_t bad = 0;
        for (size_t i = 0; i < offsets[0]; ++i) bad += gk[i] != k[i] || gv[i] != v[i];  // outside the segments: untouched
        for (size_t i = offsets[nseg]; i < n; ++i) bad += gk[i] != k[i] || gv[i] != v[i];
        for (size_t s = 0; s < nseg; ++s) {
            const std::vector<uint32_t> p = stable_perm(k, offsets[s], offsets[s + 1], false);
            bad += gathered_mismatches(gk, k, p, offsets[s]) + gathered_mismatches(gv, v, p, offsets[s]);
        }
        std::snprintf(label, sizeof label, "%s<int32_t, uint32_t>", rows ? "radix_sort_rows_pairs" : "radix_sort_segments_pairs");
        report(label, bad);
    }
    {
        const std::vector<float> k = float_keys(n, rng);
        const std::vector<int64_t> fill(n, -7);
        float* dk = upload(k);
        int64_t* di = upload(fill);
        if (rows) rsx::radix_argsort_rows(dk, di, rows, row_len, true, nullptr, ctx);
        else rsx::radix_argsort_segments(dk, di, n, d_off, nseg, true, nullptr, 0, ctx);
        ctx.synchronize_and_check();
        const std::vector<int64_t> gi = download(di, n);
        size_t bad = changed(download(dk, n), k);
        for (size_t i = 0; i < offsets[0]; ++i) bad += gi[i] != -7;
        for (size_t i = offsets[nseg]; i < n; ++i) bad += gi[i] != -7;
        for (size_t s = 0; s < nseg; ++s) {  // positions INSIDE the segment
            const std::vector<uint32_t> p = stable_perm(k, offsets[s], offsets[s + 1], true);
            for (size_t i = 0; i < p.size(); ++i) bad += gi[offsets[s] + i] != (int64_t)(p[i] - offsets[s]);
        }
        std::snprintf(label, sizeof label, "%s<float, int64_t> descending", rows ? "radix_argsort_rows" : "radix_argsort_segments");
        report(label, bad);
    }
}

static void sharded_form() {
    // two contexts on device 0, as tests/test_gpu_parity.py::test_sharded_single_process runs it
    const size_t n0 = 100003, n1 = 50001;
    std::mt19937_64 rng(31);
    std::vector<uint64_t> all(n0 + n1);
    for (auto& x : all) x = (rng() % 251) * 0x0101010101010101ull + (rng() % 3);
    const std::vector<uint64_t> a(all.begin(), all.begin() + n0), b(all.begin() + n0, all.end());
    uint64_t *d0 = upload(a), *d1 = upload(b), *t0 = device_array<uint64_t>(n0), *t1 = device_array<uint64_t>(n1);
    rsx::Context c0(0), c1(0);
    rsx::radix_sort_sharded<uint64_t>({&c0, &c1}, {d0, d1}, {t0, t1}, {n0, n1});
    c0.synchronize_and_check();
    c1.synchronize_and_check();
    std::vector<uint64_t> got = download(d0, n0);
    const std::vector<uint64_t> g1 = download(d1, n1);
    got.insert(got.end(), g1.begin(), g1.end());
    report("radix_sort_sharded<uint64_t>", gathered_mismatches(got, all, stable_perm(all, 0, all.size(), false)));
}

int main() {
    try {
        rsx::Context ctx;
        flat_forms(ctx);
        {  // ragged segments, empty ones among them, one above every LDS class; elements in front and behind are outside
            const size_t lens[] = {0, 1, 5, 0, 300, 1000, 0, 2049, 7, 0, 0, 4500, 64, 20011, 2, 0};
            std::vector<uint64_t> off(1, 3);
            for (size_t len : lens) off.push_back(off.back() + len);
            segment_forms(ctx, off, off.back() + 5, 0, 0);
        }
        {  // 37 rows of 1000
            std::vector<uint64_t> off;
            for (size_t r = 0; r <= 37; ++r) off.push_back(r * 1000);
            segment_forms(ctx, off, 37000, 37, 1000);
        }
        sharded_form();
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    for (void* p : g_allocs) (void)hipFree(p);
    if (g_bad) {
        std::printf("FAILED %d\n", g_bad);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
