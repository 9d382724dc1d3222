// The C++ host mirror (radix_sort_amd/cxx/radix_sort.hpp) on layouts without sort kernels of their own: a 40-byte
// std::pair<uint64_t, std::array<uint8_t, 32>> and a packed 6-byte user type whose RadixDigits specialisation names a
// 48-bit key, each compared with std::stable_sort by mapped key.  Run by tests/test_any_layout_host.py.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "../radix_sort_amd/cxx/radix_sort.hpp"

#pragma pack(push, 1)
struct Rec48 {  // a 48-bit unsigned key in bytes 0..5, nothing else
    unsigned char b[6];
};
#pragma pack(pop)
static_assert(sizeof(Rec48) == 6, "packed");

namespace rsx {
template <>
struct RadixDigits<Rec48> {
    static constexpr uint8_t NUMBER_OF_DIGITS = 6;
    static rsx_layout layout() { return rsx_layout{6, 0, 6, RSX_KEY_UNSIGNED}; }
    static uint8_t get_digit(const Rec48& x, uint8_t index) { return x.b[index]; }
};
}  // namespace rsx

int main() {
    int bad = 0;
    std::mt19937_64 rng(11);
    {
        using P = std::pair<uint64_t, std::array<uint8_t, 32>>;
        const size_t n = 300007;
        std::vector<P> v(n);
        for (size_t i = 0; i < n; ++i) {
            v[i].first = rng() % 5000;  // many ties: stability shows
            v[i].second.fill(0);
            std::memcpy(v[i].second.data(), &i, sizeof i);
        }
        std::vector<P> exp = v;
        std::stable_sort(exp.begin(), exp.end(), [](const P& a, const P& b) { return a.first < b.first; });
        rsx::radix_sort(v);
        const bool ok = std::memcmp(v.data(), exp.data(), n * sizeof(P)) == 0;
        std::printf("pair<u64,[u8;32]> n=%zu %s\n", n, ok ? "ok" : "MISMATCH");
        bad += !ok;
    }
    {
        const size_t n = 200003;
        std::vector<Rec48> v(n);
        for (auto& x : v) {
            const uint64_t r = rng();
            std::memcpy(x.b, &r, 6);
            x.b[5] &= 0x0F;  // ties
            x.b[4] = 0;
        }
        auto key = [](const Rec48& x) {
            uint64_t k = 0;
            std::memcpy(&k, x.b, 6);
            return k;
        };
        std::vector<Rec48> exp = v;
        std::stable_sort(exp.begin(), exp.end(), [&](const Rec48& a, const Rec48& b) { return key(a) < key(b); });
        rsx::radix_sort(v);
        const bool ok = std::memcmp(v.data(), exp.data(), n * sizeof(Rec48)) == 0;
        std::printf("Rec48 (key_bytes 6) n=%zu %s\n", n, ok ? "ok" : "MISMATCH");
        bad += !ok;
    }
    if (!bad) std::printf("ALL OK\n");
    return bad ? 1 : 0;
}
