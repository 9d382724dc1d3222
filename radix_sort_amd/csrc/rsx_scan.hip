// rsx_scan.hip -- launchers of the kernels (rsx_scan_kernels.hpp) behind rsx_scan_by_key_device: count and write per
// source, key width and value type (and the count form per value width), with the reduce kernels' tile scan between them.
// This is the translation unit of BOTH calls by key: it includes rsx_reduce.hip, the launchers of rsx_reduce_by_key_device,
// as it is, so that rsx_reduce_scan_kernel, which both launch, is instantiated once per value type in the library, and
// the scan kernels, which are built from the reduce kernels' functions, compile beside them.
#include "rsx_reduce.hip"
#include "rsx_scan_kernels.hpp"

namespace rsxh {

namespace {

template <int SRC, int KB, int VB, int VK>
void scan_typed(const ScanCall& c, const ScanArgs& a, uint32_t tiles, hipStream_t st) {
    constexpr int SK = VK == SCANBK_ONES ? 0 : VK;  // the tile scan of the count form adds unsigned counts
    hipLaunchKernelGGL((rsx_scanbk_count_kernel<SRC, KB, VB, VK>), dim3(tiles), dim3(SCANBK_WG), 0, st, a, (uint64_t)c.n, c.op, c.tile_heads,
                       c.tile_tail);
    hipLaunchKernelGGL((rsx_reduce_scan_kernel<VB, SK>), dim3(1), dim3(REDUCE_SCAN_WG), 0, st, c.tile_heads, c.tile_tail, c.tile_base, c.tile_carry,
                       (uint64_t)tiles, (uint64_t)c.n, c.op, c.out_num, static_cast<uint64_t*>(nullptr));
    hipLaunchKernelGGL((rsx_scanbk_write_kernel<SRC, KB, VB, VK>), dim3(tiles), dim3(SCANBK_WG), 0, st, a, (uint64_t)c.n, c.op,
                       c.exclusive ? 1u : 0u, c.first, c.tile_carry);
}
template <int SRC, int KB, int VB>
bool scan_vk(const ScanCall& c, const ScanArgs& a, uint32_t tiles, hipStream_t st) {
    if (!c.values) {
        scan_typed<SRC, KB, VB, SCANBK_ONES>(c, a, tiles, st);
        return true;
    }
    switch (c.vkind) {
        case 0: scan_typed<SRC, KB, VB, 0>(c, a, tiles, st); return true;
        case PAIRS_SIGNED: scan_typed<SRC, KB, VB, (int)PAIRS_SIGNED>(c, a, tiles, st); return true;
        case PAIRS_FLOAT: scan_typed<SRC, KB, VB, (int)PAIRS_FLOAT>(c, a, tiles, st); return true;
        default: return false;
    }
}
template <int SRC, int KB>
bool scan_vb(const ScanCall& c, const ScanArgs& a, uint32_t tiles, hipStream_t st) {
    if (c.vb == 4) return scan_vk<SRC, KB, 4>(c, a, tiles, st);
    if (c.vb == 8) return scan_vk<SRC, KB, 8>(c, a, tiles, st);
    return false;
}
uint32_t wide16(const void* p, uint32_t bit) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 ? bit : 0u; }

}  // namespace

uint32_t scan_tile_elems(uint32_t kb, bool runs) { return scanbk_tile(runs ? SCANBK_COLUMNS : SCANBK_POSITIONS, kb); }

// the three kernels over c.n >= 1 keys (runs) or sorted joined elements
int launch_scan_by_key(rsx_ctx* ctx, const ScanCall& c, uint32_t* launched, hipStream_t st) {
    if (c.n == 0 || (uint64_t)c.n >= (1ull << 32) || c.op > REDUCE_MAX || (!c.values && c.op != REDUCE_SUM))
        return fail(ctx, RSX_ERR_INTERNAL, "launch_scan_by_key: no kernels for this call");
    const uint32_t tile = scan_tile_elems(c.kb, c.runs);
    const uint32_t tiles = (uint32_t)(((uint64_t)c.n + tile - 1) / tile);
    ScanArgs a{};
    a.keys = static_cast<const uint8_t*>(c.keys);
    a.values = static_cast<const uint8_t*>(c.values);
    a.column = static_cast<uint8_t*>(c.column);
    a.out = static_cast<uint8_t*>(c.out);
    a.wide = wide16(c.keys, SCANBK_WIDE_KEYS) | wide16(c.values, SCANBK_WIDE_VALUES) | wide16(c.out, SCANBK_WIDE_OUT);
    LaunchTimer lt(ctx, RSX_PROF_SCAN, st);  // (count, scan, write: timed as one, like the run kernels of the other calls)
    bool ok = false;
    for_key_width(c.kb, [&](auto kb) {
        constexpr int KB = decltype(kb)::value;
        ok = c.runs ? scan_vb<SCANBK_COLUMNS, KB>(c, a, tiles, st) : scan_vb<SCANBK_POSITIONS, KB>(c, a, tiles, st);
    });
    if (!ok) return fail(ctx, RSX_ERR_ARG, "key width or value type without scan kernels");
    RSX_HIP(hipGetLastError());
    *launched = 3u;
    return RSX_OK;
}

}  // namespace rsxh
