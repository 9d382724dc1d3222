// rsx_unique.hip -- launchers of the run kernels (rsx_unique_kernels.hpp) behind rsx_unique_device.  A translation unit of
// its own, beside rsx_pairs.hip: twenty-six small kernels that compile while the element-size units do.  The compaction
// kernels of rsx_compact_device (rsx_compact_kernels.hpp) are launched from here too: they use the scan kernel of this unit.
#include "rsx_internal.hpp"
#include "rsx_unique_kernels.hpp"
#include "rsx_compact_kernels.hpp"

namespace rsxh {

namespace {

template <int KB, bool POS, int IB>
void unique_typed(const UniqueCall& c, uint32_t tiles, bool write, hipStream_t st) {
    const uint8_t* e = static_cast<const uint8_t*>(c.elems);
    hipLaunchKernelGGL((rsx_unique_count_kernel<KB, POS>), dim3(tiles), dim3(UNIQUE_WG), 0, st, e, (uint64_t)c.n, c.tile_heads);
    hipLaunchKernelGGL(rsx_unique_scan_kernel, dim3(1), dim3(UNIQUE_SCAN_WG), 0, st, c.tile_heads, c.tile_base, (uint64_t)tiles, (uint64_t)c.n,
                       c.out_num, c.out_offsets);
    if (!write) return;
    const uint32_t perm_words = (reinterpret_cast<uintptr_t>(c.out_perm) & 15) == 0 ? 1u : 0u;
    hipLaunchKernelGGL((rsx_unique_write_kernel<KB, POS, IB>), dim3(tiles), dim3(UNIQUE_WG), 0, st, e, (uint64_t)c.n, c.tile_base,
                       static_cast<uint8_t*>(c.out_keys), c.out_offsets, static_cast<uint8_t*>(c.out_perm), static_cast<uint8_t*>(c.out_inverse),
                       perm_words, c.kind, c.desc);
}
template <int KB>
void unique_kb(const UniqueCall& c, uint32_t tiles, bool write, hipStream_t st) {
    if (!c.pos) unique_typed<KB, false, 4>(c, tiles, write, st);
    else if (c.ib == 4) unique_typed<KB, true, 4>(c, tiles, write, st);
    else unique_typed<KB, true, 8>(c, tiles, write, st);
}

}  // namespace

uint32_t unique_tile_elems(uint32_t kb, bool pos) { return unique_tile(unique_elem(kb, pos)); }
uint32_t unique_scan_span() { return UNIQUE_SCAN_SPAN; }

// the scan kernel alone, for another call's per-tile counts (rsx_setops.hip): at most 4096 per tile
void launch_run_scan(const uint32_t* tile_count, uint64_t* tile_base, uint64_t tiles, uint64_t* out_num, hipStream_t st) {
    hipLaunchKernelGGL(rsx_unique_scan_kernel, dim3(1), dim3(UNIQUE_SCAN_WG), 0, st, tile_count, tile_base, tiles, (uint64_t)0, out_num,
                       static_cast<uint64_t*>(nullptr));
}

// the three run kernels over c.n >= 1 sorted joined elements; the write kernel only when it has an output
int launch_unique(rsx_ctx* ctx, const UniqueCall& c, uint32_t* launched, hipStream_t st) {
    const uint32_t es = pairs_elem_bytes(c.kb, c.pos ? 4u : 0u);
    if (es == 0 || c.n == 0 || (uint64_t)c.n >= (1ull << 32)) return fail(ctx, RSX_ERR_INTERNAL, "launch_unique: no run kernels for this call");
    const uint32_t tile = unique_tile_elems(c.kb, c.pos);
    const uint32_t tiles = (uint32_t)(((uint64_t)c.n + tile - 1) / tile);
    const bool write = c.out_keys || c.out_offsets || c.out_perm || c.out_inverse;
    LaunchTimer lt(ctx, RSX_PROF_SCAN, st);  // (count, scan, write: the three phases of one scan, timed as one)
    if (!for_key_width(c.kb, [&](auto kb) { unique_kb<decltype(kb)::value>(c, tiles, write, st); }))
        return fail(ctx, RSX_ERR_ARG, "key width without run kernels");
    RSX_HIP(hipGetLastError());
    *launched = write ? 3u : 2u;
    return RSX_OK;
}

// ---- rsx_compact_device: count, scan (the run kernels' own), write; the row gather of values without a typed kernel ----
namespace {

template <int KB, int VB>
void compact_typed(const CompactCall& c, uint32_t tiles, hipStream_t st) {
    constexpr int IPT = (int)(compact_tile(KB, VB) / COMPACT_WG);
    const uint8_t* keys = static_cast<const uint8_t*>(c.keys);
    hipLaunchKernelGGL((rsx_compact_count_kernel<KB, IPT>), dim3(tiles), dim3(COMPACT_WG), 0, st, keys, c.flags, c.lo, c.hi, (uint64_t)c.n, c.num, c.kind,
                       c.desc, c.mode, c.tile_count);
    hipLaunchKernelGGL(rsx_unique_scan_kernel, dim3(1), dim3(UNIQUE_SCAN_WG), 0, st, c.tile_count, c.tile_base, (uint64_t)tiles, (uint64_t)0, c.out_num,
                       static_cast<uint64_t*>(nullptr));
    hipLaunchKernelGGL((rsx_compact_write_kernel<KB, VB>), dim3(tiles), dim3(COMPACT_WG), 0, st, keys, c.flags, c.lo, c.hi,
                       static_cast<const uint8_t*>(c.values), (uint64_t)c.n, c.num, c.kind, c.desc, c.mode, c.tile_base, c.out_num,
                       static_cast<uint8_t*>(c.out_keys), static_cast<uint8_t*>(c.out_values), static_cast<uint8_t*>(c.out_index), c.ib);
}
template <int KB>
void compact_kb(const CompactCall& c, uint32_t tiles, hipStream_t st) {
    for_value_index_width(c.vb, 0u, [&](auto vb, auto) { compact_typed<KB, decltype(vb)::value>(c, tiles, st); });
}

}  // namespace

uint32_t compact_tile_elems(uint32_t kb, uint32_t vb) { return compact_tile(kb, vb); }

// the three launches over c.n >= 1 rows; the write launch only when it has an output
int launch_compact(rsx_ctx* ctx, const CompactCall& c, uint32_t* launched, hipStream_t st) {
    if (c.n == 0 || (uint64_t)c.n >= (1ull << 32) || !value_width_fused(c.vb) || (c.vb != 0) != (c.out_values != nullptr))
        return fail(ctx, RSX_ERR_INTERNAL, "launch_compact: no kernels for this call");
    const uint32_t tile = compact_tile(c.kb, c.vb);
    const uint32_t tiles = (uint32_t)(((uint64_t)c.n + tile - 1) / tile);
    LaunchTimer lt(ctx, RSX_PROF_SCAN, st);  // (count, scan, write: the three phases of one scan, timed as one)
    if (c.kb == 0) compact_kb<0>(c, tiles, st);
    else if (!for_key_width(c.kb, [&](auto kb) { compact_kb<decltype(kb)::value>(c, tiles, st); }))
        return fail(ctx, RSX_ERR_INTERNAL, "launch_compact: key width without kernels");
    RSX_HIP(hipGetLastError());
    *launched = 3u;
    return RSX_OK;
}

int launch_compact_gather(rsx_ctx* ctx, const CompactCall& c, const void* pos, uint32_t pb, uint32_t vb, void* out_values, hipStream_t st) {
    if (vb == 0 || (pb != 4 && pb != 8) || !pos || !out_values || !c.values) return fail(ctx, RSX_ERR_INTERNAL, "launch_compact_gather: nothing to gather");
    const bool wide = vb % 4 == 0;
    const uint32_t words = wide ? vb / 4 : vb;
    const uint64_t total = (uint64_t)c.n * words;
    const uint32_t groups = (uint32_t)std::min<uint64_t>((total + 255) / 256, 1u << 20);
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    if (wide)
        hipLaunchKernelGGL(rsx_compact_gather_kernel<uint32_t>, dim3(groups), dim3(256), 0, st, static_cast<const uint8_t*>(c.values),
                           static_cast<const uint8_t*>(pos), pb, (uint64_t)c.n, c.num, c.out_num, c.mode, words, static_cast<uint8_t*>(out_values));
    else
        hipLaunchKernelGGL(rsx_compact_gather_kernel<uint8_t>, dim3(groups), dim3(256), 0, st, static_cast<const uint8_t*>(c.values),
                           static_cast<const uint8_t*>(pos), pb, (uint64_t)c.n, c.num, c.out_num, c.mode, words, static_cast<uint8_t*>(out_values));
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}

}  // namespace rsxh
