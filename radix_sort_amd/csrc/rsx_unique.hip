// rsx_unique.hip -- launchers of the run kernels (rsx_unique_kernels.hpp) behind rsx_unique_device.  A translation unit of
// its own, beside rsx_pairs.hip: twenty-six small kernels that compile while the element-size units do.
#include "rsx_internal.hpp"
#include "rsx_unique_kernels.hpp"

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

}  // namespace rsxh
