// rsx_reduce.hip -- launchers of the run kernels (rsx_reduce_kernels.hpp) behind rsx_reduce_by_key_device.  A
// translation unit of its own, beside rsx_unique.hip: sixty-six small kernels (count and write per key width and value
// type, scan per value type) that compile while the element-size units do.
#include "rsx_internal.hpp"
#include "rsx_reduce_kernels.hpp"

namespace rsxh {

namespace {

template <int KB, int VB, int VK>
void reduce_typed(const ReduceCall& c, uint32_t tiles, hipStream_t st) {
    const uint8_t* e = static_cast<const uint8_t*>(c.elems);
    hipLaunchKernelGGL((rsx_reduce_count_kernel<KB, VB, VK>), dim3(tiles), dim3(REDUCE_WG), 0, st, e, (uint64_t)c.n, c.op, c.tile_heads,
                       c.tile_tail);
    hipLaunchKernelGGL((rsx_reduce_scan_kernel<VB, VK>), dim3(1), dim3(REDUCE_SCAN_WG), 0, st, c.tile_heads, c.tile_tail, c.tile_base, c.tile_carry,
                       (uint64_t)tiles, (uint64_t)c.n, c.op, c.out_num, c.out_offsets);
    hipLaunchKernelGGL((rsx_reduce_write_kernel<KB, VB, VK>), dim3(tiles), dim3(REDUCE_WG), 0, st, e, (uint64_t)c.n, c.op, c.tile_base,
                       c.tile_carry, static_cast<uint8_t*>(c.out_keys), static_cast<uint8_t*>(c.out_values), c.out_offsets, c.kind, c.desc);
}
template <int KB, int VB>
bool reduce_vk(const ReduceCall& c, uint32_t tiles, hipStream_t st) {
    switch (c.vkind) {
        case 0: reduce_typed<KB, VB, 0>(c, tiles, st); return true;
        case PAIRS_SIGNED: reduce_typed<KB, VB, (int)PAIRS_SIGNED>(c, tiles, st); return true;
        case PAIRS_FLOAT: reduce_typed<KB, VB, (int)PAIRS_FLOAT>(c, tiles, st); return true;
        default: return false;
    }
}
template <int KB>
bool reduce_kb(const ReduceCall& c, uint32_t tiles, hipStream_t st) {
    if (c.vb == 4) return reduce_vk<KB, 4>(c, tiles, st);
    if (c.vb == 8) return reduce_vk<KB, 8>(c, tiles, st);
    return false;
}

}  // namespace

uint32_t reduce_tile_elems(uint32_t kb, uint32_t vb) { return reduce_tile(reduce_elem(kb, vb)); }
uint32_t reduce_scan_span() { return REDUCE_SCAN_SPAN; }

// the three run kernels over c.n >= 1 sorted joined elements
int launch_reduce(rsx_ctx* ctx, const ReduceCall& c, uint32_t* launched, hipStream_t st) {
    const uint32_t es = pairs_elem_bytes(c.kb, c.vb);
    if (es == 0 || c.n == 0 || (uint64_t)c.n >= (1ull << 32) || c.op > REDUCE_MAX)
        return fail(ctx, RSX_ERR_INTERNAL, "launch_reduce: no run kernels for this call");
    const uint32_t tile = reduce_tile_elems(c.kb, c.vb);
    const uint32_t tiles = (uint32_t)(((uint64_t)c.n + tile - 1) / tile);
    LaunchTimer lt(ctx, RSX_PROF_SCAN, st);  // (count, scan, write: the three phases of one scan, timed as one)
    bool ok = false;
    for_key_width(c.kb, [&](auto kb) { ok = reduce_kb<decltype(kb)::value>(c, tiles, st); });
    if (!ok) return fail(ctx, RSX_ERR_ARG, "key width or value type without run kernels");
    RSX_HIP(hipGetLastError());
    *launched = 3u;
    return RSX_OK;
}

}  // namespace rsxh
