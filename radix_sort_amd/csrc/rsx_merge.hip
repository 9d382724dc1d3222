// rsx_merge.hip -- launchers of the merge kernels (rsx_merge_kernels.hpp) behind rsx_merge_device.  A translation unit of
// its own, beside rsx_search.hip: ninety small kernels that compile while the element-size units do.
#include "rsx_internal.hpp"
#include "rsx_merge_kernels.hpp"

namespace rsxh {

namespace {

template <int KB, int VB, int IB>
void merge_typed(const MergeCall& c, uint32_t tiles, hipStream_t st) {
    hipLaunchKernelGGL((rsx_merge_kernel<KB, VB, IB>), dim3(tiles), dim3(MERGE_WG), 0, st, static_cast<const uint8_t*>(c.a_keys),
                       static_cast<const uint8_t*>(c.a_values), (uint64_t)c.na, static_cast<const uint8_t*>(c.b_keys),
                       static_cast<const uint8_t*>(c.b_values), (uint64_t)c.nb, static_cast<uint8_t*>(c.out_keys), static_cast<uint8_t*>(c.out_values),
                       static_cast<uint8_t*>(c.out_index), c.kind, c.desc);
}

}  // namespace

uint32_t merge_tile_elems(uint32_t kb, uint32_t vb) { return merge_tile(kb, vb); }
static_assert(2u * merge_lds_bytes(16, 16) <= 160u * 1024u && 2u * merge_lds_bytes(8, 16) <= 160u * 1024u, "two workgroups per CU at least");

// one launch over c.na + c.nb >= 1 outputs (fewer than 2^31 tiles of them); c.vb is a fused width when c.out_values is given
int launch_merge(rsx_ctx* ctx, const MergeCall& c, uint32_t* launched, hipStream_t st) {
    const uint32_t tile = merge_tile(c.kb, c.vb);
    const uint64_t n = (uint64_t)c.na + c.nb;
    const uint32_t tiles = (uint32_t)((n + tile - 1) / tile);
    if (n == 0 || !tiles_fit(n, tile) || (c.out_index && c.ib != 4 && c.ib != 8) || (c.out_values && !value_width_fused(c.vb)))
        return fail(ctx, RSX_ERR_INTERNAL, "launch_merge: no kernel for this call");
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    const bool known = for_key_width(c.kb, [&](auto kb) {
        for_value_index_width(c.out_values ? c.vb : 0u, c.out_index ? c.ib : 0u, [&](auto vb, auto ib) {
            merge_typed<decltype(kb)::value, decltype(vb)::value, decltype(ib)::value>(c, tiles, st);
        });
    });
    if (!known) return fail(ctx, RSX_ERR_INTERNAL, "launch_merge: no kernel for this call");
    RSX_HIP(hipGetLastError());
    *launched = 1u;
    return RSX_OK;
}

// out_values row r = row pos[r] of a_values ++ b_values (rows of vb bytes), and out_index[r] = pos[r] when asked for
int launch_merge_gather(rsx_ctx* ctx, const MergeCall& c, const uint64_t* pos, void* out_values, void* out_index, hipStream_t st) {
    const uint64_t n = (uint64_t)c.na + c.nb;
    const uintptr_t al = reinterpret_cast<uintptr_t>(c.a_values) | reinterpret_cast<uintptr_t>(c.b_values) | reinterpret_cast<uintptr_t>(out_values) | c.vb;
    const uint32_t w = (al & 15) == 0 ? 16 : 1;
    const uint32_t words = c.vb / w;
    uint32_t gshift = 0;
    while (gshift < 4 && (1u << gshift) < words) ++gshift;  // lanes per row: at most 16, four rows or more per wave
    uint64_t blocks = (n << gshift) / 256 + 1;
    const uint64_t cap = (uint64_t)ctx->num_cu * 16;
    if (blocks > cap) blocks = cap;
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    const uint8_t* ap = static_cast<const uint8_t*>(c.a_values);
    const uint8_t* bp = static_cast<const uint8_t*>(c.b_values);
    if (w == 16)
        hipLaunchKernelGGL(rsx_merge_gather_kernel<uint4>, dim3((uint32_t)blocks), dim3(256), 0, st, ap, bp, (uint64_t)c.na, static_cast<uint8_t*>(out_values),
                           words, pos, n, gshift, static_cast<uint8_t*>(out_index), c.ib);
    else
        hipLaunchKernelGGL(rsx_merge_gather_kernel<uint8_t>, dim3((uint32_t)blocks), dim3(256), 0, st, ap, bp, (uint64_t)c.na, static_cast<uint8_t*>(out_values),
                           words, pos, n, gshift, static_cast<uint8_t*>(out_index), c.ib);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}

}  // namespace rsxh
