// rsx_setops.hip -- launchers of the set-operation kernel (rsx_setop_kernels.hpp) behind rsx_setop_device.  A translation
// unit of its own, beside rsx_merge.hip: ninety-five small kernels that compile while the element-size units do.
#include "rsx_internal.hpp"
#include "rsx_setop_kernels.hpp"

namespace rsxh {

namespace {

template <int KB, int VB, int IB, bool WRITE>
void setop_launch(const SetopCall& c, uint32_t tiles, hipStream_t st) {
    hipLaunchKernelGGL((rsx_setop_kernel<KB, VB, IB, WRITE>), dim3(tiles), dim3(MERGE_WG), 0, st, static_cast<const uint8_t*>(c.a_keys),
                       static_cast<const uint8_t*>(c.a_values), (uint64_t)c.na, c.a_num, static_cast<const uint8_t*>(c.b_keys),
                       static_cast<const uint8_t*>(c.b_values), (uint64_t)c.nb, c.b_num, c.op, c.kind, c.desc, c.tile_count, c.tile_save,
                       static_cast<const uint64_t*>(c.tile_base), static_cast<const uint64_t*>(c.raw_num), (uint64_t)c.cap,
                       static_cast<uint8_t*>(c.out_keys), static_cast<uint8_t*>(c.out_values), static_cast<uint8_t*>(c.out_index), c.out_num);
}

}  // namespace

uint32_t setop_tile_elems(uint32_t kb) { return setop_tile(kb); }
uint32_t setop_save_words() { return SETOP_SAVE; }
static_assert(2u * setop_lds_bytes(16) <= 160u * 1024u && 2u * setop_lds_bytes(8) <= 160u * 1024u && 2u * setop_lds_bytes(4) <= 160u * 1024u,
              "two workgroups per CU at least");

// count, scan, write over the tiles of c.na + c.nb >= 1 merge positions (fewer than 2^31 tiles); c.vb is a fused width
int launch_setop(rsx_ctx* ctx, const SetopCall& c, uint32_t* launched, hipStream_t st) {
    const uint32_t tile = setop_tile(c.kb);
    const uint64_t n = (uint64_t)c.na + c.nb;
    const uint32_t tiles = (uint32_t)((n + tile - 1) / tile);
    if (n == 0 || !tiles_fit(n, tile) || c.op > SETOP_SYMMETRIC_DIFFERENCE || (c.out_index && c.ib != 4 && c.ib != 8) ||
        (c.out_values && !value_width_fused(c.vb)) || !c.out_num)
        return fail(ctx, RSX_ERR_INTERNAL, "launch_setop: no kernel for this call");
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    const bool known = for_key_width(c.kb, [&](auto kb) {
        setop_launch<decltype(kb)::value, 0, 0, false>(c, tiles, st);
        launch_run_scan(c.tile_count, c.tile_base, tiles, c.raw_num, st);
        for_value_index_width(c.out_values ? c.vb : 0u, c.out_index ? c.ib : 0u, [&](auto vb, auto ib) {
            setop_launch<decltype(kb)::value, decltype(vb)::value, decltype(ib)::value, true>(c, tiles, st);
        });
    });
    if (!known) return fail(ctx, RSX_ERR_INTERNAL, "launch_setop: no kernel for this call");
    RSX_HIP(hipGetLastError());
    *launched = 3u;
    return RSX_OK;
}

}  // namespace rsxh
