// rsx_setops.hip -- launchers of the set-operation kernel (rsx_setop_kernels.hpp) behind rsx_setop_device.  A translation
// unit of its own, beside rsx_merge.hip: ninety-five small kernels that compile while the element-size units do.
#include "rsx_internal.hpp"
#include "rsx_setop_kernels.hpp"

namespace rsxh {

namespace {

bool key_width_has_kernel(uint32_t kb) { return kb == 1 || kb == 2 || kb == 4 || kb == 8 || kb == 16; }

template <int KB, int VB, int IB, bool WRITE>
void setop_launch(const SetopCall& c, uint32_t tiles, hipStream_t st) {
    hipLaunchKernelGGL((rsx_setop_kernel<KB, VB, IB, WRITE>), dim3(tiles), dim3(MERGE_WG), 0, st, static_cast<const uint8_t*>(c.a_keys),
                       static_cast<const uint8_t*>(c.a_values), (uint64_t)c.na, c.a_num, static_cast<const uint8_t*>(c.b_keys),
                       static_cast<const uint8_t*>(c.b_values), (uint64_t)c.nb, c.b_num, c.op, c.kind, c.desc, c.tile_count, c.tile_save,
                       static_cast<const uint64_t*>(c.tile_base), static_cast<const uint64_t*>(c.raw_num), (uint64_t)c.cap,
                       static_cast<uint8_t*>(c.out_keys), static_cast<uint8_t*>(c.out_values), static_cast<uint8_t*>(c.out_index), c.out_num);
}
template <int KB, int VB>
void setop_vb(const SetopCall& c, uint32_t tiles, hipStream_t st) {
    if (!c.out_index) setop_launch<KB, VB, 0, true>(c, tiles, st);
    else if (c.ib == 4) setop_launch<KB, VB, 4, true>(c, tiles, st);
    else setop_launch<KB, VB, 8, true>(c, tiles, st);
}
template <int KB>
void setop_kb(const SetopCall& c, uint32_t tiles, hipStream_t st) {
    setop_launch<KB, 0, 0, false>(c, tiles, st);
    launch_run_scan(c.tile_count, c.tile_base, tiles, c.raw_num, st);
    switch (c.out_values ? c.vb : 0u) {
        case 0: setop_vb<KB, 0>(c, tiles, st); break;
        case 1: setop_vb<KB, 1>(c, tiles, st); break;
        case 2: setop_vb<KB, 2>(c, tiles, st); break;
        case 4: setop_vb<KB, 4>(c, tiles, st); break;
        case 8: setop_vb<KB, 8>(c, tiles, st); break;
        default: setop_vb<KB, 16>(c, tiles, st); break;
    }
}

}  // namespace

uint32_t setop_tile_elems(uint32_t kb) { return setop_tile(kb); }
uint32_t setop_save_words() { return SETOP_SAVE; }
static_assert(2u * setop_lds_bytes(16) <= 160u * 1024u && 2u * setop_lds_bytes(8) <= 160u * 1024u && 2u * setop_lds_bytes(4) <= 160u * 1024u,
              "two workgroups per CU at least");
bool setop_value_fused(uint32_t vb) { return vb == 0 || vb == 1 || vb == 2 || vb == 4 || vb == 8 || vb == 16; }

// count, scan, write over the tiles of c.na + c.nb >= 1 merge positions (fewer than 2^31 tiles); c.vb is a fused width
int launch_setop(rsx_ctx* ctx, const SetopCall& c, uint32_t* launched, hipStream_t st) {
    const uint32_t tile = setop_tile(c.kb);
    const uint64_t n = (uint64_t)c.na + c.nb;
    const uint64_t tiles = (n + tile - 1) / tile;
    if (n == 0 || !key_width_has_kernel(c.kb) || tiles >= (1ull << 31) || c.op > SETOP_SYMMETRIC_DIFFERENCE || (c.out_index && c.ib != 4 && c.ib != 8) ||
        (c.out_values && !setop_value_fused(c.vb)) || !c.out_num)
        return fail(ctx, RSX_ERR_INTERNAL, "launch_setop: no kernel for this call");
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    switch (c.kb) {
        case 1: setop_kb<1>(c, (uint32_t)tiles, st); break;
        case 2: setop_kb<2>(c, (uint32_t)tiles, st); break;
        case 4: setop_kb<4>(c, (uint32_t)tiles, st); break;
        case 8: setop_kb<8>(c, (uint32_t)tiles, st); break;
        default: setop_kb<16>(c, (uint32_t)tiles, st); break;
    }
    RSX_HIP(hipGetLastError());
    *launched = 3u;
    return RSX_OK;
}

}  // namespace rsxh
