// rsx_search.hip -- launcher of the search kernel (rsx_search_kernels.hpp) behind rsx_search_sorted_device.  A translation
// unit of its own, beside rsx_unique.hip: twenty small kernels that compile while the element-size units do.
#include "rsx_internal.hpp"
#include "rsx_search_kernels.hpp"

namespace rsxh {

namespace {

bool key_width_has_kernel(uint32_t kb) { return kb == 1 || kb == 2 || kb == 4 || kb == 8 || kb == 16; }

template <int KB, bool POS, int IB>
void search_typed(const SearchCall& c, uint32_t tiles, hipStream_t st) {
    hipLaunchKernelGGL((rsx_search_kernel<KB, POS, IB>), dim3(tiles), dim3(SEARCH_WG), 0, st, static_cast<const uint8_t*>(c.sorted), (uint64_t)c.n,
                       c.sorted_num, static_cast<const uint8_t*>(c.needles), (uint64_t)c.m, static_cast<uint8_t*>(c.out_lower),
                       static_cast<uint8_t*>(c.out_upper), c.kind, c.desc);
}
template <int KB>
void search_kb(const SearchCall& c, uint32_t tiles, hipStream_t st) {
    if (!c.pos) {
        if (c.ib == 4) search_typed<KB, false, 4>(c, tiles, st);
        else search_typed<KB, false, 8>(c, tiles, st);
    } else {
        if (c.ib == 4) search_typed<KB, true, 4>(c, tiles, st);
        else search_typed<KB, true, 8>(c, tiles, st);
    }
}

}  // namespace

uint32_t search_tile_elems(uint32_t kb) { return search_tile(kb); }
uint32_t search_window_elems(uint32_t kb) { return search_window(kb); }

// one launch over c.m >= 1 needles (fewer than 2^32 tiles of them)
int launch_search(rsx_ctx* ctx, const SearchCall& c, uint32_t* launched, hipStream_t st) {
    const uint32_t tile = search_tile(c.kb);
    const uint64_t tiles = ((uint64_t)c.m + tile - 1) / tile;
    if (c.m == 0 || !key_width_has_kernel(c.kb) || tiles >= (1ull << 31) || (c.ib != 4 && c.ib != 8)) return fail(ctx, RSX_ERR_INTERNAL, "launch_search: no kernel for this call");
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    switch (c.kb) {
        case 1: search_kb<1>(c, (uint32_t)tiles, st); break;
        case 2: search_kb<2>(c, (uint32_t)tiles, st); break;
        case 4: search_kb<4>(c, (uint32_t)tiles, st); break;
        case 8: search_kb<8>(c, (uint32_t)tiles, st); break;
        case 16: search_kb<16>(c, (uint32_t)tiles, st); break;
        default: return fail(ctx, RSX_ERR_ARG, "key width without a search kernel");
    }
    RSX_HIP(hipGetLastError());
    *launched = 1u;
    return RSX_OK;
}

}  // namespace rsxh
