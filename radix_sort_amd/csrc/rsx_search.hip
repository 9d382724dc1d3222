// rsx_search.hip -- launcher of the search kernel (rsx_search_kernels.hpp) behind rsx_search_sorted_device.  A translation
// unit of its own, beside rsx_unique.hip: twenty small kernels that compile while the element-size units do.  The kernels
// of rsx_join_device (rsx_join_kernels.hpp) are built from the search kernel's functions and are launched from here too.
#include "rsx_internal.hpp"
#include "rsx_search_kernels.hpp"
#include "rsx_join_kernels.hpp"

namespace rsxh {

namespace {

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

template <int KB>
void join_count_typed(const JoinCall& c, uint32_t tiles, hipStream_t st) {
    hipLaunchKernelGGL((rsx_join_count_kernel<KB>), dim3(tiles), dim3(JOIN_WG), 0, st, static_cast<const uint8_t*>(c.a_keys), (uint64_t)c.na, c.a_num,
                       static_cast<const uint8_t*>(c.b_keys), (uint64_t)c.nb, c.b_num, c.kind, c.desc, c.how, c.ws_lo, c.ws_local, c.tile_total);
}
template <int IB>
void join_write_typed(const JoinCall& c, uint64_t tiles, hipStream_t st) {
    hipLaunchKernelGGL((rsx_join_write_kernel<IB>), dim3((uint32_t)c.write_groups), dim3(JOIN_WG), 0, st, c.ws_lo, c.ws_local, c.tile_base, tiles,
                       (uint64_t)c.na, (uint64_t)c.nb, static_cast<const uint8_t*>(c.a_index), static_cast<const uint8_t*>(c.b_index),
                       static_cast<uint8_t*>(c.out_a), static_cast<uint8_t*>(c.out_b), (uint64_t)c.capacity);
}

}  // namespace

uint32_t search_tile_elems(uint32_t kb) { return search_tile(kb); }
uint32_t search_window_elems(uint32_t kb) { return search_window(kb); }

// one launch over c.m >= 1 needles (fewer than 2^32 tiles of them)
int launch_search(rsx_ctx* ctx, const SearchCall& c, uint32_t* launched, hipStream_t st) {
    const uint32_t tile = search_tile(c.kb);
    const uint32_t tiles = (uint32_t)(((uint64_t)c.m + tile - 1) / tile);
    if (c.m == 0 || !tiles_fit(c.m, tile) || (c.ib != 4 && c.ib != 8)) return fail(ctx, RSX_ERR_INTERNAL, "launch_search: no kernel for this call");
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    if (!for_key_width(c.kb, [&](auto kb) { search_kb<decltype(kb)::value>(c, tiles, st); }))
        return fail(ctx, RSX_ERR_INTERNAL, "launch_search: no kernel for this call");
    RSX_HIP(hipGetLastError());
    *launched = 1u;
    return RSX_OK;
}

uint32_t join_tile_elems() { return JOIN_TILE; }
uint32_t join_rows() { return JOIN_ROWS; }

// the count launch, the scan and (c.write) the write launch over c.na >= 1 keys of a
int launch_join(rsx_ctx* ctx, const JoinCall& c, uint32_t* launched, hipStream_t st) {
    const uint64_t tiles = ((uint64_t)c.na + JOIN_TILE - 1) / JOIN_TILE;
    if (c.na == 0 || (uint64_t)c.na >= (1ull << 32) || (uint64_t)c.nb >= (1ull << 32) || c.how > JOIN_ANTI ||
        (c.write && (c.write_groups == 0 || c.write_groups > (1ull << 31) || !c.out_a || (c.ib != 4 && c.ib != 8))))
        return fail(ctx, RSX_ERR_INTERNAL, "launch_join: no kernel for this call");
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    if (!for_key_width(c.kb, [&](auto kb) { join_count_typed<decltype(kb)::value>(c, (uint32_t)tiles, st); }))
        return fail(ctx, RSX_ERR_INTERNAL, "launch_join: no kernel for this call");
    RSX_HIP(hipGetLastError());
    hipLaunchKernelGGL(rsx_join_scan_kernel, dim3(1), dim3(JOIN_WG), 0, st, c.tile_total, c.tile_base, tiles, c.out_num);
    RSX_HIP(hipGetLastError());
    *launched = 2u;
    if (!c.write) return RSX_OK;
    if (c.ib == 4) join_write_typed<4>(c, tiles, st);
    else join_write_typed<8>(c, tiles, st);
    RSX_HIP(hipGetLastError());
    *launched = 3u;
    return RSX_OK;
}

}  // namespace rsxh
