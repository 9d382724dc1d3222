// rsx_pairs.hip -- launchers of the join and split kernels (rsx_pairs_kernels.hpp) behind rsx_sort_pairs_device and
// rsx_argsort_device.  A translation unit of its own: the typed kernels are some ninety small instances.
#include "rsx_internal.hpp"
#include "rsx_pairs_kernels.hpp"

namespace rsxh {

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
uint32_t blocks_for(uint64_t n, uint32_t per_thread) { return (uint32_t)((n + (uint64_t)per_thread * 256 - 1) / ((uint64_t)per_thread * 256)); }

template <int KB, int VB, bool GEN>
void join_typed(const uint8_t* keys, const uint8_t* values, uint8_t* elems, uint64_t n, uint32_t kind, uint32_t desc, hipStream_t st) {
    constexpr uint32_t vec = pairs_vec(pairs_elem(KB, VB));
    hipLaunchKernelGGL((rsx_pairs_join_kernel<KB, VB, GEN>), dim3(blocks_for(n, vec)), dim3(256), 0, st, keys, values, elems, n, kind, desc);
}
template <int KB>
bool join_kb(uint32_t vb, bool gen, const uint8_t* keys, const uint8_t* values, uint8_t* elems, uint64_t n, uint32_t kind, uint32_t desc,
             hipStream_t st) {
    if (gen) {
        if (vb == 4) join_typed<KB, 4, true>(keys, values, elems, n, kind, desc, st);
        else if (vb == 8) join_typed<KB, 8, true>(keys, values, elems, n, kind, desc, st);
        else return false;
        return true;
    }
    switch (vb) {
        case 0: join_typed<KB, 0, false>(keys, values, elems, n, kind, desc, st); return true;
        case 1: join_typed<KB, 1, false>(keys, values, elems, n, kind, desc, st); return true;
        case 2: join_typed<KB, 2, false>(keys, values, elems, n, kind, desc, st); return true;
        case 4: join_typed<KB, 4, false>(keys, values, elems, n, kind, desc, st); return true;
        case 8: join_typed<KB, 8, false>(keys, values, elems, n, kind, desc, st); return true;
        case 16: join_typed<KB, 16, false>(keys, values, elems, n, kind, desc, st); return true;
        default: return false;
    }
}
template <int KB>
void join_any(uint32_t vb, const uint8_t* keys, const uint8_t* values, uint8_t* elems, uint64_t n, uint32_t kind, uint32_t desc, hipStream_t st) {
    const uint32_t voff = pairs_voff(KB, vb), es = pairs_elem(KB, vb);
    if (vb % 4 == 0)
        hipLaunchKernelGGL((rsx_pairs_join_any_kernel<KB, uint32_t>), dim3(blocks_for(n, 1)), dim3(256), 0, st, keys, values, elems, n, vb, voff, es,
                           kind, desc);
    else
        hipLaunchKernelGGL((rsx_pairs_join_any_kernel<KB, uint8_t>), dim3(blocks_for(n, 1)), dim3(256), 0, st, keys, values, elems, n, vb, voff, es,
                           kind, desc);
}

template <int KB, int VB, int MODE, int IB>
void split_typed(const uint8_t* elems, uint8_t* keys, uint8_t* values, uint64_t n, uint32_t kind, uint32_t desc, hipStream_t st) {
    constexpr uint32_t vec = pairs_vec(pairs_elem(KB, VB));
    hipLaunchKernelGGL((rsx_pairs_split_kernel<KB, VB, MODE, IB>), dim3(blocks_for(n, vec)), dim3(256), 0, st, elems, keys, values, n, kind, desc);
}
template <int KB>
bool split_kb(uint32_t vb, uint32_t mode, uint32_t ib, const uint8_t* elems, uint8_t* keys, uint8_t* values, uint64_t n, uint32_t kind,
              uint32_t desc, hipStream_t st) {
    if (mode == PAIRS_SPLIT_INDEX) {
        if (vb == 4 && ib == 4) split_typed<KB, 4, PAIRS_SPLIT_INDEX, 4>(elems, keys, values, n, kind, desc, st);
        else if (vb == 4 && ib == 8) split_typed<KB, 4, PAIRS_SPLIT_INDEX, 8>(elems, keys, values, n, kind, desc, st);
        else if (vb == 8 && ib == 8) split_typed<KB, 8, PAIRS_SPLIT_INDEX, 8>(elems, keys, values, n, kind, desc, st);
        else return false;
        return true;
    }
    if (mode == PAIRS_SPLIT_KEYS) {
        if (vb != 4) return false;
        split_typed<KB, 4, PAIRS_SPLIT_KEYS, 4>(elems, keys, values, n, kind, desc, st);
        return true;
    }
    switch (vb) {
        case 0: split_typed<KB, 0, PAIRS_SPLIT_BOTH, 4>(elems, keys, values, n, kind, desc, st); return true;
        case 1: split_typed<KB, 1, PAIRS_SPLIT_BOTH, 4>(elems, keys, values, n, kind, desc, st); return true;
        case 2: split_typed<KB, 2, PAIRS_SPLIT_BOTH, 4>(elems, keys, values, n, kind, desc, st); return true;
        case 4: split_typed<KB, 4, PAIRS_SPLIT_BOTH, 4>(elems, keys, values, n, kind, desc, st); return true;
        case 8: split_typed<KB, 8, PAIRS_SPLIT_BOTH, 4>(elems, keys, values, n, kind, desc, st); return true;
        case 16: split_typed<KB, 16, PAIRS_SPLIT_BOTH, 4>(elems, keys, values, n, kind, desc, st); return true;
        default: return false;
    }
}
template <int KB>
void split_any(uint32_t vb, uint32_t mode, uint32_t ib, const uint8_t* elems, uint8_t* keys, uint8_t* values, uint64_t n, uint32_t kind,
               uint32_t desc, hipStream_t st) {
    const uint32_t voff = pairs_voff(KB, vb), es = pairs_elem(KB, vb);
    if (vb % 4 == 0)
        hipLaunchKernelGGL((rsx_pairs_split_any_kernel<KB, uint32_t>), dim3(blocks_for(n, 1)), dim3(256), 0, st, elems, keys, values, n, vb, voff,
                           es, mode, ib, kind, desc);
    else
        hipLaunchKernelGGL((rsx_pairs_split_any_kernel<KB, uint8_t>), dim3(blocks_for(n, 1)), dim3(256), 0, st, elems, keys, values, n, vb, voff,
                           es, mode, ib, kind, desc);
}

}  // namespace

// keys (and values, or the position when gen) -> n joined elements of pairs_elem(kb, vb) bytes at `elems` (16-byte aligned)
int launch_pairs_join(rsx_ctx* ctx, const void* keys, const void* values, void* elems, size_t n, uint32_t kb, uint32_t vb, bool gen,
                      uint32_t kind, uint32_t desc, hipStream_t st) {
    if (pairs_elem(kb, vb) == 0) return fail(ctx, RSX_ERR_INTERNAL, "launch_pairs_join: no joined element for these widths");
    const uint8_t* k = static_cast<const uint8_t*>(keys);
    const uint8_t* v = gen ? nullptr : static_cast<const uint8_t*>(values);
    uint8_t* e = static_cast<uint8_t*>(elems);
    const bool typed = value_width_fused(vb) && aligned16(k) && aligned16(v) && aligned16(e);
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    bool done = false;
    if (typed) for_key_width(kb, [&](auto w) { done = join_kb<decltype(w)::value>(vb, gen, k, v, e, (uint64_t)n, kind, desc, st); });
    if (!done && !for_key_width(kb, [&](auto w) { join_any<decltype(w)::value>(vb, k, v, e, (uint64_t)n, kind, desc, st); }))
        return fail(ctx, RSX_ERR_ARG, "key width without a join kernel");
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}

// n joined elements -> keys and values (PAIRS_SPLIT_BOTH), keys (PAIRS_SPLIT_KEYS), or the position as ib bytes into
// `values` (PAIRS_SPLIT_INDEX)
int launch_pairs_split(rsx_ctx* ctx, const void* elems, void* keys, void* values, size_t n, uint32_t kb, uint32_t vb, uint32_t mode, uint32_t ib,
                       uint32_t kind, uint32_t desc, hipStream_t st) {
    if (pairs_elem(kb, vb) == 0) return fail(ctx, RSX_ERR_INTERNAL, "launch_pairs_split: no joined element for these widths");
    const uint8_t* e = static_cast<const uint8_t*>(elems);
    uint8_t* k = mode == PAIRS_SPLIT_INDEX ? nullptr : static_cast<uint8_t*>(keys);
    uint8_t* v = mode == PAIRS_SPLIT_KEYS ? nullptr : static_cast<uint8_t*>(values);
    const bool typed = value_width_fused(vb) && aligned16(k) && aligned16(v) && aligned16(e);
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    bool done = false;
    if (typed) for_key_width(kb, [&](auto w) { done = split_kb<decltype(w)::value>(vb, mode, ib, e, k, v, (uint64_t)n, kind, desc, st); });
    if (!done && !for_key_width(kb, [&](auto w) { split_any<decltype(w)::value>(vb, mode, ib, e, k, v, (uint64_t)n, kind, desc, st); }))
        return fail(ctx, RSX_ERR_ARG, "key width without a join kernel");
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}

uint32_t pairs_elem_bytes(uint32_t kb, uint32_t vb) { return pairs_elem(kb, vb); }
uint32_t pairs_value_offset(uint32_t kb, uint32_t vb) { return pairs_voff(kb, vb); }

}  // namespace rsxh
