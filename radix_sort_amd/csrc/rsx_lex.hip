// rsx_lex.hip -- launcher of the join kernel of several key columns (rsx_lex_kernels.hpp) behind rsx_lexsort_device and
// rsx_sort_columns_device.  A translation unit of its own, beside rsx_pairs.hip: ten kernels (compound key width x
// first or later round) that compile while the element-size units do.
#include "rsx_internal.hpp"
#include "rsx_lex_kernels.hpp"

namespace rsxh {

namespace {

template <int W>
void lex_join_w(const LexArgs& a, const LexJoinCall& c, hipStream_t st) {
    constexpr uint32_t vec = pairs_vec(pairs_elem(W, 4));
    const uint64_t per_block = (uint64_t)vec * 256;
    const dim3 grid((uint32_t)(((uint64_t)c.n + per_block - 1) / per_block));
    uint8_t* e = static_cast<uint8_t*>(c.elems);
    if (c.prev)
        hipLaunchKernelGGL((rsx_lex_join_kernel<W, true>), grid, dim3(256), 0, st, a, static_cast<const uint8_t*>(c.prev), c.prev_es, c.prev_voff, e,
                           (uint64_t)c.n);
    else
        hipLaunchKernelGGL((rsx_lex_join_kernel<W, false>), grid, dim3(256), 0, st, a, static_cast<const uint8_t*>(nullptr), 0u, 0u, e, (uint64_t)c.n);
}

}  // namespace

// the columns of one round -> n joined (compound key, u32 position) elements of pairs_elem(c.w, 4) bytes at c.elems
// (16-byte aligned); c.prev: the previous round's sorted elements, whose positions this round reads its keys through
int launch_lex_join(rsx_ctx* ctx, const LexJoinCall& c, hipStream_t st) {
    if (c.ncols == 0 || c.ncols > LEX_MAX_COLUMNS || c.n == 0 || (uint64_t)c.n >= (1ull << 32) || pairs_elem(c.w, 4) == 0)
        return fail(ctx, RSX_ERR_INTERNAL, "launch_lex_join: no join for this round");
    const uint32_t vec = pairs_vec(pairs_elem(c.w, 4));
    LexArgs a{};
    uint32_t used = 0;
    for (uint32_t i = 0; i < c.ncols; ++i) {
        const LexJoinCol& s = c.col[i];
        const uintptr_t p = reinterpret_cast<uintptr_t>(s.keys);
        if (!(s.kb == 1 || s.kb == 2 || s.kb == 4 || s.kb == 8 || s.kb == 16) || s.off + s.kb > c.w || !s.keys || (p & (s.kb - 1)))
            return fail(ctx, RSX_ERR_INTERNAL, "launch_lex_join: a column does not fit the compound key");
        a.col[i] = LexColumn{static_cast<const uint8_t*>(s.keys), s.kb, s.kind, s.desc ? 1u : 0u, s.off, (p & ((uintptr_t)s.kb * vec - 1)) == 0 ? 1u : 0u, 0u};
        used += s.kb;
    }
    if (used > c.w || (reinterpret_cast<uintptr_t>(c.elems) & 15) != 0 || (c.prev && (c.prev_voff + 4 > c.prev_es || (c.prev_voff & 3) || (c.prev_es & 3))))
        return fail(ctx, RSX_ERR_INTERNAL, "launch_lex_join: elements misplaced");
    a.ncols = c.ncols;
    LaunchTimer lt(ctx, RSX_PROF_OTHER, st);
    if (!for_key_width(c.w, [&](auto w) { lex_join_w<decltype(w)::value>(a, c, st); }))
        return fail(ctx, RSX_ERR_INTERNAL, "launch_lex_join: compound key width without a kernel");
    RSX_HIP(hipGetLastError());
    return RSX_OK;
}

}  // namespace rsxh
