"""Reference for rsx_merge_device / radix_merge / radix_merge_pairs, numpy only; a helper, no tests.

The definition of include/rsx.h: with c = a ++ b and p the stable permutation that sorts c by mapped key (complemented for
descending order), the outputs are c[p], (a_values ++ b_values)[p] and p itself.  That is pairs_ref.pairs_reference of the
concatenation, the statement the oracle pins for rsx_sort_pairs_device / rsx_argsort_device.

tile_ranges restates steps a and b of rsx_merge_kernel -- the two cuts of every tile on the merge path and the clamp -- on
dense ranks of the mapped keys, so that one integer comparison serves u8 and i128 alike."""
from __future__ import annotations

import numpy as np

import util
from pairs_ref import pairs_reference
from search_ref import ranks


def merge_reference(a_raw, b_raw, a_vals, b_vals, tname: str, desc: bool):
    """-> (keys, values, perm): the merged key bytes, the value bytes moved with them (None without values) and the
    stable permutation of the concatenation (int64)."""
    _es, _ko, kb, kind = util.TYPES[tname]
    a_raw = np.ascontiguousarray(a_raw, dtype=np.uint8).reshape(-1)
    b_raw = np.ascontiguousarray(b_raw, dtype=np.uint8).reshape(-1)
    n = (a_raw.size + b_raw.size) // kb
    vb, vals = 0, None
    if a_vals is not None:
        vals = np.concatenate([np.ascontiguousarray(a_vals).view(np.uint8).reshape(-1), np.ascontiguousarray(b_vals).view(np.uint8).reshape(-1)])
        vb = vals.size // n if n else 0
    keys, values, perm = pairs_reference(np.concatenate([a_raw, b_raw]), vals, kb, kind, vb, desc)
    if vals is not None and values is None:  # (no element: no width to tell)
        values = np.zeros(0, dtype=np.uint8)
    return keys, values, perm


def cut(ra, rb, d: int) -> int:
    """cut(d) for ranks ra, rb: the largest i in [max(0, d - nb), min(d, na)] with i == 0, or d - i >= nb, or
    ra[i-1] <= rb[d-i]; found as the kernel finds it, by counting the i above the lower end for which the predicate holds
    (monotone for sorted inputs; for any inputs a value inside the range)."""
    na, nb = len(ra), len(rb)
    lo, hi = max(0, d - nb), min(d, na)
    if hi == lo:
        return lo
    i = np.arange(lo + 1, hi + 1)
    return lo + int(np.count_nonzero(ra[i - 1] <= rb[d - i]))


def clamp(a0: int, a1: int, d0: int, L: int, na: int, nb: int):
    """Step b -> (b0, acnt, bcnt)."""
    b0 = d0 - a0
    lo, hi = max(0, L - (nb - b0)), min(L, na - a0)
    assert lo <= hi, (a0, a1, d0, L, na, nb)
    acnt = min(max(a1 - a0, lo), hi)
    return b0, acnt, L - acnt


def tile_ranges(a_raw, b_raw, tname: str, desc: bool, tile: int):
    """Steps a and b per tile of `tile` consecutive outputs -> a list of (a0, acnt, b0, bcnt, ties): the tile merges
    a[a0 : a0 + acnt] and b[b0 : b0 + bcnt]; ties: the last key it takes from one side equals the first key the other
    side has left behind the tile's end, or the reverse at its start (equal keys straddle a cut)."""
    ra, rb = ranks(a_raw, b_raw, tname, desc)
    na, nb = ra.size, rb.size
    n = na + nb
    out = []
    for d0 in range(0, n, tile):
        d1 = min(d0 + tile, n)
        a0, a1 = cut(ra, rb, d0), cut(ra, rb, d1)
        b0, acnt, bcnt = clamp(a0, a1, d0, d1 - d0, na, nb)
        ae, be = a0 + acnt, b0 + bcnt
        ties = False
        for ai, bi in ((a0, b0), (ae, be)):  # the keys on both sides of a cut, across the arrays
            if 0 < ai <= na and bi < nb and ra[ai - 1] == rb[bi]:
                ties = True
            if 0 < bi <= nb and ai < na and rb[bi - 1] == ra[ai]:
                ties = True
        out.append((a0, acnt, b0, bcnt, ties))
    return out
