"""Reference for rsx_search_sorted_device / radix_searchsorted, numpy only; a helper, no tests.

The definition of include/rsx.h: with M the mapped key of pairs_ref.mapped_columns (complemented for descending order) and
N = the haystack's length or `num`,
    lower[i] = #{ j < N : M(sorted[j]) <  M(needle[i]) }      upper[i] = #{ j < N : M(sorted[j]) <= M(needle[i]) }
Keys of every width are first replaced by their DENSE RANK among the haystack's and the needles' mapped keys together
(pairs_ref.stable_perm orders them; equal rank = equal in every byte), so that one integer comparison serves u8 and i128
alike."""
from __future__ import annotations

import numpy as np

import util
from pairs_ref import mapped_columns, stable_perm


def ranks(sorted_raw, needles_raw, tname: str, descending: bool):
    """-> (haystack ranks, needle ranks): int64, order-isomorphic to the mapped keys of both arrays taken together."""
    _es, _ko, kb, kind = util.TYPES[tname]
    cols = np.concatenate([mapped_columns(sorted_raw, kb, kind, descending), mapped_columns(needles_raw, kb, kind, descending)])
    total = cols.shape[0]
    n = np.ascontiguousarray(sorted_raw, dtype=np.uint8).size // kb
    if total == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    perm = stable_perm(cols)
    s = cols[perm]
    head = np.ones(total, dtype=bool)
    head[1:] = (s[1:] != s[:-1]).any(axis=1)
    rank = np.empty(total, dtype=np.int64)
    rank[perm] = np.cumsum(head, dtype=np.int64) - 1
    return rank[:n], rank[n:]


def search_reference(sorted_raw, needles_raw, tname: str, descending: bool, num=None):
    """-> (lower, upper), int64, one entry per needle.  The first N keys of the haystack must be sorted by mapped key."""
    hay, ndl = ranks(sorted_raw, needles_raw, tname, descending)
    N = hay.size if num is None else min(int(num), hay.size)
    hay = hay[:N]
    assert N < 2 or bool((hay[1:] >= hay[:-1]).all()), "the haystack is not sorted in this order"
    return np.searchsorted(hay, ndl, side="left").astype(np.int64), np.searchsorted(hay, ndl, side="right").astype(np.int64)


def tile_routes(sorted_raw, needles_raw, tname: str, descending: bool, tile: int, window: int, presorted: bool, num=None):
    """Steps a-c of rsx_search_kernel restated: per tile of `tile` consecutive needles (of the needles sorted by mapped key
    when `presorted`), True when the tile stages its window in LDS: lo = lower(smallest key of the tile), hi = upper(largest),
    hi - lo <= window."""
    hay, ndl = ranks(sorted_raw, needles_raw, tname, descending)
    N = hay.size if num is None else min(int(num), hay.size)
    hay = hay[:N]
    if presorted:
        ndl = np.sort(ndl, kind="stable")
    out = []
    for t0 in range(0, ndl.size, tile):
        part = ndl[t0:t0 + tile]
        lo = int(np.searchsorted(hay, part.min(), side="left"))
        hi = max(lo, int(np.searchsorted(hay, part.max(), side="right")))
        out.append(hi - lo <= window)
    return np.array(out, dtype=bool)
