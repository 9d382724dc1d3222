"""Reference for rsx_bin_count_device / radix_histogram / radix_bincount, numpy only; a helper, no tests.

The definition of include/rsx.h: with N = the number of keys or `num`, counts[b] = #{ i < N : bin(keys[i]) == b } for
b = 0 .. m.  Edge modes: bin = upper (mode "upper": the edges <= the key) or lower (mode "lower": the edges < the key) of
search_ref.search_reference with the edges as the haystack, counted by np.bincount(minlength = m + 1).  Index mode: the
key's integer value when it is in 0 .. m - 1, else m, restated directly."""
from __future__ import annotations

import numpy as np

import util
from search_ref import search_reference

INT_DTYPES = {"u8": "<u1", "i8": "<i1", "u16": "<u2", "i16": "<i2", "u32": "<u4", "i32": "<i4", "u64": "<u8", "i64": "<i8"}


def bin_reference(keys_raw, edges_raw, tname: str, mode: str, descending: bool = False, num=None):
    """-> int64 counts, m + 1 of them.  mode "upper" / "lower": edges_raw holds the m edges, sorted in this order;
    mode "index": edges_raw is the integer m itself and tname an integer type of at most 8 bytes."""
    kb = util.TYPES[tname][2]
    keys_raw = np.ascontiguousarray(keys_raw).view(np.uint8).reshape(-1)
    n = keys_raw.size // kb
    N = n if num is None else min(int(num), n)
    keys_raw = keys_raw[:N * kb]
    if mode == "index":
        m = int(edges_raw)
        assert not descending and tname in INT_DTYPES, (tname, descending)
        v = keys_raw.view(INT_DTYPES[tname])
        inside = (v >= 0) & (v.astype(np.uint64) < np.uint64(m)) if v.dtype.kind == "i" else v.astype(np.uint64) < np.uint64(m)
        counts = np.bincount(v[inside].astype(np.int64), minlength=m + 1).astype(np.int64)
        counts[m] = N - int(inside.sum())
        return counts
    assert mode in ("upper", "lower"), mode
    edges_raw = np.ascontiguousarray(edges_raw).view(np.uint8).reshape(-1)
    m = edges_raw.size // kb
    lower, upper = search_reference(edges_raw, keys_raw, tname, descending)
    return np.bincount(upper if mode == "upper" else lower, minlength=m + 1).astype(np.int64)
