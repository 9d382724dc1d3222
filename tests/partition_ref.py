"""Reference for rsx_multisplit_device / radix_partition, numpy only; a helper, no tests.

The definition of include/rsx.h: with N = the number of rows or `num` and bin(key) that of rsx_bin_count_device
(bin_ref.py), p is the stable argsort of the bins of the first N rows and offsets[b] = #{ i < N : bin(keys[i]) < b } for
b = 0 .. m + 1.  Edge modes: the bin is upper ("upper": the edges <= the key) or lower ("lower": the edges < it) of
search_ref.search_reference with the edges as the haystack -- what bin_ref.bin_reference counts.  Index mode: the key's
integer value when it is in 0 .. m - 1, else m."""
from __future__ import annotations

import numpy as np

import util
from bin_ref import INT_DTYPES
from search_ref import search_reference


def partition_bins(keys_raw, edges, tname: str, mode: str, descending: bool = False, num=None):
    """-> (int64 bins of the first N rows, m).  edges: the raw bytes of the m sorted edges, or m itself in the index mode."""
    kb = util.TYPES[tname][2]
    keys_raw = np.ascontiguousarray(keys_raw).view(np.uint8).reshape(-1)
    n = keys_raw.size // kb
    N = n if num is None else min(int(num), n)
    keys_raw = keys_raw[:N * kb]
    if mode == "index":
        m = int(edges)
        assert not descending and tname in INT_DTYPES, (tname, descending)
        v = keys_raw.view(INT_DTYPES[tname])
        inside = (v >= 0) & (v.astype(np.uint64) < np.uint64(m)) if v.dtype.kind == "i" else v.astype(np.uint64) < np.uint64(m)
        bins = np.full(N, m, dtype=np.int64)
        bins[inside] = v[inside].astype(np.int64)
        return bins, m
    assert mode in ("upper", "lower"), mode
    edges_raw = np.ascontiguousarray(edges).view(np.uint8).reshape(-1)
    m = edges_raw.size // kb
    lower, upper = search_reference(edges_raw, keys_raw, tname, descending)
    return np.asarray(upper if mode == "upper" else lower, dtype=np.int64).reshape(-1), m


def partition_reference(keys_raw, edges, tname: str, mode: str, descending: bool = False, num=None):
    """-> (perm int64 [N], offsets int64 [m + 2]): perm[t] = the input position of output row t."""
    bins, m = partition_bins(keys_raw, edges, tname, mode, descending, num)
    perm = np.argsort(bins, kind="stable").astype(np.int64)
    offsets = np.zeros(m + 2, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(bins, minlength=m + 1))
    return perm, offsets


def expected_rows(rows_raw, width: int, perm, n: int):
    """The bytes of an output column of n rows of `width` bytes that held 0xA5 before the call: row t < len(perm) is input
    row perm[t], the others are untouched."""
    out = np.full((n, width), 0xA5, dtype=np.uint8)
    out[:perm.size] = np.ascontiguousarray(rows_raw).view(np.uint8).reshape(-1, width)[perm]
    return out.reshape(-1)


def expected_index(perm, index_bytes: int, n: int):
    out = np.full(n * index_bytes, 0xA5, dtype=np.uint8).view("<i4" if index_bytes == 4 else "<i8").copy()
    out[:perm.size] = perm
    return out.view(np.uint8)
