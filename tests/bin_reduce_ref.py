"""Reference for rsx_bin_reduce_device / radix_bin_reduce, numpy only; a helper, no tests.

The definition of include/rsx.h: with N = the number of rows or `num` and bin(key) that of rsx_bin_count_device
(partition_ref.partition_bins, which is bin_ref.py's rule row by row), out[b] is the (+) of values[i] over
{ i < N : bin(keys[i]) == b } for b = 0 .. m and counts[b] that set's size.  An empty bin holds the operator's identity:
SUM 0 (+0.0), MIN the highest value of the order (integer maximum; the float bit pattern 0x7FFF...F), MAX the lowest
(integer minimum; 0xFFFF...F).  Integer sums wrap; float MIN and MAX go through reduce_ref's order-preserving map of the
bit patterns, so the result is one of the bin's bit patterns; a float SUM starts from +0.0 (a bin of -0.0 holds +0.0)
and has no single right answer, so as in reduce_ref there are two forms: `exact` (the sum in a wider type, rounded: THE
answer when every partial sum is exactly representable) and `sums`, `bound` (longdouble sums and g(c-1) * sum|v|)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import util
from partition_ref import partition_bins
from reduce_ref import FLOAT, MAX, MIN, SIGNED, SUM, UNIT_ROUNDOFF, float_order, float_unorder, value_dtype

BinReduced = namedtuple("BinReduced", ["values", "counts", "exact", "sums", "bound", "bins"])


def identity_bits(vb: int, vkind: int, op: int) -> int:
    """The bit pattern of an empty bin, as an unsigned integer of vb bytes."""
    ones, top = (1 << (8 * vb)) - 1, 1 << (8 * vb - 1)
    if op == SUM:
        return 0
    if op == MIN:
        return ones if vkind not in (SIGNED, FLOAT) else top - 1
    return ones if vkind == FLOAT else top if vkind == SIGNED else 0


def bin_reduce_reference(keys_raw, edges, tname: str, mode: str, values_raw, vb: int, vkind: int, op: int, descending: bool = False,
                         num=None) -> BinReduced:
    """edges: the raw bytes of the m sorted edges, or m itself in the index mode.  values: the m + 1 results as raw bytes
    (uint8), or None for a float SUM, which fills exact (raw bytes), sums and bound (longdouble, m + 1 each) instead.
    counts: int64, m + 1.  bins: the bin of each of the first N rows."""
    bins, m = partition_bins(keys_raw, edges, tname, mode, descending, num)
    N = bins.size
    dt = value_dtype(vb, vkind)
    ut = np.dtype("<u" + str(vb))
    vals = np.ascontiguousarray(values_raw, dtype=np.uint8).reshape(-1).view(dt)[:N]
    counts = np.bincount(bins, minlength=m + 1).astype(np.int64)
    order = np.argsort(bins, kind="stable")
    g = vals[order]
    full = np.flatnonzero(counts)                      # the bins that hold a row
    starts = (np.cumsum(counts) - counts)[full]
    out = np.full(m + 1, identity_bits(vb, vkind, op), dtype=ut)
    if vkind == FLOAT and op == SUM:
        wide = np.float64 if vb == 4 else np.longdouble
        exact = np.zeros(m + 1, dtype=dt)
        sums = np.zeros(m + 1, dtype=np.longdouble)
        abs_sums = np.zeros(m + 1, dtype=np.longdouble)
        if full.size:
            with np.errstate(invalid="ignore", over="ignore"):
                exact[full] = np.add.reduceat(g.astype(wide), starts).astype(dt) + dt.type(0.0)  # (from +0.0: no -0.0 sum)
                sums[full] = np.add.reduceat(g.astype(np.longdouble), starts)
                abs_sums[full] = np.add.reduceat(np.abs(g.astype(np.longdouble)), starts)
        k = np.maximum(counts - 1, 0).astype(np.longdouble)
        u = np.longdouble(UNIT_ROUNDOFF[vb])
        return BinReduced(None, counts, exact.view(np.uint8).copy(), sums, k * u / (1 - k * u) * abs_sums, bins)
    if full.size:
        if vkind == FLOAT:
            o = float_order(g.view(ut))
            out[full] = float_unorder((np.minimum if op == MIN else np.maximum).reduceat(o, starts)).astype(ut)
        else:
            fn = {SUM: np.add, MIN: np.minimum, MAX: np.maximum}[op]
            with np.errstate(over="ignore"):
                out[full] = fn.reduceat(g, starts, dtype=dt).astype(dt).view(ut)
    return BinReduced(out.view(np.uint8).copy(), counts, None, None, None, bins)


def accumulate_reference(initial_raw, result_raw, vb: int, vkind: int, op: int):
    """out (+) r on raw bytes, entry by entry: what RSX_BIN_ACCUMULATE leaves (float sums: of exactly representable values)."""
    dt, ut = value_dtype(vb, vkind), np.dtype("<u" + str(vb))
    a = np.ascontiguousarray(initial_raw, dtype=np.uint8).reshape(-1).view(dt)
    r = np.ascontiguousarray(result_raw, dtype=np.uint8).reshape(-1).view(dt)
    if op == SUM:
        with np.errstate(over="ignore", invalid="ignore"):
            return (a + r).astype(dt).view(np.uint8).copy()
    if vkind == FLOAT:
        oa, orr = float_order(a.view(ut)), float_order(r.view(ut))
        return float_unorder(np.minimum(oa, orr) if op == MIN else np.maximum(oa, orr)).astype(ut).view(np.uint8).copy()
    return (np.minimum(a, r) if op == MIN else np.maximum(a, r)).astype(dt).view(np.uint8).copy()


def key_type(tname: str):
    """(key_bytes, key_kind) of a type name of util.TYPES"""
    return util.TYPES[tname][2], util.TYPES[tname][3]
