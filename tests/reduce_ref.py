"""Reference for rsx_reduce_by_key_device / radix_reduce_by_key, numpy only; a helper, no tests.

The definition of include/rsx.h on top of unique_ref.unique_reference: p, the heads and m are those of the group call; the
values are gathered through p (so every group holds its values in input order) and combined per group:
  integers   np.add / np.minimum / np.maximum .reduceat in the value's own dtype (a sum wraps);
  float MIN and MAX   through the order-preserving map of the bit patterns to unsigned and back: -NaN lowest, -0.0 below
             +0.0, +NaN highest; the result is one of the group's bit patterns;
  float SUM  has no single right answer (the association is the kernels'), so the reference gives two forms:
             `exact`  the sum in a wider type (float64 for float32 values, longdouble for float64), rounded to the value
                      type -- THE answer for inputs whose partial sums are all exactly representable, where every
                      association gives these bytes (up to the sign of a zero sum);
             `sums`, `bound`  the longdouble sum of every group and g(c-1) * sum|v|, g(k) = k*u / (1 - k*u), u the unit
                      roundoff of the value type and c the group's size: |result - exact sum| <= bound in any order."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from unique_ref import unique_reference

UNSIGNED, SIGNED, FLOAT = 0, 1, 2
SUM, MIN, MAX = 0, 1, 2
UNIT_ROUNDOFF = {4: 2.0 ** -24, 8: 2.0 ** -53}

Reduced = namedtuple("Reduced", ["keys", "offsets", "m", "perm", "values", "exact", "sums", "bound", "abs_sums"])


def value_dtype(vb: int, vkind: int):
    return np.dtype({UNSIGNED: "<u", SIGNED: "<i", FLOAT: "<f"}[vkind] + str(vb))


def float_order(bits: np.ndarray) -> np.ndarray:
    """Unsigned bit patterns of floats -> unsigned integers in the total order (negative: all bits flipped, else the sign bit)."""
    sign = bits.dtype.type(1) << bits.dtype.type(8 * bits.dtype.itemsize - 1)
    return np.where((bits & sign) != 0, ~bits, bits | sign)


def float_unorder(o: np.ndarray) -> np.ndarray:
    sign = o.dtype.type(1) << o.dtype.type(8 * o.dtype.itemsize - 1)
    return np.where((o & sign) != 0, o & ~sign, ~o)


def reduce_reference(keys_raw, kb: int, kind: int, values_raw, vb: int, vkind: int, op: int, descending: bool, groups=None) -> Reduced:
    """keys, offsets, m, perm: those of unique_reference.  values: the m reduced values as raw bytes (uint8, m * vb), or
    None for a float SUM, which fills exact (raw bytes), sums, bound and abs_sums (longdouble, m each) instead.
    groups: what unique_reference(keys_raw, kb, kind, descending) returned, where the caller has it already."""
    out_keys, offsets, perm, _inverse, m = groups if groups is not None else unique_reference(keys_raw, kb, kind, descending)
    dt = value_dtype(vb, vkind)
    vals = np.ascontiguousarray(values_raw, dtype=np.uint8).reshape(-1).view(dt)
    assert vals.size == perm.size
    if m == 0:
        empty = np.zeros(0, dtype=np.uint8)
        ld = np.zeros(0, dtype=np.longdouble)
        fsum = vkind == FLOAT and op == SUM
        return Reduced(out_keys, offsets, 0, perm, None if fsum else empty, empty if fsum else None, ld if fsum else None,
                       ld if fsum else None, ld if fsum else None)
    g = vals[perm]
    starts = offsets[:-1]
    if vkind != FLOAT:
        fn = {SUM: np.add, MIN: np.minimum, MAX: np.maximum}[op]
        with np.errstate(over="ignore"):
            red = fn.reduceat(g, starts, dtype=dt)
        return Reduced(out_keys, offsets, m, perm, red.astype(dt).view(np.uint8).copy(), None, None, None, None)
    if op != SUM:
        o = float_order(g.view("<u" + str(vb)))
        red = (np.minimum if op == MIN else np.maximum).reduceat(o, starts)
        return Reduced(out_keys, offsets, m, perm, float_unorder(red).astype("<u" + str(vb)).view(np.uint8).copy(), None, None, None, None)
    with np.errstate(invalid="ignore", over="ignore"):
        wide = np.float64 if vb == 4 else np.longdouble
        exact = np.add.reduceat(g.astype(wide), starts).astype(dt)
        sums = np.add.reduceat(g.astype(np.longdouble), starts)
        abs_sums = np.add.reduceat(np.abs(g.astype(np.longdouble)), starts)
    k = (np.diff(offsets) - 1).astype(np.longdouble)
    u = np.longdouble(UNIT_ROUNDOFF[vb])
    bound = k * u / (1 - k * u) * abs_sums
    return Reduced(out_keys, offsets, m, perm, None, exact.view(np.uint8).copy(), sums, bound, abs_sums)
