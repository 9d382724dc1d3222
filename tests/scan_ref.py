"""Reference for rsx_scan_by_key_device / radix_scan_by_key, numpy only; a helper, no tests.

The definition of include/rsx.h.  The rows are put in GROUP ORDER -- for the grouped form through p and the offsets of
unique_ref.unique_reference (ascending; every group then holds its rows in input order), for the runs form as they lie,
a row being a head when its raw key differs from the raw key in front of it in any byte -- scanned per group, and
put back at their input positions:
  integers   np.add / np.minimum / np.maximum accumulated per group in the value's own dtype (a sum wraps);
  float MIN and MAX   through reduce_ref.float_order, the total order on bit patterns: the result is one of the
             group's bit patterns;
  float SUM  has no single right answer (the association is the kernels'), so, as in reduce_ref, two forms:
             `exact`  the prefix in a wider type (float64 for float32 values, longdouble for float64), rounded to the
                      value type -- THE answer where every partial sum is exactly representable (up to the sign of a
                      zero); `free` marks the entries whose exact prefix is zero while its values are not all -0.0:
                      those may come out as +0.0 or -0.0 and are compared as numbers;
             `sums`, `bound`  the longdouble prefix and g(c-1) * sum|v| over the prefix, g(k) = k*u / (1 - k*u), c the
                      1-based rank of the row in its group.
  exclusive  the inclusive array shifted by one inside each group, the low bytes of `first` at the heads (`heads`; there
             `free` is false and `bound` zero).
The accumulation per group is a segmented Hillis-Steele scan (log2 of the longest group passes over the array): the same
values as a loop over the groups, for the operators here, which are associative in the wider types the sums use on the
inputs the tests compare as bytes."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from reduce_ref import FLOAT, MAX, MIN, SUM, UNIT_ROUNDOFF, float_order, float_unorder, value_dtype
from unique_ref import unique_reference

Scanned = namedtuple("Scanned", ["values", "exact", "sums", "bound", "free", "heads", "num", "rank"])


def group_order(keys_raw, kb: int, kind: int, runs: bool, groups=None):
    """-> (p, head): the input positions in group order and, in that order, whether a row is the first of its group."""
    keys_raw = np.ascontiguousarray(keys_raw, dtype=np.uint8).reshape(-1)
    n = keys_raw.size // kb
    if runs:
        k = keys_raw.reshape(n, kb)
        head = np.ones(n, dtype=bool)
        if n > 1:
            head[1:] = (k[1:] != k[:-1]).any(axis=1)
        return np.arange(n, dtype=np.int64), head
    _keys, offsets, perm, _inverse, m = groups if groups is not None else unique_reference(keys_raw, kb, kind, False)
    head = np.zeros(n, dtype=bool)
    head[offsets[:m]] = True
    return perm, head


def ranks(head):
    """0-based rank of every row in its group (rows in group order)."""
    n = head.size
    idx = np.arange(n, dtype=np.int64)
    start = np.maximum.accumulate(np.where(head, idx, 0)) if n else idx
    return idx - start


def segmented_scan(x, head, fn):
    """Inclusive scan of x with fn inside every group (head marks the first row of a group)."""
    x = x.copy()
    f = head.copy()
    longest = int(ranks(head).max(initial=0)) + 1
    d = 1
    while d < longest:
        nx = x.copy()
        with np.errstate(over="ignore", invalid="ignore"):
            nx[d:] = np.where(f[d:], x[d:], fn(x[:-d], x[d:]))
        nf = f.copy()
        nf[d:] |= f[:-d]
        x, f = nx, nf
        d *= 2
    return x


def shifted(incl, head, first):
    """The exclusive array of an inclusive one (rows in group order): first at the heads."""
    out = np.empty_like(incl)
    out[1:] = incl[:-1]
    out[head] = first
    return out


def first_value(first_bits: int, dt):
    return np.array([first_bits & ((1 << (8 * dt.itemsize)) - 1)], dtype="<u" + str(dt.itemsize)).view(dt)[0]


def scan_reference(keys_raw, kb: int, kind: int, values_raw, vb: int, vkind: int, op: int, exclusive: bool, first_bits: int, runs: bool,
                   groups=None) -> Scanned:
    """values_raw None: the count form (every value the integer 1).  -> values: the n results as raw bytes (uint8, n * vb) by
    input position, or None for a float SUM, which fills exact (raw bytes), sums, bound (longdouble) and free (bool)
    instead; heads (bool, by input position), num (the number of groups) and rank (0-based, by input position)."""
    p, head = group_order(keys_raw, kb, kind, runs, groups)
    n = p.size
    dt = value_dtype(vb, vkind)
    vals = np.ones(n, dtype=dt) if values_raw is None else np.ascontiguousarray(values_raw, dtype=np.uint8).reshape(-1).view(dt)
    assert vals.size == n
    first = first_value(first_bits, dt)
    g = vals[p]
    r = ranks(head)

    def back(a):  # group order -> input positions
        out = np.empty_like(a)
        out[p] = a
        return out

    heads, rank, num = back(head), back(r), int(head.sum())
    if vkind != FLOAT or op != SUM:
        if vkind != FLOAT:
            fn = {SUM: np.add, MIN: np.minimum, MAX: np.maximum}[op]
            incl = segmented_scan(g, head, fn).astype(dt)
        else:
            o = float_order(g.view("<u" + str(vb)))
            incl = float_unorder(segmented_scan(o, head, np.minimum if op == MIN else np.maximum)).astype("<u" + str(vb)).view(dt)
        res = shifted(incl, head, first) if exclusive else incl
        return Scanned(back(res).view(np.uint8).copy(), None, None, None, None, heads, num, rank)
    wide = np.float64 if vb == 4 else np.longdouble
    with np.errstate(invalid="ignore", over="ignore"):
        exact = segmented_scan(g.astype(wide), head, np.add).astype(dt)
        sums = segmented_scan(g.astype(np.longdouble), head, np.add)
        abs_sums = segmented_scan(np.abs(g.astype(np.longdouble)), head, np.add)
    negative_zeros = segmented_scan(((g == 0) & np.signbit(g)).astype(np.int64), head, np.add)
    free = (exact == 0) & (negative_zeros != r + 1)
    k = r.astype(np.longdouble)
    u = np.longdouble(UNIT_ROUNDOFF[vb])
    bound = k * u / (1 - k * u) * abs_sums
    if exclusive:
        exact = shifted(exact, head, first)
        with np.errstate(invalid="ignore"):
            sums = shifted(sums, head, np.longdouble(first))
        bound = shifted(bound, head, np.longdouble(0))
        free = shifted(free, head, False)
    return Scanned(None, back(exact).view(np.uint8).copy(), back(sums), back(bound), back(free), heads, num, rank)
