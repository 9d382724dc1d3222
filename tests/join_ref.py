"""Reference for rsx_join_device / radix_join, numpy only; a helper, no tests.

The definition of include/rsx.h on top of search_ref.search_reference: with lo(i) / hi(i) the lower and upper bound of a[i]
in the first N_b keys of b and m(i) = hi(i) - lo(i), a[i] (i < N_a) contributes c(i) rows -- m, max(m, 1), m > 0, m == 0
for inner, left, semi, anti -- and row t = S(i) + r, S the exclusive sums of c, is (A(i), B(lo(i) + r)), the right side -1
(NONE: all bits set) for the unmatched keys of a left join."""
from __future__ import annotations

import numpy as np

from search_ref import ranks, search_reference

HOWS = {"inner": 0, "left": 1, "semi": 2, "anti": 3}


def bound(how: str, na: int, nb: int) -> int:
    """The most rows a join of na and nb keys can have."""
    return na * nb if how == "inner" else na * max(nb, 1) if how == "left" else na


def _counts(a_raw, b_raw, tname, desc, how, n_a, n_b):
    """-> (lo, m, c): per key of a (all of them; c is 0 from N_a on) its lower bound in b[:N_b], its matches and its rows."""
    lo, hi = search_reference(b_raw, a_raw, tname, desc, num=n_b)
    na = lo.size
    N_a = na if n_a is None else min(int(n_a), na)
    ra = ranks(b_raw, a_raw, tname, desc)[1][:N_a]
    assert N_a < 2 or bool((ra[1:] >= ra[:-1]).all()), "a is not sorted in this order"
    m = hi - lo
    c = {"inner": m, "left": np.maximum(m, 1), "semi": (m > 0).astype(np.int64), "anti": (m == 0).astype(np.int64)}[how].copy()
    c[N_a:] = 0
    return lo, m, c


def join_reference(a_raw, b_raw, tname: str, desc: bool, how: str, n_a=None, n_b=None, a_index=None, b_index=None):
    """-> (left, right, T): int64 arrays of T rows (right is None for semi and anti; -1 where a left join found nothing).
    a_index / b_index: integer arrays whose entries stand in for the positions."""
    lo, m, c = _counts(a_raw, b_raw, tname, desc, how, n_a, n_b)
    S = np.cumsum(c) - c
    T = int(c.sum())
    i = np.repeat(np.arange(c.size, dtype=np.int64), c)
    left = i if a_index is None else np.asarray(a_index).astype(np.int64)[i]
    if how in ("semi", "anti"):
        return left, None, T
    j = lo[i] + (np.arange(T, dtype=np.int64) - S[i])
    none = m[i] == 0
    j[none] = 0
    right = j if b_index is None else (np.asarray(b_index).astype(np.int64)[j] if j.size else j)
    right = right.copy()
    right[none] = -1
    return left, right, T


def tile_model(a_raw, b_raw, tname: str, desc: bool, how: str, tile: int, window: int, rows: int, n_a=None, n_b=None, capacity=None):
    """The kernels' tiles restated.  -> (count, write): per count tile of `tile` keys of a {"staged": its window of b (from
    the lower bound of its smallest counted key to the upper bound of its largest) holds at most `window` keys, "total": its
    rows}; per write tile of `rows` output rows below min(T, capacity) {"tiles": the count tiles its first and last row's
    keys span, "keys": the keys of a between them, both included}."""
    lo, m, c = _counts(a_raw, b_raw, tname, desc, how, n_a, n_b)
    na = c.size
    N_a = na if n_a is None else min(int(n_a), na)
    count = []
    for k0 in range(0, na, tile):
        k1 = min(k0 + tile, N_a)
        wide = 0
        if k1 > k0:
            l, h = lo[k0:k1], (lo + m)[k0:k1]
            wide = max(0, int(h.max()) - int(l.min()))  # a is sorted: the smallest key has the smallest bound
        count.append({"staged": wide <= window, "total": int(c[k0:k0 + tile].sum())})
    S = np.cumsum(c) - c
    T = int(c.sum())
    stop = T if capacity is None else min(T, capacity)
    write = []
    for t0 in range(0, stop, rows):
        t1 = min(t0 + rows, stop)
        e_lo = int(np.searchsorted(S, t0, side="right")) - 1
        e_hi = int(np.searchsorted(S, t1 - 1, side="right")) - 1
        write.append({"tiles": e_hi // tile - e_lo // tile + 1, "keys": e_hi - e_lo + 1})
    return count, write
