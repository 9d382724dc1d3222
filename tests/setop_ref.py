"""Reference for rsx_setop_device / radix_set_op / radix_set_op_pairs, numpy only; a helper, no tests.

The definition of include/rsx.h, written out on the dense ranks of search_ref.ranks (one integer comparison serves u8 and
i128 alike): with N_a, N_b the counted prefixes, A_lo(k) = #{i < N_a : a[i] < k} and B_lo likewise, a[i] of rank
r = i - A_lo(a[i]) in its run is MATCHED when B_lo(a[i]) + r < N_b and b[B_lo(a[i]) + r] == a[i]; b[j] likewise against a.
An operation keeps matched or unmatched elements of a side, and the kept elements come in the order of the stable merge of
a ++ b (equal keys of a first), each with its own value and its position in the concatenation (b's offset is the length
of the whole a array, counted or not).

tile_model restates what rsx_setop_kernel does per tile of T merge positions: the cuts and the clamp (merge_ref), whether
the run of the tile's first key begins in front of the tile on either side (the global lower-bound searches), and how many
probes land outside the staged range of the other array."""
from __future__ import annotations

import numpy as np

import util
from merge_ref import clamp, cut
from search_ref import ranks

OPS = {"union": 0, "intersection": 1, "difference": 2, "symmetric_difference": 3}


def capacity(op: str, na: int, nb: int) -> int:
    return min(na, nb) if op == "intersection" else na if op == "difference" else na + nb


def _prefix(raw, kb, n):
    raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    total = raw.size // kb
    n = total if n is None else min(int(n), total)
    return raw, total, n


def _matched(rx, ry):
    """For sorted ranks rx, ry: (matched flags of x against y, the probe positions in y)."""
    r = np.arange(rx.size, dtype=np.int64) - np.searchsorted(rx, rx, side="left")
    p = np.searchsorted(ry, rx, side="left").astype(np.int64) + r
    ok = p < ry.size
    m = np.zeros(rx.size, dtype=bool)
    m[ok] = ry[p[ok]] == rx[ok]
    return m, p


def setop_reference(a_raw, b_raw, a_vals, b_vals, tname: str, desc: bool, op: str, n_a=None, n_b=None):
    """-> (keys, values, index): the kept key bytes, the value bytes of those very elements (None without values) and their
    positions in a ++ b (int64); len(index) is the number kept.  The first n_a keys of a and n_b keys of b must be sorted."""
    assert op in OPS, op
    _es, _ko, kb, _kind = util.TYPES[tname]
    a_raw, na, Na = _prefix(a_raw, kb, n_a)
    b_raw, nb, Nb = _prefix(b_raw, kb, n_b)
    ra, rb = ranks(a_raw[:Na * kb], b_raw[:Nb * kb], tname, desc)
    assert Na < 2 or bool((ra[1:] >= ra[:-1]).all()), "a is not sorted in this order"
    assert Nb < 2 or bool((rb[1:] >= rb[:-1]).all()), "b is not sorted in this order"
    ma, _ = _matched(ra, rb)
    mb, _ = _matched(rb, ra)
    keep_a = {"union": np.ones(Na, dtype=bool), "intersection": ma, "difference": ~ma, "symmetric_difference": ~ma}[op]
    keep_b = ~mb if op in ("union", "symmetric_difference") else np.zeros(Nb, dtype=bool)
    # positions in the stable merge: a[i] behind the keys of b below it, b[j] behind the keys of a not above it
    pos_a = np.arange(Na, dtype=np.int64) + np.searchsorted(rb, ra, side="left")
    pos_b = np.arange(Nb, dtype=np.int64) + np.searchsorted(ra, rb, side="right")
    src = np.concatenate([np.arange(Na, dtype=np.int64)[keep_a], na + np.arange(Nb, dtype=np.int64)[keep_b]])
    order = np.argsort(np.concatenate([pos_a[keep_a], pos_b[keep_b]]), kind="stable")
    index = src[order]
    cat = np.concatenate([a_raw, b_raw]).reshape(na + nb, kb)
    keys = np.ascontiguousarray(cat[index]).reshape(-1)
    values = None
    if a_vals is not None:
        av = np.ascontiguousarray(a_vals).view(np.uint8).reshape(-1)
        vb = av.size // na if na else (np.ascontiguousarray(b_vals).view(np.uint8).size // nb if b_vals is not None and nb else 0)
        bv = np.ascontiguousarray(b_vals).view(np.uint8).reshape(-1) if b_vals is not None else np.zeros(nb * vb, dtype=np.uint8)
        vals = np.concatenate([av, bv]).reshape(na + nb, vb) if vb else np.zeros((na + nb, 0), dtype=np.uint8)
        values = np.ascontiguousarray(vals[index]).reshape(-1)
    return keys, values, index


def tile_model(a_raw, b_raw, tname: str, desc: bool, tile: int, n_a=None, n_b=None):
    """Per tile of `tile` consecutive positions of the merge of the counted prefixes -> a list of dicts:
    a0, acnt, b0, bcnt  the staged ranges a[a0 : a0 + acnt], b[b0 : b0 + bcnt]
    front_a, front_b    the key in front of the range equals the tile's first key: the global lower bound is searched
    outside             the probes (every element of either side, at its rank in the other side's run) that land outside
                        the other side's staged range
    ties                some key of the tile occurs in both staged ranges."""
    _es, _ko, kb, _kind = util.TYPES[tname]
    a_raw, _na, Na = _prefix(a_raw, kb, n_a)
    b_raw, _nb, Nb = _prefix(b_raw, kb, n_b)
    ra, rb = ranks(a_raw[:Na * kb], b_raw[:Nb * kb], tname, desc)
    _, pa = _matched(ra, rb)
    _, pb = _matched(rb, ra)
    out = []
    for d0 in range(0, Na + Nb, tile):
        d1 = min(d0 + tile, Na + Nb)
        a0, a1 = cut(ra, rb, d0), cut(ra, rb, d1)
        b0, acnt, bcnt = clamp(a0, a1, d0, d1 - d0, Na, Nb)
        sa, sb = ra[a0:a0 + acnt], rb[b0:b0 + bcnt]
        k0 = min(sa[0] if acnt else sb[0], sb[0] if bcnt else sa[0])
        qa, qb = pa[a0:a0 + acnt], pb[b0:b0 + bcnt]
        outside = int(np.count_nonzero((qa < b0) | (qa >= b0 + bcnt))) + int(np.count_nonzero((qb < a0) | (qb >= a0 + acnt)))
        out.append(dict(a0=a0, acnt=acnt, b0=b0, bcnt=bcnt, front_a=bool(a0 > 0 and ra[a0 - 1] == k0), front_b=bool(b0 > 0 and rb[b0 - 1] == k0),
                        outside=outside, ties=bool(np.intersect1d(sa, sb).size)))
    return out
