"""The set-operation reference (tests/setop_ref.py) held against collections.Counter on random multisets, against numpy's
set functions on distinct keys and against identities with the merge reference; its tile model held against a plain
emulation of the kernel's per-thread flags (no GPU)."""
import collections
import zlib

import numpy as np
import pytest

import util
from merge_ref import merge_reference
from pairs_ref import mapped_columns
from setop_ref import OPS, capacity, setop_reference, tile_model
from test_merge_ref import sorted_keys

TYPES = ["u8", "i16", "u32", "i64", "f32", "f64", "u128", "i128"]
SIZES = [(0, 0, 1), (0, 5, 3), (5, 0, 3), (1, 1, 1), (7, 9, 1), (40, 33, 4), (64, 64, 11), (100, 3, 50), (3, 100, 2)]


def as_tokens(raw, tname, desc):
    """One hashable, order-preserving token per key: the big-endian bytes of the mapped key."""
    _es, _ko, kb, kind = util.TYPES[tname]
    return [bytes(r[::-1]) for r in mapped_columns(raw, kb, kind, desc)]


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", TYPES)
def test_reference_is_counter_arithmetic(tname, desc):
    rng = np.random.default_rng(zlib.crc32(tname.encode()) + desc)
    kb = util.TYPES[tname][2]
    for na, nb, spread in SIZES:
        a, b = sorted_keys(tname, na, rng, desc, spread), sorted_keys(tname, nb, rng, desc, spread)
        ta, tb = as_tokens(a, tname, desc), as_tokens(b, tname, desc)
        A, B = collections.Counter(ta), collections.Counter(tb)
        want = {"union": A | B, "intersection": A & B, "difference": A - B, "symmetric_difference": (A - B) + (B - A)}
        both = np.concatenate([a, b]).reshape(-1, kb)
        for op in OPS:
            keys, vals, index = setop_reference(a, b, None, None, tname, desc, op)
            assert vals is None and index.size <= capacity(op, na, nb)
            assert np.array_equal(keys.reshape(-1, kb), both[index])
            got = [(ta + tb)[i] for i in index]
            assert got == sorted(want[op].elements()), (tname, desc, op, na, nb)  # the multiset, in sorted order
            assert len(set(index.tolist())) == index.size


@pytest.mark.parametrize("desc", [False, True])
def test_reference_is_numpy_on_distinct_keys(desc):
    rng = np.random.default_rng(5 + desc)
    for na, nb in [(0, 7), (50, 60), (300, 17)]:
        a = np.sort(rng.choice(1000, size=na, replace=False)).astype("<i4") - 500
        b = np.sort(rng.choice(1000, size=nb, replace=False)).astype("<i4") - 500
        if desc:
            a, b = a[::-1].copy(), b[::-1].copy()
        want = {"union": np.union1d(a, b), "intersection": np.intersect1d(a, b), "difference": np.setdiff1d(a, b),
                "symmetric_difference": np.setxor1d(a, b)}
        for op in OPS:
            keys, _v, _i = setop_reference(a.view(np.uint8), b.view(np.uint8), None, None, "i32", desc, op)
            w = want[op][::-1] if desc else want[op]
            assert np.array_equal(keys.view("<i4"), w), (op, desc, na, nb)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", ["u8", "u32", "f64", "i128"])
def test_identities_with_the_merge(tname, desc):
    """|union| + |intersection| = N_a + N_b; intersection and difference partition a in order; values and index are the
    merge's, restricted to the kept positions; device counts cut the inputs and leave b's offset at len(a)."""
    rng = np.random.default_rng(zlib.crc32(tname.encode()) + 2 * desc)
    kb = util.TYPES[tname][2]
    for na, nb, spread in SIZES:
        a, b = sorted_keys(tname, na, rng, desc, spread), sorted_keys(tname, nb, rng, desc, spread)
        av = np.arange(na, dtype="<u4")
        bv = np.arange(nb, dtype="<u4") | np.uint32(1 << 31)
        _mk, mv, perm = merge_reference(a, b, av, bv, tname, desc)
        res = {op: setop_reference(a, b, av, bv, tname, desc, op) for op in OPS}
        assert res["union"][2].size + res["intersection"][2].size == na + nb
        assert res["symmetric_difference"][2].size == res["union"][2].size - res["intersection"][2].size
        inter, diff = res["intersection"][2], res["difference"][2]
        assert np.array_equal(np.sort(np.concatenate([inter, diff])), np.arange(na))  # together: a, each in order
        assert bool((np.diff(inter) > 0).all()) and bool((np.diff(diff) > 0).all())
        for op in OPS:
            keys, vals, index = res[op]
            kept = np.isin(perm, index)
            assert np.array_equal(perm[kept], index), (tname, op)  # the merge's order
            assert np.array_equal(vals.view("<u4"), mv.view("<u4")[kept])
        # counts: the same as cutting the arrays, with b's positions still offset by len(a)
        ca, cb = na // 2, nb - nb // 3
        for op in OPS:
            k1, v1, i1 = setop_reference(a, b, av, bv, tname, desc, op, n_a=ca, n_b=cb)
            k2, v2, i2 = setop_reference(a[:ca * kb], b[:cb * kb], av[:ca], bv[:cb], tname, desc, op)
            assert np.array_equal(k1, k2) and np.array_equal(v1, v2)
            assert np.array_equal(i1, np.where(i2 < ca, i2, i2 - ca + na))
            k3, _v3, i3 = setop_reference(a, b, None, None, tname, desc, op, n_a=na + 9, n_b=nb + 1)  # a count above the length clamps
            assert np.array_equal(k3, res[op][0]) and np.array_equal(i3, res[op][2])


def emulate_tile_flags(a_raw, b_raw, tname, desc, T, ipt):
    """rsx_setop_kernel's flags by its own rule, thread by thread: la, lb from the thread's first key (the global bounds for
    the tile's first key, else searches in the staged ranges), reset to (ai, bi) at every change of key, one probe per
    element -> {op: kept positions in a ++ b, in tile and output order}."""
    ta, tb = as_tokens(a_raw, tname, desc), as_tokens(b_raw, tname, desc)
    na, nb = len(ta), len(tb)
    out = {op: [] for op in OPS}
    for t in tile_model(a_raw, b_raw, tname, desc, T):
        a0, acnt, b0, bcnt = t["a0"], t["acnt"], t["b0"], t["bcnt"]
        sa, sb = ta[a0:a0 + acnt], tb[b0:b0 + bcnt]
        k0 = min(sa[:1] + sb[:1])
        A_lo = sum(1 for k in ta[:a0] if k < k0) if t["front_a"] else a0
        B_lo = sum(1 for k in tb[:b0] if k < k0) if t["front_b"] else b0
        ai = bi = 0
        cur, la, lb = None, 0, 0
        for d in range(acnt + bcnt):
            take_a = ai < acnt and (bi >= bcnt or sa[ai] <= sb[bi])
            k = sa[ai] if take_a else sb[bi]
            if d % ipt == 0 or k != cur:  # a thread's first output, or a change of key
                if k == k0:
                    la, lb = A_lo - a0, B_lo - b0
                elif d % ipt == 0:
                    la, lb = sum(1 for x in sa[:ai] if x < k), sum(1 for x in sb[:bi] if x < k)
                else:
                    la, lb = ai, bi
                cur = k
            if take_a:
                p = b0 + lb + (ai - la)
                matched = p < nb and tb[p] == k
            else:
                p = a0 + la + (bi - lb)
                matched = p < na and ta[p] == k
            src = a0 + ai if take_a else na + b0 + bi
            keep = {"union": take_a or not matched, "intersection": take_a and matched, "difference": take_a and not matched,
                    "symmetric_difference": not matched}
            for op in OPS:
                if keep[op]:
                    out[op].append(src)
            ai, bi = ai + take_a, bi + (not take_a)
    return out


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", ["u8", "i64", "u128"])
def test_the_kernels_rule_gives_the_reference(tname, desc):
    """The tile-local rule of rsx_setop_kernel, emulated on small tiles with the cuts of tile_model, keeps what the definition
    keeps, whatever straddles the tile and thread edges."""
    rng = np.random.default_rng(zlib.crc32(tname.encode()) + 4 * desc)
    seen_front = seen_outside = 0
    for na, nb, spread in SIZES + [(90, 70, 2), (33, 200, 3), (257, 255, 9)]:
        a, b = sorted_keys(tname, na, rng, desc, spread), sorted_keys(tname, nb, rng, desc, spread)
        for T, ipt in ((8, 2), (32, 4), (64, 16)):
            tiles = tile_model(a, b, tname, desc, T)
            assert sum(t["acnt"] for t in tiles) == na and sum(t["bcnt"] for t in tiles) == nb
            seen_front += sum(t["front_a"] or t["front_b"] for t in tiles)
            seen_outside += sum(t["outside"] for t in tiles)
            got = emulate_tile_flags(a, b, tname, desc, T, ipt)
            for op in OPS:
                assert np.array_equal(np.array(got[op], dtype=np.int64), setop_reference(a, b, None, None, tname, desc, op)[2]), (tname, op, na, nb, T)
    assert seen_front > 0 and seen_outside > 0
