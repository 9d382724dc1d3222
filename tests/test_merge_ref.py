"""The merge reference (tests/merge_ref.py) held against a plain two-pointer loop, and its restatement of the kernel's cuts
and clamp held against the permutation (no GPU)."""
import zlib

import numpy as np
import pytest

import util
from merge_ref import clamp, cut, merge_reference, tile_ranges
from pairs_ref import mapped_columns
from search_ref import ranks

TYPES = ["u8", "i16", "u32", "i64", "f32", "f64", "u128", "i128"]


def sorted_keys(tname, n, rng, desc, spread):
    """n raw keys of few distinct values (ties), sorted by mapped key in the order asked for -> (n * kb) uint8."""
    _es, _ko, kb, kind = util.TYPES[tname]
    pool = util.make_input(tname, max(16, spread), "uniform", int(rng.integers(1 << 30))).reshape(-1, kb)[:spread]
    raw = pool[rng.integers(0, spread, size=n)] if n else np.zeros((0, kb), dtype=np.uint8)
    m = mapped_columns(raw.reshape(-1), kb, kind, desc)
    order = sorted(range(n), key=lambda i: bytes(m[i][::-1]))
    return np.ascontiguousarray(raw[order]).reshape(-1)


def two_pointer(a_raw, b_raw, tname, desc):
    """The textbook loop: take from a while a's key is not larger (a first among ties) -> positions in a ++ b."""
    _es, _ko, kb, kind = util.TYPES[tname]
    ma = [bytes(r[::-1]) for r in mapped_columns(a_raw, kb, kind, desc)]  # big-endian bytes compare like the integer
    mb = [bytes(r[::-1]) for r in mapped_columns(b_raw, kb, kind, desc)]
    i = j = 0
    out = []
    while i < len(ma) or j < len(mb):
        if j >= len(mb) or (i < len(ma) and ma[i] <= mb[j]):
            out.append(i)
            i += 1
        else:
            out.append(len(ma) + j)
            j += 1
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", TYPES)
def test_reference_is_the_two_pointer_merge(tname, desc):
    rng = np.random.default_rng(zlib.crc32(tname.encode()) + desc)
    kb = util.TYPES[tname][2]
    for na, nb, spread in [(0, 0, 1), (0, 5, 3), (5, 0, 3), (1, 1, 1), (7, 9, 1), (40, 33, 4), (64, 64, 11), (100, 3, 50)]:
        a, b = sorted_keys(tname, na, rng, desc, spread), sorted_keys(tname, nb, rng, desc, spread)
        av = np.arange(na, dtype="<u4")
        bv = np.arange(nb, dtype="<u4") | np.uint32(1 << 31)
        keys, vals, perm = merge_reference(a, b, av, bv, tname, desc)
        want = two_pointer(a, b, tname, desc)
        assert np.array_equal(perm, want), (tname, desc, na, nb)
        both = np.concatenate([a, b]).reshape(-1, kb)
        assert np.array_equal(keys.reshape(-1, kb), both[want])
        assert np.array_equal(vals.view("<u4"), np.concatenate([av, bv])[want])
        k2, v2, p2 = merge_reference(a, b, None, None, tname, desc)
        assert v2 is None and np.array_equal(k2, keys) and np.array_equal(p2, perm)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", ["u8", "u32", "i64", "u128"])
def test_cuts_count_the_elements_of_a(tname, desc):
    """cut(d) = the number of positions below na among the first d of the permutation, for every d; and every tile's ranges
    are what the permutation takes, unclamped."""
    rng = np.random.default_rng(7 + zlib.crc32(tname.encode()) + desc)
    for na, nb, spread in [(0, 9, 2), (9, 0, 2), (1, 1, 1), (13, 21, 1), (50, 47, 3), (64, 31, 40), (5, 90, 6)]:
        a, b = sorted_keys(tname, na, rng, desc, spread), sorted_keys(tname, nb, rng, desc, spread)
        _k, _v, perm = merge_reference(a, b, None, None, tname, desc)
        ra, rb = ranks(a, b, tname, desc)
        from_a = np.concatenate([[0], np.cumsum(perm < na)])
        for d in range(na + nb + 1):
            assert cut(ra, rb, d) == from_a[d], (tname, desc, na, nb, d)
        for tile in (1, 4, 16, 33):
            for t, (a0, acnt, b0, bcnt, _ties) in enumerate(tile_ranges(a, b, tname, desc, tile)):
                d0 = t * tile
                part = perm[d0:d0 + tile]
                assert a0 == from_a[d0] and b0 == d0 - a0
                assert acnt == np.count_nonzero(part < na) and bcnt == part.size - acnt


def test_tile_ranges_sees_ties_across_a_cut():
    one = np.full(8, 5, dtype="<u4").view(np.uint8)
    r = tile_ranges(one, one, "u32", False, 4)
    assert [x[:4] for x in r] == [(0, 4, 0, 0), (4, 4, 0, 0), (8, 0, 0, 4), (8, 0, 4, 4)]
    assert r[1][4] and r[2][4]  # a's last key equals b's first, across the cut at output 8
    lo, hi = np.arange(8, dtype="<u4").view(np.uint8), (8 + np.arange(8, dtype="<u4")).view(np.uint8)
    assert not any(x[4] for x in tile_ranges(lo, hi, "u32", False, 4))


@pytest.mark.parametrize("tname", ["u32", "i64", "u128"])
def test_unsorted_inputs_stay_inside_their_arrays(tname):
    """The in-bounds promise: whatever the inputs, every cut lies in its range and the clamp keeps both of a tile's ranges
    inside their arrays, with acnt + bcnt = the tile's length."""
    rng = np.random.default_rng(11)
    kb = util.TYPES[tname][2]
    for trial in range(300):
        na, nb = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        a = rng.integers(0, 4, size=(na, kb), dtype=np.uint8).reshape(-1)
        b = rng.integers(0, 4, size=(nb, kb), dtype=np.uint8).reshape(-1)
        ra, rb = ranks(a, b, tname, bool(trial & 1))
        for tile in (1, 3, 8, 64):
            n = na + nb
            for d0 in range(0, n, tile):
                d1 = min(d0 + tile, n)
                a0, a1 = cut(ra, rb, d0), cut(ra, rb, d1)
                assert max(0, d0 - nb) <= a0 <= min(d0, na) and max(0, d1 - nb) <= a1 <= min(d1, na)
                b0, acnt, bcnt = clamp(a0, a1, d0, d1 - d0, na, nb)
                assert acnt >= 0 and bcnt >= 0 and acnt + bcnt == d1 - d0
                assert 0 <= a0 and a0 + acnt <= na and 0 <= b0 and b0 + bcnt <= nb, (na, nb, tile, d0)
            got = tile_ranges(a, b, tname, bool(trial & 1), tile)
            assert len(got) == (n + tile - 1) // tile
