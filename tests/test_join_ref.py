"""The join reference (tests/join_ref.py) held against a brute-force double loop over all (i, j) on inputs of at most 40
keys: every kind of join, both orders, u8 / i32 / f32 (with -0.0, +0.0 and two NaN payloads) / u128, empty sides, counts
below and above the lengths, index arrays; and its tile model against the sums it restates (no GPU)."""
import zlib

import numpy as np
import pytest

import util
from join_ref import HOWS, bound, join_reference, tile_model
from pairs_ref import mapped_columns
from test_merge_ref import sorted_keys

TYPES = ["u8", "i32", "f32", "u128"]
SIZES = [(0, 0, 1), (0, 5, 3), (5, 0, 3), (1, 1, 1), (7, 9, 1), (40, 33, 4), (40, 40, 11), (30, 3, 20), (3, 40, 2)]
F32_POOL = np.array([0x80000000, 0x00000000, 0x7FC00000, 0x7FC00001, 0xFFC00000, 0x3F800000, 0xBF800000], dtype="<u4")


def tokens(raw, tname, desc):
    """One order-preserving token per key: the big-endian bytes of the mapped key."""
    _es, _ko, kb, kind = util.TYPES[tname]
    return [bytes(r[::-1]) for r in mapped_columns(raw, kb, kind, desc)]


def keys(tname, n, rng, desc, spread):
    if tname != "f32":
        return sorted_keys(tname, n, rng, desc, spread)
    raw = F32_POOL[rng.integers(0, min(spread + 3, F32_POOL.size), size=n)].view(np.uint8).reshape(-1, 4)
    tok = tokens(raw.reshape(-1), tname, desc)
    order = sorted(range(n), key=lambda i: tok[i])
    return np.ascontiguousarray(raw[order]).reshape(-1)


def brute(a, b, tname, desc, how, n_a, n_b):
    """Every (i, j) looked at: rows in the order i, then j."""
    ta, tb = tokens(a, tname, desc), tokens(b, tname, desc)
    N_a = len(ta) if n_a is None else min(n_a, len(ta))
    N_b = len(tb) if n_b is None else min(n_b, len(tb))
    left, right = [], []
    for i in range(N_a):
        match = [j for j in range(N_b) if tb[j] == ta[i]]
        if how == "inner" or (how == "left" and match):
            left += [i] * len(match)
            right += match
        elif how == "left":
            left.append(i)
            right.append(-1)
        elif (how == "semi") == bool(match):
            left.append(i)
    return np.array(left, dtype=np.int64), (np.array(right, dtype=np.int64) if how in ("inner", "left") else None)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", TYPES)
def test_reference_is_the_double_loop(tname, desc):
    rng = np.random.default_rng(zlib.crc32(tname.encode()) + desc)
    rows = 0
    for na, nb, spread in SIZES:
        a, b = keys(tname, na, rng, desc, spread), keys(tname, nb, rng, desc, spread)
        for n_a, n_b in ((None, None), (na // 2, nb - nb // 3), (na + 3, nb + 1), (0, nb), (na, 0)):
            for how in HOWS:
                wl, wr = brute(a, b, tname, desc, how, n_a, n_b)
                left, right, T = join_reference(a, b, tname, desc, how, n_a=n_a, n_b=n_b)
                assert T == wl.size and T <= bound(how, na, nb), (tname, how, na, nb, n_a, n_b)
                assert np.array_equal(left, wl), (tname, how, na, nb, n_a, n_b)
                assert (right is None and wr is None) or np.array_equal(right, wr), (tname, how, na, nb, n_a, n_b)
                rows += T
    assert rows > 0


def test_f32_zeros_and_nans_match_by_bit_pattern():
    a = np.array([0x80000000, 0x00000000, 0x7FC00000, 0x7FC00001], dtype="<u4")  # -0.0, +0.0, two NaNs: ascending mapped keys
    b = np.array([0x80000000, 0x7FC00001, 0x7FC00001], dtype="<u4")
    left, right, T = join_reference(a.view(np.uint8), b.view(np.uint8), "f32", False, "left")
    assert T == 5 and left.tolist() == [0, 1, 2, 3, 3] and right.tolist() == [0, -1, -1, 1, 2]
    left, _r, T = join_reference(a.view(np.uint8), b.view(np.uint8), "f32", False, "anti")
    assert left.tolist() == [1, 2]


@pytest.mark.parametrize("how", list(HOWS))
def test_index_arrays_stand_in_for_positions(how):
    rng = np.random.default_rng(9)
    a, b = sorted_keys("i32", 37, rng, False, 6), sorted_keys("i32", 29, rng, False, 6)
    pa, pb = rng.permutation(37) + 1000, rng.permutation(29) + 5000
    left, right, T = join_reference(a, b, "i32", False, how)
    l2, r2, T2 = join_reference(a, b, "i32", False, how, a_index=pa, b_index=pb)
    assert T2 == T and np.array_equal(l2, pa[left])
    if right is not None:
        assert np.array_equal(r2, np.where(right < 0, -1, pb[np.maximum(right, 0)]))


def test_tile_model_restates_the_sums():
    rng = np.random.default_rng(4)
    a, b = sorted_keys("u8", 40, rng, False, 5), sorted_keys("u8", 33, rng, False, 5)
    for how in HOWS:
        _l, _r, T = join_reference(a, b, "u8", False, how)
        count, write = tile_model(a, b, "u8", False, how, tile=8, window=16, rows=16)
        assert len(count) == 5 and sum(t["total"] for t in count) == T
        assert len(write) == (T + 15) // 16 and all(1 <= w["tiles"] <= 5 and 1 <= w["keys"] <= 40 for w in write)
        count, write = tile_model(a, b, "u8", False, how, tile=8, window=16, rows=16, n_a=11, capacity=20)
        assert all(t["total"] == 0 for t in count[2:]) and len(write) <= 2
    count, _w = tile_model(a, b, "u8", False, "inner", tile=8, window=0, rows=16)
    assert not all(t["staged"] for t in count)  # a window of no key stages nothing that matches
