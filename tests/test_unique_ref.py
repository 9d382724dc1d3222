"""The reference of the GPU tests of rsx_unique_device (tests/unique_ref.py) against numpy and by hand (no GPU)."""
import numpy as np
import pytest

import util
from unique_ref import unique_reference

INT_TYPES = ["u8", "i8", "u16", "i16", "u32", "i32", "u64", "i64", "u128", "i128"]


def _values(tname, raw):
    """The keys as numbers numpy (or, for 128 bits, Python) orders: a typed array, or an object array of ints."""
    _es, _ko, kb, kind = util.TYPES[tname]
    if kb <= 8:
        return raw.view(("<i" if kind == util.SIGNED else "<u") + str(kb))
    ints = [int.from_bytes(bytes(row), "little", signed=kind == util.SIGNED) for row in raw.reshape(-1, 16)]
    out = np.empty(len(ints), dtype=object)
    out[:] = ints
    return out


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("dist", ["two", "highbyte", "step16", "uniform"])
@pytest.mark.parametrize("tname", INT_TYPES)
def test_integers_equal_numpy_unique(tname, dist, desc):
    kb, kind = util.TYPES[tname][2], util.TYPES[tname][3]
    n = 777
    raw = util.make_input(tname, n, dist, seed=11)
    v = _values(tname, raw)
    want_keys, want_inv, want_counts = np.unique(v, return_inverse=True, return_counts=True)
    want_inv = np.asarray(want_inv).reshape(-1)
    if desc:
        want_keys, want_counts, want_inv = want_keys[::-1], want_counts[::-1], len(want_keys) - 1 - want_inv
    out_keys, offsets, perm, inverse, m = unique_reference(raw, kb, kind, desc)
    assert m == len(want_keys) and offsets.shape == (m + 1,) and offsets[0] == 0 and offsets[m] == n
    got_keys = _values(tname, out_keys)
    assert all(int(a) == int(b) for a, b in zip(got_keys, want_keys))
    assert np.array_equal(np.diff(offsets), np.asarray(want_counts, dtype=np.int64))
    assert np.array_equal(inverse, np.asarray(want_inv, dtype=np.int64))
    assert np.array_equal(np.sort(perm), np.arange(n))
    # the members of every group are in input order, and the first of them is the first occurrence
    first = np.full(m, n, dtype=np.int64)
    np.minimum.at(first, inverse, np.arange(n))
    assert np.array_equal(perm[offsets[:m]], first)
    for j in range(m):
        grp = perm[offsets[j]:offsets[j + 1]]
        assert np.all(np.diff(grp) > 0) and np.all(inverse[grp] == j)


def _f32(bits):
    return np.array(bits, dtype="<u4").view(np.uint8)


def test_signed_zeros_are_two_groups_in_that_order():
    raw = _f32([0x00000000, 0x80000000, 0x00000000, 0x80000000, 0x3F800000])  # +0, -0, +0, -0, 1
    out_keys, offsets, perm, inverse, m = unique_reference(raw, 4, util.FLOAT, False)
    assert m == 3
    assert out_keys.view("<u4").tolist() == [0x80000000, 0x00000000, 0x3F800000]
    assert offsets.tolist() == [0, 2, 4, 5] and perm.tolist() == [1, 3, 0, 2, 4] and inverse.tolist() == [1, 0, 1, 0, 2]
    out_keys, offsets, perm, inverse, m = unique_reference(raw, 4, util.FLOAT, True)
    assert out_keys.view("<u4").tolist() == [0x3F800000, 0x00000000, 0x80000000]
    assert offsets.tolist() == [0, 1, 3, 5] and perm.tolist() == [4, 0, 2, 1, 3] and inverse.tolist() == [1, 2, 1, 2, 0]


def test_nan_payloads_are_keys_of_their_own_and_sort_at_the_ends():
    pnan, pnan2, nnan, ninf, pinf = 0x7FC00000, 0x7FC00001, 0xFFC00000, 0xFF800000, 0x7F800000
    raw = _f32([pnan2, pinf, nnan, pnan, 0x00000000, ninf, pnan2, pnan])
    out_keys, offsets, perm, inverse, m = unique_reference(raw, 4, util.FLOAT, False)
    assert out_keys.view("<u4").tolist() == [nnan, ninf, 0x00000000, pinf, pnan, pnan2]
    assert m == 6 and offsets.tolist() == [0, 1, 2, 3, 4, 6, 8]
    assert perm.tolist() == [2, 5, 4, 1, 3, 7, 0, 6] and inverse.tolist() == [5, 3, 0, 4, 2, 1, 5, 4]
    raw64 = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0x7FF8000000000000], dtype="<u8").view(np.uint8)
    out_keys, offsets, _perm, _inv, m = unique_reference(raw64, 8, util.FLOAT, False)
    assert out_keys.view("<u8").tolist() == [0xFFF8000000000000, 0x7FF8000000000000, 0x7FF8000000000001] and offsets.tolist() == [0, 1, 3, 4]


def test_small_sizes():
    out_keys, offsets, perm, inverse, m = unique_reference(np.zeros(0, dtype=np.uint8), 4, util.UNSIGNED, False)
    assert m == 0 and out_keys.size == 0 and offsets.tolist() == [0] and perm.size == 0 and inverse.size == 0
    out_keys, offsets, perm, inverse, m = unique_reference(np.array([7, 0, 0, 0], dtype=np.uint8), 4, util.SIGNED, True)
    assert m == 1 and out_keys.tolist() == [7, 0, 0, 0] and offsets.tolist() == [0, 1] and perm.tolist() == [0] and inverse.tolist() == [0]
