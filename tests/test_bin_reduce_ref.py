"""CPU: tests/bin_reduce_ref.py against hand-written cases, against tests/reduce_ref.py on the bins that hold a row (the
bin ids as keys: the groups of equal ids ARE the non-empty bins, in order), and against bin_ref.py's counts."""
import numpy as np
import pytest

from bin_ref import bin_reference
from bin_reduce_ref import accumulate_reference, bin_reduce_reference, identity_bits
from reduce_ref import FLOAT, MAX, MIN, SIGNED, SUM, UNSIGNED, reduce_reference, value_dtype

TYPES = [(4, UNSIGNED), (4, SIGNED), (4, FLOAT), (8, UNSIGNED), (8, SIGNED), (8, FLOAT)]


def raw(a, dt):
    return np.asarray(a, dtype=dt).view(np.uint8)


def test_identities():
    assert identity_bits(4, UNSIGNED, SUM) == identity_bits(8, FLOAT, SUM) == 0
    assert identity_bits(4, UNSIGNED, MIN) == 0xFFFFFFFF and identity_bits(4, UNSIGNED, MAX) == 0
    assert identity_bits(4, SIGNED, MIN) == 0x7FFFFFFF and identity_bits(4, SIGNED, MAX) == 0x80000000
    assert identity_bits(4, FLOAT, MIN) == 0x7FFFFFFF and identity_bits(4, FLOAT, MAX) == 0xFFFFFFFF
    assert identity_bits(8, SIGNED, MIN) == 0x7FFFFFFFFFFFFFFF and identity_bits(8, SIGNED, MAX) == 0x8000000000000000
    assert identity_bits(8, FLOAT, MIN) == 0x7FFFFFFFFFFFFFFF and identity_bits(8, FLOAT, MAX) == 0xFFFFFFFFFFFFFFFF
    assert identity_bits(8, UNSIGNED, MIN) == 0xFFFFFFFFFFFFFFFF and identity_bits(8, UNSIGNED, MAX) == 0
    assert np.isnan(np.array([0x7FFFFFFF, 0xFFFFFFFF], dtype="<u4").view("<f4")).all()


def test_edges_by_hand():
    keys = raw([5, 1, 9, 5, 3, 7, 0], "<u4")
    edges = raw([3, 5, 8, 8], "<u4")  # bins: <3 | [3,5) | [5,8) | [8,8) | >=8
    vals = raw([10, -1, 7, 2, 4, -8, 100], "<i4")
    r = bin_reduce_reference(keys, edges, "u32", "upper", vals, 4, SIGNED, SUM)
    assert r.bins.tolist() == [2, 0, 4, 2, 1, 2, 0] and r.counts.tolist() == [2, 1, 3, 0, 1]
    assert r.values.view("<i4").tolist() == [99, 4, 4, 0, 7]
    r = bin_reduce_reference(keys, edges, "u32", "upper", vals, 4, SIGNED, MIN)
    assert r.values.view("<i4").tolist() == [-1, 4, -8, 0x7FFFFFFF, 7]
    r = bin_reduce_reference(keys, edges, "u32", "upper", vals, 4, SIGNED, MAX)
    assert r.values.view("<i4").tolist() == [100, 4, 10, -0x80000000, 7]
    # closed on the right: 3 and 5 move one bin down
    r = bin_reduce_reference(keys, edges, "u32", "lower", vals, 4, SIGNED, SUM)
    assert r.bins.tolist() == [1, 0, 4, 1, 0, 2, 0] and r.values.view("<i4").tolist() == [103, 12, -8, 0, 7]
    # the device row count
    r = bin_reduce_reference(keys, edges, "u32", "upper", vals, 4, SIGNED, SUM, num=3)
    assert r.counts.tolist() == [1, 0, 1, 0, 1] and r.values.view("<i4").tolist() == [-1, 0, 10, 0, 7]
    r = bin_reduce_reference(keys, edges, "u32", "upper", vals, 4, SIGNED, MAX, num=0)
    assert r.counts.tolist() == [0] * 5 and r.values.view("<u4").tolist() == [0x80000000] * 5
    # descending: the edges in descending order, the bins counted from the large end
    r = bin_reduce_reference(keys, raw([8, 5, 3], "<u4"), "u32", "upper", vals, 4, SIGNED, SUM, descending=True)
    assert r.bins.tolist() == [2, 3, 0, 2, 3, 1, 3] and r.values.view("<i4").tolist() == [7, -8, 12, 103]


def test_index_mode_by_hand():
    ids = raw([2, -1, 0, 7, 2, 3], "<i4")
    vals = raw([1.5, 2.0, -0.0, 4.0, 0.25, -0.0], "<f4")
    r = bin_reduce_reference(ids, 3, "i32", "index", vals, 4, FLOAT, SUM)
    assert r.counts.tolist() == [1, 0, 2, 3] and r.values is None
    assert r.exact.view("<u4").tolist() == raw([0.0, 0.0, 1.75, 6.0], "<f4").view("<u4").tolist()  # the bin of -0.0 alone: +0.0
    assert r.sums.tolist() == [0.0, 0.0, 1.75, 6.0] and r.bound[0] == 0 and r.bound[1] == 0 and r.bound[3] > 0
    r = bin_reduce_reference(ids, 3, "i32", "index", vals, 4, FLOAT, MIN)
    assert r.values.view("<u4").tolist() == [0x80000000, 0x7FFFFFFF, raw([0.25], "<f4").view("<u4")[0], 0x80000000]
    r = bin_reduce_reference(ids, 0, "i32", "index", vals, 4, FLOAT, MAX)  # m == 0: one bin
    assert r.counts.tolist() == [6] and r.values.view("<f4").tolist() == [4.0]


def test_float_min_max_follow_the_total_order():
    bits = np.array([0x7FC00000, 0xFFC00000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x3F800000], dtype="<u4")
    keys = raw([0] * 8, "<u4")
    r = bin_reduce_reference(keys, 1, "u32", "index", bits.view(np.uint8), 4, FLOAT, MIN)
    assert r.values.view("<u4").tolist() == [0xFFC00000, 0x7FFFFFFF]  # -NaN is the lowest
    r = bin_reduce_reference(keys, 1, "u32", "index", bits.view(np.uint8), 4, FLOAT, MAX)
    assert r.values.view("<u4").tolist() == [0x7FC00000, 0xFFFFFFFF]  # +NaN the highest
    r = bin_reduce_reference(keys[:8], 1, "u32", "index", bits[2:4].view(np.uint8), 4, FLOAT, MAX, num=2)
    assert r.values.view("<u4").tolist() == [0x00000000, 0xFFFFFFFF]  # +0.0 above -0.0


def test_accumulate_by_hand():
    assert accumulate_reference(raw([1, 0xFFFFFFFF], "<u4"), raw([2, 3], "<u4"), 4, UNSIGNED, SUM).view("<u4").tolist() == [3, 2]  # wraps
    assert accumulate_reference(raw([-5, 9], "<i8"), raw([3, 0x7FFFFFFFFFFFFFFF], "<i8"), 8, SIGNED, MIN).view("<i8").tolist() == [-5, 9]
    assert accumulate_reference(raw([-5, 9], "<i8"), raw([3, -0x8000000000000000], "<i8"), 8, SIGNED, MAX).view("<i8").tolist() == [3, 9]
    got = accumulate_reference(np.array([0x80000000, 0x3F800000], dtype="<u4").view(np.uint8), np.array([0, 0xFFFFFFFF], dtype="<u4").view(np.uint8),
                               4, FLOAT, MAX)
    assert got.view("<u4").tolist() == [0, 0x3F800000]
    assert accumulate_reference(raw([1.5, -2.0], "<f8"), raw([0.25, 0.0], "<f8"), 8, FLOAT, SUM).view("<f8").tolist() == [1.75, -2.0]


@pytest.mark.parametrize("vb,vkind", TYPES)
@pytest.mark.parametrize("op", (SUM, MIN, MAX))
def test_against_reduce_ref_on_the_bins_that_hold_a_row(vb, vkind, op):
    rng = np.random.default_rng(vb * 10 + vkind * 3 + op)
    n, m = 3000, 37
    keys = rng.integers(0, 1000, n).astype("<u4")
    edges = np.sort(rng.integers(0, 1000, m)).astype("<u4")
    edges[5] = edges[6] = edges[7]  # empty bins
    dt = value_dtype(vb, vkind)
    vals = rng.integers(-8, 9, n).astype(dt) if vkind != UNSIGNED else rng.integers(0, 2 ** 32, n).astype(dt)
    for mode in ("upper", "lower"):
        r = bin_reduce_reference(keys.view(np.uint8), edges.view(np.uint8), "u32", mode, vals.view(np.uint8), vb, vkind, op)
        assert np.array_equal(r.counts, bin_reference(keys.view(np.uint8), edges.view(np.uint8), "u32", mode))
        assert r.counts.sum() == n and (r.counts == 0).any()
        ids = r.bins.astype("<i4")
        ref = reduce_reference(ids.view(np.uint8), 4, SIGNED, vals.view(np.uint8), vb, vkind, op, False)
        full = np.flatnonzero(r.counts)
        assert np.array_equal(ref.keys.view("<i4")[:ref.m], full)
        got = r.exact if r.values is None else r.values
        want = ref.exact if ref.values is None else ref.values
        assert np.array_equal(got.reshape(-1, vb)[full].reshape(-1), want)  # (integers in [-8, 8]: float sums are exact, and none is -0.0)
        ident = np.array([identity_bits(vb, vkind, op)], dtype="<u" + str(vb)).view(np.uint8)
        empty = np.flatnonzero(r.counts == 0)
        assert np.array_equal(got.reshape(-1, vb)[empty], np.tile(ident, (empty.size, 1)))
        if r.values is None:
            assert np.allclose(r.sums[full].astype(np.float64), ref.sums.astype(np.float64)) and np.array_equal(r.bound[full], ref.bound)
