"""CPU: tests/partition_ref.py against a brute-force double loop over mapped keys on tiny inputs, and against
bin_ref.bin_reference: the bins' sizes are the bin counts."""
import numpy as np
import pytest

from bin_ref import INT_DTYPES, bin_reference
from partition_ref import expected_index, expected_rows, partition_bins, partition_reference
from test_bin_ref import mapped_ints, raw_keys, sorted_edges

CASES = ((0, 5, None), (1, 40, None), (9, 70, None), (12, 70, 31), (4, 0, None), (3, 20, 100), (5, 33, 0))


def brute_force(bins, m):
    """the stable grouping by a double loop: for every bin in turn, the rows that hold it, in input order"""
    perm, offsets = [], [0]
    for b in range(m + 1):
        for i, x in enumerate(bins):
            if x == b:
                perm.append(i)
        offsets.append(len(perm))
    return np.array(perm, dtype=np.int64), np.array(offsets, dtype=np.int64)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("mode", ["upper", "lower"])
@pytest.mark.parametrize("tname", ["u8", "i32", "f32", "i64", "u128"])
def test_reference_against_a_double_loop(tname, mode, desc):
    for m, n, num in CASES:
        keys = raw_keys(tname, n, 7 + m)
        edges = sorted_edges(tname, m, m, desc)
        N = n if num is None else min(num, n)
        mk, me = mapped_ints(keys, tname, desc)[:N], mapped_ints(edges, tname, desc)
        bins = [sum(1 for e in me if (e <= k if mode == "upper" else e < k)) for k in mk]
        want_perm, want_offsets = brute_force(bins, m)
        got_bins, got_m = partition_bins(keys, edges, tname, mode, desc, num)
        assert got_m == m and got_bins.tolist() == bins, (tname, mode, desc, m, n, num)
        perm, offsets = partition_reference(keys, edges, tname, mode, desc, num)
        assert perm.dtype == np.int64 and offsets.dtype == np.int64
        assert np.array_equal(perm, want_perm) and np.array_equal(offsets, want_offsets), (tname, mode, desc, m, n, num)
        assert offsets[0] == 0 and offsets[m + 1] == N and offsets.size == m + 2
        assert np.array_equal(np.diff(offsets), bin_reference(keys, edges, tname, mode, desc, num))


@pytest.mark.parametrize("tname", ["u8", "i8", "u16", "i32", "u32", "i64", "u64"])
def test_index_mode_against_a_loop(tname):
    rng = np.random.default_rng(3)
    dt = np.dtype(INT_DTYPES[tname])
    info = np.iinfo(dt)
    for m in (0, 1, 5, 200):
        v = rng.integers(max(info.min, -3), min(info.max, 2 * m + 3), 90, endpoint=True).astype(dt)
        v[:4] = [info.min, info.max, 0, min(info.max, m)]
        for num in (None, 0, 41, 500):
            N = v.size if num is None else min(num, v.size)
            bins = [x if 0 <= x < m else m for x in v[:N].tolist()]
            want_perm, want_offsets = brute_force(bins, m)
            perm, offsets = partition_reference(v.view(np.uint8), m, tname, "index", False, num)
            assert np.array_equal(perm, want_perm) and np.array_equal(offsets, want_offsets), (tname, m, num)
            assert np.array_equal(np.diff(offsets), bin_reference(v.view(np.uint8), m, tname, "index", False, num))


def test_expected_columns_leave_the_tail_untouched():
    rows = np.arange(12, dtype=np.uint8)
    perm = np.array([2, 0], dtype=np.int64)
    assert expected_rows(rows, 3, perm, 4).tolist() == [6, 7, 8, 0, 1, 2] + [0xA5] * 6
    assert expected_index(perm, 4, 3).view("<i4").tolist() == [2, 0, np.frombuffer(b"\xa5" * 4, dtype="<i4")[0]]
    assert expected_index(perm, 8, 2).view("<i8").tolist() == [2, 0]
