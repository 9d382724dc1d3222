"""CPU: the numpy model of the direct bucket kernel's two steps (bucket_direct_ref) against np.sort -- an unstable counting
pass on B bits with a random order inside every sub-bucket, then the windowed rank."""
import numpy as np
import pytest

import bucket_direct_ref as ref

CAPE = 1024 * 17  # what the 1024-thread form holds of 8-byte elements


def _check(low, b_lo, B, seed=0):
    low = np.asarray(low, dtype=np.uint64)
    for s in range(2):  # two arrival orders
        out = ref.sort_bucket(low, b_lo, B, np.random.default_rng(seed + s))
        assert out is not None
        assert np.array_equal(out, np.sort(low))


@pytest.mark.parametrize("B", [12, 11, 10])
@pytest.mark.parametrize("n", [1, 2, 1000, CAPE - 1, CAPE])
def test_uniform_keys(B, n):
    n = n >> (12 - B)  # (the smaller forms hold a half and a quarter)
    rng = np.random.default_rng(n + B)
    _check(rng.integers(0, 1 << 48, size=max(n, 1), dtype=np.uint64), 48, B)


def test_runs_of_equal_keys_up_to_the_limit():
    rng = np.random.default_rng(5)
    dig = rng.permutation(4096)[:700].astype(np.uint64)  # every run in a sub-bucket of its own
    val = (dig << np.uint64(36)) | rng.integers(0, 1 << 36, size=700, dtype=np.uint64)
    low = np.repeat(val, 1 + np.arange(700) % ref.LIMIT)
    assert ref.largest_sub_bucket(low, 48, 12) == ref.LIMIT
    _check(rng.permutation(low), 48, 12)


def test_all_keys_equal_and_the_limit():
    assert ref.sort_bucket(np.full(5000, 77, dtype=np.uint64), 48, 12, np.random.default_rng(0)) is None  # handed over
    _check(np.full(ref.LIMIT, 77, dtype=np.uint64), 48, 12)
    rng = np.random.default_rng(6)
    base = rng.integers(0, 1 << 48, size=9000, dtype=np.uint64)
    base = base[((base >> np.uint64(36)) != np.uint64(99))]
    for extra, direct in ((ref.LIMIT, True), (ref.LIMIT + 1, False)):
        sub = (np.uint64(99) << np.uint64(36)) | rng.integers(0, 1 << 36, size=extra, dtype=np.uint64)  # one sub-bucket, distinct keys
        low = rng.permutation(np.concatenate([base, sub]))
        assert (ref.largest_sub_bucket(low, 48, 12) <= ref.LIMIT) == direct
        out = ref.sort_bucket(low, 48, 12, np.random.default_rng(1))
        assert (out is not None) == direct
        if direct:
            assert np.array_equal(out, np.sort(low))


@pytest.mark.parametrize("b_lo,B", [(8, 12), (8, 10), (3, 12), (24, 12), (20, 11), (40, 12)])
def test_few_bits_below_the_window(b_lo, B):
    rng = np.random.default_rng(b_lo * 100 + B)
    n = min(2000, (1 << b_lo) * 8)
    low = rng.integers(0, 1 << b_lo, size=n, dtype=np.uint64)
    if ref.largest_sub_bucket(low, b_lo, B) > ref.LIMIT:
        assert ref.sort_bucket(low, b_lo, B, rng) is None
    else:
        _check(low, b_lo, B)
    _check(low[:16], b_lo, B)


def test_rank_identity_on_any_array():
    """With T = n the rank is exact whatever the arrangement (no counting pass at all: one sub-bucket)."""
    rng = np.random.default_rng(9)
    s = rng.integers(0, 50, size=300, dtype=np.uint64)
    rank = ref.windowed_rank(s, np.array([0, 300]), 0, 12, block=64)
    out = np.empty_like(s)
    out[rank] = s
    assert np.array_equal(np.sort(rank), np.arange(300)) and np.array_equal(out, np.sort(s))


def test_handed_over_is_sticky_per_workgroup():
    counts = np.zeros(65536, dtype=np.int64)
    largest = np.zeros(65536, dtype=np.int64)
    grid = 256
    for k in range(5):  # workgroup 8: the second bucket has a crowded sub-bucket
        counts[8 + k * grid], largest[8 + k * grid] = 10000, 33 if k == 1 else 12
    counts[9], largest[9] = 10000, 12            # workgroup 9: nothing handed over ...
    counts[9 + grid], largest[9 + grid] = 20000, 40  # ... but a bucket above cape(), which is not sticky
    counts[9 + 2 * grid], largest[9 + 2 * grid] = 10000, 12
    assert ref.handed_over(counts, largest, CAPE, grid) == 4 + 1
    assert ref.handed_over(counts, largest, CAPE, grid, everything=True) == 8
