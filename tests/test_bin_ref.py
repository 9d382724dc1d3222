"""CPU: tests/bin_ref.py against a brute-force double loop over mapped keys, and against numpy.histogram on plain floats,
which pins the relation radix_histogram's docstring states."""
import numpy as np
import pytest

import util
from bin_ref import INT_DTYPES, bin_reference
from pairs_ref import mapped_columns

F32_SPECIALS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001],
                        dtype="<u4")  # +NaN, -NaN, a signalling NaN, +0, -0, +inf, -inf, the two smallest denormals


def mapped_ints(raw, tname, desc):
    _es, _ko, kb, kind = util.TYPES[tname]
    return [int.from_bytes(bytes(row), "little") for row in mapped_columns(raw, kb, kind, desc)]


def raw_keys(tname, n, seed):
    """n keys as raw bytes: few distinct values, so that keys meet edges; f32 with every special bit pattern"""
    rng = np.random.default_rng(seed)
    kb = util.TYPES[tname][2]
    if tname == "f32":
        v = rng.integers(-6, 7, n).astype("<f4") / np.float32(2)
        raw = v.view("<u4").copy()
        k = min(n, F32_SPECIALS.size)
        raw[:k] = F32_SPECIALS[:k]
        rng.shuffle(raw)
        return raw.view(np.uint8)
    if tname == "u128":
        raw = np.zeros((n, 16), dtype=np.uint8)
        raw[:, 15] = rng.integers(0, 3, n)  # the top byte and the bottom byte decide
        raw[:, 0] = rng.integers(0, 3, n)
        return raw.reshape(-1)
    lo, hi = (0, 12) if tname[0] == "u" else (-6, 7)
    scale = 1 if kb == 1 else (1 << (8 * kb - 6))  # spread over the width: the sign and the top bits take part
    return (rng.integers(lo, hi, n) * scale).astype(INT_DTYPES[tname]).view(np.uint8)


def sorted_edges(tname, m, seed, desc):
    """m edges drawn like the keys (duplicates included), sorted by mapped key in this order"""
    kb = util.TYPES[tname][2]
    raw = raw_keys(tname, max(m, 9), seed + 1000).reshape(-1, kb)[:m]
    order = sorted(range(m), key=lambda j: mapped_ints(raw.reshape(-1), tname, desc)[j])
    return raw[order].reshape(-1)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("mode", ["upper", "lower"])
@pytest.mark.parametrize("tname", ["u8", "i32", "f32", "i64", "u128"])
def test_reference_against_a_double_loop(tname, mode, desc):
    for m, n, num in ((0, 5, None), (1, 40, None), (9, 70, None), (12, 70, 31), (4, 0, None), (3, 20, 100)):
        keys = raw_keys(tname, n, 7 + m)
        edges = sorted_edges(tname, m, m, desc)
        N = n if num is None else min(num, n)
        mk, me = mapped_ints(keys, tname, desc)[:N], mapped_ints(edges, tname, desc)
        want = np.zeros(m + 1, dtype=np.int64)
        for k in mk:
            want[sum(1 for e in me if (e <= k if mode == "upper" else e < k))] += 1
        got = bin_reference(keys, edges, tname, mode, desc, num)
        assert got.dtype == np.int64 and np.array_equal(got, want), (tname, mode, desc, m, n, num, got, want)
        assert int(got.sum()) == N


def test_float_specials_land_where_the_total_order_puts_them():
    edges = np.array([0xFF800000, 0x80000000, 0x00000000, 0x7F800000], dtype="<u4")  # -inf, -0, +0, +inf: sorted by mapped key
    counts = bin_reference(F32_SPECIALS.view(np.uint8), edges.view(np.uint8), "f32", "upper")
    # below -inf: -NaN | [-inf, -0): -inf, -denormal | [-0, +0): -0 | [+0, +inf): +0, +denormal | from +inf on: +inf, two NaNs
    assert counts.tolist() == [1, 2, 1, 2, 3]
    counts = bin_reference(F32_SPECIALS.view(np.uint8), edges.view(np.uint8), "f32", "lower")
    assert counts.tolist() == [2, 2, 1, 2, 2]


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
            want = np.zeros(m + 1, dtype=np.int64)
            for x in v[:N].tolist():
                want[x if 0 <= x < m else m] += 1
            got = bin_reference(v.view(np.uint8), m, tname, "index", False, num)
            assert np.array_equal(got, want), (tname, m, num)


def test_the_relation_to_numpy_histogram():
    rng = np.random.default_rng(11)
    x = (rng.integers(-20, 21, 500) / 4.0).astype("<f8")
    for edges in (np.array([-3.0, -1.0, 0.25, 2.0, 5.0]), np.array([-5.0, 5.0]), np.linspace(-5.0, 5.0, 41)):
        edges = edges.astype("<f8")
        m = edges.size
        counts = bin_reference(x.view(np.uint8), edges.view(np.uint8), "f64", "upper")
        hist = np.histogram(x, edges)[0]
        last = int((x == edges[-1]).sum())
        assert last > 0  # the exception is exercised
        want = counts[1:m].copy()
        want[-1] += last  # numpy closes its last bin on the right; here those keys are in counts[m]
        assert np.array_equal(hist, want)
        assert counts[0] == int((x < edges[0]).sum()) and counts[m] == int((x >= edges[-1]).sum())  # the two open ends
