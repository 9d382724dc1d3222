"""The reference of the order-statistics tests against a brute-force count (no GPU): for every rank r exactly r elements
precede element p[r] in (mapped key, position) order; and quantile_ranks against numpy.quantile."""
import numpy as np
import pytest

import util
from pairs_ref import mapped_columns
from select_ref import quantile_ranks, select_reference

KEY_TYPES = [t for t in util.PRIMS if util.TYPES[t][0] == util.TYPES[t][2]]  # the element is its key: widths 1, 2, 4, 8, 16
F32_SPECIALS = np.array([0x7FC00000, 0xFFC00000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3F800000, 0xBF800000,
                         0x00000000, 0x80000000, 0x7FC00000], dtype="<u4")
F64_SPECIALS = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x0, 0x8000000000000000, 0x7FF0000000000000,
                         0xFFF0000000000000, 0x3FF0000000000000, 0xBFF0000000000000, 0x0, 0x8000000000000000], dtype="<u8")


def _mapped_ints(raw, kb, kind, desc):
    cols = mapped_columns(raw, kb, kind, desc)
    return [int.from_bytes(bytes(row), "little") for row in cols]


def _brute_check(raw, kb, kind, desc):
    n = raw.size // kb
    m = _mapped_ints(raw, kb, kind, desc)
    ranks = list(range(n))
    keys, pos = select_reference(raw, kb, kind, ranks, desc)
    assert sorted(pos.tolist()) == ranks  # a permutation
    for r in ranks:
        i = int(pos[r])
        before = sum(1 for j in range(n) if (m[j], j) < (m[i], i))
        assert before == r, (r, i)
        assert bytes(keys[r]) == bytes(raw.reshape(n, kb)[i])


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("dist", ["uniform", "two", "equal"])
@pytest.mark.parametrize("tname", KEY_TYPES)
def test_reference_against_a_brute_force_count(tname, dist, desc):
    _es, _ko, kb, kind = util.TYPES[tname]
    _brute_check(util.make_input(tname, 37, dist, 5), kb, kind, desc)


@pytest.mark.parametrize("desc", [False, True])
def test_float_specials(desc):
    _brute_check(np.ascontiguousarray(F32_SPECIALS).view(np.uint8), 4, util.FLOAT, desc)
    _brute_check(np.ascontiguousarray(F64_SPECIALS).view(np.uint8), 8, util.FLOAT, desc)
    # the total order on bit patterns: -NaN < -inf < -1 < -0 < +0 < 1 < +inf < +NaN
    keys, pos = select_reference(np.ascontiguousarray(F32_SPECIALS).view(np.uint8), 4, util.FLOAT, [0, 10], False)
    assert keys.view("<u4").reshape(-1).tolist() == [0xFFC00000, 0x7FC00000] and pos.tolist() == [1, 10]


def test_ranks_may_repeat_and_be_empty():
    raw = util.make_input("u16", 20, "uniform", 1)
    keys, pos = select_reference(raw, 2, util.UNSIGNED, [7, 0, 7], True)
    assert pos[0] == pos[2] and keys.shape == (3, 2)
    keys, pos = select_reference(raw, 2, util.UNSIGNED, [], False)
    assert keys.shape == (0, 2) and pos.shape == (0,)


@pytest.mark.parametrize("method", ["lower", "higher", "nearest"])
@pytest.mark.parametrize("n", [1, 2, 5, 10, 101])
def test_quantile_ranks_against_numpy(n, method):
    rng = np.random.default_rng(n)
    x = rng.permutation(n).astype(np.float64) * 1.5 + 0.25  # distinct floats
    q = [0.0, 1.0, 0.5, 0.25, 0.1, 0.9, 0.3333, 0.125, 0.875] + rng.random(8).tolist()
    ranks = quantile_ranks(n, q, method)
    want = np.quantile(x, q, method=method)
    assert np.array_equal(np.sort(x)[ranks], want)
