"""CPU: tests/search_ref.py (the reference of the GPU tests of rsx_search_sorted_device) against an O(n * m) count of the
definition on python integers, against the float specials in their known order, and against numpy.searchsorted."""
import numpy as np
import pytest

import util
from pairs_ref import mapped_columns, pairs_reference
from search_ref import search_reference, tile_routes

KEY_TYPES = ["u8", "u16", "u32", "u64", "u128", "i8", "i16", "i32", "i64", "i128", "f32", "f64"]
F32_SPECIALS = np.array([0xFFC00000, 0xFF800000, 0x80000000, 0x00000000, 0x7F800000, 0x7FC00000, 0x7FC00001], dtype="<u4")
F64_SPECIALS = np.array([0xFFF8000000000000, 0xFFF0000000000000, 0x8000000000000000, 0x0, 0x7FF0000000000000, 0x7FF8000000000000,
                         0x7FF8000000000001], dtype="<u8")  # -NaN, -inf, -0.0, +0.0, +inf, NaN, NaN of another payload


def mapped_ints(raw, tname, desc):
    _es, _ko, kb, kind = util.TYPES[tname]
    return [int.from_bytes(bytes(r), "little") for r in mapped_columns(raw, kb, kind, desc)]


def sorted_haystack(tname, n, dist, seed, desc):
    _es, _ko, kb, kind = util.TYPES[tname]
    return pairs_reference(util.make_input(tname, n, dist, seed), None, kb, kind, 0, desc)[0]


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", KEY_TYPES)
def test_reference_is_the_count_of_the_definition(tname, desc):
    kb = util.TYPES[tname][2]
    for n, m, dist in ((0, 3, "uniform"), (1, 5, "two"), (37, 29, "two"), (41, 33, "lowbyte"), (64, 40, "uniform"), (50, 20, "step16")):
        hay = sorted_haystack(tname, n, dist, 3, desc)
        needles = np.concatenate([util.make_input(tname, m, dist, 4), hay[: kb * min(n, 7)]])  # strangers and members
        lower, upper = search_reference(hay, needles, tname, desc)
        hk, nk = mapped_ints(hay, tname, desc), mapped_ints(needles, tname, desc)
        assert hk == sorted(hk)
        assert lower.tolist() == [sum(1 for h in hk if h < k) for k in nk]
        assert upper.tolist() == [sum(1 for h in hk if h <= k) for k in nk]
        for num in (0, n // 2, n + 5):
            lo2, up2 = search_reference(hay, needles, tname, desc, num=num)
            assert lo2.tolist() == [sum(1 for h in hk[:num] if h < k) for k in nk]
            assert up2.tolist() == [sum(1 for h in hk[:num] if h <= k) for k in nk]


@pytest.mark.parametrize("tname", ["f32", "f64"])
def test_float_specials_are_seven_keys_in_the_total_order(tname):
    sp = (F32_SPECIALS if tname == "f32" else F64_SPECIALS)
    asc = sp.view(np.uint8).reshape(-1).copy()
    lower, upper = search_reference(asc, asc, tname, False)
    assert lower.tolist() == list(range(7)) and upper.tolist() == list(range(1, 8))
    desc = sp[::-1].copy().view(np.uint8).reshape(-1)
    lower, upper = search_reference(desc, asc, tname, True)
    assert lower.tolist() == list(range(6, -1, -1)) and upper.tolist() == list(range(7, 0, -1))
    with pytest.raises(AssertionError):
        search_reference(desc, asc, tname, False)  # the wrong order is noticed
    twice = np.repeat(sp, 2).view(np.uint8).reshape(-1)
    lower, upper = search_reference(twice, asc, tname, False)
    assert lower.tolist() == list(range(0, 14, 2)) and upper.tolist() == list(range(2, 16, 2))


@pytest.mark.parametrize("tname", ["u8", "u16", "u32", "u64", "i8", "i16", "i32", "i64"])
def test_integers_equal_numpy_searchsorted(tname):
    dt = np.dtype("<" + tname[0] + str(util.TYPES[tname][2]))
    rng = np.random.default_rng(7)
    info = np.iinfo(dt)
    span_lo, span_hi = max(info.min, -300), min(info.max, 300)
    hay = np.sort(rng.integers(span_lo, span_hi, size=500, endpoint=True).astype(dt))
    needles = np.concatenate([rng.integers(span_lo, span_hi, size=200, endpoint=True).astype(dt), np.array([info.min, info.max], dtype=dt)])
    lower, upper = search_reference(hay.view(np.uint8), needles.view(np.uint8), tname, False)
    assert np.array_equal(lower, np.searchsorted(hay, needles, side="left"))
    assert np.array_equal(upper, np.searchsorted(hay, needles, side="right"))
    rev = hay[::-1].copy()
    lower, upper = search_reference(rev.view(np.uint8), needles.view(np.uint8), tname, True)
    assert np.array_equal(lower, hay.size - np.searchsorted(hay, needles, side="right"))
    assert np.array_equal(upper, hay.size - np.searchsorted(hay, needles, side="left"))


def test_tile_routes_restates_the_window_rule():
    hay = np.arange(100, dtype="<u4")
    raw = hay.view(np.uint8)
    # ordered needles, tiles of 10: each tile spans exactly 10 keys
    assert tile_routes(raw, raw, "u32", False, 10, 10, False).tolist() == [True] * 10
    assert tile_routes(raw, raw, "u32", False, 10, 9, False).tolist() == [False] * 10
    # a short last tile takes its own needles only
    assert tile_routes(raw, raw[: 4 * 25], "u32", False, 10, 5, False).tolist() == [False, False, True]
    shuffled = np.random.default_rng(1).permutation(hay).astype("<u4").view(np.uint8)
    assert not tile_routes(raw, shuffled, "u32", False, 10, 20, False).any()
    assert tile_routes(raw, shuffled, "u32", False, 10, 10, True).all()
    # strangers outside the haystack: an empty window
    far = np.array([1000, 2000, 3000], dtype="<u4").view(np.uint8)
    assert tile_routes(raw, far, "u32", False, 10, 0, False).tolist() == [True]
    # a run of equal keys longer than the window
    ones = np.ones(50, dtype="<u4").view(np.uint8)
    assert tile_routes(ones, ones[:8], "u32", False, 10, 49, False).tolist() == [False]
    assert tile_routes(ones, ones[:8], "u32", False, 10, 49, False, num=49).tolist() == [True]
