"""The reference of the GPU tests of rsx_reduce_by_key_device (tests/reduce_ref.py) against a plain Python loop over a
dict of lists, and by hand (no GPU)."""
import struct
from fractions import Fraction

import numpy as np
import pytest

import util
from reduce_ref import FLOAT, MAX, MIN, SIGNED, SUM, UNIT_ROUNDOFF, UNSIGNED, float_order, float_unorder, reduce_reference, value_dtype

KEY_TYPES = ["u8", "i16", "u32", "f32", "i64", "u128"]
VALUE_TYPES = [(4, SIGNED), (4, UNSIGNED), (4, FLOAT), (8, SIGNED), (8, UNSIGNED), (8, FLOAT)]
OPS = [SUM, MIN, MAX]


def _key_order(raw_key: bytes, kind: int, desc: bool) -> int:
    """A Python int that orders raw keys as the library does: sign flip, float total order; complemented for descending."""
    bits = 8 * len(raw_key)
    x = int.from_bytes(raw_key, "little")
    top = 1 << (bits - 1)
    if kind == util.SIGNED:
        x ^= top
    elif kind == util.FLOAT:
        x = x ^ ((1 << bits) - 1) if x & top else x | top
    return (1 << bits) - 1 - x if desc else x


def _float_total(bits_value: int, vb: int) -> int:
    top = 1 << (8 * vb - 1)
    return bits_value ^ ((1 << 8 * vb) - 1) if bits_value & top else bits_value | top


def _loop(keys_raw, kb, kind, vals, vb, vkind, op, desc):
    """{key bytes: [values in input order]} -> (keys in order, per group: the reduced value as a Python int of its bits,
    or for a float SUM the exact Fraction and the Fraction of sum|v|), nothing shared with the reference."""
    groups = {}
    for i in range(len(vals)):
        groups.setdefault(bytes(keys_raw[i * kb:(i + 1) * kb]), []).append(vals[i])
    order = sorted(groups, key=lambda k: _key_order(k, kind, desc))
    out = []
    for k in order:
        vs = groups[k]
        if vkind != FLOAT:
            ints = [int(v) for v in vs]
            r = sum(ints) if op == SUM else min(ints) if op == MIN else max(ints)
            out.append(r % (1 << 8 * vb))  # the bits: a sum wraps, a negative value is its two's complement
        elif op != SUM:
            bits = [int(np.array(v).view("<u" + str(vb))) for v in vs]
            pick = min if op == MIN else max
            out.append(pick(bits, key=lambda b: _float_total(b, vb)))
        else:
            out.append((sum(Fraction(float(v)) for v in vs), sum(abs(Fraction(float(v))) for v in vs), len(vs)))
    return order, out


def _values(vb, vkind, n, rng, form):
    dt = value_dtype(vb, vkind)
    if vkind != FLOAT:
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, size=n, dtype=dt, endpoint=True)
    if form == "small":  # integers in [-8, 8]: every partial sum is exact
        return rng.integers(-8, 9, size=n).astype(dt)
    return (rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, size=n))).astype(dt)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("vt", VALUE_TYPES)
@pytest.mark.parametrize("tname", KEY_TYPES)
def test_reference_equals_a_python_loop(tname, vt, op, desc):
    kb, kind = util.TYPES[tname][2], util.TYPES[tname][3]
    vb, vkind = vt
    rng = np.random.default_rng(kb * 100 + vb * 10 + vkind * 3 + op)
    for n, dist in ((1, "uniform"), (37, "two"), (300, "step16"), (300, "uniform")):
        keys_raw = util.make_input(tname, n, dist, seed=n + kb)
        for form in (("small", "normal") if vkind == FLOAT else ("full",)):
            vals = _values(vb, vkind, n, rng, form)
            ref = reduce_reference(keys_raw, kb, kind, vals.view(np.uint8), vb, vkind, op, desc)
            order, want = _loop(keys_raw, kb, kind, vals, vb, vkind, op, desc)
            assert ref.m == len(order) and ref.offsets.shape == (ref.m + 1,)
            assert bytes(ref.keys) == b"".join(order)
            assert [int(x) for x in np.diff(ref.offsets)] == [sum(1 for i in range(n) if bytes(keys_raw[i * kb:(i + 1) * kb]) == k) for k in order]
            if not (vkind == FLOAT and op == SUM):
                assert ref.exact is None and ref.sums is None and ref.bound is None
                assert [int(x) for x in ref.values.view("<u" + str(vb))] == want
                continue
            assert ref.values is None
            dt = value_dtype(vb, vkind)
            u = Fraction(UNIT_ROUNDOFF[vb])
            for j, (s, a, c) in enumerate(want):
                if form == "small":  # exactly representable: the reference's `exact` IS the sum
                    assert Fraction(float(ref.exact.view(dt)[j])) == s
                gamma = (c - 1) * u / (1 - (c - 1) * u)
                # longdouble sums of at most 300 values: far inside 2^-60 of sum|v|
                assert abs(Fraction(float(ref.sums[j])) - s) <= a * Fraction(1, 2 ** 50)
                assert abs(Fraction(float(ref.abs_sums[j])) - a) <= a * Fraction(1, 2 ** 50)
                assert abs(Fraction(float(ref.bound[j])) - gamma * a) <= gamma * a * Fraction(1, 2 ** 40)
                assert (c == 1) == (ref.bound[j] == 0)


def test_integer_sums_wrap_and_compare_by_signedness():
    keys = np.array([5, 5, 9, 9, 9], dtype="<u4").view(np.uint8)
    for vb in (4, 8):
        top = 1 << (8 * vb - 1)
        s = np.array([top - 1, 1, -top, -1, 3], dtype="<i" + str(vb))  # max + 1 wraps to min; min - 1 wraps to max, and + 3 wraps back
        ref = reduce_reference(keys, 4, UNSIGNED, s.view(np.uint8), vb, SIGNED, SUM, False)
        assert ref.values.view("<i" + str(vb)).tolist() == [-top, -top + 2]
        u = s.view("<u" + str(vb))
        ref = reduce_reference(keys, 4, UNSIGNED, u.view(np.uint8), vb, UNSIGNED, SUM, False)
        assert [int(x) for x in ref.values.view("<u" + str(vb))] == [top, (top + (2 * top - 1) + 3) % (2 * top)]
        # the same bits: -1 is the largest unsigned value and below every signed one but the minimum
        assert reduce_reference(keys, 4, UNSIGNED, s.view(np.uint8), vb, SIGNED, MAX, False).values.view("<i" + str(vb)).tolist() == [top - 1, 3]
        assert [int(x) for x in reduce_reference(keys, 4, UNSIGNED, u.view(np.uint8), vb, UNSIGNED, MAX, False).values.view("<u" + str(vb))] == \
            [top - 1, 2 * top - 1]
        assert reduce_reference(keys, 4, UNSIGNED, s.view(np.uint8), vb, SIGNED, MIN, False).values.view("<i" + str(vb)).tolist() == [1, -top]
        assert [int(x) for x in reduce_reference(keys, 4, UNSIGNED, u.view(np.uint8), vb, UNSIGNED, MIN, False).values.view("<u" + str(vb))] == [1, 3]


F32 = {"-nan": 0xFFC00000, "-inf": 0xFF800000, "-0": 0x80000000, "+0": 0x00000000, "+inf": 0x7F800000, "nan": 0x7FC00000,
       "nan1": 0x7FC00001, "1": 0x3F800000, "-1": 0xBF800000}


def test_float_min_and_max_follow_the_total_order():
    names = ["-nan", "-inf", "-1", "-0", "+0", "1", "+inf", "nan", "nan1"]  # ascending in the total order
    bits = np.array([F32[x] for x in names], dtype="<u4")
    o = float_order(bits)
    assert np.all(np.diff(o.astype(np.int64)) > 0) and np.array_equal(float_unorder(o), bits)
    rng = np.random.default_rng(1)
    for lo in range(len(names)):
        for hi in range(lo, len(names)):
            vals = rng.permutation(bits[lo:hi + 1])
            keys = np.zeros(vals.size, dtype="<u2").view(np.uint8)
            assert reduce_reference(keys, 2, UNSIGNED, vals.view(np.uint8), 4, FLOAT, MIN, False).values.view("<u4").tolist() == [F32[names[lo]]]
            assert reduce_reference(keys, 2, UNSIGNED, vals.view(np.uint8), 4, FLOAT, MAX, True).values.view("<u4").tolist() == [F32[names[hi]]]
    d = np.array([0x8000000000000000, 0x0, 0xFFF8000000000000, 0x7FF8000000000001], dtype="<u8")  # -0.0, +0.0, -NaN, NaN'
    keys = np.array([1, 1, 2, 2], dtype="<i8").view(np.uint8)
    assert reduce_reference(keys, 8, SIGNED, d.view(np.uint8), 8, FLOAT, MIN, False).values.view("<u8").tolist() == [d[0], d[2]]
    assert reduce_reference(keys, 8, SIGNED, d.view(np.uint8), 8, FLOAT, MAX, False).values.view("<u8").tolist() == [d[1], d[3]]


def test_float_sums_of_specials_and_signed_zeros():
    def sums(names, vb=4):
        bits = np.array([F32[x] for x in names], dtype="<u4")
        vals = bits.view("<f4").astype("<f" + str(vb))
        keys = np.zeros(len(names), dtype=np.uint8)
        ref = reduce_reference(keys, 1, UNSIGNED, vals.view(np.uint8), vb, FLOAT, SUM, False)
        assert ref.m == 1
        return ref.exact.view("<f" + str(vb))[0]

    for vb in (4, 8):
        assert sums(["+inf", "1", "-1"], vb) == np.inf
        assert np.isnan(sums(["1", "nan", "-1"], vb))
        assert np.isnan(sums(["+inf", "1", "-inf"], vb))
        z = sums(["-0", "-0", "-0"], vb)
        assert z == 0 and np.signbit(z)  # only a group of -0.0 sums to -0.0
        z = sums(["-0", "+0"], vb)
        assert z == 0 and not np.signbit(z)
        assert struct.pack("<f", sums(["1", "-0"])) == struct.pack("<f", 1.0)


def test_groups_take_their_values_in_input_order():
    keys = np.array([3, 1, 3, 1, 3], dtype="<u4").view(np.uint8)
    vals = np.array([10, 20, 30, 40, 50], dtype="<i4")
    ref = reduce_reference(keys, 4, UNSIGNED, vals.view(np.uint8), 4, SIGNED, SUM, False)
    assert ref.m == 2 and ref.keys.view("<u4").tolist() == [1, 3] and ref.offsets.tolist() == [0, 2, 5]
    assert vals[ref.perm].tolist() == [20, 40, 10, 30, 50] and ref.values.view("<i4").tolist() == [60, 90]
    ref = reduce_reference(keys, 4, UNSIGNED, vals.view(np.uint8), 4, SIGNED, MAX, True)
    assert ref.keys.view("<u4").tolist() == [3, 1] and ref.offsets.tolist() == [0, 3, 5] and ref.values.view("<i4").tolist() == [50, 40]
    empty = reduce_reference(np.zeros(0, np.uint8), 4, UNSIGNED, np.zeros(0, np.uint8), 8, FLOAT, SUM, False)
    assert empty.m == 0 and empty.offsets.tolist() == [0] and empty.exact.size == 0 and empty.values is None
