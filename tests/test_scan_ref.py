"""The scan-by-key reference (tests/scan_ref.py) against a plain Python loop, and the condition the GPU matrix's float
inputs must meet (no GPU)."""
import numpy as np
import pytest

import radix_sort_amd as rs
import util
from reduce_ref import FLOAT, MAX, MIN, SUM, float_order, value_dtype
from scan_cases import COMBINATIONS, FIRST, KEY_TYPES, OPS, VALUE_NAMES, VALUE_TYPES, combination_id, ids_for, matrix_inputs, pairs_of, values_of
from scan_ref import first_value, scan_reference
from test_gpu_unique import SHAPES, keys_of


def loop_scan(keys_raw, kb, vals, vkind, op, exclusive, first, runs):
    """The definition, row by row: the state of every open group in a dict (grouped) or one variable (runs)."""
    n = vals.size
    dt = vals.dtype
    keys = [bytes(keys_raw[i * kb:(i + 1) * kb]) for i in range(n)]

    def combine(a, b):
        if op == SUM:
            with np.errstate(over="ignore"):
                return dt.type(a + b)
        if vkind == FLOAT:
            u = "<u" + str(dt.itemsize)
            a_less = float_order(np.array([a], dtype=dt).view(u))[0] < float_order(np.array([b], dtype=dt).view(u))[0]
        else:
            a_less = a < b
        return a if (op == MIN) == bool(a_less) else b

    out = np.empty(n, dtype=dt)
    state, heads = {}, 0
    for q in range(n):
        k = keys[q]
        if runs and (q == 0 or keys[q - 1] != k):
            state = {}
        if k not in state:
            heads += 1
            prev = None
        else:
            prev = state[k]
        incl = vals[q] if prev is None else combine(prev, vals[q])
        out[q] = (first if prev is None else prev) if exclusive else incl
        state[k] = incl
    return out, heads


@pytest.mark.parametrize("runs", [False, True])
@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("op", OPS)
def test_reference_equals_the_plain_loop(op, exclusive, runs):
    rng = np.random.default_rng(100 + op * 4 + exclusive * 2 + runs)
    for tname in ("u8", "f32", "i64", "u128"):
        kb, kind = util.TYPES[tname][2], util.TYPES[tname][3]
        for vname in VALUE_NAMES:
            vb, vkind = VALUE_TYPES[vname]
            dt = value_dtype(vb, vkind)
            first = first_value(FIRST, dt)
            for n, shape in ((1, "equal"), (2, "seven"), (17, "seven"), (40, "third"), (40, "long_run"), (33, "equal"), (40, "distinct")):
                keys_raw = keys_of(tname, ids_for(shape, n, 8, rng, runs))
                vals = values_of(vname, n, rng, "a")
                want, heads = loop_scan(keys_raw, kb, vals, vkind, op, exclusive, first, runs)
                ref = scan_reference(keys_raw, kb, kind, vals.view(np.uint8), vb, vkind, op, exclusive, FIRST, runs)
                got = ref.values if ref.values is not None else ref.exact  # (form (a): every partial sum is exact)
                tag = (tname, vname, n, shape)
                assert ref.num == heads, tag
                if ref.values is None:  # a zero may carry either sign
                    assert np.array_equal(got.view(dt), want) and np.array_equal(np.signbit(got.view(dt))[~ref.free], np.signbit(want)[~ref.free]), tag
                    assert np.all(np.abs(want.astype(np.longdouble) - ref.sums) <= ref.bound), tag
                else:
                    assert np.array_equal(got, want.view(np.uint8)), tag
    # the count form: ranks
    keys_raw = keys_of("u32", ids_for("seven", 40, 8, rng, runs))
    ones = np.ones(40, dtype="<i8")
    want, _h = loop_scan(keys_raw, 4, ones, 1, SUM, exclusive, np.int64(0), runs)
    ref = scan_reference(keys_raw, 4, 0, None, 8, 1, SUM, exclusive, 0, runs)
    assert np.array_equal(ref.values.view("<i8"), want) and np.array_equal(ref.rank + (0 if exclusive else 1), want)


def test_the_two_group_rules_differ_where_they_must():
    keys = np.array([5, 5, 9, 5, 5], dtype="<u4")
    vals = np.array([1, 2, 4, 8, 16], dtype="<i4")
    grouped = scan_reference(keys.view(np.uint8), 4, 0, vals.view(np.uint8), 4, 1, SUM, False, 0, False)
    lying = scan_reference(keys.view(np.uint8), 4, 0, vals.view(np.uint8), 4, 1, SUM, False, 0, True)
    assert list(grouped.values.view("<i4")) == [1, 3, 4, 11, 27] and grouped.num == 2
    assert list(lying.values.view("<i4")) == [1, 3, 4, 8, 24] and lying.num == 3
    excl = scan_reference(keys.view(np.uint8), 4, 0, vals.view(np.uint8), 4, 1, MAX, True, 0xFFFFFFFF80000000, False)
    assert list(excl.values.view("<i4")) == [-2 ** 31, 1, -2 ** 31, 2, 8]


def test_the_thinning_rule_covers_what_it_must():
    full = len(KEY_TYPES) * len(VALUE_NAMES) * len(OPS) * 2 * 2
    assert len(COMBINATIONS) * 2 >= full
    assert {(t, v) for t, v, _o, _x, _r, _c in COMBINATIONS} == {(t, v) for t in KEY_TYPES for v in VALUE_NAMES}
    assert {(v, o, x) for _t, v, o, x, _r, _c in COMBINATIONS} == {(v, o, x) for v in VALUE_NAMES for o in OPS for x in (False, True)}
    assert {(t, r) for t, _v, _o, _x, r, _c in COMBINATIONS} == {(t, r) for t in KEY_TYPES for r in (False, True)}
    for vb in (4, 8):
        for runs in (False, True):
            seen = {}
            for _t, v, _o, _x, r, c in COMBINATIONS:
                if VALUE_TYPES[v][0] == vb and r == runs:
                    for pair in pairs_of(c):
                        seen[pair] = seen.get(pair, 0) + 1
            assert set(seen) == {(s, shape) for s in range(7) for shape in SHAPES}
            assert min(seen.values()) >= 3, (vb, runs, seen)


FLOAT_SUMS = [cmb for cmb in COMBINATIONS if VALUE_TYPES[cmb[1]][1] == FLOAT and cmb[2] == SUM]


@pytest.mark.parametrize("tname,vname,op,exclusive,runs,c", FLOAT_SUMS, ids=[combination_id(*cmb) for cmb in FLOAT_SUMS])
def test_at_most_one_entry_in_twenty_has_a_zero_of_free_sign(tname, vname, op, exclusive, runs, c):
    """A condition on the generator, not a measurement: the entries of a form (a) float sum that are compared as numbers
    (an exact prefix of zero whose values are not all -0.0) are at most 1 in 20 of every (size, shape) the GPU matrix runs."""
    kb, kind = util.TYPES[tname][2], util.TYPES[tname][3]
    vb, vkind = VALUE_TYPES[vname]
    for n, shape, _T, keys_raw, vals in matrix_inputs(rs, tname, vname, op, runs, c):
        ref = scan_reference(keys_raw, kb, kind, vals["a"].view(np.uint8), vb, vkind, op, exclusive, FIRST, runs)
        free = int(ref.free.sum())
        print(tname, vname, n, shape, "entries", n, "with a zero of free sign", free)
        assert free * 20 <= n, (n, shape, free)
