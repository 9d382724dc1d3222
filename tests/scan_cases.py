"""Inputs and the case matrix of the scan-by-key tests (test_scan_ref.py on the CPU, test_gpu_scan.py); a helper, no tests.

Sizes come from rsx_scan_by_key_caps (T = tile, S = scan_span): 1, 2, T - 1, T, T + 1, 3T + 5 and S*T + T + 3 (the scan's
second sweep).  Shapes are the seven of test_gpu_unique.group_ids: permuted as given for the grouped form, UNPERMUTED for
the runs form -- there "seven" and "third" are random ids in input order, so the same key starts many separate runs (the
case that tells the two group rules apart), while the other shapes lie as runs.

Values.  Integers: uniform over the whole range of the type, so sums wrap.  Floats, form (a): nonzero integers in [-8, 8]
as floats (one in eight negative) and, in arrays of 64 entries and more, now and then a -0.0 or +0.0 -- every partial sum is
exact in any association, so results are compared as bytes but for the entries scan_ref marks `free` (an exact prefix of
zero whose values are not all -0.0), at most 1 in 20 of the entries of every case (test_scan_ref.py holds the generator to
that).  Form (b): standard normal values times 2^k, k uniform in [-20, 20], compared inside the bound.

The matrix.  Key types u8 i16 u32 f32 i64 u128 (index k), value types i32 u32 f32 i64 u64 f64 (v), ops sum min max (o),
inclusive / exclusive (x), grouped / runs (r): the THINNING RULE keeps the combination when k + v + o + x + r is even, 216
of the 432.  Fixing any two (or three) of the five indices leaves both parities reachable through the others, so every
(key width, value type), every (value type, op, exclusive) and both group rules of every key width are kept.  The 49
(size, shape) pairs are numbered p = 7 * size index + shape index; the c-th kept combination OF ITS VALUE WIDTH AND GROUP
RULE (c = 0 .. 53) runs the pairs with (p + c) % 16 == 0, three or four each: c takes every residue modulo 16 at least
three times, so every size with every shape runs at least three times per value width and group rule."""
import numpy as np

import util
from reduce_ref import FLOAT, MAX, MIN, SIGNED, SUM, UNSIGNED, value_dtype
from test_gpu_unique import SHAPES, group_ids, keys_of

KEY_TYPES = ["u8", "i16", "u32", "f32", "i64", "u128"]
VALUE_TYPES = {"i32": (4, SIGNED), "u32": (4, UNSIGNED), "f32": (4, FLOAT), "i64": (8, SIGNED), "u64": (8, UNSIGNED), "f64": (8, FLOAT)}
VALUE_NAMES = list(VALUE_TYPES)
OPS = [SUM, MIN, MAX]
OP_NAMES = {SUM: "sum", MIN: "min", MAX: "max"}
FIRST = 0x5A5A5A5A5A5A5A5A  # what exclusive calls store at the heads: no identity of any operator, so a combined `first` shows


class _AsTheyLie:
    """A generator whose permutation leaves the array as it is: group_ids without its last step."""

    def __init__(self, rng):
        self.rng = rng

    def integers(self, *a, **kw):
        return self.rng.integers(*a, **kw)

    def permutation(self, x):
        return x


def ids_for(shape, n, T, rng, runs):
    return group_ids(shape, n, T, _AsTheyLie(rng) if runs else rng)


def sizes_for(rs, kb, vb, runs):
    T, S = rs.scan_by_key_caps(kb, vb, runs)
    return [1, 2, T - 1, T, T + 1, 3 * T + 5, S * T + T + 3]


def values_of(vname, n, rng, form):
    vb, vkind = VALUE_TYPES[vname]
    dt = value_dtype(vb, vkind)
    if vkind != FLOAT:
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, size=n, dtype=dt, endpoint=True)
    if form == "a":
        v = rng.integers(1, 9, size=n).astype(dt)
        v[rng.random(n) < 0.125] *= -1
        if n >= 64:
            zero = rng.random(n) < 1.0 / 64
            v[zero] = np.where(rng.random(int(zero.sum())) < 0.5, dt.type(-0.0), dt.type(0.0))
        return v
    assert form == "b"
    return (rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, size=n))).astype(dt)


def kept_combinations():
    out, count = [], {}
    for k, tname in enumerate(KEY_TYPES):
        for v, vname in enumerate(VALUE_NAMES):
            for o, op in enumerate(OPS):
                for x in (0, 1):
                    for r in (0, 1):
                        if (k + v + o + x + r) % 2:
                            continue
                        slot = (VALUE_TYPES[vname][0], r)
                        c = count.get(slot, 0)
                        count[slot] = c + 1
                        out.append((tname, vname, op, bool(x), bool(r), c))
    return out


COMBINATIONS = kept_combinations()


def combination_id(t, v, o, x, r, _c):
    return f"{t}-{v}-{OP_NAMES[o]}-{'excl' if x else 'incl'}-{'runs' if r else 'grouped'}"


def pairs_of(c):
    """The (size index, shape) pairs the c-th combination of its slot runs."""
    return [(p // 7, SHAPES[p % 7]) for p in range(49) if (p + c) % 16 == 0]


def seed_of(c, vb, runs):
    return 2000 + c * 4 + (2 if vb == 8 else 0) + (1 if runs else 0)


def matrix_inputs(rs, tname, vname, op, runs, c):
    """Yields (n, shape, T, keys_raw, {form: values}) of one combination, from its own seeded generator: the GPU matrix and
    the CPU check of the 1-in-20 condition see the same arrays."""
    kb = util.TYPES[tname][2]
    vb, vkind = VALUE_TYPES[vname]
    T = rs.scan_by_key_caps(kb, vb, runs)[0]
    sizes = sizes_for(rs, kb, vb, runs)
    rng = np.random.default_rng(seed_of(c, vb, runs))
    for si, shape in pairs_of(c):
        n = sizes[si]
        keys_raw = keys_of(tname, ids_for(shape, n, T, rng, runs))
        forms = ("a", "b") if (vkind == FLOAT and op == SUM) else ("a",) if vkind == FLOAT else (None,)
        yield n, shape, T, keys_raw, {form: values_of(vname, n, rng, form) for form in forms}
