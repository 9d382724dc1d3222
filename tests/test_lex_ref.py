"""CPU: tests/lex_ref.py, the reference of the calls on several key columns, pinned two ways at n <= 2000:
against sorted() of plain Python on tuples of mapped keys computed by a second route -- the bytes of
RadixDigits.get_digit, the restatement of radix_digits.rs -- and, for integer columns in ascending order, against
np.lexsort on the native dtypes."""
import numpy as np
import pytest

import util
from lex_ref import columns_reference, lex_reference
from radix_sort_amd import RadixDigits

U, S, F = util.UNSIGNED, util.SIGNED, util.FLOAT
F32 = np.array([0xFFC00000, 0xFF800000, 0x80000000, 0x00000000, 0x7F800000, 0x7FC00000, 0x7FC00001, 0x3F800000, 0xBF800000], dtype="<u4")
F64 = np.array([0xFFF8000000000000, 0xFFF0000000000000, 0x8000000000000000, 0x0, 0x7FF0000000000000, 0x7FF8000000000000,
                0x3FF0000000000000, 0xBFF0000000000000], dtype="<u8")

COLUMN_SETS = {
    "u8,u8": [(1, U), (1, U)],
    "u16,u8": [(2, U), (1, U)],
    "i32,f32": [(4, S), (4, F)],
    "i64,i32": [(8, S), (4, S)],
    "f64,i64": [(8, F), (8, S)],
    "16xu8": [(1, U)] * 16,
    "i64,i64,i32": [(8, S), (8, S), (4, S)],
    "u128,u128,f32": [(16, U), (16, U), (4, F)],
    "i128,i8,f64,u16": [(16, S), (1, S), (8, F), (2, U)],  # 27 bytes: wider than any compound key
}


def draw(rng, n, kb, kind, few):
    """n raw keys (n, kb) uint8: from a handful of values of the type (floats: specials among them), or any bits."""
    if kind == F:
        pool = (F32 if kb == 4 else F64).view(np.uint8).reshape(-1, kb)
        if few:
            return pool[rng.integers(0, 5, size=n)]
        raw = rng.integers(0, 256, size=(n, kb), dtype=np.uint8)
        mix = rng.random(n) < 0.3
        raw[mix] = pool[rng.integers(0, len(pool), size=int(mix.sum()))]
        return raw
    if few:
        pool = rng.integers(0, 256, size=(4, kb), dtype=np.uint8)
        pool[0, -1] |= 0x80  # both signs
        pool[1, -1] &= 0x7F
        return pool[rng.integers(0, 4, size=n)]
    return rng.integers(0, 256, size=(n, kb), dtype=np.uint8)


def mapped_int(raw_row: bytes, kb, kind, desc):
    """The mapped key of one raw key as a Python int, from the digits of RadixDigits.get_digit."""
    d = RadixDigits(kb, 0, kb, kind)
    v = sum(d.get_digit(raw_row, i) << (8 * i) for i in range(kb))
    return ((1 << (8 * kb)) - 1 - v) if desc else v


@pytest.mark.parametrize("few", [True, False])
@pytest.mark.parametrize("pattern", ["asc", "desc", "alt"])
@pytest.mark.parametrize("name", list(COLUMN_SETS))
def test_against_sorted_of_python_tuples(name, pattern, few):
    specs = COLUMN_SETS[name]
    m = len(specs)
    desc = {"asc": [False] * m, "desc": [True] * m, "alt": [j % 2 == 0 for j in range(m)]}[pattern]
    rng = np.random.default_rng(len(name) * 7 + few)
    for n in (0, 1, 2, 37, 700):
        cols = [draw(rng, n, kb, kind, few) for kb, kind in specs]
        got = lex_reference(cols, specs, desc)
        keys = [tuple(mapped_int(cols[j][i].tobytes(), specs[j][0], specs[j][1], desc[j]) for j in range(m)) for i in range(n)]
        want = sorted(range(n), key=lambda i: keys[i])  # sorted() is stable
        assert got.dtype == np.int64 and got.tolist() == want, (name, pattern, few, n)


@pytest.mark.parametrize("dtypes", [("u1", "u1"), ("<u2", "u1"), ("<i8", "<i4"), ("<i8", "<i8", "<i4"), ("<i2", "<u8", "i1", "<u4"), ("<u4",)])
def test_integer_columns_against_numpy_lexsort(dtypes):
    rng = np.random.default_rng(11)
    n = 2000
    specs = [(np.dtype(dt).itemsize, S if np.dtype(dt).kind == "i" else U) for dt in dtypes]
    for few in (True, False):
        cols = [draw(rng, n, kb, kind, few) for kb, kind in specs]
        native = [np.ascontiguousarray(c).view(dt).reshape(n) for c, dt in zip(cols, dtypes)]
        want = np.lexsort(tuple(native[::-1]))  # numpy: the LAST key is the primary one
        got = lex_reference(cols, specs, [False] * len(specs))
        assert np.array_equal(got, want), (dtypes, few)


def test_columns_reference_gathers_rows():
    rng = np.random.default_rng(3)
    specs = [(4, S), (2, U)]
    n = 300
    cols = [draw(rng, n, kb, kind, True) for kb, kind in specs]
    vals = rng.integers(0, 256, size=(n, 6), dtype=np.uint8)
    out, v, perm = columns_reference(cols, specs, [True, False], vals, 6)
    assert sorted(perm.tolist()) == list(range(n))
    for j, (kb, _k) in enumerate(specs):
        assert np.array_equal(out[j].reshape(n, kb), cols[j][perm])
    assert np.array_equal(v.reshape(n, 6), vals[perm])
    assert columns_reference(cols, specs, [True, False])[1] is None
