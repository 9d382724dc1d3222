"""Host side of the calls on several key columns (no GPU): the prototypes and their bindings, rsx_lex_plan -- the plans
include/rsx.h's rule gives for the column sets the GPU tests sort --, the refusals the C calls return without a device,
and the argument errors of radix_lexsort / radix_sort_columns, which are raised before any context exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rsx_lexsort_device": 7, "rsx_sort_columns_device": 7, "rsx_ctx_reserve_lex": 5, "rsx_lex_plan": 6}
U, S, F = rs.KEY_UNSIGNED, rs.KEY_SIGNED, rs.KEY_FLOAT

# columns -> [(first_col, key bytes K, element bytes)] per round, round 0 (the least significant columns) first
PLANS = [
    ([(1, U), (1, U)], [(0, 2, 8)]),
    ([(2, U), (1, U)], [(0, 3, 8)]),
    ([(4, S), (4, F)], [(0, 8, 16)]),
    ([(8, S), (4, S)], [(0, 12, 32)]),
    ([(8, F), (8, S)], [(0, 16, 32)]),
    ([(1, U)] * 16, [(0, 16, 32)]),
    ([(8, S), (8, S), (4, S)], [(1, 12, 32), (0, 8, 16)]),
    ([(16, U), (16, U), (4, F)], [(2, 4, 8), (1, 16, 32), (0, 16, 32)]),
]


def _header():
    return open(os.path.join(ROOT, "include", "rsx.h")).read()


def test_prototypes_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsx_\w+)\s*\(([^)]*)\)\s*;", text)}
    L = _lib.load()
    for name, nargs in NAMES.items():
        assert name in protos, name
        assert name in _lib.SYMBOLS, name
        fn = getattr(L, name)  # (AttributeError: not exported)
        assert len([a for a in protos[name].split(",") if a.strip()]) == nargs == len(fn.argtypes), (name, protos[name], fn.argtypes)
        assert fn.restype is ctypes.c_int
    for name in ("radix_lexsort", "radix_sort_columns", "lex_plan", "INFO_LAST_LEX"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert callable(rs.Context.lexsort_device) and callable(rs.Context.sort_columns_device) and callable(rs.Context.reserve_lex)
    assert re.search(r"#define\s+RSX_LEX_MAX_COLUMNS\s+16\b", text) and _lib.LEX_MAX_COLUMNS == 16
    assert re.search(r"RSX_INFO_LAST_LEX\s*=\s*8\b", text) and rs.INFO_LAST_LEX == 8
    assert re.search(r"#define\s+RSX_VERSION\s+200\b", text)


def test_key_column_struct_matches_header():
    assert ctypes.sizeof(_lib.KeyColumn) == 24
    assert [f[0] for f in _lib.KeyColumn._fields_] == ["d_keys", "key_bytes", "key_kind", "descending", "reserved"]
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"typedef\s+struct\s+rsx_key_column\s*\{(.*?)\}\s*rsx_key_column\s*;", text, flags=re.S)
    assert m
    assert re.findall(r"(\w+)\s*;", m.group(1)) == ["d_keys", "key_bytes", "key_kind", "descending", "reserved"]


@pytest.mark.parametrize("specs,plan", PLANS, ids=[str(i) for i in range(len(PLANS))])
def test_the_plans_of_the_rule(specs, plan):
    assert rs.lex_plan(specs) == plan
    # the element is the joined (key of W bytes, u32 position) element of the key / value calls, W the power of two >= K
    for _first, k, es in plan:
        w = next(w for w in (1, 2, 4, 8, 16) if w >= k)
        assert es == {1: 8, 2: 8, 4: 8, 8: 16, 16: 32}[w]
    # the rounds partition the columns, the last round starts at column 0
    firsts = [p[0] for p in plan]
    assert firsts == sorted(firsts, reverse=True) and firsts[-1] == 0
    ends = [len(specs)] + firsts[:-1]
    for (first, k, _es), end in zip(plan, ends):
        assert k == sum(kb for kb, _ in specs[first:end]) <= 16


def test_a_single_column_and_a_column_that_fills_a_round():
    assert rs.lex_plan([(4, F)]) == [(0, 4, 8)]
    assert rs.lex_plan([(1, U), (16, S), (1, U)]) == [(2, 1, 8), (1, 16, 32), (0, 1, 8)]  # a column is never split
    assert rs.lex_plan([(8, U), (8, U), (1, U)]) == [(1, 9, 32), (0, 8, 16)]
    assert rs.lex_plan([(1, U)] * 16 + [])[0][1] == 16


def _plan_rc(specs, reserved=0):
    L = _lib.load()
    arr = (_lib.KeyColumn * max(1, len(specs)))()
    for j, (kb, kind) in enumerate(specs):
        arr[j] = _lib.KeyColumn(None, kb, kind, 0, reserved)
    rounds = ctypes.c_uint32(77)
    a, b, c = ((ctypes.c_uint32 * 16)() for _ in range(3))
    return L.rsx_lex_plan(arr, len(specs), ctypes.byref(rounds), a, b, c), rounds.value


def test_refusals_of_the_plan():
    assert _plan_rc([(1, U)] * 17) == (_lib.ERR_ARG, 77)
    assert _plan_rc([]) == (_lib.ERR_ARG, 77)
    assert _plan_rc([(4, U)], reserved=1) == (_lib.ERR_ARG, 77)
    assert _plan_rc([(4, U), (3, U)]) == (_lib.ERR_UNSUPPORTED, 77)
    assert _plan_rc([(2, F)]) == (_lib.ERR_UNSUPPORTED, 77)
    assert _plan_rc([(16, F)]) == (_lib.ERR_UNSUPPORTED, 77)
    assert _plan_rc([(4, 3)]) == (_lib.ERR_UNSUPPORTED, 77)
    L = _lib.load()
    r = ctypes.c_uint32()
    a = (ctypes.c_uint32 * 16)()
    col = (_lib.KeyColumn * 1)(_lib.KeyColumn(None, 4, 0, 0, 0))
    assert L.rsx_lex_plan(None, 1, ctypes.byref(r), a, a, a) == _lib.ERR_ARG
    assert L.rsx_lex_plan(col, 1, None, a, a, a) == _lib.ERR_ARG
    assert L.rsx_lex_plan(col, 1, ctypes.byref(r), None, a, a) == _lib.ERR_ARG
    for bad in ([(1, U)] * 17, [], [(3, U)], [(2, F)]):
        with pytest.raises(rs.RsxError):
            rs.lex_plan(bad)


def test_a_null_context_is_refused():
    L = _lib.load()
    col = (_lib.KeyColumn * 1)(_lib.KeyColumn(16, 4, 0, 0, 0))
    assert L.rsx_lexsort_device(None, col, 1, 16, 10, 8, None) == _lib.ERR_ARG
    assert L.rsx_sort_columns_device(None, col, 1, None, 0, 10, None) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_lex(None, 10, col, 1, 0) == _lib.ERR_ARG


def test_argument_errors_need_no_device():
    a = torch.zeros(8, dtype=torch.int32)
    b = torch.zeros(8, dtype=torch.float32)
    contexts = dict(rs.api._DEFAULT)
    for fn in (rs.radix_lexsort, rs.radix_sort_columns):
        with pytest.raises(TypeError):
            fn(a)  # one tensor is not a list of columns
        with pytest.raises(TypeError):
            fn([a.numpy(), b])
        with pytest.raises(TypeError):
            fn([a, [0.0] * 8])
        with pytest.raises(TypeError):
            fn([a, torch.zeros(8, dtype=torch.bool)])
        with pytest.raises(TypeError):
            fn([(a, rs.KEY_SIGNED, 0), b])
        with pytest.raises(ValueError, match="key columns"):
            fn([])
        with pytest.raises(ValueError, match="key columns"):
            fn([a] * 17)
        with pytest.raises(ValueError, match="length"):
            fn([a, torch.zeros(7, dtype=torch.float32)])  # mismatched lengths
        with pytest.raises(ValueError, match="contiguous"):
            fn([a, torch.zeros(8, 2, dtype=torch.float32)[:, 0]])
        with pytest.raises(ValueError, match="1-D"):
            fn([a, torch.zeros(8, 4, dtype=torch.int32)])
        with pytest.raises(ValueError, match="key_kind"):
            fn([(a, rs.KEY_SIGNED), b])  # key_kind is for 128-bit columns
        with pytest.raises(ValueError, match="128-bit"):
            fn([a, (torch.zeros(8, 16, dtype=torch.uint8), rs.KEY_FLOAT)])
        for bad in ([True], [True, False, True], [1, 0], "no", None):
            with pytest.raises((ValueError, TypeError), match="descending|iterable"):
                fn([a, b], descending=bad)
        with pytest.raises(ValueError, match="GPU"):
            fn([a, b])  # CPU tensors, everything else in order
        with pytest.raises(ValueError, match="GPU"):
            fn([a, (torch.zeros(8, 16, dtype=torch.uint8), rs.KEY_SIGNED)], descending=[True, False])
    # out of radix_lexsort
    with pytest.raises(TypeError):
        rs.radix_lexsort([a, b], out=[0] * 8)
    with pytest.raises(TypeError, match="int32 or int64"):
        rs.radix_lexsort([a, b], out=torch.zeros(8, dtype=torch.int16))
    with pytest.raises(TypeError, match="int32 or int64"):
        rs.radix_lexsort([a, b], out=torch.zeros(8, dtype=torch.float32))
    with pytest.raises(ValueError, match="out must be"):
        rs.radix_lexsort([a, b], out=torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ValueError, match="out must be"):
        rs.radix_lexsort([a, b], out=torch.zeros(8, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="out must be"):
        rs.radix_lexsort([a, b], out=torch.zeros(16, dtype=torch.int32)[::2])
    # values of radix_sort_columns
    with pytest.raises(TypeError):
        rs.radix_sort_columns([a, b], values=[0] * 8)
    with pytest.raises(ValueError, match="leading shape"):
        rs.radix_sort_columns([a, b], values=torch.zeros(7, 3, dtype=torch.int16))
    with pytest.raises(ValueError, match="leading shape"):
        rs.radix_sort_columns([a, b], values=torch.zeros(3, 8, dtype=torch.int16))
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_sort_columns([a, b], values=torch.zeros(16, dtype=torch.int16)[::2])
    with pytest.raises(ValueError, match="32768"):
        rs.radix_sort_columns([a, b], values=torch.zeros(8, 32769, dtype=torch.uint8))
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_sort_columns([a, b], values=torch.zeros(8, 3, dtype=torch.int16))
    assert rs.api._DEFAULT == contexts, "an argument error made a context"
