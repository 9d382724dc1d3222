"""Host side of the join call (no GPU): the prototypes and their bindings, rsx_join_caps, the argument errors the C calls
return without a device, and those of radix_join, which are raised before any context exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_join_device", "rsx_ctx_reserve_join", "rsx_join_caps"]
LDS_PER_CU = 160 * 1024


def _header():
    text = open(os.path.join(ROOT, "include", "rsx.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _prototypes():
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsx_\w+)\s*\(([^)]*)\)\s*;", _header())}


def test_prototypes_are_declared_exported_and_bound():
    protos = _prototypes()
    L = _lib.load()
    for name in NAMES:
        assert name in protos, name
        assert name in _lib.SYMBOLS, name
        fn = getattr(L, name)  # (AttributeError: not exported)
        nargs = len([a for a in protos[name].split(",") if a.strip() and a.strip() != "void"])
        assert len(fn.argtypes) == nargs, (name, protos[name], fn.argtypes)
        assert fn.restype is ctypes.c_int
    assert len(L.rsx_join_device.argtypes) == 19
    assert len(L.rsx_ctx_reserve_join.argtypes) == 3 and len(L.rsx_join_caps.argtypes) == 4
    for name in ("radix_join", "join_caps", "JoinResult", "JOIN_INNER", "JOIN_LEFT", "JOIN_SEMI", "JOIN_ANTI"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert rs.JoinResult._fields == ("left", "right", "num")
    assert callable(rs.Context.join_device) and callable(rs.Context.reserve_join)
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in rust, name
    cxx = open(os.path.join(ROOT, "radix_sort_amd", "cxx", "radix_sort.hpp")).read()
    assert "//     rsx::join(" in cxx and "//     rsx::join_count(" in cxx  # the header's index comment


def test_the_join_codes_are_those_of_the_header():
    enums = dict(re.findall(r"\b(RSX_JOIN_\w+)\s*=\s*(\d+)", _header()))
    assert {k: int(v) for k, v in enums.items()} == {"RSX_JOIN_INNER": 0, "RSX_JOIN_LEFT": 1, "RSX_JOIN_SEMI": 2, "RSX_JOIN_ANTI": 3}
    assert (_lib.JOIN_INNER, _lib.JOIN_LEFT, _lib.JOIN_SEMI, _lib.JOIN_ANTI) == (0, 1, 2, 3)
    assert (rs.JOIN_INNER, rs.JOIN_LEFT, rs.JOIN_SEMI, rs.JOIN_ANTI) == (0, 1, 2, 3)
    assert rs.api._JOINS == {"inner": 0, "left": 1, "semi": 2, "anti": 3}


@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16])
def test_caps(kb):
    tile, window, rows = rs.join_caps(kb)
    assert tile >= 256 and window >= 2 * tile and rows >= 256
    assert tile % 256 == 0 and window % 256 == 0 and rows % 256 == 0  # whole workgroups of 256 threads
    assert (tile, window) == rs.search_caps(kb)                      # the count kernel is the search kernel's tile
    assert 2 * (window * kb + 8 * kb + 160) <= LDS_PER_CU and 2 * (8 * rows + 32) <= LDS_PER_CU  # what include/rsx.h states


@pytest.mark.parametrize("kb", [0, 3, 5, 12, 32])
def test_caps_of_a_bad_width(kb):
    L = _lib.load()
    t, w, r = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    assert L.rsx_join_caps(kb, ctypes.byref(t), ctypes.byref(w), ctypes.byref(r)) == _lib.ERR_ARG
    assert L.rsx_join_caps(4, None, ctypes.byref(w), ctypes.byref(r)) == _lib.ERR_ARG
    assert L.rsx_join_caps(4, ctypes.byref(t), None, ctypes.byref(r)) == _lib.ERR_ARG
    assert L.rsx_join_caps(4, ctypes.byref(t), ctypes.byref(w), None) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.join_caps(kb)


def test_a_null_context_is_refused():
    L = _lib.load()
    assert L.rsx_join_device(None, 0, 16, 10, None, None, 32, 10, None, None, 4, 0, 0, 64, 128, 8, 100, 256, None) == _lib.ERR_ARG
    assert L.rsx_join_device(None, 9, 16, 10, None, None, 32, 10, None, None, 3, 0, 0, 64, 128, 3, 100, None, None) == _lib.ERR_ARG
    assert L.rsx_join_device(None, 2, None, 0, None, None, None, 0, None, None, 4, 0, 0, None, None, 8, 0, None, None) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_join(None, 10, 4) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_join(None, 10, 3) == _lib.ERR_ARG


def test_argument_errors_of_radix_join_need_no_device():
    x = torch.zeros(8, dtype=torch.int32)
    y = torch.zeros(3, dtype=torch.int32)
    i64 = lambda n, **kw: torch.zeros(n, dtype=torch.int64, **kw)  # noqa: E731
    fn = rs.radix_join
    with pytest.raises(TypeError):
        fn([1, 2], x)  # non-tensors
    with pytest.raises(TypeError):
        fn(x, [1, 2])
    with pytest.raises(TypeError, match="dtype"):
        fn(x, x.to(torch.int64))
    with pytest.raises(TypeError):
        fn(torch.zeros(4, dtype=torch.bool), torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="same device"):
        fn(x, torch.zeros(3, dtype=torch.int32, device="meta"))
    with pytest.raises(ValueError, match="1-D"):
        fn(torch.zeros(4, 4, dtype=torch.int32), x)
    with pytest.raises(ValueError, match="contiguous"):
        fn(torch.zeros(8, 2, dtype=torch.int32)[:, 0], x)
    with pytest.raises(ValueError, match="key_kind"):
        fn(x, x, key_kind=rs.KEY_SIGNED)  # key_kind= is for 128-bit keys
    for bad in ("outer", "Inner", 0, None):
        with pytest.raises(ValueError, match="anti"):
            fn(x, y, bad)
    # what goes with assume_sorted=True only
    for name, value in (("a_num", torch.zeros((), dtype=torch.int64)), ("b_num", torch.zeros((), dtype=torch.int64)), ("a_index", i64(8)), ("b_index", i64(3))):
        with pytest.raises(ValueError, match="assume_sorted"):
            fn(x, y, **{name: value})
        with pytest.raises(ValueError, match="assume_sorted"):
            fn(x, y, "semi", assume_sorted=False, **{name: value})
    # out: a pair of one length and dtype; no right-hand tensor for semi and anti
    for how in ("semi", "anti"):
        with pytest.raises(ValueError, match="right-hand"):
            fn(x, y, how, out=(i64(8), i64(8)))
        with pytest.raises(ValueError, match="right-hand"):
            fn(x, y, how, assume_sorted=True, b_index=i64(3))
        with pytest.raises(ValueError, match="GPU"):
            fn(x, y, how, out=i64(8))  # a tensor alone, or (left, None): CPU tensors are the next complaint
        with pytest.raises(ValueError, match="GPU"):
            fn(x, y, how, out=(i64(8), None))
    for how in ("inner", "left"):
        with pytest.raises(TypeError, match="pair"):
            fn(x, y, how, out=i64(8))
        with pytest.raises(TypeError, match="pair"):
            fn(x, y, how, out=(i64(8), i64(8), i64(8)))
        with pytest.raises(ValueError, match="shape"):
            fn(x, y, how, out=(i64(8), i64(9)))
        with pytest.raises(ValueError, match="shape"):
            fn(x, y, how, out=(torch.zeros(8, 2, dtype=torch.int64), torch.zeros(8, 2, dtype=torch.int64)))
        with pytest.raises(ValueError, match="shape"):
            fn(x, y, how, out=(torch.zeros(8, 2, dtype=torch.int64)[:, 0], i64(8)))  # not contiguous
        with pytest.raises(TypeError):
            fn(x, y, how, out=(i64(8), torch.zeros(8, dtype=torch.int16)))
        with pytest.raises(TypeError, match="one dtype"):
            fn(x, y, how, out=(i64(8), torch.zeros(8, dtype=torch.int32)))
        with pytest.raises(TypeError):
            fn(x, y, how, out=([0] * 8, i64(8)))
        with pytest.raises(ValueError, match="same device"):
            fn(x, y, how, out=(i64(8), i64(8, device="meta")))
        with pytest.raises(ValueError, match="disagree"):
            fn(x, y, how, capacity=9, out=(i64(8), i64(8)))
        with pytest.raises(ValueError, match="GPU"):
            fn(x, y, how, capacity=8, out=(i64(8), i64(8)))
    with pytest.raises(ValueError, match="index_dtype"):
        fn(x, y, index_dtype=torch.int16)
    for bad in (-1, 2.5, "3"):
        with pytest.raises(ValueError, match="capacity"):
            fn(x, y, capacity=bad)
    # index arrays: one word of the index dtype per key
    with pytest.raises(TypeError, match="a_index"):
        fn(x, y, assume_sorted=True, a_index=[0] * 8)
    with pytest.raises(TypeError, match="a_index"):
        fn(x, y, assume_sorted=True, a_index=torch.zeros(8, dtype=torch.int32))  # the default index dtype is int64
    with pytest.raises(TypeError, match="b_index"):
        fn(x, y, assume_sorted=True, index_dtype=torch.int32, b_index=i64(3))
    with pytest.raises(ValueError, match="a_index"):
        fn(x, y, assume_sorted=True, a_index=i64(7))
    with pytest.raises(ValueError, match="b_index"):
        fn(x, y, assume_sorted=True, b_index=torch.zeros(3, 2, dtype=torch.int64)[:, 0])
    with pytest.raises(ValueError, match="same device"):
        fn(x, y, assume_sorted=True, a_index=i64(8, device="meta"))
    for name in ("a_num", "b_num"):
        with pytest.raises(TypeError, match=name):
            fn(x, y, assume_sorted=True, **{name: 5})
        with pytest.raises(TypeError, match=name):
            fn(x, y, assume_sorted=True, **{name: torch.zeros(1, dtype=torch.int32)})
        with pytest.raises(ValueError, match="same device"):
            fn(x, y, assume_sorted=True, **{name: torch.zeros((), dtype=torch.int64, device="meta")})
    # 2^32 keys on a side: no position in them fits next to NONE, int32 indices least of all
    big = torch.zeros(1 << 32, dtype=torch.uint8, device="meta")
    small = torch.zeros(3, dtype=torch.uint8, device="meta")
    for kw in (dict(index_dtype=torch.int32), dict(index_dtype=torch.int64), dict(capacity=10)):
        with pytest.raises(ValueError, match="2\\^32"):
            fn(big, small, **kw)
        with pytest.raises(ValueError, match="2\\^32"):
            fn(small, big, "left", assume_sorted=True, **kw)
    with pytest.raises(ValueError, match="GPU"):
        fn(x, y)  # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        fn(x, y, "anti", assume_sorted=True, capacity=4, a_num=torch.zeros((), dtype=torch.int64))
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())
