"""Host side of the search call (no GPU): the prototypes and their bindings, rsx_search_caps, the argument errors the C calls
return without a device, and those of radix_searchsorted, which are raised before any context exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_search_sorted_device", "rsx_ctx_reserve_search", "rsx_search_caps"]
LDS_PER_CU = 160 * 1024


def _prototypes():
    text = open(os.path.join(ROOT, "include", "rsx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsx_\w+)\s*\(([^)]*)\)\s*;", text)}


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
    assert len(L.rsx_search_sorted_device.argtypes) == 14
    assert len(L.rsx_ctx_reserve_search.argtypes) == 3 and len(L.rsx_search_caps.argtypes) == 4
    for name in ("radix_searchsorted", "search_caps", "SEARCH_PRESORT"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert rs.SEARCH_PRESORT == 1
    assert re.search(r"enum\s*\{\s*RSX_SEARCH_PRESORT\s*=\s*1\s*\}", open(os.path.join(ROOT, "include", "rsx.h")).read())
    assert callable(rs.Context.search_sorted_device) and callable(rs.Context.reserve_search)
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in rust, name


@pytest.mark.parametrize("with_positions", [False, True])
@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16])
def test_caps(kb, with_positions):
    tile, window = rs.search_caps(kb, with_positions)
    assert tile > 0 and tile % 256 == 0  # whole workgroups of 256 threads
    assert window >= 2 * tile  # ordered needles drawn from the haystack at m = n fit, with room for short runs of equal keys
    assert 2 * window * kb <= LDS_PER_CU  # at least two workgroups per CU
    assert window * kb + 1024 <= 64 * 1024  # static LDS of one workgroup, with room for the tile's own words


@pytest.mark.parametrize("kb", [0, 3, 5, 12, 32])
def test_caps_of_a_bad_width(kb):
    L = _lib.load()
    tile, window = ctypes.c_uint32(), ctypes.c_uint32()
    for pos in (0, 1):
        assert L.rsx_search_caps(kb, pos, ctypes.byref(tile), ctypes.byref(window)) == _lib.ERR_ARG
    assert L.rsx_search_caps(4, 1, None, ctypes.byref(window)) == _lib.ERR_ARG
    assert L.rsx_search_caps(4, 0, ctypes.byref(tile), None) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.search_caps(kb)


def test_a_null_context_is_refused():
    L = _lib.load()
    assert L.rsx_search_sorted_device(None, 16, 10, None, 16, 10, 4, 0, 0, 16, 16, 8, 0, None) == _lib.ERR_ARG
    assert L.rsx_search_sorted_device(None, 16, 10, 16, 16, 10, 3, 0, 0, 16, None, 4, 1, None) == _lib.ERR_ARG
    assert L.rsx_search_sorted_device(None, None, 0, None, None, 0, 4, 0, 0, None, None, 0, 0, None) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_search(None, 10, 4) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_search(None, 10, 3) == _lib.ERR_ARG


def test_argument_errors_need_no_device():
    x = torch.zeros(8, dtype=torch.int32)
    fn = rs.radix_searchsorted
    with pytest.raises(TypeError):
        fn([1, 2], x)  # non-tensors
    with pytest.raises(TypeError):
        fn(x, [1, 2])
    with pytest.raises(TypeError):
        fn(x, x.numpy())
    with pytest.raises(TypeError, match="dtype"):
        fn(x, x.to(torch.int64))
    with pytest.raises(TypeError, match="dtype"):
        fn(x, x.to(torch.float32))
    with pytest.raises(TypeError):
        fn(torch.zeros(4, dtype=torch.bool), torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="same device"):
        fn(x, torch.zeros(3, dtype=torch.int32, device="meta"))
    with pytest.raises(ValueError, match="1-D"):
        fn(torch.zeros(4, 4, dtype=torch.int32), x)  # a haystack that is not 1-D
    with pytest.raises(ValueError, match="1-D"):
        fn(torch.zeros(4, 8, dtype=torch.uint8), torch.zeros(4, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="contiguous"):
        fn(torch.zeros(8, 2, dtype=torch.int32)[:, 0], x)
    with pytest.raises(ValueError, match="contiguous"):
        fn(x, torch.zeros(8, 2, dtype=torch.int32)[:, 0])
    with pytest.raises(ValueError, match="16"):
        fn(torch.zeros(4, 16, dtype=torch.uint8), torch.zeros(4, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="key_kind"):
        fn(x, x, key_kind=rs.KEY_SIGNED)  # key_kind= is for 128-bit keys
    with pytest.raises(ValueError, match="side"):
        fn(x, x, side="middle")
    y = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(TypeError):
        fn(x, y, out=[0] * 6)
    with pytest.raises(TypeError):
        fn(x, y, out=torch.zeros(2, 3, dtype=torch.int16))
    with pytest.raises(ValueError, match="shape"):
        fn(x, y, out=torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        fn(x, y, out=torch.zeros(3, 2, dtype=torch.int64).t())  # the right shape, not contiguous
    with pytest.raises(TypeError, match="pair"):
        fn(x, y, side="both", out=torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(TypeError, match="one dtype"):
        fn(x, y, side="both", out=(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32)))
    with pytest.raises(ValueError, match="same device"):
        fn(x, y, out=torch.zeros(2, 3, dtype=torch.int64, device="meta"))
    with pytest.raises(ValueError, match="index_dtype"):
        fn(x, y, index_dtype=torch.int16)
    with pytest.raises(TypeError, match="sorted_num"):
        fn(x, y, sorted_num=3)
    with pytest.raises(TypeError, match="sorted_num"):
        fn(x, y, sorted_num=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="GPU"):
        fn(x, y)  # CPU tensors
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())
