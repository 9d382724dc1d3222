"""Host side of the merge call (no GPU): the prototypes and their bindings, rsx_merge_caps, the argument errors the C calls
return without a device, and those of radix_merge / radix_merge_pairs, which are raised before any context exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_merge_device", "rsx_ctx_reserve_merge", "rsx_merge_caps"]
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
    assert len(L.rsx_merge_device.argtypes) == 16
    assert len(L.rsx_ctx_reserve_merge.argtypes) == 4 and len(L.rsx_merge_caps.argtypes) == 3
    for name in ("radix_merge", "radix_merge_pairs", "merge_caps"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert callable(rs.Context.merge_device) and callable(rs.Context.reserve_merge)
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in rust, name
    cxx = open(os.path.join(ROOT, "radix_sort_amd", "cxx", "radix_sort.hpp")).read()
    assert "//     rsx::merge(" in cxx and "//     rsx::merge_pairs(" in cxx  # the header's index comment


@pytest.mark.parametrize("vb", [0, 1, 4, 16, 12, 40, 32768])
@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16])
def test_caps(kb, vb):
    tile = rs.merge_caps(kb, vb)
    assert tile > 0 and tile % 256 == 0  # whole workgroups of 256 threads
    assert tile <= 65536  # a source slot of the tile is 16 bits wide
    lds = tile * (kb + 2) + 16  # mapped keys, u16 slots, the two cuts (include/rsx.h)
    assert 2 * lds <= LDS_PER_CU  # at least two workgroups per CU
    assert lds <= 64 * 1024  # static LDS of one workgroup
    if vb == 0:
        assert rs.merge_caps(kb) == tile


@pytest.mark.parametrize("kb", [0, 3, 5, 12, 32])
def test_caps_of_a_bad_width(kb):
    L = _lib.load()
    tile = ctypes.c_uint32()
    assert L.rsx_merge_caps(kb, 0, ctypes.byref(tile)) == _lib.ERR_ARG
    assert L.rsx_merge_caps(kb, 4, ctypes.byref(tile)) == _lib.ERR_ARG
    assert L.rsx_merge_caps(4, 0, None) == _lib.ERR_ARG
    assert L.rsx_merge_caps(4, 32769, ctypes.byref(tile)) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.merge_caps(kb)
    with pytest.raises(rs.RsxError):
        rs.merge_caps(4, 32769)


def test_a_null_context_is_refused():
    L = _lib.load()
    assert L.rsx_merge_device(None, 16, None, 10, 32, None, 10, 4, 0, 0, 0, 64, None, None, 8, None) == _lib.ERR_ARG
    assert L.rsx_merge_device(None, 16, 16, 10, 32, 32, 10, 3, 0, 4, 0, 64, 64, 64, 4, None) == _lib.ERR_ARG
    assert L.rsx_merge_device(None, None, None, 0, None, None, 0, 4, 0, 0, 0, None, None, None, 0, None) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_merge(None, 10, 4, 0) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_merge(None, 10, 3, 12) == _lib.ERR_ARG


def test_argument_errors_of_radix_merge_need_no_device():
    x = torch.zeros(8, dtype=torch.int32)
    fn = rs.radix_merge
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
        fn(torch.zeros(4, 4, dtype=torch.int32), x)
    with pytest.raises(ValueError, match="1-D"):
        fn(x, torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="1-D"):
        fn(torch.zeros(4, 8, dtype=torch.uint8), torch.zeros(4, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="contiguous"):
        fn(torch.zeros(8, 2, dtype=torch.int32)[:, 0], x)
    with pytest.raises(ValueError, match="contiguous"):
        fn(x, torch.zeros(8, 2, dtype=torch.int32)[:, 0])
    with pytest.raises(ValueError, match="16"):
        fn(torch.zeros(4, 16, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(ValueError, match="key_kind"):
        fn(x, x, key_kind=rs.KEY_SIGNED)  # key_kind= is for 128-bit keys
    y = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(TypeError):
        fn(x, y, out=[0] * 11)
    with pytest.raises(TypeError, match="dtype"):
        fn(x, y, out=torch.zeros(11, dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        fn(x, y, out=torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        fn(x, y, out=torch.zeros(11, 2, dtype=torch.int32)[:, 0])  # the right shape, not contiguous
    with pytest.raises(ValueError, match="same device"):
        fn(x, y, out=torch.zeros(11, dtype=torch.int32, device="meta"))
    with pytest.raises(TypeError, match="pair"):
        fn(x, y, return_index=True, out=torch.zeros(11, dtype=torch.int32))
    with pytest.raises(TypeError):
        fn(x, y, return_index=True, out=(torch.zeros(11, dtype=torch.int32), torch.zeros(11, dtype=torch.int16)))
    with pytest.raises(ValueError, match="shape"):
        fn(x, y, return_index=True, out=(torch.zeros(11, dtype=torch.int32), torch.zeros(10, dtype=torch.int64)))
    with pytest.raises(ValueError, match="same device"):
        fn(x, y, return_index=True, out=(torch.zeros(11, dtype=torch.int32), torch.zeros(11, dtype=torch.int64, device="meta")))
    with pytest.raises(ValueError, match="index_dtype"):
        fn(x, y, return_index=True, index_dtype=torch.int16)
    with pytest.raises(ValueError, match="GPU"):
        fn(x, y)  # CPU tensors
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())


def test_argument_errors_of_radix_merge_pairs_need_no_device():
    x, y = torch.zeros(8, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    vx, vy = torch.zeros(8, 3, dtype=torch.float32), torch.zeros(3, 3, dtype=torch.float32)
    fn = rs.radix_merge_pairs
    with pytest.raises(TypeError):
        fn(x, [0] * 8, y, vy)
    with pytest.raises(TypeError):
        fn(x, vx, y, None)  # values on one side only
    with pytest.raises(TypeError):
        fn(x, None, y, vy)
    with pytest.raises(TypeError, match="dtype"):
        fn(x, vx, y.to(torch.int64), vy)
    with pytest.raises(TypeError, match="dtype"):
        fn(x, vx, y, vy.to(torch.float64))
    with pytest.raises(ValueError, match="leading shape"):
        fn(x, vx[:7], y, vy)  # one row per key
    with pytest.raises(ValueError, match="leading shape"):
        fn(x, vx, y, vx)
    with pytest.raises(ValueError, match="trailing shape"):
        fn(x, vx, y, torch.zeros(3, 4, dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        fn(x, torch.zeros(8, 3, 2, dtype=torch.float32)[:, :, 0], y, vy)
    with pytest.raises(ValueError, match="32768"):
        fn(x, torch.zeros(8, 8193, dtype=torch.float32), y, torch.zeros(3, 8193, dtype=torch.float32))
    with pytest.raises(ValueError, match="same device"):
        fn(x, vx, y, torch.zeros(3, 3, dtype=torch.float32, device="meta"))
    with pytest.raises(TypeError, match="pair"):
        fn(x, vx, y, vy, out=torch.zeros(11, dtype=torch.int32))
    with pytest.raises(TypeError, match="dtype"):
        fn(x, vx, y, vy, out=(torch.zeros(11, dtype=torch.int32), torch.zeros(11, 3, dtype=torch.float64)))
    with pytest.raises(ValueError, match="shape"):
        fn(x, vx, y, vy, out=(torch.zeros(11, dtype=torch.int32), torch.zeros(11, dtype=torch.float32)))
    with pytest.raises(ValueError, match="shape"):
        fn(x, vx, y, vy, out=(torch.zeros(12, dtype=torch.int32), torch.zeros(11, 3, dtype=torch.float32)))
    with pytest.raises(ValueError, match="GPU"):
        fn(x, vx, y, vy)  # CPU tensors
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())
