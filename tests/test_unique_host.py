"""Host side of the group calls (no GPU): the prototypes and their bindings, rsx_unique_caps, the argument errors the C
calls return without a device, and those of radix_group / radix_unique, which are raised before any context exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_unique_device", "rsx_ctx_reserve_unique", "rsx_unique_caps"]


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
    assert len(_lib.load().rsx_unique_device.argtypes) == 13
    for name in ("radix_group", "radix_unique", "unique_caps", "Group"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert rs.Group._fields == ("num", "keys", "offsets", "perm", "inverse")
    assert callable(rs.Context.unique_device) and callable(rs.Context.reserve_unique)


@pytest.mark.parametrize("with_positions", [False, True])
@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16])
def test_caps(kb, with_positions):
    tile, span = rs.unique_caps(kb, with_positions)
    assert tile > 0 and span > 0
    assert tile % 256 == 0  # whole workgroups of 256 threads
    # one sweep of the scan kernel sums at most tile heads per tile in 32 bits
    assert tile * span < 2 ** 32
    joined = kb if not with_positions else {1: 8, 2: 8, 4: 8, 8: 16, 16: 32}[kb]
    assert tile * joined >= 4096, "a workgroup should move at least 4 KiB"


@pytest.mark.parametrize("kb", [0, 3, 5, 12, 32])
def test_caps_of_a_bad_width(kb):
    L = _lib.load()
    tile, span = ctypes.c_uint32(), ctypes.c_uint32()
    for pos in (0, 1):
        assert L.rsx_unique_caps(kb, pos, ctypes.byref(tile), ctypes.byref(span)) == _lib.ERR_ARG
    assert L.rsx_unique_caps(4, 1, None, ctypes.byref(span)) == _lib.ERR_ARG
    assert L.rsx_unique_caps(4, 1, ctypes.byref(tile), None) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.unique_caps(kb)


def test_a_null_context_is_refused():
    L = _lib.load()
    assert L.rsx_unique_device(None, 16, 10, 4, 0, 0, 16, 16, 16, 16, 8, 16, None) == _lib.ERR_ARG
    assert L.rsx_unique_device(None, 16, 10, 3, 0, 0, 16, 16, None, None, 8, 16, None) == _lib.ERR_ARG
    assert L.rsx_unique_device(None, None, 0, 4, 0, 0, None, None, None, None, 0, None, None) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_unique(None, 10, 4, 1) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_unique(None, 10, 3, 0) == _lib.ERR_ARG


def test_argument_errors_need_no_device():
    x = torch.zeros(8, dtype=torch.float32)
    for fn in (rs.radix_group, rs.radix_unique):
        with pytest.raises(TypeError):
            fn([1.0, 2.0])
        with pytest.raises(TypeError):
            fn(x.numpy())
        with pytest.raises(ValueError, match="contiguous"):
            fn(torch.zeros(8, 2, dtype=torch.float32)[:, 0])
        with pytest.raises(ValueError, match="GPU"):
            fn(x)  # a CPU tensor
        with pytest.raises(ValueError, match="1-D"):
            fn(torch.zeros(4, 4, dtype=torch.int32))  # 2-D, not uint8
        with pytest.raises(ValueError, match="1-D"):
            fn(torch.zeros(4, 8, dtype=torch.uint8))  # 2-D uint8, not 16 wide
        with pytest.raises(ValueError, match="key_kind"):
            fn(x, key_kind=rs.KEY_SIGNED)  # key_kind= is for 128-bit keys
        with pytest.raises(ValueError, match="128-bit"):
            fn(torch.zeros(4, 16, dtype=torch.uint8), key_kind=rs.KEY_FLOAT)
        with pytest.raises(TypeError):
            fn(torch.zeros(4, dtype=torch.bool))
    for bad in (torch.int16, torch.float32, torch.uint8):
        with pytest.raises(ValueError, match="index_dtype"):
            rs.radix_group(x, index_dtype=bad)
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())
