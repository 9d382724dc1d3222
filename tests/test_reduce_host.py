"""Host side of the reduce-by-key calls (no GPU): the prototypes and their bindings, rsx_reduce_caps, the argument errors
the C calls return without a device, and those of radix_reduce_by_key, which are raised before any context exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_reduce_by_key_device", "rsx_ctx_reserve_reduce", "rsx_reduce_caps"]
JOINED = {(1, 4): 8, (2, 4): 8, (4, 4): 8, (1, 8): 12, (2, 8): 12, (4, 8): 12, (8, 4): 16, (8, 8): 16, (16, 4): 32, (16, 8): 32}


def _header():
    return open(os.path.join(ROOT, "include", "rsx.h")).read()


def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
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
    assert len(L.rsx_reduce_by_key_device.argtypes) == 15
    for name in ("radix_reduce_by_key", "reduce_caps", "Reduced"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert rs.Reduced._fields == ("num", "keys", "values", "offsets")
    assert callable(rs.Context.reduce_by_key_device) and callable(rs.Context.reserve_reduce)
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"enum\s*\{\s*RSX_REDUCE_SUM\s*=\s*(\d+)\s*,\s*RSX_REDUCE_MIN\s*=\s*(\d+)\s*,\s*RSX_REDUCE_MAX\s*=\s*(\d+)\s*\}", text)
    assert m and tuple(int(x) for x in m.groups()) == (_lib.REDUCE_SUM, _lib.REDUCE_MIN, _lib.REDUCE_MAX) == (0, 1, 2)


@pytest.mark.parametrize("vb", [4, 8])
@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16])
def test_caps(kb, vb):
    tile, span = rs.reduce_caps(kb, vb)
    assert tile > 0 and span > 0
    assert tile % 256 == 0  # whole workgroups of 256 threads
    per_thread = tile // 256 * JOINED[kb, vb]
    assert per_thread % 16 == 0, "a thread's run is a whole number of 16-byte words"
    assert 48 <= per_thread <= 64
    assert tile * span < 2 ** 32  # one sweep of the scan kernel sums at most tile heads per tile in 32 bits
    assert span * tile + tile + 3 <= 1.1e6  # the second sweep of the scan is reached by a test of about 10^6 elements


@pytest.mark.parametrize("kb,vb", [(0, 4), (3, 4), (5, 8), (12, 4), (32, 8), (4, 0), (4, 1), (4, 2), (4, 3), (4, 12), (4, 16), (8, 5)])
def test_caps_of_bad_widths(kb, vb):
    L = _lib.load()
    tile, span = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.rsx_reduce_caps(kb, vb, ctypes.byref(tile), ctypes.byref(span)) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.reduce_caps(kb, vb)


def test_caps_needs_both_outputs():
    L = _lib.load()
    tile, span = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.rsx_reduce_caps(4, 4, None, ctypes.byref(span)) == _lib.ERR_ARG
    assert L.rsx_reduce_caps(4, 4, ctypes.byref(tile), None) == _lib.ERR_ARG


def test_a_null_context_is_refused():
    L = _lib.load()
    assert L.rsx_reduce_by_key_device(None, 16, 16, 10, 4, 0, 4, 2, 0, 0, 16, 16, 16, 16, None) == _lib.ERR_ARG
    assert L.rsx_reduce_by_key_device(None, None, None, 0, 4, 0, 4, 0, 0, 0, None, None, None, None, None) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_reduce(None, 10, 4, 4) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_reduce(None, 10, 3, 4) == _lib.ERR_ARG


def test_argument_errors_need_no_device():
    fn = rs.radix_reduce_by_key
    x = torch.zeros(8, dtype=torch.float32)
    v = torch.zeros(8, dtype=torch.float32)
    with pytest.raises(TypeError):
        fn([1.0, 2.0], v)
    with pytest.raises(TypeError):
        fn(x.numpy(), v)
    with pytest.raises(TypeError):
        fn(x, [0.0] * 8)
    with pytest.raises(TypeError):
        fn(x, v.numpy())
    with pytest.raises(TypeError):
        fn(torch.zeros(4, dtype=torch.bool), v[:4])
    with pytest.raises(ValueError, match="contiguous"):
        fn(torch.zeros(8, 2, dtype=torch.float32)[:, 0], v)
    with pytest.raises(ValueError, match="1-D"):
        fn(torch.zeros(4, 4, dtype=torch.int32), v[:4])
    with pytest.raises(ValueError, match="key_kind"):
        fn(x, v, key_kind=rs.KEY_SIGNED)  # key_kind= is for 128-bit keys
    with pytest.raises(ValueError, match="128-bit"):
        fn(torch.zeros(4, 16, dtype=torch.uint8), v[:4], key_kind=rs.KEY_FLOAT)
    for op in ("mean", "prod", 0, None):
        with pytest.raises(ValueError, match="op"):
            fn(x, v, op=op)
    for bad in (torch.int8, torch.uint8, torch.int16, torch.float16, torch.bfloat16, torch.bool, torch.complex64):
        with pytest.raises(ValueError, match="values must be"):
            fn(x, torch.zeros(8, dtype=bad))
    with pytest.raises(ValueError, match="one entry per key"):
        fn(x, torch.zeros(7, dtype=torch.float32))
    with pytest.raises(ValueError, match="one entry per key"):
        fn(x, torch.zeros(8, 1, dtype=torch.float32))  # rows of values are out of scope
    with pytest.raises(ValueError, match="contiguous"):
        fn(x, torch.zeros(16, dtype=torch.float32)[::2])
    with pytest.raises(ValueError, match="GPU"):
        fn(x, v)  # CPU tensors, everything else in order
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())
