"""Host side of the scan-by-key calls (no GPU): the prototypes and their bindings, rsx_scan_by_key_caps, the argument errors
the C calls return without a device, and those of radix_scan_by_key, which are raised before any context exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_scan_by_key_device", "rsx_ctx_reserve_scan_by_key", "rsx_scan_by_key_caps"]


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
    assert len(L.rsx_scan_by_key_device.argtypes) == 14
    assert len(L.rsx_ctx_reserve_scan_by_key.argtypes) == 5
    assert len(L.rsx_scan_by_key_caps.argtypes) == 5
    for name in ("radix_scan_by_key", "scan_by_key_caps", "SCAN_EXCLUSIVE", "SCAN_RUNS"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert callable(rs.Context.scan_by_key_device) and callable(rs.Context.reserve_scan_by_key)
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"enum\s*\{\s*RSX_SCAN_EXCLUSIVE\s*=\s*(\d+)\s*,\s*RSX_SCAN_RUNS\s*=\s*(\d+)\s*\}", text)
    assert m and tuple(int(x) for x in m.groups()) == (_lib.SCAN_EXCLUSIVE, _lib.SCAN_RUNS) == (1, 2)
    assert rs.SCAN_EXCLUSIVE == 1 and rs.SCAN_RUNS == 2
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert re.search(r"\bfn\s+" + name + r"\s*\(", rust), name


@pytest.mark.parametrize("runs", [False, True])
@pytest.mark.parametrize("vb", [4, 8])
@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16])
def test_caps(kb, vb, runs):
    tile, span = rs.scan_by_key_caps(kb, vb, runs)
    assert tile > 0 and span > 0
    assert tile % 256 == 0  # whole workgroups of 256 threads
    if runs:  # a thread's share of BOTH columns is a whole number of 16-byte words
        assert (tile // 256 * kb) % 16 == 0 and (tile // 256 * vb) % 16 == 0
    assert tile * span < 2 ** 32  # one sweep of the scan kernel sums at most tile heads per tile in 32 bits
    if runs and kb == 1:
        # One-byte keys in whole 16-byte words are 16 rows per thread and 4096 per workgroup at the least, and the scan
        # kernel's sweep is rsx_reduce_scan_kernel's own 512 tiles: the second sweep is out of reach of 1.1e6 elements
        # whatever the kernel does.  The tile is held to that least value instead.
        assert tile == 4096 and span * tile + tile + 3 <= 2.2e6
    else:
        assert span * tile + tile + 3 <= 1.1e6  # the second sweep of the scan is reached by a test of about 10^6 elements
    L = _lib.load()
    t2, s2 = ctypes.c_uint32(), ctypes.c_uint32()
    flags = (_lib.SCAN_RUNS if runs else 0) | _lib.SCAN_EXCLUSIVE
    assert L.rsx_scan_by_key_caps(kb, vb, flags, ctypes.byref(t2), ctypes.byref(s2)) == _lib.OK and (t2.value, s2.value) == (tile, span)


@pytest.mark.parametrize("kb,vb", [(0, 4), (3, 4), (5, 8), (12, 4), (32, 8), (4, 0), (4, 1), (4, 2), (4, 3), (4, 12), (4, 16), (8, 5)])
def test_caps_of_bad_widths(kb, vb):
    L = _lib.load()
    tile, span = ctypes.c_uint32(), ctypes.c_uint32()
    for flags in (0, _lib.SCAN_RUNS):
        assert L.rsx_scan_by_key_caps(kb, vb, flags, ctypes.byref(tile), ctypes.byref(span)) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.scan_by_key_caps(kb, vb)
    with pytest.raises(rs.RsxError):
        rs.scan_by_key_caps(kb, vb, runs=True)


def test_caps_needs_both_outputs_and_known_flags():
    L = _lib.load()
    tile, span = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.rsx_scan_by_key_caps(4, 4, 0, None, ctypes.byref(span)) == _lib.ERR_ARG
    assert L.rsx_scan_by_key_caps(4, 4, 0, ctypes.byref(tile), None) == _lib.ERR_ARG
    assert L.rsx_scan_by_key_caps(4, 4, 4, ctypes.byref(tile), ctypes.byref(span)) == _lib.ERR_ARG


def test_a_null_context_is_refused():
    L = _lib.load()
    assert L.rsx_scan_by_key_device(None, 16, 16, 10, 4, 0, 4, 2, 0, 0, 0, 16, 16, None) == _lib.ERR_ARG
    assert L.rsx_scan_by_key_device(None, None, None, 0, 4, 0, 4, 0, 0, 0, 0, None, None, None) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_scan_by_key(None, 10, 4, 4, 0) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_scan_by_key(None, 10, 3, 4, _lib.SCAN_RUNS) == _lib.ERR_ARG


def test_argument_errors_need_no_device():
    fn = rs.radix_scan_by_key
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
    # the count form
    for op in ("min", "max"):
        with pytest.raises(ValueError, match="count form"):
            fn(x, None, op=op)
    with pytest.raises(ValueError, match="index_dtype"):
        fn(x, None, index_dtype=torch.float32)
    with pytest.raises(ValueError, match="index_dtype"):
        fn(x, v, index_dtype=torch.int32)  # the result has the dtype of values
    # out
    with pytest.raises(TypeError):
        fn(x, v, out=v.numpy())
    with pytest.raises(ValueError, match="out must be"):
        fn(x, v, out=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        fn(x, v, out=torch.zeros(7, dtype=torch.float32))
    with pytest.raises(ValueError, match="out must be"):
        fn(x, None, out=torch.zeros(8, dtype=torch.int32))  # int64 unless index_dtype says int32
    with pytest.raises(ValueError, match="contiguous"):
        fn(x, v, out=torch.zeros(16, dtype=torch.float32)[::2])
    # first
    with pytest.raises(TypeError, match="first"):
        fn(x, torch.zeros(8, dtype=torch.int32), exclusive=True, first=1.5)
    with pytest.raises(ValueError, match="first"):
        fn(x, torch.zeros(8, dtype=torch.int32), exclusive=True, first=2 ** 31)
    with pytest.raises(TypeError, match="first"):
        fn(x, v, exclusive=True, first=torch.zeros(()))
    with pytest.raises(ValueError, match="GPU"):
        fn(x, v)  # CPU tensors, everything else in order
    with pytest.raises(ValueError, match="GPU"):
        fn(x, None, exclusive=True, runs=True, return_num=True)
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())


def test_default_first_values():
    bits = rs.api._scan_first_bits
    assert bits(None, "sum", torch.float32) == 0 and bits(None, "sum", torch.int64) == 0
    assert bits(None, "min", torch.int32) == 0x7FFFFFFF and bits(None, "max", torch.int32) == 0x80000000
    assert bits(None, "min", torch.int64) == 2 ** 63 - 1 and bits(None, "max", torch.int64) == 2 ** 63
    assert bits(None, "min", torch.float32) == 0x7F800000 and bits(None, "max", torch.float32) == 0xFF800000
    assert bits(None, "min", torch.float64) == 0x7FF0000000000000 and bits(None, "max", torch.float64) == 0xFFF0000000000000
    assert bits(-1, "sum", torch.int32) == 0xFFFFFFFF and bits(-0.0, "sum", torch.float64) == 2 ** 63
