"""Host side of the bin-count calls (no GPU): the prototypes and their bindings, rsx_bin_caps, the argument errors the C call
returns with a null context, and those of radix_histogram and radix_bincount, which are raised before any context
exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_bin_count_device", "rsx_bin_caps"]


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
    assert len(L.rsx_bin_count_device.argtypes) == 14 and len(L.rsx_bin_caps.argtypes) == 4
    assert sorted(_lib.SYMBOLS) == sorted(re.findall(r"\b(rsx_\w+)\s*\(", _header()))  # what test_cabi.py holds the list to
    defines = dict(re.findall(r"#define\s+(RSX_BIN_\w+)\s+(\d+)u", _header()))
    assert defines == {"RSX_BIN_UPPER": "0", "RSX_BIN_LOWER": "1", "RSX_BIN_INDEX": "2", "RSX_BIN_ACCUMULATE": "1"}
    assert (rs.BIN_UPPER, rs.BIN_LOWER, rs.BIN_INDEX, rs.BIN_ACCUMULATE) == (0, 1, 2, 1)
    for name in ("radix_histogram", "radix_bincount", "bin_caps"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert callable(rs.Context.bin_count_device)
    assert callable(rs.Context.histogram_device)  # the 256-bin digit count keeps its name
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in rust, name
    cxx = open(os.path.join(ROOT, "radix_sort_amd", "cxx", "radix_sort.hpp")).read()
    assert "rsx_bin_count_device(" in cxx and "rsx_bin_caps(" in cxx
    assert re.search(r"\bvoid bin_count\(", cxx) and re.search(r"\bBinCaps bin_caps\(", cxx)


@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16])
def test_caps(kb):
    max_edges, index_lds, share = rs.bin_caps(kb)
    assert max_edges >= (2048 if kb == 16 else 4096)
    assert index_lds >= 16384
    assert share >= 1024 and share % 16 == 0  # whole 16-byte words of every key width
    assert max_edges * kb + (max_edges + 1) * 4 <= 80 * 1024  # edges and counters: two workgroups per CU
    assert index_lds * 4 <= 80 * 1024


@pytest.mark.parametrize("kb", [0, 3, 5, 12, 32])
def test_caps_of_a_bad_width(kb):
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(3)]
    assert L.rsx_bin_caps(kb, *[ctypes.byref(o) for o in out]) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.bin_caps(kb)


def test_caps_of_a_null_pointer():
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(3)]
    for missing in range(3):
        args = [None if i == missing else ctypes.byref(o) for i, o in enumerate(out)]
        assert L.rsx_bin_caps(4, *args) == _lib.ERR_ARG


def test_a_null_context_is_refused():
    L = _lib.load()
    #                              ctx  keys n  num  kb kind edges m mode order counts cb flags stream
    assert L.rsx_bin_count_device(None, 16, 10, None, 4, 0, 32, 2, 0, 0, 64, 8, 0, None) == _lib.ERR_ARG
    assert L.rsx_bin_count_device(None, 16, 10, None, 4, 0, None, 9, 2, 0, 64, 4, 1, None) == _lib.ERR_ARG
    assert L.rsx_bin_count_device(None, None, 0, None, 3, 0, None, 0, 7, 5, None, 3, 9, None) == _lib.ERR_ARG


def test_argument_errors_need_no_device():
    x = torch.zeros(8, dtype=torch.int32)
    e = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(TypeError):
        rs.radix_histogram([1, 2, 3], e)  # not a tensor
    with pytest.raises(TypeError):
        rs.radix_histogram(x, [0, 1])
    with pytest.raises(TypeError, match="dtype"):
        rs.radix_histogram(x, e.to(torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_histogram(torch.zeros(8, 2, dtype=torch.int32)[:, 0], e)
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_histogram(x, torch.zeros(3, 2, dtype=torch.int32)[:, 0])
    with pytest.raises(ValueError, match="1-D"):
        rs.radix_histogram(x, torch.zeros(2, 2, dtype=torch.int32))  # 2-D edges
    with pytest.raises(TypeError):
        rs.radix_histogram(torch.zeros(4, dtype=torch.bool), torch.zeros(2, dtype=torch.bool))
    with pytest.raises(ValueError, match="side"):
        rs.radix_histogram(x, e, side="both")
    with pytest.raises(ValueError, match="key_kind"):
        rs.radix_histogram(x, e, key_kind=rs.KEY_SIGNED)  # key_kind= is for 128-bit keys
    with pytest.raises(ValueError, match=r"\(\.\.\., 16\)"):
        rs.radix_histogram(torch.zeros(5, dtype=torch.uint8), torch.zeros(2, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="accumulate"):
        rs.radix_histogram(x, e, accumulate=True)  # nothing to add to
    with pytest.raises(ValueError, match="count_dtype"):
        rs.radix_histogram(x, e, count_dtype=torch.int16)
    with pytest.raises(TypeError, match="out must be"):
        rs.radix_histogram(x, e, out=torch.zeros(4, dtype=torch.float32))
    with pytest.raises(ValueError, match="shape"):
        rs.radix_histogram(x, e, out=torch.zeros(3, dtype=torch.int64))  # m + 1 = 4 counts
    with pytest.raises(TypeError, match="count_dtype"):
        rs.radix_histogram(x, e, out=torch.zeros(4, dtype=torch.int64), count_dtype=torch.int32)
    for num in (3, torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(TypeError, match="num"):
            rs.radix_histogram(x, e, num=num)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_histogram(x, e)  # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_histogram(x.view(2, 4), e, side="left", descending=True, out=torch.zeros(4, dtype=torch.int32), accumulate=True)

    with pytest.raises(TypeError):
        rs.radix_bincount([1, 2], 4)
    for bad in (torch.zeros(4, dtype=torch.float32), torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.bool)):
        with pytest.raises(TypeError):
            rs.radix_bincount(bad, 4)
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_bincount(torch.zeros(8, 2, dtype=torch.int32)[:, 0], 4)
    with pytest.raises(TypeError):
        rs.radix_bincount(x, 1.5)
    for bins in (-1, (1 << 32) - 1):
        with pytest.raises(ValueError, match="num_bins"):
            rs.radix_bincount(x, bins)
    with pytest.raises(ValueError, match="accumulate"):
        rs.radix_bincount(x, 4, accumulate=True)
    with pytest.raises(ValueError, match="shape"):
        rs.radix_bincount(x, 4, out=torch.zeros(4, dtype=torch.int64))  # num_bins + 1 = 5 counts
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_bincount(x, 4)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_bincount(x.view(2, 2, 2), 0, count_dtype=torch.int32)
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())
