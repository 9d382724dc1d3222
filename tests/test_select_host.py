"""Host side of the order-statistics calls (no GPU): the prototypes and their bindings, rsx_select_caps, the argument errors
the C calls return without a device, and those of radix_select, radix_kthvalue, radix_median and radix_quantile, which are
raised before any context exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_select_device", "rsx_ctx_reserve_select", "rsx_select_caps"]


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
    assert len(L.rsx_select_device.argtypes) == 12
    assert len(L.rsx_ctx_reserve_select.argtypes) == 3 and len(L.rsx_select_caps.argtypes) == 6
    for name in ("radix_select", "radix_kthvalue", "radix_median", "radix_quantile", "select_caps"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert callable(rs.Context.select_device) and callable(rs.Context.reserve_select)
    assert rs.api._select_by_sort(1 << 16, 4) in (False, True)
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in rust, name
    cxx = open(os.path.join(ROOT, "radix_sort_amd", "cxx", "radix_sort.hpp")).read()
    assert "rsx_select_device(" in cxx and "rsx_select_caps(" in cxx
    assert re.search(r"\bvoid select\(", cxx) and re.search(r"\bSelectCaps select_caps\(", cxx)


@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16])
def test_caps(kb):
    max_ranks, digit_bits, tile, cand_div, cand_floor = rs.select_caps(kb)
    assert max_ranks >= 4
    assert 1 <= digit_bits <= 16
    assert tile > 0 and tile % 256 == 0  # whole workgroups of 256 threads
    assert cand_div >= 2
    assert cand_floor >= 0
    assert max_ranks * (1 << digit_bits) * 4 <= 80 * 1024  # the count kernel's counters: two workgroups per CU


@pytest.mark.parametrize("kb", [0, 3, 5, 12, 32])
def test_caps_of_a_bad_width(kb):
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(5)]
    assert L.rsx_select_caps(kb, *[ctypes.byref(o) for o in out]) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.select_caps(kb)


def test_caps_of_a_null_pointer():
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(5)]
    for missing in range(5):
        args = [None if i == missing else ctypes.byref(o) for i, o in enumerate(out)]
        assert L.rsx_select_caps(4, *args) == _lib.ERR_ARG


def test_a_null_context_is_refused():
    L = _lib.load()
    ranks = (ctypes.c_uint64 * 2)(0, 1)
    assert L.rsx_select_device(None, 16, 10, 4, 0, ranks, 2, 16, 16, 8, 0, None) == _lib.ERR_ARG
    assert L.rsx_select_device(None, 16, 10, 3, 0, ranks, 2, 16, None, 4, 1, None) == _lib.ERR_ARG
    assert L.rsx_select_device(None, None, 0, 4, 0, None, 0, None, None, 0, 0, None) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_select(None, 10, 4) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_select(None, 10, 3) == _lib.ERR_ARG


def test_argument_errors_need_no_device():
    x = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(TypeError):
        rs.radix_select([1, 2, 3], 0)  # not a tensor
    with pytest.raises(ValueError, match="1-D"):
        rs.radix_select(torch.zeros(4, 4, dtype=torch.int32), 0)  # 2-D keys
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_select(torch.zeros(8, 2, dtype=torch.int32)[:, 0], 0)
    with pytest.raises(TypeError):
        rs.radix_select(torch.zeros(4, dtype=torch.bool), 0)
    for r in (8, -9, [0, 8], [-9]):
        with pytest.raises(ValueError, match="rank"):
            rs.radix_select(x, r)
    with pytest.raises(ValueError, match="rank"):
        rs.radix_select(torch.zeros(0, dtype=torch.int32), 0)  # no keys: no rank is in range
    with pytest.raises(TypeError):
        rs.radix_select(x, 1.5)
    with pytest.raises(ValueError, match="index_dtype"):
        rs.radix_select(x, 0, return_index=True, index_dtype=torch.int16)
    with pytest.raises(ValueError, match="key_kind"):
        rs.radix_select(x, 0, key_kind=rs.KEY_SIGNED)  # key_kind= is for 128-bit keys
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_select(x, 0)  # a CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_select(x, [0, -1, 3], return_index=True)
    y = torch.zeros(3, 8, dtype=torch.float32)
    for k in (0, 9, -1):
        with pytest.raises(ValueError, match="k must be"):
            rs.radix_kthvalue(y, k)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_kthvalue(y, 8)
    with pytest.raises(ValueError, match="1-D"):
        rs.radix_median(y)
    with pytest.raises(ValueError, match="median"):
        rs.radix_median(torch.zeros(0, dtype=torch.float32))
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_median(x)
    for q in (-0.1, 1.5, float("nan"), [0.5, 2.0]):
        with pytest.raises(ValueError, match="q must"):
            rs.radix_quantile(x, q)
    with pytest.raises(ValueError, match="method"):
        rs.radix_quantile(x, 0.5, method="linear")
    with pytest.raises(ValueError, match="1-D"):
        rs.radix_quantile(y, 0.5)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_quantile(x, [0.0, 0.5, 1.0], method="nearest")
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())
