"""Host side of the set-operation call (no GPU): the prototypes and their bindings, rsx_setop_caps, the argument errors the
C calls return without a device, and those of radix_set_op / radix_set_op_pairs, which are raised before any context
exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_setop_device", "rsx_ctx_reserve_setop", "rsx_setop_caps"]
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
    assert len(L.rsx_setop_device.argtypes) == 20
    assert len(L.rsx_ctx_reserve_setop.argtypes) == 3 and len(L.rsx_setop_caps.argtypes) == 2
    for name in ("radix_set_op", "radix_set_op_pairs", "setop_caps"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert callable(rs.Context.setop_device) and callable(rs.Context.reserve_setop)
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in rust, name
    cxx = open(os.path.join(ROOT, "radix_sort_amd", "cxx", "radix_sort.hpp")).read()
    assert "//     rsx::set_op(" in cxx and "//     rsx::set_op_pairs(" in cxx  # the header's index comment


def test_the_operation_codes_are_those_of_the_header():
    enums = dict(re.findall(r"\b(RSX_SETOP_\w+)\s*=\s*(\d+)", _header()))
    assert {k: int(v) for k, v in enums.items()} == {"RSX_SETOP_UNION": 0, "RSX_SETOP_INTERSECTION": 1, "RSX_SETOP_DIFFERENCE": 2,
                                                     "RSX_SETOP_SYMMETRIC_DIFFERENCE": 3}
    assert (_lib.SETOP_UNION, _lib.SETOP_INTERSECTION, _lib.SETOP_DIFFERENCE, _lib.SETOP_SYMMETRIC_DIFFERENCE) == (0, 1, 2, 3)
    assert rs.api._SET_OPS == {"union": 0, "intersection": 1, "difference": 2, "symmetric_difference": 3}


@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16])
def test_caps(kb):
    tile = rs.setop_caps(kb)
    assert tile > 0 and tile % 256 == 0  # whole workgroups of 256 threads
    assert tile <= 4096                  # what the scan kernel's 32-bit sweep sums allow per tile; a source slot is 16 bits wide
    assert tile == rs.merge_caps(kb)     # the merge's tile: the same staging
    lds = tile * (kb + 2) + 64           # mapped keys, u16 slots, the cuts, the bounds, the waves' totals (include/rsx.h)
    assert 2 * lds <= LDS_PER_CU and lds <= 64 * 1024


@pytest.mark.parametrize("kb", [0, 3, 5, 12, 32])
def test_caps_of_a_bad_width(kb):
    L = _lib.load()
    tile = ctypes.c_uint32()
    assert L.rsx_setop_caps(kb, ctypes.byref(tile)) == _lib.ERR_ARG
    assert L.rsx_setop_caps(4, None) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.setop_caps(kb)


def test_a_null_context_is_refused():
    L = _lib.load()
    assert L.rsx_setop_device(None, 0, 16, None, 10, None, 32, None, 10, None, 4, 0, 0, 0, 64, None, None, 8, 128, None) == _lib.ERR_ARG
    assert L.rsx_setop_device(None, 9, 16, 16, 10, None, 32, 32, 10, None, 3, 0, 12, 0, 64, 64, 64, 4, None, None) == _lib.ERR_ARG
    assert L.rsx_setop_device(None, 1, None, None, 0, None, None, None, 0, None, 4, 0, 0, 0, None, None, None, 0, None, None) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_setop(None, 10, 4) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_setop(None, 10, 3) == _lib.ERR_ARG


def test_argument_errors_of_radix_set_op_need_no_device():
    x = torch.zeros(8, dtype=torch.int32)
    y = torch.zeros(3, dtype=torch.int32)
    fn = rs.radix_set_op
    with pytest.raises(TypeError):
        fn([1, 2], x, "union")  # non-tensors
    with pytest.raises(TypeError):
        fn(x, [1, 2], "union")
    with pytest.raises(TypeError, match="dtype"):
        fn(x, x.to(torch.int64), "union")
    with pytest.raises(TypeError):
        fn(torch.zeros(4, dtype=torch.bool), torch.zeros(4, dtype=torch.bool), "union")
    with pytest.raises(ValueError, match="same device"):
        fn(x, torch.zeros(3, dtype=torch.int32, device="meta"), "union")
    with pytest.raises(ValueError, match="1-D"):
        fn(torch.zeros(4, 4, dtype=torch.int32), x, "union")
    with pytest.raises(ValueError, match="contiguous"):
        fn(torch.zeros(8, 2, dtype=torch.int32)[:, 0], x, "union")
    with pytest.raises(ValueError, match="16"):
        fn(torch.zeros(4, 16, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8), "union")
    with pytest.raises(ValueError, match="key_kind"):
        fn(x, x, "union", key_kind=rs.KEY_SIGNED)  # key_kind= is for 128-bit keys
    for bad in ("xor", "Union", 0, None):
        with pytest.raises(ValueError, match="symmetric_difference"):
            fn(x, y, bad)
    # the capacity of out follows the operation: 11, 3, 8, 11 rows
    for op, cap in (("union", 11), ("intersection", 3), ("difference", 8), ("symmetric_difference", 11)):
        with pytest.raises(ValueError, match="shape"):
            fn(x, y, op, out=torch.zeros(cap + 1, dtype=torch.int32))
        with pytest.raises(ValueError, match="shape"):
            fn(x, y, op, return_index=True, out=(torch.zeros(cap, dtype=torch.int32), torch.zeros(cap - 1, dtype=torch.int64)))
        with pytest.raises(ValueError, match="GPU"):
            fn(x, y, op, out=torch.zeros(cap, dtype=torch.int32))  # the right shape: CPU tensors are the next complaint
    with pytest.raises(TypeError):
        fn(x, y, "union", out=[0] * 11)
    with pytest.raises(TypeError, match="dtype"):
        fn(x, y, "union", out=torch.zeros(11, dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        fn(x, y, "union", out=torch.zeros(11, 2, dtype=torch.int32)[:, 0])  # the right shape, not contiguous
    with pytest.raises(ValueError, match="same device"):
        fn(x, y, "union", out=torch.zeros(11, dtype=torch.int32, device="meta"))
    with pytest.raises(TypeError, match="pair"):
        fn(x, y, "union", return_index=True, out=torch.zeros(11, dtype=torch.int32))
    with pytest.raises(TypeError):
        fn(x, y, "union", return_index=True, out=(torch.zeros(11, dtype=torch.int32), torch.zeros(11, dtype=torch.int16)))
    with pytest.raises(ValueError, match="same device"):
        fn(x, y, "union", return_index=True, out=(torch.zeros(11, dtype=torch.int32), torch.zeros(11, dtype=torch.int64, device="meta")))
    with pytest.raises(ValueError, match="index_dtype"):
        fn(x, y, "union", return_index=True, index_dtype=torch.int16)
    for name in ("a_num", "b_num"):
        with pytest.raises(TypeError, match=name):
            fn(x, y, "union", **{name: 5})
        with pytest.raises(TypeError, match=name):
            fn(x, y, "union", **{name: torch.zeros(1, dtype=torch.int32)})
        with pytest.raises(TypeError, match=name):
            fn(x, y, "union", **{name: torch.zeros(2, dtype=torch.int64)})
        with pytest.raises(ValueError, match="same device"):
            fn(x, y, "union", **{name: torch.zeros((), dtype=torch.int64, device="meta")})
    with pytest.raises(ValueError, match="GPU"):
        fn(x, y, "union", a_num=torch.zeros((), dtype=torch.int64))  # CPU tensors
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())


def test_argument_errors_of_radix_set_op_pairs_need_no_device():
    x, y = torch.zeros(8, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    vx, vy = torch.zeros(8, 2, dtype=torch.float32), torch.zeros(3, 2, dtype=torch.float32)
    fn = rs.radix_set_op_pairs
    with pytest.raises(TypeError):
        fn(x, [0] * 8, y, vy, "union")
    with pytest.raises(TypeError):
        fn(x, None, y, vy, "union")
    for op in ("union", "symmetric_difference"):
        with pytest.raises(TypeError, match="b_values"):
            fn(x, vx, y, None, op)  # these emit from b
    for op in ("intersection", "difference"):
        with pytest.raises(ValueError, match="GPU"):
            fn(x, vx, y, None, op)  # these do not: the next complaint is about CPU tensors
    with pytest.raises(ValueError, match="symmetric_difference"):
        fn(x, vx, y, vy, "minus")
    with pytest.raises(TypeError, match="dtype"):
        fn(x, vx, y.to(torch.int64), vy, "union")
    with pytest.raises(TypeError, match="dtype"):
        fn(x, vx, y, vy.to(torch.float64), "union")
    with pytest.raises(ValueError, match="leading shape"):
        fn(x, vx[:7], y, vy, "union")  # one row per key
    with pytest.raises(ValueError, match="trailing shape"):
        fn(x, vx, y, torch.zeros(3, 4, dtype=torch.float32), "union")
    with pytest.raises(ValueError, match="contiguous"):
        fn(x, torch.zeros(8, 2, 2, dtype=torch.float32)[:, :, 0], y, vy, "union")
    for width in (3, 5, 6):  # 12, 20 and 24 bytes: the kernel does not move them
        with pytest.raises(ValueError, match="return_index=True"):
            fn(x, torch.zeros(8, width, dtype=torch.float32), y, torch.zeros(3, width, dtype=torch.float32), "union")
    with pytest.raises(ValueError, match="same device"):
        fn(x, vx, y, torch.zeros(3, 2, dtype=torch.float32, device="meta"), "union")
    with pytest.raises(TypeError, match="pair"):
        fn(x, vx, y, vy, "union", out=torch.zeros(11, dtype=torch.int32))
    with pytest.raises(TypeError, match="dtype"):
        fn(x, vx, y, vy, "union", out=(torch.zeros(11, dtype=torch.int32), torch.zeros(11, 2, dtype=torch.float64)))
    with pytest.raises(ValueError, match="shape"):
        fn(x, vx, y, vy, "difference", out=(torch.zeros(8, dtype=torch.int32), torch.zeros(11, 2, dtype=torch.float32)))
    with pytest.raises(ValueError, match="shape"):
        fn(x, vx, y, vy, "intersection", out=(torch.zeros(8, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.float32)))
    with pytest.raises(TypeError, match="a_num"):
        fn(x, vx, y, vy, "union", a_num=3)
    with pytest.raises(ValueError, match="GPU"):
        fn(x, vx, y, vy, "union")  # CPU tensors
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())
