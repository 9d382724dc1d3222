"""Host side of the top-k calls (no GPU): the prototypes and their bindings, rsx_topk_caps, and the argument errors of
radix_topk, which are raised before any context or device is touched."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_topk_rows_device", "rsx_ctx_reserve_topk", "rsx_topk_caps"]


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
    assert L.rsx_version() == 200


@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16])
def test_caps(kb):
    caps, max_k = rs.topk_caps(kb)
    assert len(caps) == _lib.SEG_CLASSES and all(c > 0 for c in caps)
    assert caps == sorted(caps) and len(set(caps)) == len(caps)
    assert 0 < max_k <= caps[-1] // 2
    # the classes of the joined (key, u32 position) element, unless the kernel's own register budget lowered them
    pairs = rs.segment_pairs_caps(kb, 4)
    assert all(c <= p for c, p in zip(caps, pairs)), (caps, pairs)


@pytest.mark.parametrize("kb", [0, 3, 5, 12, 32])
def test_caps_of_a_bad_width(kb):
    L = _lib.load()
    caps = (ctypes.c_uint32 * _lib.SEG_CLASSES)()
    max_k = ctypes.c_uint32()
    assert L.rsx_topk_caps(kb, caps, ctypes.byref(max_k)) == _lib.ERR_ARG
    assert L.rsx_topk_caps(4, None, ctypes.byref(max_k)) == _lib.ERR_ARG
    assert L.rsx_topk_caps(4, caps, None) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.topk_caps(kb)


def test_argument_errors_need_no_device():
    x = torch.zeros(3, 8, dtype=torch.float32)
    with pytest.raises(TypeError):
        rs.radix_topk([1.0, 2.0], 1)
    with pytest.raises(TypeError):
        rs.radix_topk(x.numpy(), 1)
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_topk(x.t(), 1)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_topk(x, 1)
    with pytest.raises(ValueError, match="k must be"):
        rs.radix_topk(x, -1)
    with pytest.raises(ValueError, match="k must be"):
        rs.radix_topk(x, 9)
    for bad in (torch.int16, torch.float32, torch.uint8):
        with pytest.raises(ValueError, match="index_dtype"):
            rs.radix_topk(x, 2, index_dtype=bad)
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())


def test_a_null_context_is_refused():
    L = _lib.load()
    assert L.rsx_topk_rows_device(None, 16, 16, 16, 2, 10, 3, 4, 0, 8, 0, None) == _lib.ERR_ARG
    assert L.rsx_ctx_reserve_topk(None, 2, 10, 3, 4) == _lib.ERR_ARG
