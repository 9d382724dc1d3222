"""Host side of the compaction calls (no GPU): the prototypes and their bindings, rsx_compact_caps, the argument errors the C
call answers before it looks at its context -- so a null context shows every one of them --, and those of radix_compact
and radix_nonzero, which are raised before any context exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_compact_device", "rsx_ctx_reserve_compact", "rsx_compact_caps"]
WIDTHS = (0, 1, 2, 4, 8, 16)


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
    assert [len(getattr(L, name).argtypes) for name in NAMES] == [19, 5, 5]
    assert sorted(_lib.SYMBOLS) == sorted(re.findall(r"\b(rsx_\w+)\s*\(", _header()))  # what test_cabi.py holds the list to
    defines = dict(re.findall(r"#define\s+(RSX_COMPACT_\w+)\s+(\d+)u", _header()))
    assert defines == {"RSX_COMPACT_INVERT": "1", "RSX_COMPACT_PARTITION": "2"}
    assert (rs.COMPACT_INVERT, rs.COMPACT_PARTITION) == (1, 2)
    for name in ("radix_compact", "radix_nonzero", "compact_caps", "Compacted", "COMPACT_INVERT", "COMPACT_PARTITION"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert rs.Compacted._fields == ("keys", "values", "index", "num")
    assert callable(rs.Context.compact_device) and callable(rs.Context.reserve_compact)
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in rust, name
    cxx = open(os.path.join(ROOT, "radix_sort_amd", "cxx", "radix_sort.hpp")).read()
    assert "rsx_compact_device(" in cxx and "rsx_compact_caps(" in cxx
    assert re.search(r"\bvoid compact\(", cxx) and re.search(r"\bCompactCaps compact_caps\(", cxx)


@pytest.mark.parametrize("kb", WIDTHS)
def test_caps(kb):
    for vb in WIDTHS:
        for ib in (0, 4, 8):
            tile, span = rs.compact_caps(kb, vb, ib)
            assert tile >= 256 and tile % 256 == 0 and tile <= 4096  # whole rows per thread; the scan takes at most 4096 per tile
            assert span >= 64
            # static LDS of the write kernel: a key, a value and a two-byte slot per row, the waves' totals: two workgroups per CU
            assert tile * (kb + vb + 2) + 64 <= 80 * 1024, (kb, vb, ib, tile)
    assert rs.compact_caps(kb, 0, 0)[0] >= rs.compact_caps(kb, 16, 8)[0]  # the tile shrinks with the widths, never grows
    # a value width without a typed kernel rides behind positions: the kernels see no values
    assert rs.compact_caps(kb, 12, 0) == rs.compact_caps(kb, 0, 0) == rs.compact_caps(kb, 40, 4)


@pytest.mark.parametrize("widths", [(3, 0, 0), (5, 4, 4), (12, 0, 0), (32, 0, 0), (4, 32769, 0), (4, 4, 2), (4, 4, 16), (0, 0, 1)])
def test_caps_of_bad_widths(widths):
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(2)]
    assert L.rsx_compact_caps(*widths, *[ctypes.byref(o) for o in out]) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.compact_caps(*widths)


def test_caps_of_a_null_pointer():
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(2)]
    for missing in range(2):
        args = [None if i == missing else ctypes.byref(o) for i, o in enumerate(out)]
        assert L.rsx_compact_caps(4, 4, 8, *args) == _lib.ERR_ARG


def _call(**over):
    """rsx_compact_device with a null context on made-up, suitably aligned addresses: a call that is in order (so the
    null context is all that is wrong with it) unless `over` changes an argument."""
    a = dict(keys=0x1000, n=10, num=0x2000, kb=4, kind=0, order=0, flags_p=0x3000, lo=0x4000, hi=0x5000, values=0x6000, vb=8, flags=0,
             out_keys=0x7000, out_values=0x8000, out_index=0x9000, ib=8, out_num=0xA000)
    a.update(over)
    L = _lib.load()
    return L.rsx_compact_device(None, a["keys"] or None, a["n"], a["num"] or None, a["kb"], a["kind"], a["order"], a["flags_p"] or None, a["lo"] or None,
                                a["hi"] or None, a["values"] or None, a["vb"], a["flags"], a["out_keys"] or None, a["out_values"] or None,
                                a["out_index"] or None, a["ib"], a["out_num"] or None, None)


def test_argument_errors_are_answered_before_the_context():
    ARG, UNSUPPORTED = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED
    assert _call() == ARG  # nothing wrong but the null context
    assert _call(n=1 << 32) == UNSUPPORTED  # ... which therefore is looked at last: this one is not ERR_ARG
    assert _call(n=(1 << 32) - 1) == ARG
    for kb in (0, 3, 5, 12, 32):
        assert _call(kb=kb, n=1 << 32) == ARG, kb          # a bad width comes before the size
    assert _call(kind=3, n=1 << 32) == ARG
    assert _call(kb=16, kind=2, n=1 << 32) == ARG          # no 128-bit floats
    assert _call(order=2, n=1 << 32) == ARG and _call(order=-1, n=1 << 32) == ARG
    assert _call(flags=4, n=1 << 32) == ARG and _call(flags=0x80000000, n=1 << 32) == ARG
    assert _call(flags=3, n=1 << 32) == UNSUPPORTED        # both bits together are fine
    assert _call(ib=2, n=1 << 32) == ARG and _call(ib=16, n=1 << 32) == ARG
    assert _call(ib=2, out_index=0, n=1 << 32) == UNSUPPORTED  # index_bytes is not looked at without an index output
    assert _call(out_num=0, n=1 << 32) == ARG
    assert _call(vb=32769, n=1 << 32) == ARG
    assert _call(vb=0, n=1 << 32) == ARG                   # value pointers without a width
    assert _call(values=0, n=1 << 32) == ARG               # a value output without values
    assert _call(keys=0, n=1 << 32) == ARG and _call(keys=0) == ARG  # a needed pointer NULL with n > 0 ...
    assert _call(keys=0, n=0) == ARG                       # (n == 0 needs none: only the null context is left to refuse)
    assert _call(keys=0, lo=0, hi=0, out_keys=0, kb=7, kind=9, n=1 << 32) == UNSUPPORTED  # ... a pure mask call ignores the key type
    # misaligned pointers: keys and bounds to key_bytes, values as rsx_sort_pairs_device, index to index_bytes, num words to 8
    for name in ("keys", "lo", "hi", "out_keys"):
        assert _call(**{name: 0x1002, "n": 1 << 32}) == ARG, name
        assert _call(**{name: 0x1008, "kb": 16, "n": 1 << 32}) == ARG, name
        assert _call(**{name: 0x1001, "kb": 1, "n": 1 << 32}) == UNSUPPORTED, name
    for name in ("values", "out_values"):
        assert _call(**{name: 0x6004, "n": 1 << 32}) == ARG, name
        assert _call(**{name: 0x6004, "vb": 12, "n": 1 << 32}) == UNSUPPORTED, name  # 12-byte values: 4-byte aligned
        assert _call(**{name: 0x6002, "vb": 12, "n": 1 << 32}) == ARG, name
    assert _call(out_index=0x9004, n=1 << 32) == ARG and _call(out_index=0x9004, ib=4, n=1 << 32) == UNSUPPORTED
    assert _call(num=0x2004, n=1 << 32) == ARG and _call(out_num=0xA004, n=1 << 32) == ARG
    assert _call(flags_p=0x3001, n=1 << 32) == UNSUPPORTED  # flag bytes need no alignment
    # an output pointer equal to an input pointer
    assert _call(out_keys=0x1000, n=1 << 32) == ARG and _call(out_values=0x6000, n=1 << 32) == ARG
    assert _call(out_index=0x3000, n=1 << 32) == ARG and _call(out_num=0x2000, n=1 << 32) == ARG
    assert _call(out_keys=0x4000, n=1 << 32) == ARG  # the bound's own word
    L = _lib.load()
    assert L.rsx_ctx_reserve_compact(None, 10, 4, 4, 8) == ARG


def test_argument_errors_need_no_device():
    x = torch.zeros(8, dtype=torch.int32)
    m = torch.zeros(8, dtype=torch.bool)
    v = torch.zeros(8, 3, dtype=torch.float32)
    with pytest.raises(TypeError):
        rs.radix_compact([1, 2, 3], mask=m)  # not a tensor
    with pytest.raises(ValueError, match="needs a mask"):
        rs.radix_compact(None)
    with pytest.raises(ValueError, match="key_kind"):
        rs.radix_compact(None, mask=m, key_kind=rs.KEY_SIGNED)
    with pytest.raises(ValueError, match="key_kind"):
        rs.radix_compact(x, mask=m, key_kind=rs.KEY_SIGNED)  # key_kind= is for 128-bit keys
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_compact(torch.zeros(8, 2, dtype=torch.int32)[:, 0], mask=m)
    with pytest.raises(TypeError):
        rs.radix_compact(torch.zeros(8, dtype=torch.bool), mask=m)  # no bool keys
    for bad in ([1, 0], torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.float32)):
        with pytest.raises(TypeError, match="mask"):
            rs.radix_compact(x, mask=bad)
    with pytest.raises(ValueError, match="mask"):
        rs.radix_compact(x, mask=torch.zeros(7, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask"):
        rs.radix_compact(x, mask=torch.zeros(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask"):
        rs.radix_compact(x, mask=torch.zeros(8, 2, dtype=torch.uint8)[:, 0])
    with pytest.raises(ValueError, match="lo needs keys"):
        rs.radix_compact(None, mask=m, lo=3)
    with pytest.raises(TypeError, match="dtype"):
        rs.radix_compact(x, lo=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="one key"):
        rs.radix_compact(x, hi=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError, match="hi"):
        rs.radix_compact(x, hi="3")
    with pytest.raises(TypeError, match="lo"):
        rs.radix_compact(torch.zeros(4, 16, dtype=torch.uint8), lo=5)  # a 128-bit bound is a tensor
    with pytest.raises(ValueError, match="leading shape"):
        rs.radix_compact(x, mask=m, values=torch.zeros(7, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_compact(x, mask=m, values=torch.zeros(8, 2, dtype=torch.int32)[:, 0])
    with pytest.raises(ValueError, match="index_dtype"):
        rs.radix_compact(x, mask=m, return_index=True, index_dtype=torch.int16)
    for num in (3, torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(TypeError, match="num"):
            rs.radix_compact(x, mask=m, num=num)
    num = torch.zeros((), dtype=torch.int64)
    with pytest.raises(TypeError, match="Compacted"):
        rs.radix_compact(x, mask=m, out=(x, num))
    with pytest.raises(TypeError, match="dtype"):
        rs.radix_compact(x, mask=m, out=rs.Compacted(torch.zeros(8, dtype=torch.int64), None, None, num))
    with pytest.raises(ValueError, match="shape"):
        rs.radix_compact(x, mask=m, out=rs.Compacted(torch.zeros(7, dtype=torch.int32), None, None, num))
    with pytest.raises(ValueError, match="needs values"):
        rs.radix_compact(x, mask=m, out=rs.Compacted(None, v.clone(), None, num))
    with pytest.raises(ValueError, match="needs keys"):
        rs.radix_compact(None, mask=m, out=rs.Compacted(x.clone(), None, None, num))
    with pytest.raises(ValueError, match="shape"):
        rs.radix_compact(x, mask=m, values=v, out=rs.Compacted(None, torch.zeros(8, 2, dtype=torch.float32), None, num))
    with pytest.raises(TypeError, match="int32 or int64"):
        rs.radix_compact(x, mask=m, out=rs.Compacted(None, None, torch.zeros(8, dtype=torch.int16), num))
    with pytest.raises(TypeError, match="index_dtype"):
        rs.radix_compact(x, mask=m, index_dtype=torch.int32, out=rs.Compacted(None, None, torch.zeros(8, dtype=torch.int64), num))
    with pytest.raises(ValueError, match="out.index"):
        rs.radix_compact(x, mask=m, return_index=True, out=rs.Compacted(x.clone(), None, None, num))
    for bad in (None, 3, torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(TypeError, match="out.num"):
            rs.radix_compact(x, mask=m, out=rs.Compacted(x.clone(), None, None, bad))
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_compact(x, mask=m)  # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_compact(x, lo=2, hi=5, values=v, descending=True, invert=True, partition=True, return_index=True, index_dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_compact(None, mask=m, values=v, out=rs.Compacted(None, v.clone(), torch.zeros(8, dtype=torch.int32), num))

    with pytest.raises(TypeError, match="mask"):
        rs.radix_nonzero(None)
    with pytest.raises(TypeError, match="mask"):
        rs.radix_nonzero(x)
    with pytest.raises(ValueError, match="mask"):
        rs.radix_nonzero(torch.zeros(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="index_dtype"):
        rs.radix_nonzero(m, index_dtype=torch.float32)
    with pytest.raises(TypeError, match="pair"):
        rs.radix_nonzero(m, out=torch.zeros(8, dtype=torch.int64))
    with pytest.raises(TypeError, match="pair"):
        rs.radix_nonzero(m, out=(None, num))
    with pytest.raises(ValueError, match="shape"):
        rs.radix_nonzero(m, out=(torch.zeros(9, dtype=torch.int64), num))
    with pytest.raises(TypeError, match="num"):
        rs.radix_nonzero(m, num=4)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_nonzero(m)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_nonzero(m.to(torch.uint8), index_dtype=torch.int32, out=(torch.zeros(8, dtype=torch.int32), num))
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())
