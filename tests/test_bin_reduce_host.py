"""Host side of the per-bin reduction (no GPU): the prototypes and their bindings, rsx_bin_reduce_caps, the argument errors
the C call answers before it looks at its context -- so a null context shows every one of them --, and those of
radix_bin_reduce, radix_histogram(weights=) and radix_bincount(weights=), which are raised before any context exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_bin_reduce_device", "rsx_ctx_reserve_bin_reduce", "rsx_bin_reduce_caps"]
WAVES = 4  # of the first launch: one row of m + 1 accumulators each


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
    assert [len(getattr(L, name).argtypes) for name in NAMES] == [19, 5, 6]
    for name in ("radix_bin_reduce", "bin_reduce_caps"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert callable(rs.Context.bin_reduce_device) and callable(rs.Context.reserve_bin_reduce)
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in rust, name
    cxx = open(os.path.join(ROOT, "radix_sort_amd", "cxx", "radix_sort.hpp")).read()
    assert "rsx_bin_reduce_device(" in cxx and "rsx_bin_reduce_caps(" in cxx
    assert re.search(r"\bvoid bin_reduce\(", cxx) and re.search(r"\bBinReduceCaps bin_reduce_caps\(", cxx)


@pytest.mark.parametrize("kb", (1, 2, 4, 8, 16))
@pytest.mark.parametrize("vb", (4, 8))
def test_caps(kb, vb):
    max_edges, max_index_bins, tile, share = rs.bin_reduce_caps(kb, vb)
    assert 1023 <= max_edges <= 2047 and 1023 <= max_index_bins <= 2047  # the 11 bits of the wave match
    assert tile >= 256 and tile % 256 == 0  # whole rounds of the four waves
    assert share == rs.bin_caps(kb)[2]      # the shares of the bin count
    # static LDS of the first launch: the mapped edges, m + 1 accumulators per wave, m + 1 counters: two workgroups per CU ...
    assert max_edges * kb + (max_edges + 1) * (WAVES * vb + 4) <= 80 * 1024
    assert (max_index_bins + 1) * (WAVES * vb + 4) <= 80 * 1024
    # ... and the largest m that allows it, up to the alignment of the three arrays
    if max_edges < 2047:
        assert (max_edges + 2) * kb + (max_edges + 3) * (WAVES * vb + 4) > 80 * 1024
    assert max_index_bins == 2047
    assert max_edges <= rs.partition_caps(kb)[0]


@pytest.mark.parametrize("kb,vb", [(0, 4), (3, 4), (5, 8), (12, 4), (32, 8), (4, 0), (4, 1), (4, 2), (4, 16), (8, 12)])
def test_caps_of_bad_widths(kb, vb):
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(4)]
    assert L.rsx_bin_reduce_caps(kb, vb, *[ctypes.byref(o) for o in out]) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.bin_reduce_caps(kb, vb)


def test_caps_of_a_null_pointer():
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(4)]
    for missing in range(4):
        args = [None if i == missing else ctypes.byref(o) for i, o in enumerate(out)]
        assert L.rsx_bin_reduce_caps(4, 4, *args) == _lib.ERR_ARG


def _call(**over):
    """rsx_bin_reduce_device with a null context on made-up, suitably aligned addresses: a call that is in order (so the
    null context is all that is wrong with it) unless `over` changes an argument."""
    a = dict(keys=0x10000, values=0x40000, n=10, num=0x20000, kb=4, kind=0, edges=0x30000, m=5, mode=0, order=0, vb=8, vkind=1, op=0,
             out_values=0x60000, out_counts=0x70000, cb=8, flags=0)
    a.update(over)
    L = _lib.load()
    return L.rsx_bin_reduce_device(None, a["keys"] or None, a["values"] or None, a["n"], a["num"] or None, a["kb"], a["kind"], a["edges"] or None,
                                   a["m"], a["mode"], a["order"], a["vb"], a["vkind"], a["op"], a["out_values"] or None, a["out_counts"] or None,
                                   a["cb"], a["flags"], None)


def test_argument_errors_are_answered_before_the_context():
    ARG, UNSUPPORTED = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED
    far = dict(keys=1 << 40, values=2 << 40)  # columns of 2^32 rows apart
    big = dict(far, n=1 << 32)
    assert _call() == ARG  # nothing wrong but the null context
    assert _call(**big) == UNSUPPORTED  # ... which therefore is looked at last: this one is not ERR_ARG
    assert _call(**dict(far, n=(1 << 32) - 1)) == ARG
    for kb in (1, 2, 4, 8, 16):
        for vb in (4, 8):
            E, EI, _t, _s = rs.bin_reduce_caps(kb, vb)
            assert _call(kb=kb, vb=vb, m=E) == ARG and _call(kb=kb, vb=vb, m=E + 1) == UNSUPPORTED, (kb, vb)
            if kb <= 8:
                assert _call(kb=kb, vb=vb, mode=2, edges=0, m=EI) == ARG and _call(kb=kb, vb=vb, mode=2, edges=0, m=EI + 1) == UNSUPPORTED, (kb, vb)
    for kb in (0, 3, 5, 12, 32):
        assert _call(**dict(big, kb=kb)) == ARG, kb              # a bad width comes before the size
    assert _call(**dict(big, kind=3)) == ARG
    assert _call(**dict(big, kb=16, kind=2)) == ARG              # no 128-bit floats
    for vb in (0, 1, 2, 3, 12, 16):
        assert _call(**dict(big, vb=vb)) == ARG, vb
    assert _call(**dict(big, vkind=3)) == ARG
    assert _call(**dict(big, op=3)) == ARG and _call(**dict(big, op=-1)) == ARG
    assert _call(**dict(big, mode=3)) == ARG
    assert _call(**dict(big, flags=2)) == ARG and _call(**dict(big, flags=1)) == UNSUPPORTED
    assert _call(**dict(big, order=2)) == ARG and _call(**dict(big, order=-1)) == ARG
    assert _call(**dict(big, mode=2)) == ARG                     # the index mode takes no edges ...
    assert _call(**dict(big, mode=2, edges=0, order=1)) == ARG   # ... and no order
    assert _call(**dict(big, mode=2, edges=0)) == UNSUPPORTED
    assert _call(mode=2, edges=0, kind=2) == UNSUPPORTED         # ... and integer keys of at most 8 bytes
    assert _call(mode=2, edges=0, kb=16) == UNSUPPORTED
    assert _call(**dict(big, cb=2)) == ARG and _call(**dict(big, cb=16)) == ARG
    assert _call(**dict(big, cb=2, out_counts=0)) == UNSUPPORTED  # count_bytes is not looked at without a count output
    assert _call(**dict(big, out_values=0)) == ARG               # the values are required
    assert _call(**dict(big, out_counts=0)) == UNSUPPORTED       # the counts are optional
    assert _call(**dict(big, keys=0)) == ARG and _call(keys=0) == ARG  # a needed pointer NULL with n > 0 ...
    assert _call(**dict(big, values=0)) == ARG and _call(values=0) == ARG
    assert _call(keys=0, values=0, n=0) == ARG                   # (n == 0 needs none: only the null context is left to refuse)
    assert _call(**dict(big, edges=0)) == ARG                    # ... or with m > 0
    assert _call(**dict(big, edges=0, m=0)) == UNSUPPORTED
    assert _call(**dict(big, edges=0, m=0, keys=0)) == UNSUPPORTED  # m == 0 reads no key
    # misaligned pointers: keys and edges to key_bytes, values to value_bytes, counts to count_bytes, d_num to 8
    assert _call(**dict(big, keys=far["keys"] + 2)) == ARG
    assert _call(**dict(big, kb=16, keys=far["keys"] + 8)) == ARG
    assert _call(**dict(big, kb=1, keys=far["keys"] + 1)) == UNSUPPORTED
    assert _call(**dict(big, edges=0x30002)) == ARG and _call(**dict(big, kb=1, edges=0x30001)) == UNSUPPORTED
    assert _call(**dict(big, values=far["values"] + 4)) == ARG and _call(**dict(big, vb=4, values=far["values"] + 4)) == UNSUPPORTED
    assert _call(**dict(big, out_values=0x60004)) == ARG and _call(**dict(big, vb=4, out_values=0x60004)) == UNSUPPORTED
    assert _call(**dict(big, out_counts=0x70004)) == ARG and _call(**dict(big, cb=4, out_counts=0x70004)) == UNSUPPORTED
    assert _call(**dict(big, num=0x20004)) == ARG
    # any overlap of an output with an input, or with the other output
    assert _call(out_values=0x10000) == ARG and _call(out_values=0x10000 + 32) == ARG and _call(out_values=0x10000 + 40, n=1 << 32) == ARG
    assert _call(out_values=0x40000 + 72) == ARG and _call(out_counts=0x40000) == ARG
    assert _call(out_values=0x20000) == ARG and _call(out_counts=0x20000) == ARG   # the device row count
    assert _call(out_values=0x30000 + 16) == ARG                 # the edges
    assert _call(out_values=0x30000 - 40) == ARG                 # m + 1 values reach the edges
    assert _call(**dict(big, out_values=0x30000 - 40)) == ARG and _call(**dict(big, out_values=0x30000 - 48)) == UNSUPPORTED
    assert _call(out_counts=0x60000 + 40) == ARG                 # the two outputs
    assert _call(**dict(big, out_counts=0x60000 + 48)) == UNSUPPORTED
    L = _lib.load()
    assert L.rsx_ctx_reserve_bin_reduce(None, 10, 5, 4, 4) == ARG


def test_argument_errors_need_no_device():
    x = torch.zeros(8, dtype=torch.int32)
    e = torch.zeros(3, dtype=torch.int32)
    w = torch.zeros(8, dtype=torch.float32)
    with pytest.raises(ValueError, match="exactly one"):
        rs.radix_bin_reduce(x, w)
    with pytest.raises(ValueError, match="exactly one"):
        rs.radix_bin_reduce(x, w, edges=e, num_bins=4)
    with pytest.raises(TypeError):
        rs.radix_bin_reduce([1, 2, 3], w, num_bins=4)  # not a tensor
    with pytest.raises(TypeError):
        rs.radix_bin_reduce(x, [1.0] * 8, num_bins=4)
    with pytest.raises(TypeError, match="edges"):
        rs.radix_bin_reduce(x, w, edges=[1, 2])
    with pytest.raises(TypeError, match="dtype"):
        rs.radix_bin_reduce(x, w, edges=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="op must be"):
        rs.radix_bin_reduce(x, w, edges=e, op="mean")
    for dtype in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(TypeError, match="values must be"):
            rs.radix_bin_reduce(x, torch.zeros(8, dtype=dtype), edges=e)
        with pytest.raises(TypeError, match="values must be"):
            rs.radix_histogram(x, e, weights=torch.zeros(8, dtype=dtype))
        with pytest.raises(TypeError, match="values must be"):
            rs.radix_bincount(x, 4, weights=torch.zeros(8, dtype=dtype))
    with pytest.raises(ValueError, match="side"):
        rs.radix_bin_reduce(x, w, edges=e, side="middle")
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_bin_reduce(torch.zeros(8, 2, dtype=torch.int32)[:, 0], w, edges=e)
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_bin_reduce(x, torch.zeros(8, 2, dtype=torch.float32)[:, 0], edges=e)
    with pytest.raises(ValueError, match="one entry per key"):
        rs.radix_bin_reduce(x, torch.zeros(7, dtype=torch.float32), edges=e)
    with pytest.raises(TypeError, match="integer keys"):
        rs.radix_bin_reduce(torch.zeros(8, dtype=torch.float32), w, num_bins=4)
    with pytest.raises(TypeError, match="integer keys"):
        rs.radix_bin_reduce(torch.zeros(8, 16, dtype=torch.uint8), w, num_bins=4, key_kind=rs.KEY_UNSIGNED)  # 128-bit keys
    with pytest.raises(ValueError, match="descending"):
        rs.radix_bin_reduce(x, w, num_bins=4, descending=True)
    with pytest.raises(ValueError, match="num_bins"):
        rs.radix_bin_reduce(x, w, num_bins=-1)
    with pytest.raises(TypeError):
        rs.radix_bin_reduce(x, w, num_bins=2.5)
    for num in (3, torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(TypeError, match="num"):
            rs.radix_bin_reduce(x, w, edges=e, num=num)
    with pytest.raises(ValueError, match="accumulate"):
        rs.radix_bin_reduce(x, w, edges=e, accumulate=True)
    with pytest.raises(ValueError, match="accumulate"):
        rs.radix_bin_reduce(x, w, edges=e, out=torch.zeros(4), accumulate=True, return_counts=True)  # nothing to add the counts to
    with pytest.raises(TypeError, match="out must be"):
        rs.radix_bin_reduce(x, w, edges=e, out=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TypeError, match="out must be"):
        rs.radix_bin_reduce(x, w, edges=e, out=(torch.zeros(4), torch.zeros(4, dtype=torch.int64), None), return_counts=True)
    with pytest.raises(ValueError, match="shape"):
        rs.radix_bin_reduce(x, w, edges=e, out=torch.zeros(5))
    with pytest.raises(ValueError, match="shape"):
        rs.radix_bin_reduce(x, w, num_bins=4, out=torch.zeros(4))  # num_bins + 1 values
    with pytest.raises(ValueError, match="return_counts"):
        rs.radix_bin_reduce(x, w, edges=e, out=(torch.zeros(4), torch.zeros(4, dtype=torch.int64)))
    with pytest.raises(TypeError, match="int32 or int64"):
        rs.radix_bin_reduce(x, w, edges=e, out=(torch.zeros(4), torch.zeros(4, dtype=torch.int16)), return_counts=True)
    with pytest.raises(ValueError, match="count_dtype"):
        rs.radix_bin_reduce(x, w, edges=e, return_counts=True, count_dtype=torch.int16)
    with pytest.raises(ValueError, match="count_dtype"):
        rs.radix_histogram(x, e, weights=w, count_dtype=torch.int32)
    with pytest.raises(ValueError, match="count_dtype"):
        rs.radix_bincount(x, 4, weights=w, count_dtype=torch.int32)
    # past the caps a device row count has no route
    E, EI, _t, _s = rs.bin_reduce_caps(4, 4)
    num = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match=f"{E} edges or {EI} bins"):
        rs.radix_bin_reduce(x, w, edges=torch.zeros(E + 1, dtype=torch.int32), num=num)
    with pytest.raises(ValueError, match=f"{E} edges or {EI} bins"):
        rs.radix_bin_reduce(x, w, num_bins=EI + 1, num=num)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_bin_reduce(x, w, edges=e)  # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_bin_reduce(x, w.to(torch.float64), num_bins=3, op="max", return_counts=True, count_dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_histogram(x, e, weights=w, side="left", descending=True, out=torch.zeros(4), accumulate=True)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_bincount(x, 5, weights=torch.zeros(8, dtype=torch.int64))
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())
