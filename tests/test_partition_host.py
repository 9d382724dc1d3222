"""Host side of the multi-way partition (no GPU): the prototypes and their bindings, rsx_multisplit_caps, the argument
errors the C call answers before it looks at its context -- so a null context shows every one of them --, and those of
radix_partition, which are raised before any context exists."""
import ctypes
import os
import re

import pytest
import torch

import radix_sort_amd as rs
from radix_sort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rsx_multisplit_device", "rsx_ctx_reserve_multisplit", "rsx_multisplit_caps"]
WAVES = 4  # of the write kernel: one set of m + 1 counters each


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
    assert [len(getattr(L, name).argtypes) for name in NAMES] == [18, 6, 5]
    for name in ("radix_partition", "partition_caps", "Partitioned"):
        assert name in rs.__all__ and hasattr(rs, name)
    assert rs.Partitioned._fields == ("keys", "values", "index", "offsets")
    assert callable(rs.Context.multisplit_device) and callable(rs.Context.reserve_multisplit)
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in rust, name
    cxx = open(os.path.join(ROOT, "radix_sort_amd", "cxx", "radix_sort.hpp")).read()
    assert "rsx_multisplit_device(" in cxx and "rsx_multisplit_caps(" in cxx
    assert re.search(r"\bvoid multisplit\(", cxx) and re.search(r"\bMultisplitCaps multisplit_caps\(", cxx)


@pytest.mark.parametrize("kb", (1, 2, 4, 8, 16))
def test_caps(kb):
    max_edges, max_index_bins, tile, share = rs.partition_caps(kb)
    assert max_edges >= 2047 and max_index_bins >= 2047
    assert tile >= 256 and tile % 256 == 0  # whole rounds of the four waves
    assert share == rs.bin_caps(kb)[2]      # the shares of the bin count
    # static LDS of the write kernel: the mapped edges, m + 1 cursors, m + 1 counters per wave: two workgroups per CU
    assert max_edges * kb + (max_edges + 1) * 4 + WAVES * (max_edges + 1) * 4 <= 80 * 1024
    assert (max_index_bins + 1) * 4 + WAVES * (max_index_bins + 1) * 4 <= 80 * 1024


@pytest.mark.parametrize("kb", (0, 3, 5, 12, 32))
def test_caps_of_bad_widths(kb):
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(4)]
    assert L.rsx_multisplit_caps(kb, *[ctypes.byref(o) for o in out]) == _lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.partition_caps(kb)


def test_caps_of_a_null_pointer():
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(4)]
    for missing in range(4):
        args = [None if i == missing else ctypes.byref(o) for i, o in enumerate(out)]
        assert L.rsx_multisplit_caps(4, *args) == _lib.ERR_ARG


def _call(**over):
    """rsx_multisplit_device with a null context on made-up, suitably aligned addresses: a call that is in order (so the
    null context is all that is wrong with it) unless `over` changes an argument."""
    a = dict(keys=0x10000, n=10, num=0x20000, kb=4, kind=0, edges=0x30000, m=5, mode=0, order=0, values=0x40000, vb=8, out_keys=0x50000,
             out_values=0x60000, out_index=0x70000, ib=8, out_offsets=0x80000)
    a.update(over)
    L = _lib.load()
    return L.rsx_multisplit_device(None, a["keys"] or None, a["n"], a["num"] or None, a["kb"], a["kind"], a["edges"] or None, a["m"], a["mode"],
                                   a["order"], a["values"] or None, a["vb"], a["out_keys"] or None, a["out_values"] or None,
                                   a["out_index"] or None, a["ib"], a["out_offsets"] or None, None)


def test_argument_errors_are_answered_before_the_context():
    ARG, UNSUPPORTED = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED
    E = rs.partition_caps(4)[0]
    far = dict(keys=1 << 40, values=2 << 40, out_keys=3 << 40, out_values=4 << 40, out_index=5 << 40)  # columns of 2^32 rows apart
    big = dict(far, n=1 << 32)
    assert _call() == ARG  # nothing wrong but the null context
    assert _call(**big) == UNSUPPORTED  # ... which therefore is looked at last: this one is not ERR_ARG
    assert _call(**dict(far, n=(1 << 32) - 1)) == ARG
    assert _call(m=E) == ARG and _call(m=E + 1) == UNSUPPORTED
    assert _call(mode=2, edges=0, m=E + 1) == UNSUPPORTED and _call(mode=2, edges=0, m=E) == ARG
    for kb in (0, 3, 5, 12, 32):
        assert _call(**dict(big, kb=kb)) == ARG, kb              # a bad width comes before the size
    assert _call(**dict(big, kind=3)) == ARG
    assert _call(**dict(big, kb=16, kind=2)) == ARG              # no 128-bit floats
    assert _call(**dict(big, mode=3)) == ARG
    assert _call(**dict(big, order=2)) == ARG and _call(**dict(big, order=-1)) == ARG
    assert _call(**dict(big, mode=2)) == ARG                     # the index mode takes no edges ...
    assert _call(**dict(big, mode=2, edges=0, order=1)) == ARG   # ... and no order
    assert _call(**dict(big, mode=2, edges=0)) == UNSUPPORTED
    assert _call(mode=2, edges=0, kind=2) == UNSUPPORTED         # ... and integer keys of at most 8 bytes
    assert _call(mode=2, edges=0, kb=16) == UNSUPPORTED
    assert _call(**dict(big, ib=2)) == ARG and _call(**dict(big, ib=16)) == ARG
    assert _call(**dict(big, ib=2, out_index=0)) == UNSUPPORTED  # index_bytes is not looked at without an index output
    assert _call(**dict(big, out_offsets=0)) == ARG
    assert _call(**dict(big, vb=32769)) == ARG
    assert _call(**dict(big, vb=0)) == ARG                       # value pointers without a width
    assert _call(**dict(big, values=0)) == ARG                   # a value output without values
    assert _call(**dict(big, keys=0)) == ARG and _call(keys=0) == ARG  # a needed pointer NULL with n > 0 ...
    assert _call(keys=0, n=0) == ARG                             # (n == 0 needs none: only the null context is left to refuse)
    assert _call(**dict(big, edges=0)) == ARG                    # ... or with m > 0
    assert _call(**dict(big, edges=0, m=0)) == UNSUPPORTED
    assert _call(**dict(big, out_keys=0, out_values=0, out_index=0)) == UNSUPPORTED  # every row output is optional
    # misaligned pointers: keys and edges to key_bytes, values as rsx_sort_pairs_device, index to index_bytes, words to 8
    for name in ("keys", "out_keys"):
        assert _call(**dict(big, **{name: far[name] + 2})) == ARG, name
        assert _call(**dict(big, kb=16, **{name: far[name] + 8})) == ARG, name
        assert _call(**dict(big, kb=1, **{name: far[name] + 1})) == UNSUPPORTED, name
    assert _call(**dict(big, edges=0x30002)) == ARG and _call(**dict(big, kb=1, edges=0x30001)) == UNSUPPORTED
    for name in ("values", "out_values"):
        assert _call(**dict(big, **{name: far[name] + 4})) == ARG, name
        assert _call(**dict(big, vb=12, **{name: far[name] + 4})) == UNSUPPORTED, name  # 12-byte values: 4-byte aligned
        assert _call(**dict(big, vb=12, **{name: far[name] + 2})) == ARG, name
    assert _call(**dict(big, out_index=far["out_index"] + 4)) == ARG
    assert _call(**dict(big, out_index=far["out_index"] + 4, ib=4)) == UNSUPPORTED
    assert _call(**dict(big, num=0x20004)) == ARG and _call(**dict(big, out_offsets=0x80004)) == ARG
    # any overlap of an output with an input, or with another output
    assert _call(out_keys=0x10000) == ARG and _call(out_keys=0x10000 + 36) == ARG and _call(out_keys=0x10000 + 40, n=1 << 32) == ARG
    assert _call(out_values=0x40000 + 72) == ARG and _call(out_index=0x20000) == ARG and _call(out_offsets=0x20000) == ARG
    assert _call(out_keys=0x30000 + 16) == ARG                   # the edges
    assert _call(out_offsets=0x30000 - 48) == ARG                # m + 2 offsets reach the edges
    assert _call(**dict(big, out_offsets=0x30000 - 56)) == UNSUPPORTED
    assert _call(out_index=0x50000 + 32) == ARG                  # two outputs
    L = _lib.load()
    assert L.rsx_ctx_reserve_multisplit(None, 10, 5, 4, 4, 8) == ARG


def test_argument_errors_need_no_device():
    x = torch.zeros(8, dtype=torch.int32)
    e = torch.zeros(3, dtype=torch.int32)
    v = torch.zeros(8, 3, dtype=torch.float32)
    off = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="exactly one"):
        rs.radix_partition(x)
    with pytest.raises(ValueError, match="exactly one"):
        rs.radix_partition(x, edges=e, num_bins=4)
    with pytest.raises(TypeError):
        rs.radix_partition([1, 2, 3], num_bins=4)  # not a tensor
    with pytest.raises(TypeError, match="edges"):
        rs.radix_partition(x, edges=[1, 2])
    with pytest.raises(TypeError, match="dtype"):
        rs.radix_partition(x, edges=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="side"):
        rs.radix_partition(x, edges=e, side="middle")
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_partition(torch.zeros(8, 2, dtype=torch.int32)[:, 0], edges=e)
    with pytest.raises(ValueError, match="key_kind"):
        rs.radix_partition(x, edges=e, key_kind=rs.KEY_SIGNED)  # key_kind= is for 128-bit keys
    with pytest.raises(TypeError, match="integer keys"):
        rs.radix_partition(torch.zeros(8, dtype=torch.float32), num_bins=4)
    with pytest.raises(TypeError, match="integer keys"):
        rs.radix_partition(torch.zeros(8, 16, dtype=torch.uint8), num_bins=4)
    with pytest.raises(ValueError, match="descending"):
        rs.radix_partition(x, num_bins=4, descending=True)
    with pytest.raises(ValueError, match="num_bins"):
        rs.radix_partition(x, num_bins=-1)
    with pytest.raises(TypeError):
        rs.radix_partition(x, num_bins=2.5)
    with pytest.raises(ValueError, match="leading shape"):
        rs.radix_partition(x, edges=e, values=torch.zeros(7, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_partition(x, edges=e, values=torch.zeros(8, 2, dtype=torch.int32)[:, 0])
    with pytest.raises(ValueError, match="index_dtype"):
        rs.radix_partition(x, edges=e, return_index=True, index_dtype=torch.int16)
    for num in (3, torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(TypeError, match="num"):
            rs.radix_partition(x, edges=e, num=num)
    with pytest.raises(TypeError, match="Partitioned"):
        rs.radix_partition(x, edges=e, out=(x, off))
    with pytest.raises(TypeError, match="dtype"):
        rs.radix_partition(x, edges=e, out=rs.Partitioned(torch.zeros(8, dtype=torch.int64), None, None, off))
    with pytest.raises(ValueError, match="shape"):
        rs.radix_partition(x, edges=e, out=rs.Partitioned(torch.zeros(7, dtype=torch.int32), None, None, off))
    with pytest.raises(ValueError, match="needs values"):
        rs.radix_partition(x, edges=e, out=rs.Partitioned(None, v.clone(), None, off))
    with pytest.raises(ValueError, match="shape"):
        rs.radix_partition(x, edges=e, values=v, out=rs.Partitioned(None, torch.zeros(8, 2, dtype=torch.float32), None, off))
    with pytest.raises(TypeError, match="int32 or int64"):
        rs.radix_partition(x, edges=e, out=rs.Partitioned(None, None, torch.zeros(8, dtype=torch.int16), off))
    with pytest.raises(TypeError, match="index_dtype"):
        rs.radix_partition(x, edges=e, index_dtype=torch.int32, out=rs.Partitioned(None, None, torch.zeros(8, dtype=torch.int64), off))
    with pytest.raises(ValueError, match="out.index"):
        rs.radix_partition(x, edges=e, return_index=True, out=rs.Partitioned(x.clone(), None, None, off))
    for bad in (None, 3, torch.zeros(5, dtype=torch.int32)):
        with pytest.raises(TypeError, match="out.offsets"):
            rs.radix_partition(x, edges=e, out=rs.Partitioned(x.clone(), None, None, bad))
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(6, dtype=torch.int64), torch.zeros(5, 2, dtype=torch.int64)[:, 0]):
        with pytest.raises(ValueError, match="out.offsets"):
            rs.radix_partition(x, edges=e, out=rs.Partitioned(x.clone(), None, None, bad))
    with pytest.raises(ValueError, match="out.offsets"):
        rs.radix_partition(x, num_bins=4, out=rs.Partitioned(x.clone(), None, None, off))  # num_bins + 2 offsets
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_partition(x, edges=e)  # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_partition(x, num_bins=3, values=v, return_index=True, index_dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_partition(x, edges=e, values=v, side="left", descending=True, out=rs.Partitioned(None, v.clone(), torch.zeros(8, dtype=torch.int32), off))
    assert not rs.api._DEFAULT or all(isinstance(c, rs.Context) for c in rs.api._DEFAULT.values())
