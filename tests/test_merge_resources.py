"""Register and LDS budget of the kernels of rsx_merge_device (no GPU needed: hipcc reports it at compile time; the method
of tests/test_search_resources.py).

rsx_merge_kernel keeps the mapped keys and source slots of a thread's few outputs in registers and indexes them only with
constants, so any spill and any scratch, in any instantiation, is a defect: the bounds are 0.  Its static LDS is the
tile's mapped keys, the tile's u16 slots where values or positions are asked for, and the two cuts."""
import re

import radix_sort_amd as rs
from radix_sort_amd import _build
from resources import kernel_resources

LDS_PER_CU = 160 * 1024


def _template_ints(name):
    """<KB, VB, IB> of a mangled kernel name: ...ILi4ELi0ELi8EE..."""
    m = re.search(r"ILi(\d+)ELi(\d+)ELi(\d+)EE", name)
    assert m, name
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def _clean(name, r):
    assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r and "LDS Size [bytes/block]" in r, (name, r)
    assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
    assert r["ScratchSize [bytes/lane]"] == 0, (name, r)


def test_the_merge_unit_is_part_of_the_library():
    assert "rsx_merge.hip" in _build.DEPS and "rsx_merge_kernels.hpp" in _build.DEPS
    assert [src for src, _obj, _flags in _build.UNITS].count("rsx_merge.hip") == 1
    lib = open(_build.LIB, "rb").read()
    assert b"rsx_merge_kernel" in lib and b"rsx_merge_gather_kernel" in lib


def test_merge_kernels_use_no_scratch_and_the_lds_of_their_tile():
    res = kernel_resources("rsx_merge.hip")
    kernels = {n: r for n, r in res.items() if "rsx_merge_kernel" in n}
    seen = set()
    for name, r in kernels.items():
        print(name, r)
        _clean(name, r)
        kb, vb, ib = _template_ints(name)
        tile = rs.merge_caps(kb, vb)
        slots = 2 * tile if (vb or ib) else 2
        own = 2 * 8 + 32  # the two cuts, alignment
        assert tile * kb <= r["LDS Size [bytes/block]"] <= tile * kb + slots + own, (name, r, tile)
        assert r["LDS Size [bytes/block]"] <= tile * (kb + 2) + 16 + 32  # what include/rsx.h states for rsx_merge_caps
        assert 2 * r["LDS Size [bytes/block]"] <= LDS_PER_CU, (name, r)
        seen.add((kb, vb, ib))
    assert seen == {(kb, vb, ib) for kb in (1, 2, 4, 8, 16) for vb in (0, 1, 2, 4, 8, 16) for ib in (0, 4, 8)}, sorted(seen)


def test_merge_gather_kernels_use_no_scratch_and_no_lds():
    res = kernel_resources("rsx_merge.hip")
    kernels = {n: r for n, r in res.items() if "rsx_merge_gather_kernel" in n}
    assert len(kernels) == 2, sorted(kernels)  # 16-byte words and bytes
    for name, r in kernels.items():
        print(name, r)
        _clean(name, r)
        assert r["LDS Size [bytes/block]"] == 0, (name, r)
