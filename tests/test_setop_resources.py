"""Register and LDS budget of the kernel of rsx_setop_device (no GPU needed: hipcc reports it at compile time; the method of
tests/test_merge_resources.py).

rsx_setop_kernel keeps the mapped keys of a thread's few outputs in registers, indexed only with constants, and its flags
and sides in two words, so any spill and any scratch, in any instantiation, is a defect: the bounds are 0.  Its static LDS
is the merge tile's mapped keys, the tile's u16 slots where values or positions are asked for, and 64 bytes at most of
cuts, bounds and wave totals."""
import re

import radix_sort_amd as rs
from radix_sort_amd import _build
from resources import kernel_resources

LDS_PER_CU = 160 * 1024


def _template_args(name):
    """<KB, VB, IB, WRITE> of a mangled kernel name: ...ILi4ELi0ELi8ELb1EE..."""
    m = re.search(r"ILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE", name)
    assert m, name
    return int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4) == "1"


def test_the_setops_unit_is_part_of_the_library():
    units = [src for src, _obj, _flags in _build.UNITS]
    assert units.count("rsx_setops.hip") == 1 and len(units) == 16
    assert "rsx_setops.hip" in _build.DEPS and "rsx_setop_kernels.hpp" in _build.DEPS
    lib = open(_build.LIB, "rb").read()
    assert b"rsx_setop_kernel" in lib


def test_setop_kernels_use_no_scratch_and_the_lds_of_the_merge_tile():
    res = kernel_resources("rsx_setops.hip")
    kernels = {n: r for n, r in res.items() if "rsx_setop_kernel" in n}
    assert len(kernels) == len(res), sorted(set(res) - set(kernels))  # the scan kernel lives in rsx_unique.hip
    seen = set()
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r and "LDS Size [bytes/block]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        kb, vb, ib, write = _template_args(name)
        tile = rs.setop_caps(kb)
        slots = 2 * tile if (vb or ib) else 2
        lds = r["LDS Size [bytes/block]"]
        assert tile * kb <= lds <= tile * kb + slots + 64, (name, r, tile)
        assert lds <= tile * (kb + 2) + 64           # what include/rsx.h states for rsx_setop_caps
        assert lds <= rs.merge_caps(kb, vb) * (kb + 2) + 16 + 256  # the merge tile's, plus a fixed few hundred bytes
        assert 2 * lds <= LDS_PER_CU, (name, r)      # two workgroups per CU at least ...
        assert r["Occupancy [waves/SIMD]"] >= 2, (name, r)  # ... by registers too: a workgroup is one wave per SIMD
        if not write:
            assert vb == 0 and ib == 0, name
        seen.add((kb, vb, ib, write))
    want = {(kb, 0, 0, False) for kb in (1, 2, 4, 8, 16)} | {(kb, vb, ib, True) for kb in (1, 2, 4, 8, 16) for vb in (0, 1, 2, 4, 8, 16) for ib in (0, 4, 8)}
    assert seen == want, sorted(seen ^ want)
