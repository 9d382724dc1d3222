"""Register and LDS budget of the kernels of rsx_bin_reduce_device (no GPU needed: hipcc reports it at compile time; the
method of tests/test_partition_resources.py).  They live in rsx.hip, beside the bin and multisplit kernels whose search,
match and shares they take, through rsx_binred_kernels.hpp: no translation unit of their own.

Nothing in them has a reason to leave the registers, so any spill and any scratch is a defect: the bounds are 0.  The
first launch's static LDS is max_edges mapped keys (none in the index mode), four waves' rows of max_edges + 1
accumulators of the value's width and max_edges + 1 counters; at most 80 KiB so that two workgroups fit a CU's 160 KiB, at
two waves per SIMD or more.  The kernels come per key width, value width, float or integer values, and index or edge
mode (the two edge modes share a kernel, as signed and unsigned integers do)."""
import re

import radix_sort_amd as rs
from radix_sort_amd import _build
from resources import kernel_resources

WIDTHS = (1, 2, 4, 8, 16)
VALUES = (4, 8)
WAVES = 4


def _template_args(name):
    m = re.search(r"I((?:L[ib]\d+E)+)E", name)
    assert m, name
    return tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1)))


def test_the_binred_kernels_are_part_of_the_host_unit():
    units = [src for src, _obj, _flags in _build.UNITS]
    assert len(units) == 16 and len(_build.UNITS) == 16 and units.count("rsx.hip") == 1  # no translation unit of their own
    assert "rsx_binred_kernels.hpp" in _build.DEPS
    lib = open(_build.LIB, "rb").read()
    assert b"rsx_binred_part_kernel" in lib and b"rsx_binred_final_kernel" in lib


def test_binred_kernels_use_no_scratch_and_the_lds_the_header_states():
    res = kernel_resources("rsx.hip")
    kernels = {n: r for n, r in res.items() if "rsx_binred_" in n}
    forms = {"part": set(), "final": set()}
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r and "LDS Size [bytes/block]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["Occupancy [waves/SIMD]"] >= 2, (name, r)
        lds = r["LDS Size [bytes/block]"]
        assert lds <= 80 * 1024, (name, r)
        args = _template_args(name)
        if "rsx_binred_final_kernel" in name:
            forms["final"].add(args)
            assert lds == 0, (name, r)
            continue
        assert "rsx_binred_part_kernel" in name, name
        forms["part"].add(args)
        kb, vb, _flt, index = args
        max_edges, max_index_bins, _tile, _share = rs.bin_reduce_caps(kb, vb)
        if index:
            assert lds >= (max_index_bins + 1) * (WAVES * vb + 4), (name, r)
        else:
            assert lds >= max_edges * kb + (max_edges + 1) * (WAVES * vb + 4), (name, r)
    assert forms["part"] == {(kb, vb, flt, index) for kb in WIDTHS for vb in VALUES for flt in (0, 1) for index in ((0, 1) if kb <= 8 else (0,))}
    assert forms["final"] == {(vb, flt) for vb in VALUES for flt in (0, 1)}
