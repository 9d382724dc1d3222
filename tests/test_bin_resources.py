"""Register and LDS budget of the kernels of rsx_bin_count_device (no GPU needed: hipcc reports it at compile time; the
method of tests/test_select_resources.py).  They live in rsx.hip, the unit of the size-independent kernels, through
rsx_bin_kernels.hpp: no translation unit of their own.

Nothing in them has a reason to leave the registers, so any spill and any scratch is a defect: the bounds are 0.  The
edge kernel's static LDS is max_edges mapped keys and max_edges + 1 four-byte counters, the index kernel's LDS variant
max_index_bins_lds counters and one for the outside bin; each at most 80 KiB so that two workgroups fit a CU's 160 KiB, at two waves per SIMD or more."""
import re

import radix_sort_amd as rs
from radix_sort_amd import _build
from resources import kernel_resources

KERNELS = ("zero", "edge", "index")


def _template_ints(name):
    m = re.search(r"ILi(\d+)ELb([01])EE", name)
    assert m, name
    return int(m.group(1)), int(m.group(2))


def test_the_bin_kernels_are_part_of_the_host_unit():
    units = [src for src, _obj, _flags in _build.UNITS]
    assert len(units) == 16 and len(_build.UNITS) == 16 and units.count("rsx.hip") == 1  # no translation unit of their own
    assert "rsx_bin_kernels.hpp" in _build.DEPS
    assert b"rsx_bin_edge_kernel" in open(_build.LIB, "rb").read()


def test_bin_kernels_use_no_scratch_and_the_lds_the_header_states():
    res = kernel_resources("rsx.hip")
    kernels = {n: r for n, r in res.items() if "rsx_bin_" in n}
    forms = {k: set() for k in KERNELS}
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r and "LDS Size [bytes/block]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["Occupancy [waves/SIMD]"] >= 2, (name, r)
        lds = r["LDS Size [bytes/block]"]
        assert lds <= 80 * 1024, (name, r)
        kind = next((k for k in KERNELS if f"rsx_bin_{k}_kernel" in name), None)
        assert kind is not None, name
        if kind == "zero":
            forms[kind].add(0)
            continue
        kb, flag = _template_ints(name)
        forms[kind].add((kb, flag))
        max_edges, index_lds, _share = rs.bin_caps(kb)
        if kind == "edge":
            assert lds >= max_edges * kb + (max_edges + 1) * 4, (name, r)
        elif flag:
            assert lds >= index_lds * 4, (name, r)
        else:
            assert lds <= 64, (name, r)  # atomics straight into the counts
    assert forms["edge"] == {(kb, up) for kb in (1, 2, 4, 8, 16) for up in (0, 1)}  # both sides of every key width
    assert forms["index"] == {(kb, v) for kb in (1, 2, 4, 8) for v in (0, 1)}       # both variants of every integer width
    assert forms["zero"] == {0}
