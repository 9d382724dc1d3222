"""Register and LDS budget of the kernels of rsx_select_device (no GPU needed: hipcc reports it at compile time; the method
of tests/test_join_resources.py).  They live in rsx.hip, the unit of the size-independent kernels, through
rsx_select_kernels.hpp: no translation unit of their own.

Nothing in them has a reason to leave the registers, so any spill and any scratch is a defect: the bounds are 0.  The
count kernel's static LDS is its counters, max_ranks rows of 2^digit_bits four-byte words, and at most 80 KiB so that two
workgroups fit a CU's 160 KiB; every other kernel stays below 64 KiB and at two waves per SIMD or more."""
import re

import radix_sort_amd as rs
from radix_sort_amd import _build
from resources import kernel_resources

KERNELS = ("count", "pick", "compact", "tile", "scan", "find", "write")


def _template_int(name):
    m = re.search(r"ILi(\d+)EE", name)
    assert m, name
    return int(m.group(1))


def test_the_select_kernels_are_part_of_the_host_unit():
    units = [src for src, _obj, _flags in _build.UNITS]
    assert len(units) == 16 and len(_build.UNITS) == 16 and units.count("rsx.hip") == 1  # no translation unit of their own
    assert "rsx_select_kernels.hpp" in _build.DEPS
    assert b"rsx_select_count_kernel" in open(_build.LIB, "rb").read()


def test_select_kernels_use_no_scratch_and_the_lds_the_header_states():
    res = kernel_resources("rsx.hip")
    kernels = {n: r for n, r in res.items() if "rsx_select_" in n}
    max_ranks, digit_bits, _tile, _div, _floor = rs.select_caps(4)
    widths = {k: set() for k in KERNELS}
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r and "LDS Size [bytes/block]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        lds = r["LDS Size [bytes/block]"]
        kind = next((k for k in KERNELS if f"rsx_select_{k}_kernel" in name), None)
        assert kind is not None, name
        if kind == "count":
            assert max_ranks * (1 << digit_bits) * 4 <= lds <= 80 * 1024, (name, r)
            assert r["Occupancy [waves/SIMD]"] >= 2, (name, r)
        else:
            assert lds <= 64 * 1024, (name, r)
            assert r["Occupancy [waves/SIMD]"] >= 2, (name, r)
        widths[kind].add(_template_int(name) if "ILi" in name else 0)
    for kind in ("count", "compact", "tile", "find", "write"):
        assert widths[kind] == {1, 2, 4, 8, 16}, (kind, widths[kind])
    assert widths["pick"] == {0} and widths["scan"] == {0}
