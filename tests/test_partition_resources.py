"""Register and LDS budget of the kernels of rsx_multisplit_device (no GPU needed: hipcc reports it at compile time; the
method of tests/test_bin_resources.py).  They live in rsx.hip, beside the bin kernels whose body the count launch shares,
through rsx_msplit_kernels.hpp: no translation unit of their own.

Nothing in them has a reason to leave the registers, so any spill and any scratch is a defect: the bounds are 0.  The
write kernel's static LDS is max_edges mapped keys (none in the index mode), max_edges + 1 cursors and as many counters
for each of its four waves; the count kernel's the edges and one set of counters; each at most 80 KiB so that two
workgroups fit a CU's 160 KiB, at two waves per SIMD or more."""
import re

import radix_sort_amd as rs
from radix_sort_amd import _build
from resources import kernel_resources

KERNELS = ("count", "scan", "offsets", "write")
WIDTHS = (1, 2, 4, 8, 16)
VALUES = (0, 1, 2, 4, 8, 16)
UPPER, LOWER, INDEX = 0, 1, 2
WAVES = 4


def _template_ints(name):
    m = re.search(r"I((?:Li\d+E)+)E", name)
    assert m, name
    return tuple(int(x) for x in re.findall(r"Li(\d+)E", m.group(1)))


def test_the_msplit_kernels_are_part_of_the_host_unit():
    units = [src for src, _obj, _flags in _build.UNITS]
    assert len(units) == 16 and len(_build.UNITS) == 16 and units.count("rsx.hip") == 1  # no translation unit of their own
    assert "rsx_msplit_kernels.hpp" in _build.DEPS
    lib = open(_build.LIB, "rb").read()
    assert b"rsx_msplit_write_kernel" in lib and b"rsx_msplit_count_kernel" in lib


def test_msplit_kernels_use_no_scratch_and_the_lds_the_header_states():
    res = kernel_resources("rsx.hip")
    kernels = {n: r for n, r in res.items() if "rsx_msplit_" in n}
    forms = {k: set() for k in KERNELS}
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r and "LDS Size [bytes/block]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["Occupancy [waves/SIMD]"] >= 2, (name, r)
        lds = r["LDS Size [bytes/block]"]
        assert lds <= 80 * 1024, (name, r)
        kind = next((k for k in KERNELS if f"rsx_msplit_{k}_kernel" in name), None)
        assert kind is not None, name
        if kind in ("scan", "offsets"):
            forms[kind].add(0)
            assert lds <= 64, (name, r)
            continue
        ints = _template_ints(name)
        forms[kind].add(ints)
        kb, mode = ints[0], ints[-1]
        max_edges, max_index_bins, _tile, _share = rs.partition_caps(kb)
        sets = WAVES + 1 if kind == "write" else 1  # the cursors and the waves' counters; the count kernel's counters
        if mode == INDEX:
            assert lds >= sets * (max_index_bins + 1) * 4, (name, r)
        else:
            assert lds >= max_edges * kb + sets * (max_edges + 1) * 4, (name, r)
    modes = {kb: (UPPER, LOWER) + ((INDEX,) if kb <= 8 else ()) for kb in WIDTHS}
    assert forms["count"] == {(kb, mode) for kb in WIDTHS for mode in modes[kb]}
    assert forms["write"] == {(kb, vb, mode) for kb in WIDTHS for vb in VALUES for mode in modes[kb]}
    assert forms["scan"] == {0} and forms["offsets"] == {0}
