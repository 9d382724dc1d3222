"""Register and LDS budget of the kernels of rsx_join_device (no GPU needed: hipcc reports it at compile time; the method of
tests/test_search_resources.py).  They live in the search kernel's translation unit, whose own kernels must not change.

The count kernel is the search kernel with four running sums per thread, the write kernel keeps eight rows per thread in
step; nothing in them has a reason to leave the registers, so any spill and any scratch is a defect: the bounds are 0.
Static LDS is what include/rsx.h states at rsx_join_caps: the count kernel the search window plus one smallest and one
largest key per wave and 160 bytes of window ends and wave totals, the write kernel eight bytes per row plus 32, the scan
kernel 32 bytes."""
import re

import radix_sort_amd as rs
from radix_sort_amd import _build
from resources import kernel_resources

LDS_PER_CU = 160 * 1024


def _template_int(name):
    m = re.search(r"ILi(\d+)EE", name)
    assert m, name
    return int(m.group(1))


def test_the_join_kernels_are_part_of_the_search_unit():
    units = [src for src, _obj, _flags in _build.UNITS]
    assert len(units) == 16 and units.count("rsx_search.hip") == 1  # no translation unit of their own
    assert "rsx_join_kernels.hpp" in _build.DEPS and "rsx_search.hip" in _build.DEPS
    assert b"rsx_join_count_kernel" in open(_build.LIB, "rb").read()


def test_join_kernels_use_no_scratch_and_the_lds_the_header_states():
    res = kernel_resources("rsx_search.hip")
    search = {n for n in res if "rsx_search_kernel" in n}
    assert len(search) == 20, sorted(search)  # the search kernel's instantiations are what they were
    kernels = {n: r for n, r in res.items() if "rsx_join_" in n}
    assert len(kernels) + len(search) == len(res), sorted(set(res) - set(kernels) - search)
    count, write, scan = set(), set(), 0
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r and "LDS Size [bytes/block]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        lds = r["LDS Size [bytes/block]"]
        assert 2 * lds <= LDS_PER_CU and lds <= 64 * 1024, (name, r)
        assert r["Occupancy [waves/SIMD]"] >= 2, (name, r)  # two workgroups per CU by registers too
        if "rsx_join_count_kernel" in name:
            kb = _template_int(name)
            _tile, window, _rows = rs.join_caps(kb)
            assert window * kb <= lds <= window * kb + 8 * kb + 160, (name, r, window)
            count.add(kb)
        elif "rsx_join_write_kernel" in name:
            assert lds <= 8 * rs.join_caps(4)[2] + 32, (name, r)
            write.add(_template_int(name))
        else:
            assert "rsx_join_scan_kernel" in name and lds <= 32, (name, r)
            scan += 1
    assert count == {1, 2, 4, 8, 16} and write == {4, 8} and scan == 1
