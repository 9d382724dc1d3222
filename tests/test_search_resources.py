"""Register and LDS budget of the kernel of rsx_search_sorted_device (no GPU needed: hipcc reports it at compile time; the
method of tests/test_unique_resources.py).

rsx_search_kernel keeps four needles, their bounds and a few cursors per thread; nothing in it has a reason to leave the
registers, so any spill and any scratch, in any instantiation, is a defect: the bounds are 0.  Its static LDS is the
window of mapped keys plus the tile's own words: one smallest and one largest key per wave and the two ends of the
window."""
import re

import radix_sort_amd as rs
from radix_sort_amd import _build
from resources import kernel_resources


def _template_ints(name):
    """<KB, POS, IB> of a mangled kernel name: ...ILi4ELb1ELi8EE..."""
    m = re.search(r"ILi(\d+)ELb([01])ELi(\d+)EE", name)
    assert m, name
    return int(m.group(1)), m.group(2) == "1", int(m.group(3))


def test_the_search_unit_is_part_of_the_library():
    assert "rsx_search.hip" in _build.DEPS and "rsx_search_kernels.hpp" in _build.DEPS
    assert b"rsx_search_kernel" in open(_build.LIB, "rb").read()


def test_search_kernels_use_no_scratch_and_the_lds_of_their_window():
    res = kernel_resources("rsx_search.hip")
    kernels = {n: r for n, r in res.items() if "rsx_search_kernel" in n}
    seen = set()
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r and "LDS Size [bytes/block]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        kb, pos, ib = _template_ints(name)
        tile, window = rs.search_caps(kb, pos)
        waves = 256 // 64
        own = 2 * waves * kb + 2 * 8 + 16  # smallest and largest key per wave, the window's two ends, alignment
        assert window * kb <= r["LDS Size [bytes/block]"] <= window * kb + own, (name, r, window, own)
        assert 2 * r["LDS Size [bytes/block]"] <= 160 * 1024, (name, r)
        seen.add((kb, pos, ib))
    assert seen == {(kb, pos, ib) for kb in (1, 2, 4, 8, 16) for pos in (False, True) for ib in (4, 8)}, sorted(seen)
