"""Register and LDS budget of the kernel of rsx_search_sorted_device (no GPU needed: hipcc reports it at compile time; the
method of tests/test_unique_resources.py).

rsx_search_kernel keeps four needles, their bounds and a few cursors per thread; nothing in it has a reason to leave the
registers, so any spill and any scratch, in any instantiation, is a defect: the bounds are 0.  Its static LDS is the
window of mapped keys plus the tile's own words: one smallest and one largest key per wave and the two ends of the
window."""
import functools
import os
import re
import subprocess
import tempfile

import radix_sort_amd as rs
from radix_sort_amd import _build


@functools.lru_cache(maxsize=None)
def _resources():
    with tempfile.TemporaryDirectory() as d:
        cmd = [_build.hipcc()] + _build.CXXFLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                    os.path.join(_build.CSRC, "rsx_search.hip"), "-o", os.path.join(d, "o.o")]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def _template_ints(name):
    """<KB, POS, IB> of a mangled kernel name: ...ILi4ELb1ELi8EE..."""
    m = re.search(r"ILi(\d+)ELb([01])ELi(\d+)EE", name)
    assert m, name
    return int(m.group(1)), m.group(2) == "1", int(m.group(3))


def test_the_search_unit_is_part_of_the_library():
    assert "rsx_search.hip" in _build.DEPS and "rsx_search_kernels.hpp" in _build.DEPS
    assert b"rsx_search_kernel" in open(_build.LIB, "rb").read()


def test_search_kernels_use_no_scratch_and_the_lds_of_their_window():
    res = _resources()
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
