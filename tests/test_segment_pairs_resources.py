"""Register budget of the fused segmented key / value kernels (no GPU needed: hipcc reports it at compile time; the
method of tests/test_kernel_resources.py).

rsx_segment_pairs_kernel runs the passes of rsx_segment_sort_kernel on the same number of elements per thread; what it
adds are the temporaries of its column load and store -- at most one element plus a key word.  So every instantiation
is held against the rsx_segment_sort_kernel instantiation of the same element size, workgroup size and memory form IN
THE SAME COMPILE OUTPUT: at most 16 more spilled VGPRs and 64 more bytes of scratch per lane than that sibling."""
import re

import pytest

from test_kernel_resources import _resources

SPILL_MARGIN, SCRATCH_MARGIN = 16, 64


def _form(name):
    """(workgroup size, through memory) of a mangled segment kernel name: ...Li<WG>ELb<MEM>EEE..."""
    m = re.search(r"Li(\d+)ELb([01])EEEv", name)
    assert m, name
    return int(m.group(1)), m.group(2) == "1"


@pytest.mark.parametrize("es", [8, 16])
def test_fused_kernels_stay_within_a_margin_of_their_sibling(es):
    res = _resources(es)
    siblings = {_form(n): r for n, r in res.items() if "rsx_segment_sort_kernel" in n}
    assert set(siblings) == {(256, False), (1024, False), (1024, True)}, sorted(siblings)
    fused = {n: r for n, r in res.items() if "rsx_segment_pairs_kernel" in n}
    # every (key, value) width pair whose joined element has this size, in the three forms
    pairs = {8: 6, 16: 5}[es]
    assert len(fused) == 3 * pairs, sorted(fused)
    for name, r in fused.items():
        sib = siblings[_form(name)]
        print(name, r, "sibling", sib)
        assert r.get("VGPRs Spill", 0) <= sib.get("VGPRs Spill", 0) + SPILL_MARGIN, (name, r, sib)
        assert r.get("ScratchSize [bytes/lane]", 0) <= sib.get("ScratchSize [bytes/lane]", 0) + SCRATCH_MARGIN, (name, r, sib)
