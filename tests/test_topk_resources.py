"""Register budget of the top-k kernels (no GPU needed: hipcc reports it at compile time; the method of
tests/test_kernel_resources.py).

rsx_topk_kernel holds the elements per thread of rsx_segment_pairs_kernel and ends in the same passes; what it adds are
two bit masks (live, taken) and the few scalars of the select.  So every instantiation is held against the
rsx_segment_pairs_kernel of the same joined element size, key width (value: the four-byte position) and workgroup size,
non-memory form, IN THE SAME COMPILE OUTPUT, with the margins of tests/test_segment_pairs_resources.py and for its
reason: a kernel with much scratch takes long to dispatch.  Should a change miss the margin, the top-k kernel's own
elements per thread (and rsx_topk_caps) come down; the margin does not go up."""
import re

import pytest

from test_kernel_resources import _resources
from test_segment_pairs_resources import SCRATCH_MARGIN, SPILL_MARGIN


def _ints(name, count):
    """the leading `count` integer template arguments of a mangled kernel name: ...ILi8ELi4E..."""
    m = re.search(r"I((?:Li\d+E){%d})" % count, name)
    assert m, name
    return tuple(int(x) for x in re.findall(r"Li(\d+)E", m.group(1)))


@pytest.mark.parametrize("es", [8, 16])
def test_topk_kernels_stay_within_a_margin_of_their_sibling(es):
    res = _resources(es)
    siblings = {}
    for n, r in res.items():
        if "rsx_segment_pairs_kernel" in n and "Lb0EEE" in n:  # <ES, KB, VB, KPT, WG, MEM = false>
            s_es, kb, vb, _, wg = _ints(n, 5)
            if vb == 4:
                siblings[(s_es, kb, wg)] = r
    topk = {n: r for n, r in res.items() if "rsx_topk_kernel" in n}  # <ES, KB, KPT, WG>
    assert not any("rsx_segment_pairs_kernel" in n or "rsx_segment_sort_kernel" in n for n in topk), sorted(topk)
    forms = set()
    for name, r in topk.items():
        t_es, kb, _, wg = _ints(name, 4)
        assert t_es == es, name
        forms.add(wg)
        sib = siblings[(es, kb, wg)]
        print(name, r, "sibling", sib)
        assert r.get("VGPRs Spill", 0) <= sib.get("VGPRs Spill", 0) + SPILL_MARGIN, (name, r, sib)
        assert r.get("ScratchSize [bytes/lane]", 0) <= sib.get("ScratchSize [bytes/lane]", 0) + SCRATCH_MARGIN, (name, r, sib)
    assert forms == {256, 1024}, sorted(topk)
