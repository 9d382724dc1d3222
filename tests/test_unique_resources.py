"""Register budget of the run kernels of rsx_unique_device (no GPU needed: hipcc reports it at compile time; the method
of tests/test_kernel_resources.py).

rsx_unique_count_kernel, rsx_unique_scan_kernel and rsx_unique_write_kernel are streaming kernels: 64 bytes of elements
per thread, one word of flags, a few ranks.  Nothing in them has a reason to leave the registers, so any spill and any
scratch, in any instantiation, is a defect and not a tuning matter: the bounds are 0."""
import re

from resources import kernel_resources


def _template_ints(name):
    """<KB, POS[, IB]> of a mangled kernel name: ...ILi4ELb1ELi8EE..."""
    m = re.search(r"ILi(\d+)ELb([01])E(?:Li(\d+)E)?E", name)
    assert m, name
    return int(m.group(1)), m.group(2) == "1", int(m.group(3)) if m.group(3) else None


def _joined(kb, pos):
    return {1: 8, 2: 8, 4: 8, 8: 16, 16: 32}[kb] if pos else kb


def test_run_kernels_use_no_scratch():
    res = kernel_resources("rsx_unique.hip")
    kernels = {n: r for n, r in res.items() if "rsx_unique_" in n and "_kernel" in n}
    seen = {"count": set(), "write": set(), "scan": 0}
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        if "rsx_unique_scan_kernel" in name:
            seen["scan"] += 1
            continue
        kb, pos, ib = _template_ints(name)
        which = "count" if "rsx_unique_count_kernel" in name else "write"
        assert which == "count" or "rsx_unique_write_kernel" in name, name
        seen[which].add((_joined(kb, pos), kb, pos, ib))
    assert seen["scan"] == 1, sorted(kernels)
    # every key width by both routes; the write kernels of the route with positions in both index widths
    routes = {(kb, pos) for kb in (1, 2, 4, 8, 16) for pos in (False, True)}
    assert {(kb, pos) for _e, kb, pos, _ib in seen["count"]} == routes, sorted(seen["count"])
    assert {(kb, pos, ib) for _e, kb, pos, ib in seen["write"]} == \
        {(kb, False, 4) for kb in (1, 2, 4, 8, 16)} | {(kb, True, ib) for kb in (1, 2, 4, 8, 16) for ib in (4, 8)}, sorted(seen["write"])
    for which in ("count", "write"):
        assert {e for e, _kb, _pos, _ib in seen[which]} == {1, 2, 4, 8, 16, 32}, (which, sorted(seen[which]))
