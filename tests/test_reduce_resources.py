"""Register budget of the run kernels of rsx_reduce_by_key_device (no GPU needed: hipcc reports it at compile time; the
method of tests/test_unique_resources.py).

rsx_reduce_count_kernel, rsx_reduce_scan_kernel and rsx_reduce_write_kernel are streaming kernels: at most 64 bytes of
elements per thread, one word of flags, as many partial values as elements, a few ranks.  Nothing in them has a reason to
leave the registers, so any spill and any scratch, in any instantiation, is a defect and not a tuning matter: the bounds
are 0."""
import re

from radix_sort_amd import _build
from resources import kernel_resources

KEY_WIDTHS = (1, 2, 4, 8, 16)
VALUE_TYPES = {(vb, vk) for vb in (4, 8) for vk in (0, 1, 2)}  # u32 i32 f32 u64 i64 f64


def _template_ints(name):
    """<KB, VB, VK> or <VB, VK> of a mangled kernel name: ...ILi4ELi8ELi2EE..."""
    m = re.search(r"I((?:Li\d+E)+)E", name)
    assert m, name
    return tuple(int(x) for x in re.findall(r"Li(\d+)E", m.group(1)))


def test_the_unit_is_part_of_the_library():
    assert "rsx_reduce.hip" in _build.DEPS and "rsx_reduce_kernels.hpp" in _build.DEPS


def test_run_kernels_use_no_scratch():
    res = kernel_resources("rsx_reduce.hip")
    kernels = {n: r for n, r in res.items() if "rsx_reduce_" in n and "_kernel" in n}
    seen = {"count": [], "write": [], "scan": []}
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        which = next(w for w in ("count", "scan", "write") if f"rsx_reduce_{w}_kernel" in name)
        seen[which].append(_template_ints(name))
    # the scan kernel once per value type; count and write once per (key width, value type)
    assert sorted(seen["scan"]) == sorted(VALUE_TYPES), seen["scan"]
    every = sorted((kb, vb, vk) for kb in KEY_WIDTHS for vb, vk in VALUE_TYPES)
    assert sorted(seen["count"]) == every, seen["count"]
    assert sorted(seen["write"]) == every, seen["write"]
