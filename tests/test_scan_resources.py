"""Register budget of the kernels of rsx_scan_by_key_device (no GPU needed: hipcc reports it at compile time; the method of
tests/test_reduce_resources.py on rsx_scan.hip).

rsx_scanbk_count_kernel and rsx_scanbk_write_kernel are the reduce kernels' streaming scan with one store per element:
at most 16 keys, values and partial results per thread, one word of flags.  Nothing in them has a reason to leave the
registers, so any spill and any scratch, in any instantiation, is a defect and not a tuning matter: the bounds are 0."""
import re

from radix_sort_amd import _build
from resources import kernel_resources

SOURCES = (0, 1)  # SCANBK_COLUMNS (RSX_SCAN_RUNS), SCANBK_POSITIONS (grouped)
KEY_WIDTHS = (1, 2, 4, 8, 16)
VALUE_TYPES = {(vb, vk) for vb in (4, 8) for vk in (0, 1, 2)}  # u32 i32 f32 u64 i64 f64
COUNT_FORMS = {(vb, 3) for vb in (4, 8)}  # SCANBK_ONES: every value is 1


def _template_ints(name):
    """<SRC, KB, VB, VK> of a mangled kernel name: ...ILi0ELi4ELi8ELi2EE..."""
    m = re.search(r"I((?:Li\d+E)+)E", name)
    assert m, name
    return tuple(int(x) for x in re.findall(r"Li(\d+)E", m.group(1)))


def test_the_unit_is_part_of_the_library():
    units = [src for src, _obj, _flags in _build.UNITS]
    assert units.count("rsx_scan.hip") == 1
    assert "rsx_reduce.hip" not in units  # the reduce launchers are compiled inside it: one unit for both calls by key
    assert "rsx_scan.hip" in _build.DEPS and "rsx_scan_kernels.hpp" in _build.DEPS and "rsx_reduce.hip" in _build.DEPS
    lib = open(_build.LIB, "rb").read()
    assert b"rsx_scanbk_count_kernel" in lib and b"rsx_scanbk_write_kernel" in lib and b"rsx_reduce_write_kernel" in lib


def test_scan_kernels_use_no_scratch():
    res = kernel_resources("rsx_scan.hip")
    kernels = {n: r for n, r in res.items() if "rsx_scanbk_" in n and "_kernel" in n}
    seen = {"count": [], "write": []}
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        which = next(w for w in ("count", "write") if f"rsx_scanbk_{w}_kernel" in name)
        seen[which].append(_template_ints(name))
    # count and write once per (source, key width, value type), and once per (source, key width, value width) for the count form
    every = sorted((src, kb, vb, vk) for src in SOURCES for kb in KEY_WIDTHS for vb, vk in VALUE_TYPES | COUNT_FORMS)
    assert sorted(seen["count"]) == every, seen["count"]
    assert sorted(seen["write"]) == every, seen["write"]
    # the tile scan is the reduce kernels' own: the unit holds it once per value type, for both calls
    scans = sorted(_template_ints(n) for n in res if "rsx_reduce_scan_kernel" in n)
    assert scans == sorted(VALUE_TYPES), scans
