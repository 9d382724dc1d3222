"""Register and LDS budget of the kernels of rsx_compact_device (no GPU needed: hipcc reports it at compile time; the method
of tests/test_select_resources.py).  They live in rsx_unique.hip, whose scan kernel they launch, through
rsx_compact_kernels.hpp: no translation unit of their own.

Nothing in them has a reason to leave the registers, so any spill and any scratch is a defect: the bounds are 0.  The write
kernel's static LDS is a key, a value and a two-byte slot per row of its tile and
the waves' totals; at most 80 KiB so that two workgroups fit a CU's 160 KiB, at two waves per SIMD or more.  The count
kernel holds the waves' totals only."""
import re

import radix_sort_amd as rs
from radix_sort_amd import _build
from resources import kernel_resources

WIDTHS = (0, 1, 2, 4, 8, 16)


def _template_ints(name):
    m = re.search(r"ILi(\d+)ELi(\d+)EE", name)
    assert m, name
    return int(m.group(1)), int(m.group(2))


def test_the_compact_kernels_are_part_of_the_unique_unit():
    units = [src for src, _obj, _flags in _build.UNITS]
    assert len(units) == 16 and len(_build.UNITS) == 16 and units.count("rsx_unique.hip") == 1  # no translation unit of their own
    assert "rsx_compact_kernels.hpp" in _build.DEPS
    lib = open(_build.LIB, "rb").read()
    assert b"rsx_compact_write_kernel" in lib and b"rsx_compact_count_kernel" in lib


def test_compact_kernels_use_no_scratch_and_the_lds_the_header_states():
    res = kernel_resources("rsx_unique.hip")
    kernels = {n: r for n, r in res.items() if "rsx_compact_" in n}  # (rsx_select_compact_kernel is another call's, in another unit)
    assert not any("select" in n for n in kernels)
    forms = {"count": set(), "write": set(), "gather": set()}
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r and "LDS Size [bytes/block]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["Occupancy [waves/SIMD]"] >= 2, (name, r)
        lds = r["LDS Size [bytes/block]"]
        assert lds <= 80 * 1024, (name, r)
        kind = next((k for k in forms if f"rsx_compact_{k}_kernel" in name), None)
        assert kind is not None, name
        if kind == "gather":
            forms[kind].add(name)
            assert lds == 0, (name, r)
            continue
        a, b = _template_ints(name)
        forms[kind].add((a, b))
        if kind == "count":
            assert lds <= 64, (name, r)  # the waves' totals
        else:
            tile = rs.compact_caps(a, b, 0)[0]
            want = tile * (a + b + 2)
            assert want <= lds <= want + 64, (name, r, tile)
    # the write kernel: every key width (0: the call has no use for the keys) with every fused value width (0: none)
    assert forms["write"] == {(kb, vb) for kb in WIDTHS for vb in WIDTHS}
    # the count kernel: every key width with the rows per thread its tiles have
    assert forms["count"] == {(kb, rs.compact_caps(kb, vb, 0)[0] // 256) for kb in WIDTHS for vb in WIDTHS}
    assert len(forms["gather"]) == 2  # rows in 4-byte words, or byte by byte
