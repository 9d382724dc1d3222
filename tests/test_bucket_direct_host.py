"""CPU: RSX_OPT_BUCKET_DIRECT and RSX_INFO_LAST_DIRECT as the header, the ctypes binding and the host code state them.
A context needs a device, so the option's default, its range check and the info value before any sort are asserted on
one, in test_gpu_bucket_direct.py::test_option_default_range_and_info_before_any_sort."""
import ctypes
import os
import re

import radix_sort_amd as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_enums():
    text = open(os.path.join(ROOT, "include", "rsx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {k: int(v) for k, v in re.findall(r"\b(RSX_(?:OPT|INFO)_[A-Z_0-9]+)\s*=\s*(\d+)", text)}


def test_binding_matches_the_header():
    enums = _header_enums()
    assert enums["RSX_OPT_BUCKET_DIRECT"] == 15 == rs.OPT_BUCKET_DIRECT
    assert enums["RSX_INFO_LAST_DIRECT"] == 7 == rs.INFO_LAST_DIRECT
    for name, value in enums.items():  # every option and info id of the header has the same value in the binding
        assert getattr(rs._lib, name[4:]) == value, name
    assert len(set(v for k, v in enums.items() if k.startswith("RSX_OPT_"))) == len([k for k in enums if k.startswith("RSX_OPT_")])


def test_null_context_is_rejected():
    from radix_sort_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    out = ctypes.c_uint64(5)
    assert lib.rsx_ctx_set_option(None, rs.OPT_BUCKET_DIRECT, 1) == -1
    assert lib.rsx_ctx_get_info(None, rs.INFO_LAST_DIRECT, ctypes.byref(out)) == -1 and out.value == 5
