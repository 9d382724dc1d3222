"""CPU: the host side of the segmented sort (rsx_sort_segments_device, rsx_sort_rows_device, rsx_segment_caps) -- the
size classes of every direct layout, the Python argument checks (which raise before any context is made), the register
and scratch budget of the new kernels, and the C++ mirror (tests/cxx_segments_test.cpp; run under -m gpu)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import radix_sort_amd as rs
from test_kernel_resources import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BYTES = 160 * 1024
SIZES = (1, 2, 4, 8, 12, 16, 24, 32)
WIDTHS = (1, 2, 4, 8, 16)


def _direct_layouts():
    for es in SIZES:
        for kb in WIDTHS:
            for kind in (rs.KEY_UNSIGNED, rs.KEY_SIGNED, rs.KEY_FLOAT):
                if kb > es or (kind == rs.KEY_FLOAT and kb not in (4, 8)):
                    continue
                for off in sorted({0, es - kb}):
                    yield rs.RadixDigits(es, off, kb, kind)


def test_segment_caps_of_every_direct_layout():
    seen = 0
    for d in _direct_layouts():
        caps = rs.segment_caps(d)
        assert len(caps) == rs._lib.SEG_CLASSES >= 2, d
        assert all(c > 0 for c in caps) and caps == sorted(caps) and len(set(caps)) == len(caps), (d, caps)
        assert caps[-1] * d.elem_bytes < LDS_BYTES, (d, caps)
        seen += 1
    assert seen > 100
    assert rs.segment_caps(rs.PRIMITIVES["u32"]) == [7168, 28672]  # 256 and 1024 threads x 28 elements
    assert rs.segment_caps(rs.PRIMITIVES["u64"]) == [4352, 17408]  # ... x 17


def test_segment_caps_refuses_other_layouts():
    with pytest.raises(rs.RsxError) as e:
        rs.segment_caps(rs.RadixDigits(6, 0, 2, rs.KEY_UNSIGNED))
    assert e.value.status == rs._lib.ERR_UNSUPPORTED
    with pytest.raises(rs.RsxError) as e:
        rs.segment_caps(rs.RadixDigits(4, 2, 4, rs.KEY_UNSIGNED))  # the key does not fit the element
    assert e.value.status == rs._lib.ERR_ARG
    L = rs._lib.load()
    lay = rs.PRIMITIVES["u32"].layout()
    assert L.rsx_segment_caps(ctypes.byref(lay), None) == rs._lib.ERR_ARG
    assert L.rsx_segment_caps(None, (ctypes.c_uint32 * 2)()) == rs._lib.ERR_ARG


def test_entry_points_refuse_bad_arguments_without_a_device():
    L = rs._lib.load()
    lay = rs.PRIMITIVES["u32"].layout()
    assert L.rsx_sort_segments_device(None, None, None, 10, ctypes.byref(lay), None, 1, 0, None) == rs._lib.ERR_ARG
    assert L.rsx_sort_rows_device(None, None, None, 10, 10, ctypes.byref(lay), None) == rs._lib.ERR_ARG


def test_python_argument_checks_need_no_device():
    """Host arrays, wrong dtypes and non-contiguous arguments are refused before any context is made."""
    import torch
    made = []
    orig = rs.api.default_context
    rs.api.default_context = lambda dev: made.append(dev)  # any attempt to make a context is recorded
    try:
        offs = torch.tensor([0, 4, 8], dtype=torch.int64)
        x = torch.zeros((4, 8), dtype=torch.int32)
        with pytest.raises(TypeError):
            rs.radix_sort_segments(np.zeros(8, dtype=np.uint32), offs)  # numpy input
        with pytest.raises(TypeError):
            rs.radix_sort_rows(np.zeros((2, 4), dtype=np.uint32))
        with pytest.raises(TypeError):
            rs.radix_sort_rows([[3, 1, 2]])
        with pytest.raises(ValueError, match="GPU"):
            rs.radix_sort_segments(x.view(-1), offs)  # CPU tensor
        with pytest.raises(ValueError, match="GPU"):
            rs.radix_sort_rows(x)
        with pytest.raises(TypeError, match="int64 or uint64"):
            rs.radix_sort_segments(x.view(-1), torch.tensor([0, 4, 8], dtype=torch.int32))  # offsets of int32
        with pytest.raises(TypeError):
            rs.radix_sort_segments(x.view(-1), np.array([0, 4, 8], dtype=np.int64))  # offsets on the host, as numpy
        with pytest.raises(ValueError, match="contiguous"):
            rs.radix_sort_segments(x.view(-1), torch.zeros(6, dtype=torch.int64)[::2])
        with pytest.raises(ValueError, match="contiguous"):
            rs.radix_sort_rows(x.t())  # non-contiguous x
        with pytest.raises(ValueError, match="contiguous"):
            rs.radix_sort_segments(x.t(), offs)
    finally:
        rs.api.default_context = orig
    assert made == []


@pytest.mark.parametrize("es", [4, 8, 16])
def test_segment_kernels_fit_their_registers(es):
    """By the method of test_kernel_resources.py: the LDS classes are made of local_sort / local_sort_skip and keep to the
    bounds that file applies to the kernels made of them; every instance is enqueued whenever max_seg_len is 0, so its
    scratch stays below what makes a kernel slow to dispatch (test_gated_kernels_dispatch_without_a_scratch_penalty)."""
    res = _resources(es)
    names = [n for n in res if "rsx_segment_sort_kernel" in n]
    lds = [n for n in names if n.endswith("Lb0EEEvNS_9SmallArgsENS_7SegArgsE")]
    mem = [n for n in names if n.endswith("Lb1EEEvNS_9SmallArgsENS_7SegArgsE")]
    assert any("Li256E" in n for n in lds) and any("Li1024E" in n for n in lds) and mem, sorted(res)
    assert len(lds) + len(mem) == len(names)
    for n in lds:
        assert res[n].get("VGPRs Spill", 0) <= 16, (n, res[n])
        assert res[n].get("ScratchSize [bytes/lane]", 0) <= 128, (n, res[n])
    for n in names:
        assert res[n].get("ScratchSize [bytes/lane]", 0) <= 256, (n, res[n])


def _build(tmp_path):
    from radix_sort_amd import _build
    lib = _build.build()
    exe = str(tmp_path / "cxx_segments_test")
    # plain g++ against the HIP runtime API (the macro only tells the HIP headers which platform they are on)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx_segments_test.cpp"), lib, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cxx_segments_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cxx_segments_sorts(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "ALL OK" in out.stdout
