"""CPU (and one GPU run): the host side of layouts without sort kernels of their own -- digits_of on structured dtypes
of odd sizes and void keys, get_digit of odd key widths against the CPU oracle, and the C++ mirror on a 40-byte pair
and a packed 6-byte record with a 48-bit key (tests/cxx_any_layout_test.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import radix_sort_amd as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_digits_of_odd_structured_dtypes():
    assert rs.digits_of(np.dtype([("k", "<u2"), ("v", "V4")])) == rs.RadixDigits(6, 0, 2, rs.KEY_UNSIGNED)
    assert rs.digits_of(np.dtype([("k", "<u4"), ("v", "V16")])) == rs.RadixDigits(20, 0, 4, rs.KEY_UNSIGNED)
    assert rs.digits_of(np.dtype([("k", "<u8"), ("v", "V32")])) == rs.RadixDigits(40, 0, 8, rs.KEY_UNSIGNED)
    assert rs.digits_of(np.dtype([("k", "<i2"), ("v", "u1")])) == rs.RadixDigits(3, 0, 2, rs.KEY_SIGNED)
    for w in range(1, 17):  # V1..V16: unsigned key of that width
        dt = np.dtype([("k", f"V{w}"), ("v", "V5")])
        assert rs.digits_of(dt) == rs.RadixDigits(w + 5, 0, w, rs.KEY_UNSIGNED)
    off = np.dtype({"names": ["k", "v"], "formats": ["V6", "u1"], "offsets": [1, 0], "itemsize": 7})
    assert rs.digits_of(off) == rs.RadixDigits(7, 1, 6, rs.KEY_UNSIGNED)
    with pytest.raises(TypeError):
        rs.digits_of(np.dtype([("k", "V17"), ("v", "u1")]))


@pytest.mark.parametrize("lay", [(3, 0, 3, 0), (6, 1, 5, 1), (7, 0, 6, 1), (13, 1, 12, 0), (20, 4, 12, 1), (40, 3, 7, 0),
                                 (11, 2, 9, 1), (5, 0, 3, 1)])
def test_get_digit_odd_widths(orc, lay):
    es, ko, kb, kind = lay
    d = rs.RadixDigits(*lay)
    L = orc.lib()
    olay = orc.Layout(*lay)
    rng = np.random.default_rng(es * 31 + kb)
    raw = rng.integers(0, 256, size=(64, es), dtype=np.uint8)
    for i in range(64):
        e = np.ascontiguousarray(raw[i])
        for idx in range(kb):
            assert d.get_digit(bytes(e), idx) == L.orc_get_digit(e.ctypes.data, ctypes.byref(olay), idx)


def test_flat_byte_array_needs_the_element_shape():
    """A layout without kernels of its own is read from an array that states its element (dtype itemsize or last
    dimension); a flat byte array with such a descriptor is refused before any device is touched."""
    with pytest.raises(rs.RsxError) as e:
        rs.radix_sort(np.zeros(12, dtype=np.uint8), digits=rs.RadixDigits(3, 0, 2, rs.KEY_UNSIGNED))
    assert e.value.status == rs._lib.ERR_UNSUPPORTED
    with pytest.raises(rs.RsxError):
        rs.radix_sort(np.zeros((4, 6), dtype=np.uint8), digits=rs.RadixDigits(3, 0, 2, rs.KEY_UNSIGNED))


def _build(tmp_path):
    from radix_sort_amd import _build
    lib = _build.build()
    exe = str(tmp_path / "cxx_any_layout_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cxx_any_layout_test.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cxx_any_layout_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cxx_any_layout_sorts(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "ALL OK" in out.stdout
