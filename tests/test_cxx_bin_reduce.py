"""CPU: rsx::bin_reduce and rsx::bin_reduce_caps of the C++ host mirror (radix_sort_amd/cxx/radix_sort.hpp) compile with
hipcc for uint32_t, int64_t, float and double keys and every value type (tests/cxx_bin_reduce_test.cpp; compile only)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cxx_bin_reduce_compiles(tmp_path):
    from radix_sort_amd import _build
    obj = str(tmp_path / "cxx_bin_reduce_test.o")
    p = subprocess.run([_build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-c", os.path.join(ROOT, "tests", "cxx_bin_reduce_test.cpp"), "-o", obj],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.getsize(obj) > 0
