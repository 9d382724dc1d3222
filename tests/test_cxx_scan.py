"""CPU: rsx::scan_by_key of the C++ host mirror (radix_sort_amd/cxx/radix_sort.hpp) compiles with hipcc for uint32_t and
double keys, float, int64_t, uint32_t and double values and the count form (tests/cxx_scan_test.cpp; compile only)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cxx_scan_compiles(tmp_path):
    from radix_sort_amd import _build
    obj = str(tmp_path / "cxx_scan_test.o")
    p = subprocess.run([_build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-c", os.path.join(ROOT, "tests", "cxx_scan_test.cpp"), "-o", obj],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.getsize(obj) > 0
