"""The device-resident templates of the C++ host mirror (radix_sort_amd/cxx/radix_sort.hpp) -- radix_sort_device,
radix_sort_pairs, radix_sort_keys, radix_argsort, the segment and row forms with values and indices, radix_sort_sharded:
tests/cxx_device_forms_test.cpp instantiates every one of them, compiles and links without a GPU, and on one compares
each with std::stable_sort."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    from radix_sort_amd import _build
    lib = _build.build()
    exe = str(tmp_path / "cxx_device_forms_test")
    # plain g++ against the HIP runtime API (the macro only tells the HIP headers which platform they are on)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx_device_forms_test.cpp"), lib, "-L/opt/rocm/lib", "-lamdhip64", "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cxx_device_forms_compile_and_link(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cxx_device_forms_against_stable_sort(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "ALL OK" in out.stdout
