"""CPU: the digit widths and the limit of rsx_bucket16_direct_kernel as the kernel source states them are the numpy
models' (bucket_direct_ref.BITS: the counter words; bucket_direct_packed_ref.COUNT_BITS: the digit of the counting pass),
and the counters are packed, whatever the build."""
import os
import re

import bucket_direct_packed_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source():
    text = open(os.path.join(ROOT, "radix_sort_amd", "csrc", "rsx_small_kernel.hpp")).read()
    return re.sub(r"//[^\n]*", "", text)


def test_library_bits_match_the_models():
    text = _source()
    m = re.search(r"constexpr uint32_t direct_bits\(\)\s*\{\s*return WG >= 1024 \? (\d+)u : WG >= 512 \? (\d+)u : (\d+)u;", text)
    assert m, "direct_bits() not found"
    words = dict(zip((1024, 512, 256), (int(v) for v in m.groups())))
    assert words == ref.BITS
    raw = open(os.path.join(ROOT, "radix_sort_amd", "csrc", "rsx_small_kernel.hpp")).read()
    assert "RSX_DIRECT_" + "PACKED" not in raw, "the counters are packed: the build switch that chose otherwise is gone"
    m = re.search(r"constexpr uint32_t DIRECT_EXTRA_BITS = (\d+)u;", text)
    assert m and m.group(1) == "1", "DIRECT_EXTRA_BITS = 1u not found"
    assert {wg: b + int(m.group(1)) for wg, b in words.items()} == ref.COUNT_BITS
    assert re.search(r"constexpr uint32_t BC = B \+ DIRECT_EXTRA_BITS;", text), "the kernel counts on B + DIRECT_EXTRA_BITS bits"
    m = re.search(r"constexpr uint32_t DIRECT_LIMIT = (\d+);", text)
    assert m and int(m.group(1)) == ref.LIMIT
    # a count and a start fit a 16-bit half: the largest bucket a workgroup holds (1024 threads x 17 keys) leaves room
    assert 17 * 1024 < 1 << 16
