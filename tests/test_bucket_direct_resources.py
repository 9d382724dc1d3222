"""Register budget of rsx_bucket16_direct_kernel (no GPU needed: hipcc reports it at compile time), by the method of
test_kernel_resources.py: every instantiation for 8- and 16-byte elements keeps its spills and scratch small and reaches
the waves per SIMD its form is launched for (two workgroups of 512 threads / three of 256 per CU need 4 / 3)."""
import pytest

from test_kernel_resources import _resources


@pytest.mark.parametrize("es", [8, 16])
def test_direct_kernels_fit_their_registers(es):
    res = _resources(es)
    names = [n for n in res if "rsx_bucket16_direct_kernel" in n]
    assert len(names) >= 3, sorted(res)  # 1024, 512 and 256 threads (16-byte elements: two 1024-thread forms)
    assert {w for w in (1024, 512, 256) if any(f"Li{w}E" in n for n in names)} == {1024, 512, 256}, names
    for name in names:
        r = res[name]
        assert r.get("VGPRs Spill", 0) <= 16, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) <= 128, (name, r)
        assert r.get("Occupancy [waves/SIMD]", 0) >= (3 if "Li256E" in name else 4), (name, r)
