"""Register budget of rsx_bucket16_direct_kernel with the pipelined load (no GPU needed: hipcc reports it at compile time,
the method of test_bucket_direct_resources.py).  The 8-byte elements' 1024- and 512-thread forms keep the next bucket's
loads in flight across the rank loop: that must cost them neither a spill nor a byte of scratch nor a wave -- one
workgroup of 1024 threads or two of 512 per CU need 4 waves per SIMD.  The 256-thread form (three per CU) needs 3 and has
no scratch either; the 16-byte forms keep the bounds they had."""
import pytest

from test_kernel_resources import _resources


def _direct(es):
    res = _resources(es)
    return {n: r for n, r in res.items() if "rsx_bucket16_direct_kernel" in n}


@pytest.mark.parametrize("wg", [1024, 512])
def test_pipelined_forms_have_no_scratch_at_four_waves(wg):
    forms = {n: r for n, r in _direct(8).items() if f"Li{wg}E" in n}
    assert forms, sorted(_direct(8))
    for name, r in forms.items():
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]", 0) >= 4, (name, r)


def test_256_thread_form_has_no_scratch_at_three_waves():
    forms = {n: r for n, r in _direct(8).items() if "Li256E" in n}
    assert forms, sorted(_direct(8))
    for name, r in forms.items():
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]", 0) >= 3, (name, r)


def test_sixteen_byte_forms_keep_their_bounds():
    forms = _direct(16)
    assert {w for w in (1024, 512, 256) if any(f"Li{w}E" in n for n in forms)} == {1024, 512, 256}, sorted(forms)
    for name, r in forms.items():
        assert r.get("VGPRs Spill", 0) <= 16, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) <= 128, (name, r)
        assert r.get("Occupancy [waves/SIMD]", 0) >= (3 if "Li256E" in name else 4), (name, r)
