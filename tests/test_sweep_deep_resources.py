"""Register budget of the hybrid's deep second sweep (no GPU needed: hipcc reports it at compile time).

The wide-key hybrid's second sweep of 8-byte elements runs rsx_sweep_kernel<8, 18, 512, S, 0, false, false, true>: 18 keys
per thread instead of 14, in the LDS that the next pass's count matrix takes in the first sweep.  Its 73 728-byte tile
leaves room for two workgroups per CU only; those are 16 waves per CU, 4 per SIMD, so the kernel has to stay within 128
VGPRs -- and a spill would put scratch traffic into a kernel that is bound by memory.  This test compiles the 8-byte unit
with -Rpass-analysis=kernel-resource-usage, the way test_count16_resources.py does, and asks every instantiation at 18
keys per thread for no spilled VGPR, no scratch and 4 waves per SIMD.  (Every sweep instantiation, at 14 keys too, moves
some SGPRs into VGPR lanes under the kernel's 102-SGPR cap -- 15 and 17 here, as many as the same form at 14 keys: that
costs no memory traffic and is not what this test is about.)"""
from test_kernel_resources import _resources

HYB_KPT8 = 18  # hyb_kpt_for(8), rsx_internal.hpp


def test_deep_sweep_kernels_spill_nothing_and_keep_four_waves():
    res = _resources(8)
    deep = [n for n in res if f"rsx_sweep_kernelILi8ELi{HYB_KPT8}ELi512E" in n]
    # one per status word width (regions of up to 2^30 elements, and above): the STR form that counts for no next pass
    assert len(deep) == 2, sorted(n for n in res if "rsx_sweep_kernel" in n)
    for name in deep:
        r = res[name]
        print(name, r)
        assert "VGPRs" in r, (name, r)  # (the remarks were parsed at all)
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]", 0) >= 4, (name, r)
        assert r["VGPRs"] <= 128, (name, r)
