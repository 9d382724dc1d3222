"""Register budget of rsx_count16top_kernel (no GPU needed: hipcc reports it at compile time).

The kernel keeps RSX_COUNT16_UNROLL 16-byte words in flight per thread next to the plan's reference and masks, with
1024 threads per workgroup: a spill would put scratch traffic into a kernel that is bound by its loads.  This test
compiles the 8- and 16-byte units with -Rpass-analysis=kernel-resource-usage, the way test_kernel_resources.py does,
and asks every instantiation for no spill and no scratch."""
import pytest

from test_kernel_resources import _resources


@pytest.mark.parametrize("es", [8, 16])
def test_count16top_kernel_spills_nothing(es):
    res = _resources(es)
    names = [n for n in res if "rsx_count16top_kernel" in n]
    assert len(names) == 2, sorted(res)  # the MAP and the non-MAP form
    for name in names:
        assert res[name].get("VGPRs Spill", 0) == 0, (name, res[name])
        assert res[name].get("ScratchSize [bytes/lane]", 0) == 0, (name, res[name])
        assert "VGPRs" in res[name], (name, res[name])  # (the remarks were parsed at all)
