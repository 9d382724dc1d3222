"""CPU: why the clustered inputs of tests/test_gpu_hybrid_clustered.py bite, shown without a GPU.

For every case the input is built and what the case relies on is asserted (hybrid_clustered_inputs.conditions: exact
(chunk, bin) counts over the mirror's chunks, at most 8 hot buckets, each above the largest workgroup and below medium_max,
together at most n / 64).  Then rsx_count16top_kernel's packed 16-bit counters are emulated with their parking rule, and
the first sweep's count matrix is made both ways: as rsx_marginal16_kernel makes it, from the counters alone, and as a
count of the array.  The two differ -- by multiples of 0x8000, in the hot buckets' low digits, in the regions of the chunks
that parked -- exactly in the cases meant to park, and are equal in every other case.  The overflow table, added to the
counters per BIN, always restores the bin totals (rsx_total16_kernel): the totals, the starts and the verdict are right
either way, which is why only a flag from the count kernel can tell the verdict that the marginal is short."""
import numpy as np
import pytest

import hybrid_clustered_inputs as hci
import util


def test_geometry_mirror_known_shapes():
    """make_geom and sort_wide's parts / k at the sizes the cases use (256 CUs)."""
    g = hci.geometry(hci.N22, 8, cap=1)
    assert (g.region_shift, g.num_regions, g.k) == (23, 1, 256) and g.chunks[3] == (3 * 32768, 4 * 32768)
    g = hci.geometry(hci.N23, 8)
    assert (g.region_shift, g.num_regions, g.k) == (20, 9, 28) and g.chunks[1] == (37450, 74900)
    assert g.chunks[27] == (27 * 37450, 1 << 20) and g.chunks[28] == (1 << 20, (1 << 20) + 37450)  # a region's last chunk is cut
    assert g.chunks[8 * 28] == (1 << 23, hci.N23) and g.chunks[-1] == (hci.N23, hci.N23)     # the last region: one element
    g = hci.geometry(hci.N24, 8)
    assert (g.region_shift, g.num_regions, g.k) == (20, 16, 16) and g.chunks[17] == ((1 << 20) + 65536, (1 << 20) + 131072)
    g = hci.geometry(hci.N23, 16)
    assert (g.region_shift, g.num_regions, g.k) == (21, 5, 51) and g.chunks[0] == (0, 41121)
    assert hci.geometry((1 << 22) + 1, 8) == hci.geometry((1 << 22) + 1, 8, cap=16) and hci.geometry((1 << 22) + 1, 8).num_regions == 9
    assert hci.wide_cap(8) == 17408 and hci.medium_max(8) == 15360 * 150 and hci.mid_max(16) == 1 << 20


def test_counter_emulation_parks_at_0x8000():
    """the packed counter on hand-made counts: 0x7FFF stays, 0x8000 leaves nothing, 0x10001 leaves one"""
    c = np.zeros((2, 65536), dtype=np.int64)
    c[0, 6], c[0, 7], c[1, 7], c[1, 0x1234] = 0x7FFF, 0x8000, 0x10001, 0xFFFF
    P, ovf = hci.emulate_counters(c)
    assert P[0, 3] == 0x7FFF and P[1, 3] == 1 << 16 and P[1, 0x1234 >> 1] == 0x7FFF
    assert ovf[6] == 0 and ovf[7] == 0x18000 and ovf[0x1234] == 0x8000 and int(ovf.sum()) == 0x20000
    g = hci.Geometry(0, 2, 1, None)
    short = hci.true_marginal(c, g) - hci.marginal_of_counters(P, g)
    assert short[0, 7] == 0x8000 and short[1, 7] == 0x10000 and short[1, 0x34] == 0x8000 and int(short.sum()) == 0x20000


@pytest.mark.parametrize("name", list(hci.CASES))
def test_marginal_of_the_counters_is_short_exactly_when_a_counter_parks(name):
    case = hci.CASES[name]
    raw, geom, runs = hci.build(case)
    c = hci.conditions(case, raw, geom, runs)
    P, ovf = hci.emulate_counters(c)
    # the bin totals come out right with the overflow table (rsx_total16_kernel) ...
    unpacked = np.empty_like(c)
    unpacked[:, 0::2], unpacked[:, 1::2] = P & 0xFFFF, P >> 16
    assert np.array_equal(unpacked.sum(axis=0) + ovf, np.bincount(hci.bins(raw, case.t), minlength=65536))
    # ... the first sweep's count matrix does not
    short = hci.true_marginal(c, geom) - hci.marginal_of_counters(P, geom)
    assert short.min() >= 0 and not np.any(short % hci.PARK)
    if not case.parks:
        assert not short.any(), name
        return
    assert int(short.sum()) == int(ovf.sum()) >= hci.PARK, name
    hot_low = {int(b) & 0xFF for b in hci.map_top16(hci.hot_values(case.t, case.nhot), util.TYPES[case.t][3])}
    regions, digits = np.nonzero(short)
    assert set(digits.tolist()) == hot_low, (name, digits)  # every hot bucket's digit is short somewhere, and nothing else
    touched = {p >> geom.region_shift for _j, start, length in runs for p in (start, start + length - 1)}
    assert set(regions.tolist()) <= set(range(min(touched), max(touched) + 1)), (name, regions, touched)
