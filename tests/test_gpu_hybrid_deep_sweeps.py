"""GPU: the wide-key hybrid of 8-byte elements, whose second sweep runs tiles of 512 x 18 keys over the regions that the
first sweep fills in tiles of 512 x 14 -- byte for byte against the CPU oracle's stable sort.

What can go wrong is arithmetic on tile and region boundaries: the second sweep's tile counts, its status rows (a prefix of
the rows the first sweep zeroed by ITS tile numbering), the workgroups it gives each region, and the tickets of the dynamic
schedule.  So the sizes sit where that arithmetic changes, just above 2^22 elements (the smallest array the hybrid takes,
RSX_OPT_WIDE_SORT = 3):
  * 1 region (RSX_OPT_MAX_REGIONS = 1): n = m * 512 * K - 1, exactly, + 1 for K = 14 and K = 18 -- a last tile that is
    full for one sweep and not the other, and one of a single key;
  * 2 regions (cap 2: regions of 2^22): a last region of 1 key, of one tile of either depth less one key, exactly, and
    plus one key;
  * the default cap: 9 regions (n = 2^22 + 1, fewer than 16), 16 regions (n = 2^23, all full; and a last region of one
    key, and of three deep tiles plus one key), and 2^23 + 1 (regions of 2^20 again).
Types: u64 everywhere; i64, f64 and (u32,u32) -- payload = index, so that a lost tie shows -- on one size per region
count.  Keys below 2^40, and keys of one value range of 32 (five fixed top bits), put the window's digits across a dword
boundary of the element.  Every input is uniform over its range, so every 16-bit bucket (64 to 128 keys on average) fits
the bucket kernel's workgroup and the device takes the hybrid: the test asks RSX_INFO_LAST_PASSES for that."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

T14, T18 = 512 * 14, 512 * 18
BASE = 1 << 22  # mid_max_elems(8): the hybrid takes arrays above it
M14, M18 = 586, 456  # the fewest tiles of either depth above 2^22 elements
assert (M14 - 1) * T14 <= BASE < M14 * T14 and (M18 - 1) * T18 <= BASE < M18 * T18

ONE_REGION = [M14 * T14 - 1, M14 * T14, M14 * T14 + 1, M18 * T18 - 1, M18 * T18, M18 * T18 + 1]
TWO_REGIONS = [BASE + d for d in (1, T14 - 1, T14, T14 + 1, T18 - 1, T18, T18 + 1)]
R16 = (1 << 23) - (1 << 19)  # 15 full regions of 2^19
DEFAULT_CAP = [BASE + 1, 1 << 23, R16 + 1, R16 + 3 * T18 + 1, (1 << 23) + 1]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def rs():
    import radix_sort_amd as rs
    return rs


def regions_of(n, cap):
    """make_geom for 8-byte elements: the smallest power-of-two region of at least 64 tiles of 512 x 14 that covers n with
    at most `cap` regions (0: the default, 16)."""
    k = 13 + 6
    while -(-n // (1 << k)) > (cap or 16):
        k += 1
    return -(-n // (1 << k)), k


_CASES = {}  # (type, n, range) -> (input, expected): made once, shared, never changed


def _case(orc, t, n, key_range):
    key = (t, n, key_range)
    if key not in _CASES:
        raw = util.make_input(t, n, "uniform", 9000 + n % 1009 + util.TYPES[t][3])
        if key_range is not None:  # u64 only: (bits, base)
            bits, base = key_range
            k = raw.view("<u8")
            k &= np.uint64((1 << bits) - 1)
            k |= np.uint64(base)
        exp = orc.sort_parallel(raw, orc.Layout(*util.TYPES[t]), 8)
        raw.setflags(write=False)
        exp.setflags(write=False)
        _CASES[key] = (raw, exp)
    return _CASES[key]


def _run(rs, torch, orc, t, n, cap, regions, schedule=0, key_range=None):
    assert regions_of(n, cap)[0] == regions, (n, cap, regions_of(n, cap))
    raw, exp = _case(orc, t, n, key_range)
    es = util.TYPES[t][0]
    c = rs.Context(torch.cuda.current_device())
    try:
        c.set_option(rs.OPT_WIDE_SORT, 3)
        c.set_option(rs.OPT_MAX_REGIONS, cap)
        c.set_option(rs.OPT_TILE_SCHEDULE, schedule)
        x = torch.from_numpy(raw.copy()).cuda()
        rs.radix_sort(x, digits=rs.RadixDigits(*util.TYPES[t]), ctx=c)
        c.check()
        lp = c.get_info(rs.INFO_LAST_PASSES)
        got = x.cpu().numpy()
    finally:
        c.close()
    assert (lp >> 24) & 15 == 5 and lp & 0xFF == 2, (t, n, hex(lp))  # the hybrid, and the device took it: two sweeps
    if schedule == 1:
        assert (lp >> 8) & 0xFF == 0, hex(lp)  # both by tickets
    assert np.array_equal(got, exp), (t, n, cap, int(np.flatnonzero(got != exp)[0]) // es)


@pytest.mark.parametrize("n", ONE_REGION)
def test_one_region_tile_multiples(rs, torch, orc, n):
    _run(rs, torch, orc, "u64", n, 1, 1)


@pytest.mark.parametrize("n", TWO_REGIONS)
def test_two_regions_short_last_region(rs, torch, orc, n):
    _run(rs, torch, orc, "u64", n, 2, 2)


@pytest.mark.parametrize("n", DEFAULT_CAP)
def test_default_regions(rs, torch, orc, n):
    _run(rs, torch, orc, "u64", n, 0, {BASE + 1: 9, (1 << 23) + 1: 9}.get(n, 16))


@pytest.mark.parametrize("n,cap,regions", [(M18 * T18 + 1, 1, 1), (BASE + T18 - 1, 2, 2), (R16 + 3 * T18 + 1, 0, 16)])
@pytest.mark.parametrize("t", ["i64", "f64", "(u32,u32)"])
def test_signed_float_and_payload(rs, torch, orc, t, n, cap, regions):
    _run(rs, torch, orc, t, n, cap, regions)


@pytest.mark.parametrize("n,cap,regions", [(M18 * T18 + 1, 1, 1), (BASE + 1, 2, 2), (R16 + 3 * T18 + 1, 0, 16)])
@pytest.mark.parametrize("t", ["u64", "(u32,u32)"])
def test_ticketed_tiles(rs, torch, orc, t, n, cap, regions):
    """RSX_OPT_TILE_SCHEDULE = 1: every tile of both sweeps by a ticket of its region, each counted in that sweep's tiles."""
    _run(rs, torch, orc, t, n, cap, regions, schedule=1)


@pytest.mark.parametrize("key_range", [(40, 0), (59, 0x5 << 59)], ids=["below-2^40", "one-range-of-32"])
@pytest.mark.parametrize("n,cap,regions", [(BASE + T18 + 1, 2, 2), (R16 + 3 * T18 + 1, 0, 16)])
def test_window_across_a_dword(rs, torch, orc, n, cap, regions, key_range):
    _run(rs, torch, orc, "u64", n, cap, regions, key_range=key_range)
