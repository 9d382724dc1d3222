"""GPU: the 16-byte streaming loads of rsx_count16top_kernel (8- and 16-byte elements).

The kernel reads a workgroup's chunk [p0, p1) in 16-byte words: an 8-byte element ahead of the chunk's first 16-byte
boundary and an odd one at its end are counted one by one.  What can go wrong is membership (an element counted twice,
never, or into the neighbour's row of the counters) and an element that misses the check of the bits above the window.
Every case runs from the start of its buffer and from one element into it (8-byte elements: a base that is 8-byte
aligned and not 16), with a guard element at the buffer's other end that must come back untouched.  Parity with the
oracle is on the raw bytes; the reported path is that of test_gpu_parity.py's hybrid tests."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

UNROLL = 4  # RSX_COUNT16_UNROLL: 16-byte loads in flight per thread
TYPES = ["u64", "i64", "f64", "(u64,u64)", "u128"]  # MAP and non-MAP forms, 8- and 16-byte elements
BUCKET_KEYS = {8: 17, 16: 7}


def _mid_max(es):
    return 1 << 22 if es == 8 else 1024 * BUCKET_KEYS[es] * 256 * 4 // 7


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def rs():
    import radix_sort_amd as rs
    return rs


def _sort_at(rs, torch, c, raw, d, lead):
    """Sorts `raw` on the device from `lead` elements into a buffer of n + 1 elements; returns the sorted bytes."""
    es = d.elem_bytes
    n = raw.size // es
    host = np.full((n + 1) * es, 0xA5, dtype=np.uint8)
    host[lead * es:(lead + n) * es] = raw
    buf = torch.from_numpy(host).cuda()
    tmp = torch.empty_like(buf)
    c.sort_device(buf.data_ptr() + lead * es, tmp.data_ptr(), n, d)
    c.check()
    out = buf.cpu().numpy()
    guard = out[:es] if lead else out[n * es:]
    assert np.all(guard == 0xA5), "the element beside the array was written"
    return out[lead * es:(lead + n) * es]


def _path(rs, c):
    return (c.get_info(rs.INFO_LAST_PASSES) >> 24) & 15


@pytest.mark.parametrize("extra", [1, 2, 3, 4097] + [2 * 1024 * UNROLL * k + s for k in (1, 2, 3) for s in (-1, 1)])
@pytest.mark.parametrize("t", TYPES)
def test_chunks_inside_regions(rs, torch, orc, t, extra):
    """RSX_OPT_WIDE_SORT = 3: k chunks per region, the first sweep's count matrix taken from the counters.  Sizes right
    above the middle sizes whose chunks hold fewer words than one unrolled round, one short of a round and one past it."""
    d = rs.RadixDigits(*util.TYPES[t])
    lay = orc.Layout(*util.TYPES[t])
    n = _mid_max(d.elem_bytes) + extra
    raw = util.make_input(t, n, "uniform", seed=7000 + extra)
    exp = orc.sort_parallel(raw, lay, 8)
    c = rs.Context(torch.cuda.current_device())
    for lead in (0, 1):
        c.set_option(rs.OPT_WIDE_SORT, 3)
        got = _sort_at(rs, torch, c, raw, d, lead)
        info = c.get_info(rs.INFO_LAST_PASSES)
        assert (info >> 24) & 15 == 5 and info & 255 == 2, (t, n, lead, hex(info))
        assert np.array_equal(got, exp), (t, n, lead)
    c.close()


@pytest.mark.parametrize("n", [65536, 65537, 65539, 70001])
@pytest.mark.parametrize("t", TYPES)
def test_flat_shares(rs, torch, orc, t, n):
    """RSX_OPT_WIDE_SORT = 2 (forced): the array cut into flat shares, whose starts are odd for odd shares."""
    d = rs.RadixDigits(*util.TYPES[t])
    lay = orc.Layout(*util.TYPES[t])
    raw = util.make_input(t, n, "uniform", seed=7100 + n)
    exp = orc.sort_parallel(raw, lay, 8)
    c = rs.Context(torch.cuda.current_device())
    c.set_option(rs.OPT_WIDE_SORT, 2)
    for lead in (0, 1):
        assert np.array_equal(_sort_at(rs, torch, c, raw, d, lead), exp), (t, n, lead)
    c.close()


N40 = (1 << 22) + 4097
REGION = 1 << 19  # the sweeps' region length at this size: the smallest power of two that cuts the array into <= 16
_SEEDED = [int(p) for p in np.random.default_rng(4097).integers(2, N40 - 2, size=3)]
OUTLIERS = [0, 1, N40 - 2, N40 - 1] + [m + s for m in range(REGION, N40, REGION) for s in (-1, 0)] + _SEEDED


@pytest.fixture(scope="module")
def keys40():
    """u64 keys below 2^40 (the window then sits below the key's top), shared and left unchanged."""
    rng = np.random.default_rng(40)
    k = rng.integers(0, 1 << 40, size=N40, dtype=np.uint64)
    k.setflags(write=False)
    return k


@pytest.mark.parametrize("pos", OUTLIERS)
def test_the_check_above_the_window_sees_every_element(rs, torch, orc, keys40, pos):
    """One element with a bit above the sampled range: at the array's ends, on both sides of every region edge (chunk
    edges lie on region edges) and at seeded positions; with both bases it is once a peeled element, once inside a
    word.  Where the plan's sample does not hold it (the plan looks at every (n / 16384)-th element and the last one)
    the count must find it and the device refuse the hybrid: path 0, as test_wide_key_hybrid_follows_the_range_of_the_keys
    expects for its outlier.  Where the sample holds it the window moves; the sort stays correct either way."""
    assert REGION * 16 >= N40 > REGION * 8
    d = rs.RadixDigits(*util.TYPES["u64"])
    lay = orc.Layout(*util.TYPES["u64"])
    k = keys40.copy()
    k[pos] ^= np.uint64(0x40 << 56)
    raw = k.view(np.uint8)
    exp = orc.sort_parallel(raw, lay, 8)
    step = N40 // 16384
    sampled = pos == N40 - 1 or (pos % step == 0 and pos // step < 16383)
    c = rs.Context(torch.cuda.current_device())
    for lead in (0, 1):
        c.set_option(rs.OPT_WIDE_SORT, 3)  # (a refusal is followed by sorts without a try: start over)
        got = _sort_at(rs, torch, c, raw, d, lead)
        if not sampled:
            assert _path(rs, c) == 0, (pos, lead, hex(c.get_info(rs.INFO_LAST_PASSES)))
        assert np.array_equal(got, exp), (pos, lead)
    c.close()


def test_the_keys_below_2_40_take_the_hybrid_without_an_outlier(rs, torch, orc, keys40):
    """(The counterpart of the test above: no outlier, no refusal -- so that path 0 there is the outlier's doing.)"""
    d = rs.RadixDigits(*util.TYPES["u64"])
    raw = keys40.view(np.uint8)
    exp = orc.sort_parallel(raw, orc.Layout(*util.TYPES["u64"]), 8)
    c = rs.Context(torch.cuda.current_device())
    for lead in (0, 1):
        c.set_option(rs.OPT_WIDE_SORT, 3)
        got = _sort_at(rs, torch, c, raw, d, lead)
        assert _path(rs, c) == 5, (lead, hex(c.get_info(rs.INFO_LAST_PASSES)))
        assert np.array_equal(got, exp), lead
    c.close()


def _crowded(n, first, count, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    k[first:first + count] = (k[first:first + count] & np.uint64((1 << 48) - 1)) | np.uint64(0xBEEF << 48)
    return k.view(np.uint8)


@pytest.mark.parametrize("first", [1000, 1001])
def test_a_crowded_bin_in_small_flat_shares(rs, torch, orc, first):
    """Forced mode, 70001 u64 of which 40000 contiguous keys share their top 16 bits, starting at an even and at an odd
    element.  (At this size a workgroup's share is n / 4 = 17501 elements, so no half reaches 0x8000 here: the test
    below has shares that do.)"""
    d = rs.RadixDigits(*util.TYPES["u64"])
    raw = _crowded(70001, first, 40000, seed=first)
    exp = orc.sort_parallel(raw, orc.Layout(*util.TYPES["u64"]), 8)
    c = rs.Context(torch.cuda.current_device())
    c.set_option(rs.OPT_WIDE_SORT, 2)
    for lead in (0, 1):
        assert np.array_equal(_sort_at(rs, torch, c, raw, d, lead), exp), (first, lead)
    c.close()


def test_a_parked_half_still_parks(rs, torch, orc):
    """Forced mode with shares of 40001 elements (one workgroup per CU, so n = 40001 * CUs - 5): the first 120003 keys
    share their top 16 bits, so the workgroups of shares 0 (even start), 1 (odd start) and 2 each add more than 0x8000
    times to one half of a packed counter and must park it in the overflow table."""
    d = rs.RadixDigits(*util.TYPES["u64"])
    c = rs.Context(torch.cuda.current_device())
    cu = c.get_info(rs._lib.INFO_NUM_CU)
    n = 40001 * cu - 5
    assert n * 8 // 131072 >= cu  # one share per CU
    raw = _crowded(n, 0, 3 * 40001, seed=5)
    exp = orc.sort_parallel(raw, orc.Layout(*util.TYPES["u64"]), 8)
    c.set_option(rs.OPT_WIDE_SORT, 2)
    for lead in (0, 1):
        assert np.array_equal(_sort_at(rs, torch, c, raw, d, lead), exp), lead
    c.close()
