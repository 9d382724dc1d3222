"""GPU: the end of a bucket in rsx_bucket16_kernel -- isolated pairs mended in LDS ahead of the read-back
(local_mend_pairs), the registers stored straight to memory, longer runs left to the list mend -- bit for bit against
the CPU oracle, payload = index where the type has one.

The parity tests' inputs put a few keys into each of the 65536 buckets, so the 512- and 1024-thread forms and a second
bucket per workgroup are met only at sizes of 2^28 and more.  Here a few dozen values of the key's top 16 bits hold
thousands of keys each (the sizes name the form: rsx_scan16_kernel picks the smallest workgroup that holds all but eight
buckets), and they sit `grid` apart -- workgroup w takes buckets w, w + grid, w + 2 grid ... -- so that every workgroup
that has one bucket has a chain of them.  Every input's bucket sizes are checked with numpy before it is used."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

TYPES = ["u64", "(u64,u64)", "u128"]
CAP = {8: 1024 * 17, 16: 1024 * 7}  # what the 1024-thread form holds (cape()); the 512-thread form: half, the 256-thread one: a quarter
OPTIONS = [(1, 1), (0, 1), (1, 0)]  # (OPT_BUCKET_SKIP, OPT_BUCKET_GROUP): the default, every pass, no groups on offer


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def rs():
    import radix_sort_amd as rs
    return rs


@pytest.fixture(scope="module")
def num_cu(torch):
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _bucket(rng, kb, w, m, plants):
    """(m, kb) key bytes of the bucket of window value w, in the order the LDS passes leave them: the three bytes below
    the window (what the passes of a bucket of this size sort by: `mid`) ascending, natural ties included; the bytes
    below those (`low`: the skipped digits) uniform.  plants: (kind, r, length) -- the keys r-1 .. r+length-2 agree on mid:
    "pair" / "run" with random low bytes (in and out of order), "equal" with equal low bytes (equal keys)."""
    mid = np.sort(rng.integers(16, (1 << 24) - 16, size=m, dtype=np.int64))
    low = rng.integers(0, 256, size=(m, kb - 5), dtype=np.uint8)
    for kind, r, length in plants:
        if r < 1 or r + length - 1 > m:
            continue
        mid[r:r + length - 1] = mid[r - 1]
        if kind == "equal":
            low[r:r + length - 1] = low[r - 1]
    key = np.zeros((m, kb), dtype=np.uint8)
    key[:, :kb - 5] = low
    for j in range(3):
        key[:, kb - 5 + j] = (mid >> (8 * j)) & 0xFF
    key[:, kb - 2] = w & 0xFF
    key[:, kb - 1] = w >> 8
    return key


def _plants(m, wg, fallback=False, equal_runs=False):
    """Where ties are planted in a bucket of m keys sorted by a workgroup of wg threads (tile indices)."""
    p = [("pair", 1, 2), ("pair", m - 1, 2),                            # tile indices 0/1 and m-2/m-1
         ("pair", wg, 2), ("pair", 2 * wg, 2), ("pair", 3 * wg + 64, 2),  # across i = k wg and i = k 64
         ("pair", 192, 2), ("equal", 300, 2), ("equal", 5 * 64, 2), ("equal", wg + 64, 2),
         ("pair", 700, 2), ("pair", 702, 2),                            # back to back, not tied to each other
         ("pair", 64 * 9 + 1, 2), ("pair", 64 * 9 + 3, 2)]
    p += [("pair", 1000 + 37 * k, 2) for k in range(12) if 1000 + 37 * k < m - 4]
    if equal_runs:  # long runs of equal keys: no fallback, nothing moves
        p += [("equal", 1500, 40), ("equal", wg - 3, 9)]
    if fallback:    # runs of three and four that differ in the skipped digits: the check, the list, the store from LDS
        p += [("run", 1600, 3), ("run", 1700, 4), ("run", 2 * wg - 1, 3)]
    return p


def _assemble(rng, t, buckets):
    """buckets: {window value: (m, plants)} -> (raw bytes in a seeded random order with payload = index, counts by window value)"""
    es, ko, kb, _kind = util.TYPES[t]
    keys = np.concatenate([_bucket(rng, kb, w, m, pl) for w, (m, pl) in sorted(buckets.items())])
    n = len(keys)
    keys = keys[rng.permutation(n)]
    raw = np.zeros((n, es), dtype=np.uint8)
    raw[:, ko:ko + kb] = keys
    idx = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8)
    for j, b in enumerate(b for b in range(es) if not ko <= b < ko + kb):
        raw[:, b] = idx[:, j] if j < 8 else 0
    window = keys[:, kb - 2].astype(np.int64) | (keys[:, kb - 1].astype(np.int64) << 8)
    return raw.reshape(-1), np.bincount(window, minlength=65536)


def _chains(bases, length, grid):
    return [[b + k * grid for k in range(length)] for b in bases]


def _input_big(t, form, num_cu):
    """48 buckets in 6 chains of 8, every one above half of what the form's workgroup holds and below all of it:
    1024 threads: 9000 .. 17000 keys of 17408 (8-byte elements), 512 threads: 5000 .. 8500 of 8704."""
    es = util.TYPES[t][0]
    cap = CAP[es] * form // 1024
    rng = np.random.default_rng(1000 + es + form + util.TYPES[t][2])
    lo, hi = (9000, 17000) if form == 1024 else (5000, 8500)
    lo, hi = lo * CAP[es] // CAP[8], hi * CAP[es] // CAP[8]
    grid = num_cu * (1024 // form)
    # (512: the chains in adjacent pairs, so that no aligned group of four or more buckets fits a 512-thread workgroup and
    # the verdict is the plain 512-thread form, not groups)
    bases = [8, 1100, 9000, 33000, 40004, 50100] if form == 1024 else [8, 9, 1100, 1101, 40004, 40005]
    buckets = {}
    for c, chain in enumerate(_chains(bases, 8, grid)):
        for k, w in enumerate(chain):
            m = int(rng.integers(lo, hi + 1))
            buckets[w] = (m, _plants(m, form, fallback=(c == 1 and k == 2), equal_runs=(c + k) % 3 == 0))
    raw, counts = _assemble(rng, t, buckets)
    occ = counts[counts > 0]
    assert len(occ) == 48 and occ.min() > cap // 2 and occ.max() <= cap, (t, form, occ.min(), occ.max())
    assert np.count_nonzero(counts[:32768]) and np.count_nonzero(counts[32768:])  # the window is the key's top 16 bits
    assert all(counts[w + grid] > 0 for ch in _chains(bases, 7, grid) for w in ch)  # every bucket but a chain's last has a next one
    if form == 512:
        assert np.count_nonzero(counts.reshape(-1, 4).sum(axis=1) > cap) > 8
    return raw


def _input_edges(t, num_cu):
    """The 1024-thread form (more than eight buckets above the 512-thread form's workgroup) with chains whose buckets have
    the sizes the pair loop and the register store have edges at: 1, 2, odd and even counts (the buckets behind an odd
    count start at an odd element index), cape() and cape() - 1, an empty bucket between occupied ones, one above cape()
    (the medium kernel's) inside a chain, a bucket that falls back followed by ordinary ones, and the array's last bucket."""
    es = util.TYPES[t][0]
    cap = CAP[es]
    rng = np.random.default_rng(2000 + es + util.TYPES[t][2])
    grid = num_cu
    big = lambda: int(rng.integers(cap // 2 + 100, cap - 100))
    sizes = [big() | 1, 1, 2, big() | 1, big() & ~1, cap, cap - 1, 0, big(), cap + 37, big() | 1, big(), big(), big() | 1]
    fallback_at = 11
    buckets = {}
    for k, m in enumerate(sizes):
        if m:
            buckets[8 + k * grid] = (m, _plants(m, 1024, fallback=k == fallback_at, equal_runs=k == 4))
    last = [65535 - (3 - k) * grid for k in range(4)]  # ... 65535: the array's last bucket, an odd count
    for k, w in enumerate(last):
        m = big() | 1
        buckets[w] = (m, _plants(m, 1024))
    raw, counts = _assemble(rng, t, buckets)
    assert [int(counts[8 + k * grid]) for k in range(len(sizes))] == sizes and counts[65535] % 2 == 1
    assert np.count_nonzero(counts) == len(sizes) - 1 + 4
    assert np.count_nonzero(counts > cap // 2) > 8 and np.count_nonzero(counts > cap) == 1
    starts = np.concatenate([[0], np.cumsum(counts)])[:-1]
    assert np.count_nonzero(starts[counts > 0] % 2 == 1) >= 4  # buckets that start at an odd element index
    return raw


_CASES = {}  # (t, name) -> (input, expected): made once, shared by the option settings, never changed


def _case(orc, t, name, num_cu):
    if (t, name) not in _CASES:
        raw = _input_edges(t, num_cu) if name == "edges" else _input_big(t, int(name), num_cu)
        exp = orc.sort_parallel(raw, orc.Layout(*util.TYPES[t]), 8)
        raw.setflags(write=False)
        exp.setflags(write=False)
        _CASES[(t, name)] = (raw, exp)
    return _CASES[(t, name)]


def _run(rs, torch, orc, t, name, num_cu, skip, group):
    raw, exp = _case(orc, t, name, num_cu)
    c = rs.Context(torch.cuda.current_device())
    c.set_option(rs.OPT_WIDE_SORT, 2)
    c.set_option(rs.OPT_BUCKET_SKIP, skip)
    c.set_option(rs.OPT_BUCKET_GROUP, group)
    x = torch.from_numpy(raw.copy()).cuda()
    rs.radix_sort(x, digits=rs.RadixDigits(*util.TYPES[t]), ctx=c)
    c.check()
    info = c.get_info(rs.INFO_LAST_PASSES)
    got = x.cpu().numpy()
    c.close()
    assert (info >> 24) & 15 == 5, (t, name, hex(info))
    assert np.array_equal(got, exp), (t, name, skip, group, int(np.flatnonzero(got != exp)[0]) // util.TYPES[t][0])


@pytest.mark.parametrize("skip,group", OPTIONS)
@pytest.mark.parametrize("form", [1024, 512])
@pytest.mark.parametrize("t", TYPES)
def test_big_forms_mend_pairs(rs, torch, orc, num_cu, t, form, skip, group):
    """Chains of eight buckets per workgroup in the 1024- and the 512-thread form: natural ties (a handful of isolated
    pairs per bucket) and planted ones -- pairs in and out of order, pairs of equal keys, at the tile's first and last two
    indices, across i = k WG and i = k 64, back to back; runs of three and four that differ in the skipped digits (one
    bucket of a chain: the fallback, and ordinary buckets behind it); long runs of equal keys."""
    _run(rs, torch, orc, t, str(form), num_cu, skip, group)


@pytest.mark.parametrize("skip,group", OPTIONS)
@pytest.mark.parametrize("t", TYPES)
def test_bucket_size_edges(rs, torch, orc, num_cu, t, skip, group):
    """Bucket counts of 1, 2 (the pair is the whole tile), odd, even, cape() and cape() - 1, odd element starts, empty
    buckets inside a chain, a bucket for the medium kernel, a fallback inside a chain, the array's last bucket."""
    _run(rs, torch, orc, t, "edges", num_cu, skip, group)
