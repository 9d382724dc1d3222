"""Clustered inputs for the wide-key hybrid in its default mode (RSX_OPT_WIDE_SORT 1 and 3), numpy only; a helper, no tests.

In those modes rsx_count16top_kernel's workgroups are laid out k per region of the sweeps' geometry, and the first sweep's
count matrix is the marginal of their packed 16-bit counters.  A half-counter that reaches 0x8000 is "parked": 0x8000 of it
move to a table that is per bin, not per workgroup, so the marginal of the counters alone is then short by a multiple of
0x8000.  That takes 0x8000 elements of ONE bucket inside ONE count chunk -- which a uniform input never has, and zero
padding or a pre-sorted block has at once.  The verdict accepts such inputs for the hybrid (up to 8 buckets above the
largest workgroup, each below medium_max, together at most n / 64), so the count kernel reports a parked counter and the
verdict then gives the sort to the LSD passes.

This module
  * mirrors the host's geometry (make_geom, sort_wide's parts / k, the count chunks [p0, p1)) and the verdict's bounds;
  * builds the inputs: a uniform background in which no key has a hot value of its top 16 bits (those are moved to a
    neighbouring value), plus runs of hot keys at stated places, so that every (chunk, bin) count is exact;
  * emulates the packed counters with their parking rule and the two count matrices (marginal of the counters / true);
  * checks, on the CPU, what each case relies on (conditions) -- if a change of the geometry breaks one, that assert
    fails instead of the case quietly testing nothing.
tests/test_hybrid_clustered_inputs.py runs all of it without a GPU; tests/test_gpu_hybrid_clustered.py sorts the inputs."""
from __future__ import annotations

import zlib
from collections import namedtuple

import numpy as np

import util

NUM_CU = 256  # MI355X: what the CPU test assumes; the GPU test asks the device (RSX_INFO_NUM_CU)

# ---- the host's arithmetic, restated (rsx_internal.hpp, rsx.hip sort_wide) ----
LDS_PER_CU = 163840
TILE = {8: 512 * 14, 16: 512 * 5}    # tile_elems
DEFAULT_CAP = {8: 16, 16: 8}         # regions
BUCKET_KPT = {8: 17, 16: 7}
WIDE_KPT = {8: 17, 16: 9}
MEDIUM_KPT = {8: 15, 16: 9}
REGION_FLOOR = 6
FEW = 8                              # buckets above the largest workgroup that the verdict tolerates
PARK = 0x8000


def _lds_tile_fixed(wg):
    return wg // 64 * 256 * 4 + 64 + 3 * 256 * 4


def bucket_cape(es, kpt, wg):
    room = ((LDS_PER_CU - 1024 - _lds_tile_fixed(wg)) // es) & ~3
    return min(wg * kpt, room)


def mid_max(es):
    return 1 << 22 if es == 8 else 1024 * BUCKET_KPT[es] * 256 * 4 // 7


def wide_cap(es):
    """what the hybrid's largest (1024-thread) workgroup holds"""
    return bucket_cape(es, WIDE_KPT[es], 1024)


def medium_max(es):
    """the largest bucket the medium kernel is given"""
    return bucket_cape(es, MEDIUM_KPT[es], 1024) * 150


Geometry = namedtuple("Geometry", "region_shift num_regions k chunks")


def geometry(n, es, cap=0, num_cu=NUM_CU):
    """make_geom + sort_wide: regions of 2^region_shift elements, k count workgroups per region, and their chunks
    [p0, p1) in workgroup order (chunk b belongs to region b // k; a chunk past the end of the array is empty)."""
    shift = (TILE[es] - 1).bit_length() + REGION_FLOOR
    while -(-n // (1 << shift)) > (cap or DEFAULT_CAP[es]):
        shift += 1
    regions = max(1, -(-n // (1 << shift)))
    parts = min(n * es // (32768 * 4), num_cu)
    k = parts // regions
    chunks = []
    if k > 0:
        rl = 1 << shift
        per = -(-rl // k)
        for b in range(k * regions):
            r0 = (b // k) << shift
            p0 = min(r0 + (b % k) * per, r0 + rl, n)
            chunks.append((p0, max(p0, min(p0 + per, r0 + rl, n))))
    return Geometry(shift, regions, k, chunks)


# ---- the cases ----
# runs(geom, n) -> [(hot index, first element, length)]; background: "uniform", or for inputs without hot keys "sorted",
# "reversed", "blocks" (uniform keys sorted inside blocks of 2^16); parks: whether some counter must park; path: what
# RSX_INFO_LAST_PASSES reports in modes 1 and 3 (5 the hybrid, 0 the LSD passes -- every parked input, and nine hot buckets)
Case = namedtuple("Case", "name t n cap nhot runs background parks path exact_in_chunk")

N22, N23, N24 = (1 << 22) + 200001, (1 << 23) + 1, 1 << 24
CASES = {}


def _add(name, t, n, cap, nhot, runs, background="uniform", parks=True, path=0, exact_in_chunk=None):
    assert name not in CASES
    CASES[name] = Case(name, t, n, cap, nhot, runs, background, parks, path, exact_in_chunk)


def _run_len(n):
    return n // 80


# Threshold: one region, one hot bin, all of it inside count chunk 3.  A chunk of the smallest array holds 32768
# elements (256 CUs), so the counts above 0x8000 take the next sizes: chunks of 65536 and 131072.
for _count, _n in ((0x7FFF, N22), (0x8000, N22), (0xFFFF, N23), (0x10000, N23), (0x10001, N24 + 1)):
    _add("threshold-%#x" % _count, "u64", _n, 1, 1, (lambda c: lambda g, n: [(0, g.chunks[3][0], c)])(_count),
         parks=_count >= PARK, path=0 if _count >= PARK else 5, exact_in_chunk=_count)

# Placement: a run of n / 80, at least two chunks long, wherever it starts
PLACEMENTS = {
    "at-0": lambda g, n: [(0, 0, _run_len(n))],
    "ends-at-n": lambda g, n: [(0, n - _run_len(n), _run_len(n))],
    "across-chunks": lambda g, n: [(0, (g.chunks[5][0] + g.chunks[5][1]) // 2, _run_len(n))],
    "across-regions": lambda g, n: [(0, (3 << g.region_shift) - _run_len(n) // 2, _run_len(n))],
    # two halves in two regions, each from the start of a chunk that holds 0x8000 or more
    "two-regions": lambda g, n: [(0, g.chunks[2][0], _run_len(n) // 2), (0, g.chunks[2 * g.k + 1][0], _run_len(n) // 2)],
}
for _p, _runs in PLACEMENTS.items():
    _add("u64-" + _p, "u64", N23, 0, 1, _runs)
_add("u64-2^24-across-regions", "u64", N24, 0, 1, PLACEMENTS["across-regions"])

# Types: one placement each (i64 and f64: the hot value has the sign bit set, see hot_values)
_add("i64-across-regions", "i64", N24, 0, 1, PLACEMENTS["across-regions"])
_add("f64-across-chunks", "f64", N23, 0, 1, PLACEMENTS["across-chunks"])
_add("(u32,u32)-ends-at-n", "(u32,u32)", N23, 0, 1, PLACEMENTS["ends-at-n"])
_add("(u64,u64)-across-regions", "(u64,u64)", N23, 0, 1, PLACEMENTS["across-regions"])
_add("u128-at-0", "u128", N23, 0, 1, PLACEMENTS["at-0"])

# Several hot buckets: three contiguous runs of 80000 from the start of a chunk (each has 0x8000 in some chunk of 65536;
# 240000 together, under n / 64 = 262144), and nine buckets of 20000, which park nothing and are refused by their number
_add("three-hot", "u64", N24, 0, 3, lambda g, n: [(j, g.chunks[7][0] + j * 80000, 80000) for j in range(3)])
_add("nine-hot", "u64", N24, 0, 9, lambda g, n: [(j, g.chunks[7][0] + j * 20000, 20000) for j in range(9)], parks=False, path=0)

# Locally ordered, globally uniform, just above mid_max: every bucket is contiguous in the input, and small
for _bg in ("sorted", "reversed", "blocks"):
    _add("u64-" + _bg, "u64", (1 << 22) + 4099, 0, 0, None, background=_bg, parks=False, path=5)
_add("(u64,u64)-sorted", "(u64,u64)", mid_max(16) + 4099, 0, 0, None, background="sorted", parks=False, path=5)

# a plain uniform input (graph replays, the sort after a refusal)
_add("u64-uniform", "u64", N23, 0, 0, None, parks=False, path=5)


def hot_values(t, nhot):
    """raw top 16 bits of the hot keys: consecutive values; for signed and float keys with the sign bit set"""
    kind = util.TYPES[t][3]
    base = 0x5A3C if kind == util.UNSIGNED else 0xC1A5  # (f64: finite negative numbers)
    return [base + j for j in range(nhot)]


def top16(raw, t):
    """raw top 16 key bits of every element"""
    es, ko, kb, _kind = util.TYPES[t]
    e = raw.reshape(-1, es)
    return e[:, ko + kb - 2].astype(np.uint32) | (e[:, ko + kb - 1].astype(np.uint32) << 8)


def bins(raw, t):
    """the count kernel's bin: the top 16 bits of the MAPPED key (radix_digits.rs: signed keys flip the sign, floats flip
    the sign or, if it is set, everything) -- the window of keys whose top bit differs among the samples"""
    return map_top16(top16(raw, t), util.TYPES[t][3])


def map_top16(top, kind):
    top = np.asarray(top, dtype=np.uint32)
    if kind == util.UNSIGNED:
        return top
    if kind == util.SIGNED:
        return top ^ np.uint32(0x8000)
    return np.where(top & 0x8000, ~top & 0xFFFF, top ^ 0x8000).astype(np.uint32)


def build(case, num_cu=NUM_CU):
    """-> (raw bytes, geometry, runs): seeded by the case's name"""
    es, ko, kb, _kind = util.TYPES[case.t]
    n = case.n
    geom = geometry(n, es, case.cap, num_cu)
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    key = rng.integers(0, 256, size=(n, kb), dtype=np.uint8)
    if case.background != "uniform":
        assert kb == 8 and case.runs is None
        v = key.view("<u8").reshape(n)
        if case.background == "blocks":
            for i in range(0, n, 1 << 16):
                v[i:i + (1 << 16)].sort()
        else:
            v.sort()
            if case.background == "reversed":
                v[:] = v[::-1].copy()
    runs = case.runs(geom, n) if case.runs else []
    if runs:
        hots = hot_values(case.t, case.nhot)
        spare = hots[-1] + 1  # the neighbour that takes the background's hot keys
        top = key[:, kb - 2].astype(np.uint32) | (key[:, kb - 1].astype(np.uint32) << 8)
        stray = np.isin(top, hots)
        key[stray, kb - 2] = spare & 0xFF
        key[stray, kb - 1] = spare >> 8
        for j, start, length in runs:
            assert 0 <= start and start + length <= n, (case.name, start, length)
            key[start:start + length, kb - 2] = hots[j] & 0xFF  # the bits below stay random: the bucket is still to be sorted
            key[start:start + length, kb - 1] = hots[j] >> 8
    raw = np.zeros((n, es), dtype=np.uint8)
    raw[:, ko:ko + kb] = key
    pay = [b for b in range(es) if not ko <= b < ko + kb]
    if pay:  # payload = index: a lost tie shows
        idx = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8)
        for j, b in enumerate(pay):
            raw[:, b] = idx[:, j] if j < 8 else 0
    return raw.reshape(-1), geom, runs


def chunk_counts(raw, t, geom):
    """c[chunk, bin]: what each count workgroup sees (np.bincount over the mirror's chunks)"""
    b = bins(raw, t)
    lens = np.array([p1 - p0 for p0, p1 in geom.chunks], dtype=np.int64)
    assert geom.chunks[0][0] == 0 and geom.chunks[-1][1] == b.size
    assert all(geom.chunks[i][1] == geom.chunks[i + 1][0] for i in range(len(lens) - 1))  # the chunks tile the array in order
    chunk = np.repeat(np.arange(len(lens), dtype=np.uint32), lens)
    return np.bincount(chunk * np.uint32(65536) + b, minlength=len(lens) * 65536).reshape(len(lens), 65536)


def emulate_counters(c):
    """rsx_count16top_kernel on exact counts c[chunk, bin]: -> (P, ovf).  P[chunk, word] packs the counters of bins 2 w and
    2 w + 1 in 16 bits each; a half that reaches 0x8000 gives 0x8000 to ovf[bin] and goes on from what is left."""
    half = c % PARK
    ovf = (c - half).sum(axis=0)
    P = (half[:, 0::2] | (half[:, 1::2] << 16)).astype(np.uint32)
    return P, ovf


def marginal_of_counters(P, geom):
    """rsx_marginal16_kernel: J[region, v] = sum over the region's chunks and the top byte h of the counter of bin h * 256 + v"""
    lo, hi = (P & 0xFFFF).astype(np.int64), (P >> 16).astype(np.int64)
    per_bin = np.empty((P.shape[0], 65536), dtype=np.int64)
    per_bin[:, 0::2], per_bin[:, 1::2] = lo, hi
    return per_bin.reshape(geom.num_regions, geom.k, 256, 256).sum(axis=(1, 2))


def true_marginal(c, geom):
    """the first sweep's count matrix as a count kernel of its own makes it: the low digit's histogram per region"""
    return c.reshape(geom.num_regions, geom.k, 256, 256).sum(axis=(1, 2))


def conditions(case, raw, geom, runs, es=None):
    """What the case relies on, asserted; -> c[chunk, bin].  es: the size of the elements that are sorted when it is not the
    input's (the key / value calls sort joined elements: `geom` is then the geometry of that size, the bounds follow it)."""
    kb = util.TYPES[case.t][2]
    es = es or util.TYPES[case.t][0]
    n = case.n
    assert geom.k > 0, (case.name, geom)  # the counters are laid out per region: the marginal is used
    assert n > mid_max(es) and n // 65536 < wide_cap(es) and kb >= 4, case.name  # the host tries the hybrid (mode 3)
    c = chunk_counts(raw, case.t, geom)
    totals = c.sum(axis=0)
    assert int(totals.sum()) == n
    hots = hot_values(case.t, case.nhot)
    hot_bins = [int(b) for b in map_top16(hots, util.TYPES[case.t][3])] if hots else []
    cold = np.ones(65536, dtype=bool)
    if hots:
        want = [0] * case.nhot
        for j, _start, length in runs:
            want[j] += length
        cold[hot_bins] = False
        for j, hb in enumerate(hot_bins):
            assert int(totals[hb]) == want[j], (case.name, j, int(totals[hb]), want[j])  # exact: no background key is hot
            assert wide_cap(es) < want[j] < medium_max(es), (case.name, want[j])         # a bucket for the medium kernel
        if case.nhot <= FEW:
            assert sum(want) <= n // 64, (case.name, sum(want), n // 64)                 # the verdict's crowd bound
    assert int(totals[cold].max()) <= bucket_cape(es, BUCKET_KPT[es], 1024) // 4, case.name  # the background fits the smallest form
    assert int(c[:, cold].max()) < PARK
    if case.parks:
        assert case.nhot <= FEW  # ... so the verdict alone would keep the hybrid
        for hb in hot_bins:
            assert int(c[:, hb].max()) >= PARK, (case.name, hb, int(c[:, hb].max()))  # every hot bucket parks somewhere
    else:
        assert int(c.max()) < PARK, (case.name, int(c.max()))
    if case.exact_in_chunk is not None:
        p0, p1 = geom.chunks[3]
        assert p1 - p0 >= case.exact_in_chunk, (case.name, p1 - p0)
        assert int(c[3, hot_bins[0]]) == case.exact_in_chunk == int(totals[hot_bins[0]]), case.name
    if case.name.endswith("two-regions"):
        per_region = c[:, hot_bins[0]].reshape(geom.num_regions, geom.k).max(axis=1)
        assert int(np.count_nonzero(per_region >= PARK)) == 2, (case.name, per_region)
    return c
