"""GPU: the fused segment key / value kernels (rsx_segment_pairs_kernel<ES, KB, VB, KPT, WG, MEM>) over their whole instance
space and every way work is handed to a workgroup -- what test_gpu_segment_pairs.py, thorough about contents, leaves out:

  width matrix      every (key width, value width) pair in all three size classes (256 threads, 1024 threads, through
                    memory), wide values behind positions included, in both orders
  rows              more rows than workgroups: a workgroup sorts a second and a third row, after a row on which it fell
                    back to every pass, mended ties or found all keys equal
  offsets           so many segments that every workgroup walks blocks of 64 segments alone (team == 1)
  alignment         columns that are naturally aligned and no more
  max_seg_len       a vouched bound that is too small: the long segments' keys and values stay together

Every comparison is on all bytes of an allocation the test owns (segment_pairs_gpu.guarded) against the numpy reference of
tests/segment_pairs_ref.py, which shares no code with the kernels.  Capacities come from rs.segment_pairs_caps and the CU
count from the context: nothing here knows a device's numbers."""
import numpy as np
import pytest

import util
from segment_pairs_gpu import argsort, check_all, expected_info, guarded, joined_elem, key_dtype, same, sort_pairs
from segment_pairs_ref import GUARD, expected_index, segments_reference, segments_reference_fast, with_guards

pytestmark = pytest.mark.gpu

# one key type per width, the kind varying; f64 and u64 so that every 8-byte kind reaches the through-memory class
MATRIX_KEYS = ["u8", "i16", "f32", "i64", "u128", "f64", "u64"]
# 0: keys only; 1 .. 16 ride in the joined element; 3, 12 and 40 behind four-byte positions and a gather
MATRIX_VALUES = [0, 1, 2, 4, 8, 16, 3, 12, 40]


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
def ctx(rs, torch):
    return rs.Context(torch.cuda.current_device())


@pytest.fixture(scope="module")
def num_cu(rs, ctx):
    cu = ctx.get_info(rs._lib.INFO_NUM_CU)
    assert cu >= 1
    return cu


def value_align(vb):
    """include/rsx.h: a value column is aligned to the largest power of two <= 16 that divides the value width."""
    a = 1
    while a < 16 and vb % (2 * a) == 0:
        a *= 2
    return a


def position_values(rng, n, vb):
    """n values of vb random bytes whose first four bytes (or all of them, below four) hold the element's position: two
    neighbours never carry the same value, so a tie that left its input order shows."""
    if not vb:
        return None
    v = rng.integers(0, 256, size=(n, vb), dtype=np.uint8)
    w = min(4, vb)
    v[:, :w] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)[:, :w]
    return v.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# 1. every width pair in every size class
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vb", MATRIX_VALUES)
@pytest.mark.parametrize("tname", MATRIX_KEYS)
def test_width_matrix(rs, torch, ctx, tname, vb):
    """One call per order, max_seg_len unknown, so all three classes launch: segments of 0, 1, 2 and 65 elements and of
    the lengths around both LDS capacities of the joined element, the last one far in the through-memory class, in a
    shuffled order behind a head of 3 and before a tail of 5 elements that no segment covers."""
    kb = util.TYPES[tname][2]
    cap0, cap1 = rs.segment_pairs_caps(kb, vb)
    assert 65 < cap0 - 1 and cap0 + 1 < cap1
    rng = np.random.default_rng(1000 * MATRIX_KEYS.index(tname) + vb)
    lens = rng.permutation(np.array([0, 1, 2, 65, cap0 - 1, cap0, cap0 + 1, cap1, cap1 + 1, cap1 + cap0 + 7], dtype=np.int64))
    offs = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1]) + 5
    # `two`: two distinct keys, nothing but ties; `uniform`: every byte random, floats with their specials
    dist = "two" if (MATRIX_KEYS.index(tname) + MATRIX_VALUES.index(vb)) % 2 else "uniform"
    keys_raw = util.make_input(tname, n, dist, seed=31)
    values_raw = position_values(rng, n, vb)
    for desc in (False, True):
        check_all(rs, torch, ctx, tname, keys_raw, values_raw, vb, offs, desc,
                  index_types=(torch.int32, torch.int64) if vb == 4 else None, what=(tname, vb, dist))
        assert ctx.get_info(rs.INFO_LAST_PAIRS) == expected_info(kb, vb), (tname, vb)
        assert ctx.get_info(rs.INFO_LAST_PASSES) == (6 << 24) | 3


# ---------------------------------------------------------------------------------------------------------------------
# 2. rows: a workgroup's second trip
# ---------------------------------------------------------------------------------------------------------------------
FALLBACK, FULL, MENDED, EQUAL = 0, 1, 2, 3


def row_keys(rng, kinds, row_len, kb):
    """Raw key bytes of len(kinds) rows.  The kinds, as bit patterns of the key:
      FALLBACK  below 2^16: passes that start at a high digit find every neighbour tied and the workgroup falls back
      FULL      every byte random
      MENDED    every byte random, the key at 97 j + 1 a copy of the one at 97 j: a few ties, which are mended
      EQUAL     one key"""
    k = rng.integers(0, 256, size=(len(kinds), row_len, kb), dtype=np.uint8)
    k[kinds == FALLBACK, :, 2:] = 0
    m = np.nonzero(kinds == MENDED)[0]
    copies = len(range(1, row_len, 97))
    k[m[:, None], np.arange(1, row_len, 97)[None, :]] = k[m[:, None], np.arange(0, row_len, 97)[None, :copies]]
    e = kinds == EQUAL
    k[e] = k[e, :1]
    return k.reshape(-1)


def rows_call(rs, torch, c, tname, kmid, other, rows, row_len, vb, desc, ib=0):
    """The row form through the Python entry points; 128-bit keys, which have no dtype, through the context's methods.
    other: the value column (vb bytes each), or the index column (ib bytes each) for argsort."""
    kb, kind = util.TYPES[tname][2:]
    dt = key_dtype(torch, tname)
    if dt is None:
        stream = torch.cuda.current_stream().cuda_stream
        if ib:
            c.argsort_rows_device(kmid.data_ptr(), other.data_ptr(), rows, row_len, kb, kind, ib, desc, stream)
        else:
            c.sort_rows_pairs_device(kmid.data_ptr(), other.data_ptr() if vb else 0, rows, row_len, kb, kind, vb, desc, stream)
        return
    keys = kmid.view(dt).view(rows, row_len)
    if ib:
        out = other.view(torch.int32 if ib == 4 else torch.int64).view(rows, row_len)
        assert rs.radix_argsort_rows(keys, descending=desc, out=out, ctx=c) is out
    elif vb == 8:
        rs.radix_sort_rows_pairs(keys, other.view(torch.int64).view(rows, row_len), descending=desc, ctx=c)
    else:
        rs.radix_sort_rows_pairs(keys, other.view(rows, row_len, vb) if vb else None, descending=desc, ctx=c)


def check_rows(rs, torch, c, num_cu, tname, rows, row_len, vb, seed, per_cu, orders=(False, True)):
    """rows x row_len keys of the four kinds, vb-byte values: both orders of the pairs call and of argsort into int32,
    whole allocations against the reference (the per-segment loop: on rows it is the faster form).  per_cu: workgroups
    of this class that launch_segment_pairs_kv starts per CU (min(LDS that fits, 1024 / WG)); used only to say that the
    INPUT holds every sequence of two kinds in one workgroup: workgroup w sorts the rows w, w + grid, w + 2 grid, and the
    first sixteen workgroups get the sixteen ordered pairs on their first two rows, whatever the generator drew."""
    kb, kind = util.TYPES[tname][2:]
    rng = np.random.default_rng(seed)
    grid = per_cu * num_cu
    assert grid >= 16 and rows > 2 * grid  # (a third trip for the first workgroups)
    kinds = rng.integers(0, 4, size=rows)
    kinds[:16] = np.arange(16) // 4
    kinds[grid:grid + 16] = np.arange(16) % 4
    keys_raw = row_keys(rng, kinds, row_len, kb)
    seen = set(zip(kinds[:-grid].tolist(), kinds[grid:].tolist()))
    assert len(seen) == 16, "some kind of row never follows some other in one workgroup"
    n = rows * row_len
    values_raw = position_values(rng, n, vb)
    offs = np.arange(rows + 1, dtype=np.int64) * row_len
    for desc in orders:
        wk, wv, local = segments_reference(keys_raw, values_raw, kb, kind, vb, desc, offs)
        kbuf, kmid = guarded(torch, keys_raw)
        vbuf, vmid = guarded(torch, values_raw)
        rows_call(rs, torch, c, tname, kmid, vmid, rows, row_len, vb, desc)
        c.check()
        assert c.get_info(rs.INFO_LAST_PAIRS) == expected_info(kb, vb)
        assert c.get_info(rs.INFO_LAST_PASSES) == (6 << 24) | 1
        assert same(kbuf.cpu().numpy(), with_guards(wk), ("row keys", tname, rows, row_len, desc))
        assert same(vbuf.cpu().numpy(), with_guards(wv), ("row values", tname, rows, row_len, desc))
        kbuf, kmid = guarded(torch, keys_raw)
        ibuf, imid = guarded(torch, np.full(n * 4, 0xA5, dtype=np.uint8))
        rows_call(rs, torch, c, tname, kmid, imid, rows, row_len, 0, desc, ib=4)
        c.check()
        assert c.get_info(rs.INFO_LAST_PAIRS) == expected_info(kb, 4)
        assert same(kbuf.cpu().numpy(), with_guards(keys_raw), ("argsort_rows changed the keys", tname, desc))
        assert same(ibuf.cpu().numpy(), with_guards(expected_index(local, 4)), ("row index", tname, rows, row_len, desc))


def test_rows_second_trip_u64(rs, torch, ctx, num_cu):
    """8 CU + 3 rows of 1000 (u64, u32): at most 4 CU workgroups of 256 threads, each sorts two or three rows; with
    16-byte joined elements the skip-and-mend plan runs and what a workgroup learnt on one row it carries to the next."""
    assert 1000 <= rs.segment_pairs_caps(8, 4)[0] and joined_elem(8, 4) >= 8
    check_rows(rs, torch, ctx, num_cu, "u64", 8 * num_cu + 3, 1000, 4, seed=41, per_cu=4)


def test_rows_second_trip_u128(rs, torch, ctx, num_cu):
    """(u128, 16-byte value): 32-byte joined elements, rows of 300."""
    assert 300 <= rs.segment_pairs_caps(16, 16)[0]
    check_rows(rs, torch, ctx, num_cu, "u128", 8 * num_cu + 3, 300, 16, seed=42, per_cu=4)


def test_rows_second_trip_1024_threads(rs, torch, ctx, num_cu):
    """2 CU + 1 rows one element above the first capacity: the 1024-thread class, one workgroup per CU."""
    cap0, cap1 = rs.segment_pairs_caps(8, 4)
    assert cap0 + 1 <= cap1
    check_rows(rs, torch, ctx, num_cu, "u64", 2 * num_cu + 1, cap0 + 1, 4, seed=43, per_cu=1)


@pytest.mark.parametrize("desc", [False, True])
def test_rows_second_trip_through_memory(rs, torch, ctx, num_cu, desc):
    """2 CU + 1 rows one element above the last capacity, (f32, u32): the through-memory class, one workgroup per CU,
    which joins its second row into the workspace where its first row lay.  (One order per case: the reference of nine
    million elements takes two seconds.)"""
    cap1 = rs.segment_pairs_caps(4, 4)[-1]
    check_rows(rs, torch, ctx, num_cu, "f32", 2 * num_cu + 1, cap1 + 1, 4, seed=44, per_cu=1, orders=(desc,))


@pytest.mark.parametrize("tname", ["i16", "u8"])
def test_rows_of_narrow_keys_with_int64_values(rs, torch, ctx, num_cu, tname):
    """12-byte joined elements whose 8-byte value sits at offset 4; judged against the reference, not torch.sort."""
    kb = util.TYPES[tname][2]
    assert joined_elem(kb, 8) == 12 and 1000 <= rs.segment_pairs_caps(kb, 8)[0]
    check_rows(rs, torch, ctx, num_cu, tname, 8 * num_cu + 3, 1000, 8, seed=45 + kb, per_cu=4)


# ---------------------------------------------------------------------------------------------------------------------
# 3. offsets: every workgroup walks its blocks alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname,vb", [("u32", 4), ("u64", 8)])
def test_offsets_with_teams_of_one(rs, torch, ctx, num_cu, tname, vb):
    """64 * 4 CU + 100 segments of 0 .. 40 elements, a dozen of them replaced by one just above each LDS capacity, in
    the first, the last, a middle and six more blocks of 64 segments.

    Why team == 1 (derived from launch_segment_pairs_kv, not observed on the device): a launch has
    full = num_cu * per_cu workgroups with per_cu <= 1024 / WG, so full <= 4 num_cu for the 256-thread class and
    full <= num_cu for the two 1024-thread classes.  The host doubles `team` while nblocks * team < full, and here
    nblocks = ceil(nseg / 64) = 4 num_cu + 2 > full already at team == 1: it never doubles.  Then grid == full < nblocks,
    each workgroup sorts every member of its block and strides on to block + full; the last two blocks (at least) are a
    second trip."""
    kb, kind = util.TYPES[tname][2:]
    cap0, cap1 = rs.segment_pairs_caps(kb, vb)
    nseg = 64 * 4 * num_cu + 100
    nblocks = (nseg + 63) // 64
    assert nblocks > 4 * num_cu
    rng = np.random.default_rng(600 + kb)
    lens = rng.integers(0, 41, size=nseg).astype(np.int64)
    blocks = [0, nblocks - 1, nblocks // 2]
    blocks += [int(b) for b in rng.choice(np.setdiff1d(np.arange(1, nblocks - 1), blocks), size=6, replace=False)]
    for j, b in enumerate(blocks):
        members = np.arange(b * 64, min(b * 64 + 64, nseg))
        if j < 3:  # both long lengths in the first, the last and the middle block
            i0, i1 = rng.choice(members, size=2, replace=False)
            lens[i0], lens[i1] = cap0 + 1, cap1 + 1
        else:
            lens[rng.choice(members)] = cap0 + 1 if j % 2 else cap1 + 1
    assert np.count_nonzero(lens > 40) == 12
    offs = np.concatenate([[2], 2 + np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1]) + 3
    keys_raw = util.make_input(tname, n, "uniform", seed=61)
    keys_raw.reshape(n, kb)[1::5] = keys_raw.reshape(n, kb)[0::5][:len(range(1, n, 5))]  # ties in every segment
    values_raw = position_values(rng, n, vb)
    for desc in (False, True):
        check_all(rs, torch, ctx, tname, keys_raw, values_raw, vb, offs, desc, index_types=(torch.int64,),
                  what=(tname, vb, "teams of one"), reference=segments_reference_fast)
        assert ctx.get_info(rs.INFO_LAST_PASSES) == (6 << 24) | 3


# ---------------------------------------------------------------------------------------------------------------------
# 4. columns that are naturally aligned and no more
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vb", [1, 2, 4, 8, 12, 40])
@pytest.mark.parametrize("tname", ["u8", "i16", "f32", "i64"])
def test_columns_only_naturally_aligned(rs, torch, ctx, tname, vb):
    """The keys start one key behind a 16-byte boundary, the values one alignment unit of theirs, the int32 index four
    bytes: what include/rsx.h promises to accept.  300 ragged segments and one of the through-memory class."""
    kb = util.TYPES[tname][2]
    cap1 = rs.segment_pairs_caps(kb, vb)[-1]
    rng = np.random.default_rng(700 + 50 * kb + vb)
    lens = rng.choice(np.array([0, 1, 2, 63, 64, 65, 1000], dtype=np.int64), size=300)
    lens = np.insert(lens, int(rng.integers(0, 301)), cap1 + 1)
    offs = np.concatenate([[1], 1 + np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1]) + 2
    keys_raw = util.make_input(tname, n, "uniform" if vb in (2, 8, 40) else "two", seed=71)
    values_raw = position_values(rng, n, vb)
    shifts = (kb, value_align(vb), 4)
    for desc in (False, True):
        check_all(rs, torch, ctx, tname, keys_raw, values_raw, vb, offs, desc,
                  index_types=(torch.int32,) if vb == 4 else None, what=(tname, vb, "aligned to", shifts), shifts=shifts)
        assert ctx.get_info(rs.INFO_LAST_PAIRS) == expected_info(kb, vb)


# ---------------------------------------------------------------------------------------------------------------------
# 5. a vouched max_seg_len that is too small
# ---------------------------------------------------------------------------------------------------------------------
def _piece(allocation, b, e, width):
    return allocation[GUARD + b * width:GUARD + e * width]


@pytest.mark.parametrize("tname,vb", [("u32", 4), ("u64", 20)])
def test_segments_above_a_vouched_bound(rs, torch, ctx, tname, vb):
    """max_seg_len = the first capacity, two segments above it.  include/rsx.h: such a segment is "left unsorted or
    sorted, never out of bounds"; with two columns that must hold for both together.  The short segments are sorted, the
    tail and the guards intact, and check() has nothing to report."""
    kb, kind = util.TYPES[tname][2:]
    cap0, cap1 = rs.segment_pairs_caps(kb, vb)
    lens = [10, cap0 + 5, 70, cap1 + 5, 3]
    long_ones = (1, 3)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1]) + 6
    rng = np.random.default_rng(800 + vb)
    keys_raw = util.make_input(tname, n, "uniform", seed=81)
    values_raw = position_values(rng, n, vb)
    for desc in (False, True):
        wk, wv, local = segments_reference(keys_raw, values_raw, kb, kind, vb, desc, offs)
        gk, gv = sort_pairs(rs, torch, ctx, tname, keys_raw, values_raw, vb, offs, desc, max_seg_len=cap0)  # (calls check())
        ek, ev = wk.copy(), wv.copy()
        for i in long_ones:
            b, e = int(offs[i]), int(offs[i + 1])
            assert not np.array_equal(wk[b * kb:e * kb], keys_raw[b * kb:e * kb])  # (the two outcomes differ)
            as_input = np.array_equal(_piece(gk, b, e, kb), keys_raw[b * kb:e * kb]) and np.array_equal(_piece(gv, b, e, vb), values_raw[b * vb:e * vb])
            as_sorted = np.array_equal(_piece(gk, b, e, kb), wk[b * kb:e * kb]) and np.array_equal(_piece(gv, b, e, vb), wv[b * vb:e * vb])
            assert as_input or as_sorted, ("a long segment's keys and values are neither both as they were nor both sorted", i, desc)
            if as_input:
                ek[b * kb:e * kb] = keys_raw[b * kb:e * kb]
                ev[b * vb:e * vb] = values_raw[b * vb:e * vb]
        assert same(gk, with_guards(ek), ("keys", tname, vb, desc))
        assert same(gv, with_guards(ev), ("values", tname, vb, desc))
        for idt, ib in ((torch.int32, 4), (torch.int64, 8)):
            gk, gi = argsort(rs, torch, ctx, tname, keys_raw, offs, desc, idt, max_seg_len=cap0)
            assert same(gk, with_guards(keys_raw), ("argsort changed the keys", tname, desc))
            ei = expected_index(local, ib)
            for i in long_ones:
                b, e = int(offs[i]), int(offs[i + 1])
                if np.all(_piece(gi, b, e, ib) == 0xA5):
                    ei[b * ib:e * ib] = 0xA5
            assert same(gi, with_guards(ei), ("index", tname, desc, idt))
