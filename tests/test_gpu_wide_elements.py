"""GPU: elements and values up to RSX_MAX_ELEM_BYTES = 32768 bytes, and byte offsets past 2^31 and 2^32.

What the other GPU tests leave out: the re-layout kernel with fewer than 16 elements per tile (one element larger than the
nominal tile from 16 KiB on), its unaligned copy branch, the row gather at every word width with rows of thousands of
words, and all of them where element * size crosses 2^32 bytes -- through rsx_sort_device, the pairs calls, the segmented
pairs calls, rsx_sort_columns_device, rsx_sort_host, the bounds calls; and the limit itself at every entry point.

Payloads: util.make_input_layout leaves every deep byte of a wide element zero, so bytes swapped between two elements
far inside would go unseen.  Here every element and value is seeded random bytes over its whole width, the key field
written over them, the row's index in the first 8 bytes outside the key.

References.  Arrays up to 64 MiB: the CPU oracle, byte for byte.  Larger ones stay on the device: the key column alone
is copied back, tests/pairs_ref.py (segment_pairs_ref.py, lex_ref.py) gives the stable permutation, and the expected array
is the input's rows index_select-ed through it on the device.  All comparisons are exact."""
import bisect
import ctypes

import numpy as np
import pytest

import util
from lex_ref import columns_reference
from pairs_ref import pairs_reference
from segment_pairs_gpu import guarded, same
from segment_pairs_ref import segments_reference, with_guards
from test_gpu_host_slice import host_sort
from test_gpu_pairs import Guarded, make_values
from test_gpu_shard_kernels import _clamp, _dev_u64, _host_u64, _pairs, _query_pool, _random_ranges

pytestmark = pytest.mark.gpu

U, S, F = util.UNSIGNED, util.SIGNED, util.FLOAT
MIB = 1 << 20
ORACLE_MAX = 64 * MIB  # bytes up to which the CPU oracle makes the expected array
DISTS = ["uniform", "two", "step16", "equal"]


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
    c = rs.Context(torch.cuda.current_device())
    yield c
    c.close()


@pytest.fixture()
def fresh(rs, torch):
    """A context of its own for the 4 GiB cases; its workspace and the allocator's cache are given back afterwards."""
    c = rs.Context(torch.cuda.current_device())
    torch.cuda.reset_peak_memory_stats()
    yield c
    c.close()
    torch.cuda.empty_cache()


# ---- inputs ----------------------------------------------------------------------------------------------------------
def key_bytes_of(kb, kind, n, dist, seed):
    """(n, kb) uint8 raw keys; float keys drawn "uniform" carry util.make_input's NaN, +-0 and +-inf patterns."""
    if kind == F:
        return util.make_input("f32" if kb == 4 else "f64", n, dist, seed).reshape(n, kb)
    return util._key_ints(dist, n, kb, np.random.default_rng(seed)) if n else np.zeros((0, kb), dtype=np.uint8)


def random_rows(torch, n, w, seed):
    """(n, w) uint8 on the device, seeded random bytes (filled in pieces of at most 512 MiB)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.empty((n, w), dtype=torch.uint8, device="cuda")
    step = max(1, (1 << 29) // w)
    for a in range(0, n, step):
        x[a:a + step].random_(0, 256, generator=g)
    return x


def put_index(torch, x, skip_from, skip_to):
    """The row's index, little-endian, into the first 8 columns of x outside [skip_from, skip_to)."""
    n, w = x.shape
    idx = torch.arange(n, dtype=torch.int64, device="cuda").view(torch.uint8).reshape(n, 8)
    cols = [b for b in range(min(w, skip_to + 8)) if not skip_from <= b < skip_to][:8]
    j = 0
    while j < len(cols):  # runs of neighbouring columns, one strided copy each
        k = j
        while k + 1 < len(cols) and cols[k + 1] == cols[k] + 1:
            k += 1
        x[:, cols[j]:cols[k] + 1] = idx[:, j:k + 1]
        j = k + 1


def wide_elements(torch, lay, n, dist, seed):
    """(n, es) uint8 on the device: random bytes, the key over them, the row's index in the first 8 non-key bytes."""
    es, ko, kb, kind = lay
    x = random_rows(torch, n, es, seed)
    if n:
        x[:, ko:ko + kb] = torch.from_numpy(key_bytes_of(kb, kind, n, dist, seed + 1)).cuda()
        put_index(torch, x, ko, ko + kb)
    return x


def wide_values(torch, n, vb, seed):
    """(n, vb) uint8 on the device: random bytes with the row's index in the first 8 (or vb) of them."""
    v = random_rows(torch, n, vb, seed)
    if n:
        put_index(torch, v, 0, 0)
    return v


def select_rows(torch, src, perm):
    """src[perm] for a 16-byte aligned contiguous (n, w) uint8 tensor, on the device, in the widest words w allows, at most
    2^24 indices per index_select call."""
    n, w = src.shape
    p = perm if isinstance(perm, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int64)).cuda()
    dt = next(t for t, b in ((torch.int64, 8), (torch.int32, 4), (torch.int16, 2), (torch.uint8, 1)) if w % b == 0)
    assert src.data_ptr() % 16 == 0 and src.is_contiguous()
    words = src.view(dt)
    out = torch.empty((p.numel(), words.shape[1]), dtype=dt, device="cuda")
    for a in range(0, p.numel(), 1 << 24):
        torch.index_select(words, 0, p[a:a + (1 << 24)], out=out[a:a + (1 << 24)])
    return out.view(torch.uint8)


def route_of(c, rs):
    return (c.get_info(rs.INFO_LAST_PASSES) >> 28) & 3


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def sort_wide_device(rs, torch, c, orc, lay, n, dist, seed, od=0, ot=0, what=None):
    """rsx_sort_device on a guarded copy of wide_elements(...) that starts `od` bytes behind a 256-byte boundary, with a
    guarded d_tmp `ot` bytes behind one.  Reference: the oracle up to ORACLE_MAX bytes, else the permutation of the keys."""
    es, ko, kb, kind = lay
    src = wide_elements(torch, lay, n, dist, seed)
    gd, gt = Guarded(torch, n * es, shift=od), Guarded(torch, n * es, shift=ot)
    gd.bytes().copy_(src.reshape(-1))
    c.sort_device(gd.buf.data_ptr() + gd.lo, gt.buf.data_ptr() + gt.lo, n, rs.RadixDigits(*lay), stream_of(torch))
    c.check()
    assert gd.intact() and gt.intact(), ("guards", what)
    got = gd.bytes().view(n, es)
    if n * es <= ORACLE_MAX:
        want = orc.sort_parallel(src.cpu().numpy().reshape(-1), orc.Layout(*lay), 4)
        assert np.array_equal(got.cpu().numpy().reshape(-1), want), what
    else:
        keys_raw = src[:, ko:ko + kb].contiguous().cpu().numpy()
        perm = pairs_reference(keys_raw, None, kb, kind, 0, False)[2]
        assert torch.equal(got, select_rows(torch, src, perm)), what
    if n > 1:
        assert route_of(c, rs) == 2, what


# ---- 1. rsx_sort_device, route 2, wide elements, small arrays ------------------------------------------------------------
WIDE_SIZES = [1040, 2048, 16384, 20000, 32768,  # the gather moves 16-byte words (8-byte ones at a pointer offset of 8)
              32764,  # dwords
              16386,  # 2-byte words
              1025, 4097, 16385, 32767]  # bytes
KEY_FORMS = [(kb, kind) for kb in (1, 3, 4, 8, 16) for kind in (U, S)] + [(4, F), (8, F)]
OFFSETS = [(od, ot) for od in (0, 1, 3, 8) for ot in (0, 1, 3, 8)]


def layouts_of(es):
    """Three layouts per size: the key at offset 0, at es - kb, and at an odd offset in the middle: es // 2 - 1, or one more
    where that is even (16386, 32767).  Whether a key there straddles a 16-byte chunk depends on the size: the 3-byte key
    at 519 of 1040 does not, the 16-byte keys and the keys at 8191 and 16383 do.  The key forms rotate over the sizes."""
    si = WIDE_SIZES.index(es)
    out = []
    for j in range(3):
        kb, kind = KEY_FORMS[(3 * si + j + si // 4) % len(KEY_FORMS)]
        out.append((es, (0, es - kb, (es // 2 - 1) | 1)[j], kb, kind))
    return out


def test_every_key_form_occurs():
    forms = {(kb, kind) for es in WIDE_SIZES for (_es, _ko, kb, kind) in layouts_of(es)}
    assert forms == set(KEY_FORMS)
    assert all(ko + kb <= es and ko >= 0 for es in WIDE_SIZES for (es, ko, kb, _k) in layouts_of(es))


@pytest.mark.parametrize("es", WIDE_SIZES)
def test_sort_device_wide_elements(rs, torch, ctx, orc, es):
    cu = ctx.get_info(rs._lib.INFO_NUM_CU)
    tile = max(1, min(4096, 16384 // es))
    sizes = [0, 1, 2, 3, tile, tile + 1, 2 * tile + 1, 257]
    if es <= 4097:  # the grid-stride loops: the move kernel has 8 blocks per CU, the gather 16 blocks of 16 rows per CU
        sizes += [8 * cu * tile + 5, 16 * cu * 16 + 7]
    case = WIDE_SIZES.index(es) * 5  # every size starts the rotation of the pointer offsets elsewhere
    seen = set()
    for lay in layouts_of(es):
        for n in sizes:
            dist = DISTS[(case // 3) % len(DISTS)]
            # both arrays aligned (the gather's widest words), then one of the 15 other pairings of 0, 1, 3, 8 in turn
            for od, ot in ((0, 0), OFFSETS[1 + case % (len(OFFSETS) - 1)]):
                seen.add((od, ot))
                sort_wide_device(rs, torch, ctx, orc, lay, n, dist, seed=es * 100 + case, od=od, ot=ot, what=(lay, n, dist, od, ot))
            case += 1
    assert seen == set(OFFSETS)  # d_data at 0, 1, 3, 8 and d_tmp at 0, 1, 3, 8, every pairing


# ---- 2. past 2^31 and 2^32 bytes with few elements ------------------------------------------------------------------------
N32K = 131075  # x 32768 bytes = 2^32 + 98304: the last three rows lie past 2^32
N20K = 214749  # x 20000 bytes = 2^32 + 12704: 2^31 and 2^32 fall inside an element


MEMORY_BUDGET = 32 << 30  # bytes of tensors one 4 GiB case may hold at its peak (measured: 20 GiB at the most)


class timed:
    """The body of a 4 GiB case: its tensors stay below MEMORY_BUDGET at their peak, counted from what was allocated when
    the case began (the library's own workspace, at most two 4 GiB arrays and a copy, is not torch's and comes on top)."""

    def __init__(self, torch, name):
        self.torch, self.name = torch, name

    def __enter__(self):
        self.torch.cuda.synchronize()
        self.torch.cuda.reset_peak_memory_stats()
        self.base = self.torch.cuda.memory_allocated()

    def __exit__(self, kind, value, trace):
        self.torch.cuda.synchronize()
        peak = self.torch.cuda.max_memory_allocated() - self.base
        if kind is None:
            assert peak < MEMORY_BUDGET, (self.name, f"{peak / (1 << 30):.1f} GiB of tensors at the peak")


@pytest.mark.parametrize("lay,n,od,ot,dist", [((32768, 0, 8, U), N32K, 0, 0, "uniform"), ((20000, 19992, 8, S), N20K, 4, 12, "step16"),
                                              ((20000, 19992, 8, S), N20K, 4, 14, "two")],
                         ids=["32768x131075", "20000x214749", "20000x214749-unaligned-copy"])
def test_sort_device_past_2pow32_bytes(rs, torch, fresh, orc, lay, n, od, ot, dist):
    """Route 2 with the proxies' positions times the element size beyond 32 bits.  The second case puts d_data 4 and d_tmp
    12 bytes behind a 16-byte boundary: the gather moves dwords; the two differ by 8, so the copy into d_tmp still takes
    its dword branch.  The third puts d_tmp 14 bytes behind: the copy assembles every dword from bytes, past 2^31 and 2^32
    bytes too, and the gather moves 2-byte words (a swap of two bytes in that branch passed the first two cases)."""
    assert ((256 + ot) - (256 + od)) % 4 == (2 if ot == 14 else 0)
    assert n * lay[0] > (1 << 32) >= (n - 3) * lay[0]
    with timed(torch, f"sort_device {lay} n={n}"):
        sort_wide_device(rs, torch, fresh, orc, lay, n, dist, seed=n, od=od, ot=ot, what=(lay, n))


def _pairs_past_2pow32(rs, torch, c, tname, vb, n, desc, vshift, dist):
    _es, _ko, kb, kind = util.TYPES[tname]
    keys_in = util.make_input(tname, n, dist, seed=vb)
    vin = wide_values(torch, n, vb, seed=vb + n)
    gk, gv = Guarded(torch, n * kb), Guarded(torch, n * vb, shift=vshift)
    gk.bytes().copy_(torch.from_numpy(keys_in))
    gv.bytes().copy_(vin.reshape(-1))
    c.sort_pairs_device(gk.buf.data_ptr() + gk.lo, gv.buf.data_ptr() + gv.lo, n, kb, kind, vb, desc, stream_of(torch))
    c.check()
    assert gk.intact() and gv.intact()
    assert c.get_info(rs.INFO_LAST_PAIRS) & 0xFF == 2
    want_keys, _v, perm = pairs_reference(keys_in, None, kb, kind, 0, desc)
    assert np.array_equal(gk.bytes().cpu().numpy(), want_keys)
    assert torch.equal(gv.bytes().view(n, vb), select_rows(torch, vin, perm))


def test_pairs_u32_values_of_32768_bytes_past_2pow32(rs, torch, fresh):
    with timed(torch, "sort_pairs u32, 32768-byte values, descending"):
        _pairs_past_2pow32(rs, torch, fresh, "u32", 32768, N32K, True, 0, "step16")


def test_pairs_i64_values_of_20000_bytes_past_2pow32(rs, torch, fresh):
    """The value array starts one alignment unit (16 bytes) behind a 256-byte boundary."""
    with timed(torch, "sort_pairs i64, 20000-byte values, ascending"):
        _pairs_past_2pow32(rs, torch, fresh, "i64", 20000, N20K, False, 16, "uniform")


def test_pairs_u128_joined_array_past_2pow32(rs, torch, fresh):
    """Route 1: 2^27 + 7 joined elements of 32 bytes, 4 GiB + 224 bytes.  Checked as
    test_gpu_pairs.py::test_large_u32_pairs_checked_on_the_device: the keys a permutation in order by the verifier, and
    with p the row index in bytes 0..3 of each value, keys_in[p] == keys_out and values_in[p] == values_out."""
    c = fresh
    n = (1 << 27) + 7
    d = rs.PRIMITIVES["u128"]
    with timed(torch, "sort_pairs u128 keys, 16-byte values, joined"):
        keys_in = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
        c.generate_device(keys_in.data_ptr(), n, d, rs.GEN_UNIFORM, 2025)
        ver = torch.zeros(3, dtype=torch.int64, device="cuda")
        c.verify_device(keys_in.data_ptr(), n, d, ver.data_ptr())
        c.check()
        sum_in = int(ver[1])
        vals_in = make_values(torch, n, 16)
        keys, vals = keys_in.clone(), vals_in.clone()
        rs.radix_sort_pairs(keys, vals, ctx=c)
        c.check()
        assert c.get_info(rs.INFO_LAST_PAIRS) == (1 | 32 << 8)
        c.verify_device(keys.data_ptr(), n, d, ver.data_ptr())
        c.check()
        assert int(ver[0]) == 0 and int(ver[1]) == sum_in, (int(ver[0]), "descents; checksum", int(ver[1]), sum_in)
        p = vals.view(torch.int32)[:, 0].to(torch.int64)
        assert int(p.min()) >= 0 and int(p.max()) < n
        assert torch.equal(select_rows(torch, keys_in, p), keys), "keys_in[p] != keys_out"
        assert torch.equal(select_rows(torch, vals_in, p), vals), "values_in[p] != values_out"
        del keys, vals, keys_in, vals_in, p


def test_segments_pairs_values_of_32768_bytes_past_2pow32(rs, torch, fresh):
    """Route 4: f32 keys, about 1000 segments of seeded random lengths, a few rows uncovered in front and behind."""
    c = fresh
    n, vb = N32K, 32768
    rng = np.random.default_rng(7)
    cuts = np.sort(rng.choice(np.arange(6, n - 8), size=999, replace=False))
    offs = np.concatenate([[5], cuts, [n - 7]]).astype(np.int64)
    keys_in = util.make_input("f32", n, "uniform", seed=8)
    with timed(torch, "sort_segments_pairs f32, 32768-byte values"):
        vin = wide_values(torch, n, vb, seed=9)
        gk, gv = Guarded(torch, n * 4), Guarded(torch, n * vb)
        gk.bytes().copy_(torch.from_numpy(keys_in))
        gv.bytes().copy_(vin.reshape(-1))
        o = torch.from_numpy(offs).cuda()
        rs.radix_sort_segments_pairs(gk.bytes().view(torch.float32), gv.bytes().view(n, vb), o, ctx=c)
        c.check()
        assert gk.intact() and gv.intact()
        assert c.get_info(rs.INFO_LAST_PAIRS) & 0xFF == 4
        want_keys, _v, local = segments_reference(keys_in, None, 4, F, 0, False, offs)
        pos = np.arange(n, dtype=np.int64)
        start = offs[np.searchsorted(offs, pos, side="right") - 1]
        perm = np.where(local >= 0, start + local, pos)  # uncovered rows stay where they are
        assert (perm[:5] == pos[:5]).all() and (perm[n - 7:] == pos[n - 7:]).all() and (local[5:n - 7] >= 0).all()
        assert np.array_equal(gk.bytes().cpu().numpy(), want_keys)
        assert torch.equal(gv.bytes().view(n, vb), select_rows(torch, vin, perm))


def test_sort_columns_values_of_32768_bytes_past_2pow32(rs, torch, fresh):
    c = fresh
    n, vb = N32K, 32768
    rng = np.random.default_rng(10)
    a = rng.integers(0, 50, size=n, dtype=np.uint32) * np.uint32(0x05050505)  # few values: the second column decides
    b = rng.integers(-300, 300, size=n, dtype=np.int16)
    with timed(torch, "sort_columns (u32, i16 descending), 32768-byte values"):
        vin = wide_values(torch, n, vb, seed=11)
        ga, gb, gv = Guarded(torch, n * 4), Guarded(torch, n * 2), Guarded(torch, n * vb)
        ga.bytes().copy_(torch.from_numpy(a.view(np.uint8)))
        gb.bytes().copy_(torch.from_numpy(b.view(np.uint8)))
        gv.bytes().copy_(vin.reshape(-1))
        rs.radix_sort_columns([ga.bytes().view(torch.uint32), gb.bytes().view(torch.int16)], values=gv.bytes().view(n, vb),
                              descending=[False, True], ctx=c)
        c.check()
        assert ga.intact() and gb.intact() and gv.intact()
        wcols, _wv, perm = columns_reference([a, b], [(4, U), (2, S)], [False, True])
        assert np.array_equal(ga.bytes().cpu().numpy(), wcols[0]) and np.array_equal(gb.bytes().cpu().numpy(), wcols[1])
        assert torch.equal(gv.bytes().view(n, vb), select_rows(torch, vin, perm))


def test_bounds_and_splitter_past_2pow32_bytes(rs, torch, fresh):
    """Zeros on the device with a sorted key column at byte 100 of every 32768-byte element; the queries, ranges and bisect
    reference of test_gpu_shard_kernels.py::test_bounds_and_splitter_take_any_element_size, and queries that land in the
    last three elements (past 2^32 bytes)."""
    c = fresh
    lay = (32768, 100, 8, U)
    n, kb = N32K, 8
    d = rs.RadixDigits(*lay)
    rng = np.random.default_rng(15)
    kcol = np.sort(rng.integers(0, 1 << 62, size=n, dtype=np.uint64) // np.uint64(3) * np.uint64(3))
    kcol[n - 3:] = kcol[n - 4] + np.array([3, 6, 9], dtype=np.uint64)  # three distinct keys at the very end
    keys = [int(k) for k in kcol]
    with timed(torch, "bounds, bounds_ranges, splitter_count on 32768-byte elements"):
        x = torch.zeros((n, 32768), dtype=torch.uint8, device="cuda")
        x[:, 100:108] = torch.from_numpy(kcol.view(np.uint8).reshape(n, 8)).cuda()
        tail = [keys[n - 3], keys[n - 2], keys[n - 1], keys[n - 2] - 1, keys[n - 1] + 1, keys[n - 3] - 1]
        qs = (tail + _query_pool(keys, kb, rng, 100))[:300]
        nq = len(qs)
        ranges = [(n - 3, n), (n - 2, n + 5), (0, n)] + _random_ranges(keys, n, nq - 3, rng)
        dq, dr = _dev_u64(torch, _pairs(qs)), _dev_u64(torch, [v for r in ranges for v in r])
        out = torch.full((2 * nq,), -1, dtype=torch.int64, device="cuda")
        c.bounds_device(x.data_ptr(), n, d, dq.data_ptr(), nq, out.data_ptr())
        got = _host_u64(out)
        assert got == [bisect.bisect_left(keys, q) for q in qs] + [bisect.bisect_right(keys, q) for q in qs]
        assert got[0] == n - 3 and got[nq + 2] == n
        c.bounds_ranges_device(x.data_ptr(), n, d, dq.data_ptr(), dr.data_ptr(), nq, out.data_ptr())
        got = _host_u64(out)
        for qi, ((b, e), q) in enumerate(zip(ranges, qs)):
            b2, e2 = _clamp(b, e, n)
            assert (got[qi], got[nq + qi]) == (bisect.bisect_left(keys, q, b2, e2) - b2, bisect.bisect_right(keys, q, b2, e2) - b2), qi
        nb = 20
        less = torch.full((nb * 256,), -1, dtype=torch.int64, device="cuda")
        for digit in range(kb - 1, -1, -1):
            low = (1 << (8 * (digit + 1))) - 1
            prefixes = [keys[n - 1] & ~low, keys[n - 3] & ~low] + [keys[int(i)] & ~low for i in rng.integers(0, n, size=nb - 2)]
            dp = _dev_u64(torch, _pairs(prefixes))
            c.splitter_count_device(x.data_ptr(), n, d, dr.data_ptr(), dp.data_ptr(), nb, digit, less.data_ptr())
            got = _host_u64(less)
            for b, ((beg, end), p) in enumerate(zip(ranges[:nb], prefixes)):
                b2, e2 = _clamp(beg, end, n)
                assert got[b * 256:(b + 1) * 256] == [bisect.bisect_left(keys, p | (j << (8 * digit)), b2, e2) - b2 for j in range(256)], (digit, b)
        c.check()
        del x


# ---- 3. wide values, small arrays ----------------------------------------------------------------------------------------
VALUE_WIDTHS = [1024, 16400, 32768,  # aligned to 16
                1028,  # 4
                4098, 32766,  # 2
                4097]  # 1
WIDE_KEY_TYPES = ["u8", "f32", "i64"]


def value_align(vb):
    return next(a for a in (16, 8, 4, 2, 1) if vb % a == 0)


def pairs_dist(tname, i):
    return "uniform" if tname == "f32" else DISTS[i % len(DISTS)]  # f32 uniform: NaN of both signs, +-0, +-inf


@pytest.mark.parametrize("vb", VALUE_WIDTHS)
def test_pairs_wide_values(rs, torch, ctx, vb):
    sizes = [0, 1, 2, 255] + ([65543] if vb <= 1028 else [])  # 65543 rows: the gather's second sweep over its grid
    i = 0
    for tname in WIDE_KEY_TYPES + ["u128"]:
        _es, _ko, kb, kind = util.TYPES[tname]
        for n in sizes:
            keys_in = util.make_input(tname, n, pairs_dist(tname, i), seed=vb + i)
            vin = wide_values(torch, n, vb, seed=3 * vb + i)
            i += 1
            for desc in (False, True):
                want_keys, _v, perm = pairs_reference(keys_in, None, kb, kind, 0, desc)
                want_vals = select_rows(torch, vin, perm)
                for shift in (0, 1):  # 1: both arrays one key / one alignment unit of the value behind a 256-byte boundary
                    what = (tname, vb, n, desc, shift)
                    gk, gv = Guarded(torch, n * kb, shift=shift * kb), Guarded(torch, n * vb, shift=shift * value_align(vb))
                    gk.bytes().copy_(torch.from_numpy(keys_in))
                    gv.bytes().copy_(vin.reshape(-1))
                    ctx.sort_pairs_device(gk.buf.data_ptr() + gk.lo, gv.buf.data_ptr() + gv.lo, n, kb, kind, vb, desc, stream_of(torch))
                    ctx.check()
                    assert gk.intact() and gv.intact(), ("guards", what)
                    assert np.array_equal(gk.bytes().cpu().numpy(), want_keys), ("keys", what)
                    assert torch.equal(gv.bytes().view(n, vb), want_vals), ("values", what)
                    if n > 1:
                        assert ctx.get_info(rs.INFO_LAST_PAIRS) & 0xFF == 2, what


SEG_N = 7 * 300
# a segment of length 0, one of length 1, a good one, a decreasing pair (2050 > 3: left untouched, error word set), two good ones
SEG_OFFSETS = [1200, 1200, 1201, 2050, 3, 700, 1100]


@pytest.mark.parametrize("tname", WIDE_KEY_TYPES)
@pytest.mark.parametrize("vb", [1028, 4097, 32768])
def test_segments_and_rows_pairs_wide_values(rs, torch, vb, tname):
    c = rs.Context(torch.cuda.current_device())
    _es, _ko, kb, kind = util.TYPES[tname]
    n = SEG_N
    keys_in = util.make_input(tname, n, pairs_dist(tname, vb), seed=vb)
    vin_dev = wide_values(torch, n, vb, seed=vb + 1)
    vin = vin_dev.cpu().numpy().reshape(-1)
    good = [0, 0, 1, 1, 500, n - 1, n - 1]
    kt = {"u8": torch.uint8, "f32": torch.float32, "i64": torch.int64}[tname]
    for desc in (False, True):
        for offs, bad in ((SEG_OFFSETS, True), (good, False)):
            wk, wv, _local = segments_reference(keys_in, vin, kb, kind, vb, desc, offs)
            kbuf, kmid = guarded(torch, keys_in)
            vbuf, vmid = guarded(torch, vin)
            o = torch.tensor(offs, dtype=torch.int64, device="cuda")
            rs.radix_sort_segments_pairs(kmid.view(kt), vmid.view(n, vb), o, descending=desc, ctx=c)
            if bad:
                with pytest.raises(rs.RsxError) as e:
                    c.check()
                assert e.value.status == rs._lib.ERR_INTERNAL
            c.check()
            assert c.get_info(rs.INFO_LAST_PAIRS) & 0xFF == 4
            assert same(kbuf.cpu().numpy(), with_guards(wk), ("segment keys", tname, vb, desc, bad))
            assert same(vbuf.cpu().numpy(), with_guards(wv), ("segment values", tname, vb, desc, bad))
        rows = [300 * r for r in range(8)]
        wk, wv, _local = segments_reference(keys_in, vin, kb, kind, vb, desc, rows)
        kbuf, kmid = guarded(torch, keys_in)
        vbuf, vmid = guarded(torch, vin)
        rs.radix_sort_rows_pairs(kmid.view(kt).view(7, 300), vmid.view(7, 300, vb), descending=desc, ctx=c)
        c.check()
        assert c.get_info(rs.INFO_LAST_PAIRS) & 0xFF == 4
        assert same(kbuf.cpu().numpy(), with_guards(wk), ("row keys", tname, vb, desc))
        assert same(vbuf.cpu().numpy(), with_guards(wv), ("row values", tname, vb, desc))
    c.close()


@pytest.mark.parametrize("vb", [4097, 32768])
def test_sort_columns_wide_values(rs, torch, ctx, vb):
    """Two rounds (i64, i64, i32); every column from a few values, so that the later columns and the input order decide."""
    names, specs = ["i64", "i64", "i32"], [(8, S), (8, S), (4, S)]
    dts = [torch.int64, torch.int64, torch.int32]
    for n in (2, 255, 1031):
        rng = np.random.default_rng(n + vb)
        cols = [rng.integers(-2, 2, size=n).astype(np.int64) * (1 << 40), rng.integers(-2, 2, size=n).astype(np.int64),
                rng.integers(-3, 3, size=n).astype(np.int32)]
        vin = wide_values(torch, n, vb, seed=n + vb).cpu().numpy().reshape(-1)
        for desc in ([False, False, False], [True, False, True]):
            wcols, wv, _perm = columns_reference(cols, specs, desc, vin, vb)
            bufs = [guarded(torch, col) for col in cols]
            vbuf, vmid = guarded(torch, vin)
            rs.radix_sort_columns([mid.view(dt) for (_b, mid), dt in zip(bufs, dts)], values=vmid.view(n, vb), descending=desc, ctx=ctx)
            ctx.check()
            for j in range(3):
                assert same(bufs[j][0].cpu().numpy(), with_guards(wcols[j]), ("column", j, names[j], n, vb, desc))
            assert same(vbuf.cpu().numpy(), with_guards(wv), ("values", n, vb, desc))
            assert ctx.get_info(rs.INFO_LAST_LEX) & 0xFF == 2


# ---- 4. the host slice -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [4096, 65536, None], ids=["4096", "65536", "default"])
@pytest.mark.parametrize("lay,n", [((32768, 0, 8, U), 300), ((16385, 7, 3, S), 1000)], ids=["32768x300", "16385x1000"])
def test_host_slice_wide_elements(rs, torch, orc, lay, n, chunk):
    """At 4096-byte pieces one 32768-byte element spans eight pieces of the copy pipeline."""
    c = rs.Context(torch.cuda.current_device())
    if chunk is not None:
        c.set_option(rs.OPT_HOST_CHUNK, chunk)
    for dist in ("uniform", "two"):
        raw = wide_elements(torch, lay, n, dist, seed=n).cpu().numpy().reshape(-1)
        want = orc.sort_parallel(raw, orc.Layout(*lay), 4)
        got = host_sort(rs, c, raw, lay, guard=max(4096, 5 * (chunk or 0)))
        assert np.array_equal(got, want), (lay, n, chunk, dist)
        assert route_of(c, rs) == 2
    c.close()


# ---- 6. the limit itself ---------------------------------------------------------------------------------------------------
LIMIT = 32768


class Filled:
    """Device and host buffers that a refused call must leave as they were.  No two hold the same bytes and none is
    constant, and element arrays and key columns hold descending keys: a sort, a copy between two of them, a generator
    or a memset that did get enqueued changes bytes."""

    def __init__(self, torch):
        self.torch, self.kept, self.made = torch, [], 0

    def _pattern(self, nbytes):
        self.made += 1
        return ((np.arange(nbytes, dtype=np.int64) * (2 * self.made + 1) + 40 * self.made) % 251).astype(np.uint8)

    def _keep(self, a, device):
        t = self.torch.from_numpy(a).cuda() if device else a
        self.kept.append((t, t.clone() if device else a.copy()))
        return t

    def device(self, nbytes):
        return self._keep(self._pattern(nbytes), True)

    def elements(self, rows, width, key_offset, device=True):
        """rows x width pattern bytes with 8-byte unsigned keys rows, rows - 1, ... 1 at key_offset."""
        a = self._pattern(rows * width).reshape(rows, width)
        a[:, key_offset:key_offset + 8] = np.arange(rows, 0, -1, dtype="<u8").view(np.uint8).reshape(rows, 8)
        return self._keep(a.reshape(-1), device)

    def words(self, values, dtype):
        return self._keep(np.array(values, dtype=dtype).view(np.uint8), True)

    def untouched(self):
        self.torch.cuda.synchronize()
        return all(self.torch.equal(t, k) if isinstance(t, self.torch.Tensor) else np.array_equal(t, k) for t, k in self.kept)


def refused(rs, c, status, want, word):
    msg = c._L.rsx_last_error(c._h).decode()
    assert status == want, (status, msg)
    assert word in msg, msg
    return True


def test_limit_of_the_layout_calls(rs, torch, orc):
    """rsx_sort_device, rsx_sort_host, rsx_ctx_reserve, rsx_generate_device, rsx_verify_device: 32768-byte elements are
    taken (n = 3, result checked), 32769-byte ones are RSX_ERR_UNSUPPORTED, nothing enqueued, the reason named."""
    c = rs.Context(torch.cuda.current_device())
    L, h, st = c._L, c._h, stream_of(torch)
    lay = (LIMIT, 5, 8, U)
    d = rs.RadixDigits(*lay)
    c.reserve(3, d)
    src = wide_elements(torch, lay, 3, "uniform", seed=1)
    raw = src.cpu().numpy().reshape(-1)
    want = orc.sort_parallel(raw, orc.Layout(*lay), 1)
    x, tmp = src.clone(), torch.empty_like(src)
    c.sort_device(x.data_ptr(), tmp.data_ptr(), 3, d, st)
    c.check()
    assert np.array_equal(x.cpu().numpy().reshape(-1), want)
    assert np.array_equal(host_sort(rs, c, raw, lay), want)
    g = torch.empty(3 * LIMIT, dtype=torch.uint8, device="cuda")
    c.generate_device(g.data_ptr(), 3, d, rs.GEN_REVERSED, 1, 0.0, 7)
    assert np.array_equal(g.cpu().numpy(), orc.generate(3, orc.Layout(*lay), orc.GEN_REVERSED, 1, 0.0, 7))
    out = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    c.verify_device(x.data_ptr(), 3, d, out.data_ptr())
    c.check()
    assert tuple(int(v) for v in out.cpu().numpy().astype(np.uint64)) == util.verify_reference(want, lay, orc)

    over = rs._lib.Layout(LIMIT + 1, 5, 8, U)
    UNS = rs._lib.ERR_UNSUPPORTED
    f = Filled(torch)
    a, b, o3 = f.elements(3, LIMIT + 1, 5), f.device(3 * (LIMIT + 1)), f.device(24)
    ha = f.elements(3, LIMIT + 1, 5, device=False)
    assert refused(rs, c, L.rsx_sort_device(h, a.data_ptr(), b.data_ptr(), 3, ctypes.byref(over), st), UNS, "RSX_MAX_ELEM_BYTES")
    assert refused(rs, c, L.rsx_sort_host(h, ha.ctypes.data, 3, ctypes.byref(over)), UNS, "RSX_MAX_ELEM_BYTES")
    assert refused(rs, c, L.rsx_ctx_reserve(h, 3, ctypes.byref(over)), UNS, "RSX_MAX_ELEM_BYTES")
    assert refused(rs, c, L.rsx_generate_device(h, a.data_ptr(), 3, ctypes.byref(over), 0, 1, 0.0, 0, st), UNS, "RSX_MAX_ELEM_BYTES")
    assert refused(rs, c, L.rsx_verify_device(h, a.data_ptr(), 3, ctypes.byref(over), o3.data_ptr(), st), UNS, "RSX_MAX_ELEM_BYTES")
    assert L.rsx_sort_device(h, a.data_ptr(), b.data_ptr(), 0, ctypes.byref(over), st) == UNS  # whatever n
    c.check()
    assert f.untouched()
    # the wrapper: an (n, 32769) byte tensor with digits= raises and stays as it was
    t = f.elements(4, LIMIT + 1, 0).view(4, LIMIT + 1)
    with pytest.raises(rs.RsxError) as e:
        rs.radix_sort(t, digits=rs.RadixDigits(LIMIT + 1, 0, 8, U), ctx=c)
    assert e.value.status == UNS
    ht = f.elements(4, LIMIT + 1, 0, device=False).reshape(4, LIMIT + 1)
    with pytest.raises(rs.RsxError) as e:
        rs.radix_sort(ht, digits=rs.RadixDigits(LIMIT + 1, 0, 8, U), ctx=c)
    assert e.value.status == UNS
    assert f.untouched()
    c.close()


def test_limit_of_the_value_calls(rs, torch):
    """rsx_sort_pairs_device, rsx_ctx_reserve_pairs, rsx_sort_segments_pairs_device, rsx_sort_rows_pairs_device,
    rsx_sort_columns_device, rsx_ctx_reserve_lex: values of 32768 bytes are taken (n = 3, result checked), 32769 is
    RSX_ERR_ARG, nothing enqueued, the reason named; the Python wrappers raise before any call."""
    c = rs.Context(torch.cuda.current_device())
    L, h, st = c._L, c._h, stream_of(torch)
    keys_in = np.array([7, -2, 7], dtype=np.int32)
    vin = wide_values(torch, 3, LIMIT, seed=2)
    perm = torch.tensor([1, 0, 2], device="cuda")
    col = (rs._lib.KeyColumn * 1)()

    def fresh_pair():
        return torch.from_numpy(keys_in.copy()).cuda(), vin.clone()

    c.reserve_pairs(3, 4, LIMIT)
    k, v = fresh_pair()
    c.sort_pairs_device(k.data_ptr(), v.data_ptr(), 3, 4, S, LIMIT, False, st)
    c.check()
    assert k.tolist() == [-2, 7, 7] and torch.equal(v, vin[perm])
    k, v = fresh_pair()
    o = torch.tensor([0, 3], dtype=torch.int64, device="cuda")
    c.sort_segments_pairs_device(k.data_ptr(), v.data_ptr(), 3, 4, S, LIMIT, o.data_ptr(), 1, False, 0, st)
    c.check()
    assert k.tolist() == [-2, 7, 7] and torch.equal(v, vin[perm])
    k, v = fresh_pair()
    c.sort_rows_pairs_device(k.data_ptr(), v.data_ptr(), 1, 3, 4, S, LIMIT, False, st)
    c.check()
    assert k.tolist() == [-2, 7, 7] and torch.equal(v, vin[perm])
    k, v = fresh_pair()
    c.reserve_lex(3, [(0, 4, S, False)], LIMIT)
    c.sort_columns_device([(k.data_ptr(), 4, S, False)], v.data_ptr(), LIMIT, 3, st)
    c.check()
    assert k.tolist() == [-2, 7, 7] and torch.equal(v, vin[perm])

    ARG = rs._lib.ERR_ARG
    f = Filled(torch)
    kk, vv, oo = f.words([9, 5, -1], "<i4"), f.device(3 * (LIMIT + 1)), f.words([0, 3], "<i8")  # descending keys, one segment
    col[0] = rs._lib.KeyColumn(kk.data_ptr(), 4, S, 0, 0)
    p, q = kk.data_ptr(), vv.data_ptr()
    assert refused(rs, c, L.rsx_sort_pairs_device(h, p, q, 3, 4, S, LIMIT + 1, 0, st), ARG, "RSX_MAX_ELEM_BYTES")
    assert refused(rs, c, L.rsx_ctx_reserve_pairs(h, 3, 4, LIMIT + 1), ARG, "width")
    assert refused(rs, c, L.rsx_sort_segments_pairs_device(h, p, q, 3, 4, S, LIMIT + 1, 0, oo.data_ptr(), 1, 0, st), ARG, "RSX_MAX_ELEM_BYTES")
    assert refused(rs, c, L.rsx_sort_rows_pairs_device(h, p, q, 1, 3, 4, S, LIMIT + 1, 0, st), ARG, "RSX_MAX_ELEM_BYTES")
    assert refused(rs, c, L.rsx_sort_columns_device(h, col, 1, q, LIMIT + 1, 3, st), ARG, "RSX_MAX_ELEM_BYTES")
    assert refused(rs, c, L.rsx_ctx_reserve_lex(h, 3, col, 1, LIMIT + 1), ARG, "RSX_MAX_ELEM_BYTES")
    c.check()
    assert f.untouched()
    # the wrappers
    keys = f.words([9, 5, -1], "<i4").view(torch.int32)
    vals = f.device(3 * (LIMIT + 1)).view(3, LIMIT + 1)
    offs = torch.tensor([0, 3], dtype=torch.int64, device="cuda")
    before = c.get_info(rs.INFO_LAST_PAIRS), c.get_info(rs.INFO_LAST_LEX)
    for call in (lambda: rs.radix_sort_pairs(keys, vals, ctx=c),
                 lambda: rs.radix_sort_columns([keys], values=vals, ctx=c),
                 lambda: rs.radix_sort_segments_pairs(keys, vals, offs, ctx=c),
                 lambda: rs.radix_sort_rows_pairs(keys.view(1, 3), vals.view(1, 3, LIMIT + 1), ctx=c)):
        with pytest.raises(ValueError):
            call()
    assert (c.get_info(rs.INFO_LAST_PAIRS), c.get_info(rs.INFO_LAST_LEX)) == before
    assert f.untouched() and offs.tolist() == [0, 3]
    c.close()
