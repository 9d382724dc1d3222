"""GPU: rsx_bin_count_device / radix_histogram / radix_bincount against tests/bin_ref.py.

Every comparison is np.array_equal on all bytes of an allocation the test owns: 64 guard bytes of 0xA5, the counts, 64
guard bytes; the counts are pre-filled with 0xA5 too unless a test accumulates, so a count that is not written shows.  The
key and edge columns are compared with their inputs afterwards, and ctx.check() runs after each call.  Sizes come from
bin_caps: S = share, E = max_edges, L = max_index_bins_lds."""
import numpy as np
import pytest

import util
from bin_ref import INT_DTYPES, bin_reference
from pairs_ref import mapped_columns, stable_perm
from segment_pairs_gpu import guarded, key_tensor, same
from segment_pairs_ref import with_guards

pytestmark = pytest.mark.gpu

KEY_TYPES = ["u8", "i16", "u32", "i32", "f32", "u64", "i64", "f64", "u128"]
MODES = {"upper": 0, "lower": 1, "index": 2}
F32_SPECIALS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001], dtype="<u4")
F64_SPECIALS = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0, 0x8000000000000000, 0x7FF0000000000000,
                         0xFFF0000000000000, 1, 0x8000000000000001], dtype="<u8")


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


def count_bytes_of(counts, cb):
    return np.asarray(counts, dtype="<i4" if cb == 4 else "<i8").view(np.uint8).reshape(-1)


def sort_edges(raw, tname, desc):
    """the edge rows of `raw` in the order of their mapped keys"""
    _es, _ko, kb, kind = util.TYPES[tname]
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1, kb)
    return raw[stable_perm(mapped_columns(raw.reshape(-1), kb, kind, desc))].reshape(-1)


def make_keys(tname, n, seed, spread=40):
    """n keys of few distinct values (so that keys meet edges and each other), floats with every special bit pattern"""
    rng = np.random.default_rng(seed)
    kb = util.TYPES[tname][2]
    if tname in ("f32", "f64"):
        v = (rng.integers(-spread, spread + 1, n) / 4.0).astype("<f4" if kb == 4 else "<f8")
        raw = v.view("<u4" if kb == 4 else "<u8").copy()
        sp = F32_SPECIALS if kb == 4 else F64_SPECIALS
        k = min(n, sp.size)
        raw[:k] = sp[:k]
        rng.shuffle(raw)
        return raw.view(np.uint8)
    if tname == "u128":
        raw = np.zeros((n, 16), dtype=np.uint8)
        raw[:, 15] = rng.integers(0, 7, n)  # the top byte and the bottom byte decide
        raw[:, 0] = rng.integers(0, 7, n)
        return raw.reshape(-1)
    if kb == 1:
        spread = min(spread, 127)
    lo, hi = (0, 2 * spread) if tname[0] == "u" else (-spread, spread)
    scale = 1 if kb == 1 else (1 << (8 * kb - 1)) // (2 * spread + 2)  # spread over the width: the sign and the top bits take part
    return (rng.integers(lo, hi + 1, n) * scale).astype(INT_DTYPES[tname]).view(np.uint8)


def make_edges(tname, m, seed, desc, spread=40):
    """m edges drawn like the keys, duplicates included, sorted in this order"""
    kb = util.TYPES[tname][2]
    return sort_edges(make_keys(tname, max(m, 16), seed + 77, spread).reshape(-1, kb)[:m], tname, desc)


class Call:
    """One key column on the GPU (guarded, `shift` bytes behind a 16-byte boundary) and the calls made on it through
    Context.bin_count_device on raw pointers."""

    def __init__(self, torch, c, tname, keys_raw, shift=0):
        self.torch, self.c, self.tname = torch, c, tname
        self.kb, self.kind = util.TYPES[tname][2], util.TYPES[tname][3]
        self.keys_raw = np.ascontiguousarray(keys_raw).view(np.uint8).reshape(-1)
        self.n = self.keys_raw.size // self.kb
        self.shift = shift if self.n else 0  # (an empty view has no address to be aligned)
        self.kbuf, self.kmid = guarded(torch, self.keys_raw, self.shift)

    def run(self, edges, mode, desc=False, cb=8, num=None, initial=None, accumulate=False, status=None, n=None, key_offset=0):
        """-> the counts allocation as numpy bytes.  edges: the raw edge bytes, or m itself in the index mode.  initial: the
        counts before the call (default: 0xA5 bytes).  n, key_offset: a sub-range of the column."""
        torch = self.torch
        if mode == "index":
            m, emid, ebuf = int(edges), None, None
        else:
            edges = np.ascontiguousarray(edges).view(np.uint8).reshape(-1)
            m = edges.size // self.kb
            ebuf, emid = guarded(torch, edges)
        init = np.full((m + 1) * cb, 0xA5, dtype=np.uint8) if initial is None else count_bytes_of(initial, cb)
        cbuf, cmid = guarded(torch, init)
        dnum = torch.tensor([num], dtype=torch.int64, device="cuda") if num is not None else None
        n = self.n if n is None else n
        args = (self.kmid.data_ptr() + key_offset * self.kb if self.n else 0, n, self.kb, self.kind, emid.data_ptr() if emid is not None and m else 0, m,
                MODES[mode], cmid.data_ptr(), cb, desc, dnum.data_ptr() if dnum is not None else 0, 1 if accumulate else 0,
                torch.cuda.current_stream().cuda_stream)
        if status is None:
            self.c.bin_count_device(*args)
            self.c.check()
        else:
            import radix_sort_amd as rs
            with pytest.raises(rs.RsxError) as e:
                self.c.bin_count_device(*args)
            assert e.value.status == status, e.value
            torch.cuda.synchronize()
        if ebuf is not None:
            assert same(ebuf.cpu().numpy(), with_guards(edges), ("the edges", self.tname))
        return cbuf.cpu().numpy()

    def check(self, edges, mode, desc=False, cb=8, num=None, what=None):
        want = bin_reference(self.keys_raw, edges, self.tname, mode, desc, num)
        got = self.run(edges, mode, desc, cb, num)
        assert same(got, with_guards(count_bytes_of(want, cb)), ("counts", self.tname, what, mode, desc, cb, num))
        return want

    def keys_unchanged(self):
        assert same(self.kbuf.cpu().numpy(), with_guards(self.keys_raw, self.shift), ("the key column", self.tname))


def info(rs, c):
    """(path, kernels launched, every other bit) of RSX_INFO_LAST_PASSES"""
    v = c.get_info(rs.INFO_LAST_PASSES)
    return (v >> 24) & 0x1F, v & 0xFF, v & ~((0x1F << 24) | 0xFF)


@pytest.mark.parametrize("one_behind", [False, True])
def test_sizes_around_the_share(rs, torch, ctx, one_behind):
    """The loader's head and tail and one to five workgroups: the key pointer on a 16-byte boundary and one key behind it."""
    S = rs.bin_caps(4)[2]
    for tname in ("u32", "u8", "u128"):
        kb = util.TYPES[tname][2]
        edges = make_edges(tname, 64, 1, False)
        for n in (0, 1, 3, 17, S - 1, S, S + 1, 2 * S + 3, 5 * S + 5):
            call = Call(torch, ctx, tname, make_keys(tname, n, n), shift=kb if one_behind else 0)
            want = call.check(edges, "upper", what=("n", n))
            assert int(want.sum()) == n
            assert info(rs, ctx) == (16, 2 if n else 1, 0)
            call.keys_unchanged()


@pytest.mark.parametrize("tname", KEY_TYPES)
def test_key_types_sides_and_orders(rs, torch, ctx, tname):
    S = rs.bin_caps(util.TYPES[tname][2])[2]
    call = Call(torch, ctx, tname, make_keys(tname, 2 * S + 3, 5), shift=0)
    for desc in (False, True):
        edges = make_edges(tname, 63, 2, desc)
        for mode, cb in (("upper", 8), ("lower", 4)):
            call.check(edges, mode, desc, cb)
    call.keys_unchanged()


@pytest.mark.parametrize("tname", ["u32", "i64", "u128", "u8"])
def test_edge_counts(rs, torch, ctx, tname):
    """m from 0 to max_edges; one more is refused by the C call and answered by radix_histogram through the index form."""
    kb = util.TYPES[tname][2]
    E, _L, S = rs.bin_caps(kb)
    call = Call(torch, ctx, tname, make_keys(tname, S + 1, 9, spread=2000), shift=kb)
    for m in (0, 1, 2, 63, 64, 1000, E):
        for mode, desc in (("upper", False), ("lower", True)):
            call.check(make_edges(tname, m, m, desc, spread=2000), mode, desc, what=("m", m))
    for mode, desc in (("upper", True), ("lower", False)):
        edges = make_edges(tname, E + 1, 4, desc, spread=2000)
        got = call.run(edges, mode, desc, status=rs._lib.ERR_UNSUPPORTED)
        assert same(got, with_guards(np.full((E + 2) * 8, 0xA5, dtype=np.uint8)), "nothing was enqueued")
        _eb, emid = guarded(torch, edges)
        out = rs.radix_histogram(key_tensor(torch, call.kmid, tname), key_tensor(torch, emid, tname), side="right" if mode == "upper" else "left",
                                 descending=desc, ctx=ctx)
        ctx.check()
        assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), bin_reference(call.keys_raw, edges, tname, mode, desc))
        assert info(rs, ctx)[:2] == (16, 2)  # the index form behind radix_searchsorted
    call.keys_unchanged()


def test_inputs(rs, torch, ctx):
    S = rs.bin_caps(4)[2]
    n = 2 * S + 3
    rng = np.random.default_rng(1)
    edges = (np.arange(100, dtype="<u4") * 1000 + 5000)
    # duplicate edges: empty bins between them
    call = Call(torch, ctx, "u32", rng.integers(0, 120000, n).astype("<u4"))
    dup = np.repeat(edges[::10], 10)
    for mode in ("upper", "lower"):
        want = call.check(dup, mode, what="duplicate edges")
        assert int((want == 0).sum()) >= 90
        call.check(np.full(64, 7777, dtype="<u4"), mode, what="all edges equal")
    # every key equal to one edge
    call = Call(torch, ctx, "u32", rng.choice(edges, n))
    assert call.check(edges, "upper", what="keys on edges")[0] == 0
    assert call.check(edges, "lower", what="keys on edges")[100] == 0
    # all keys equal: many workgroups flushing into one counter, every wave through the uniform shortcut
    call = Call(torch, ctx, "u32", np.full(5 * S + 5, edges[40], dtype="<u4"))
    for cb in (4, 8):
        assert call.check(edges, "upper", cb=cb, what="all keys equal")[41] == 5 * S + 5
    # all keys below the first and above the last edge
    assert Call(torch, ctx, "u32", rng.integers(0, 5000, n).astype("<u4")).check(edges, "upper", what="below")[0] == n
    assert Call(torch, ctx, "u32", rng.integers(105000, 1 << 32, n).astype("<u4")).check(edges, "lower", what="above")[100] == n
    # sorted keys: waves of one bin and waves that straddle an edge
    call = Call(torch, ctx, "i32", np.sort(rng.integers(-60000, 60000, n)).astype("<i4"))
    call.check(np.arange(-50000, 50000, 1000, dtype="<i4"), "upper", what="sorted keys")
    call.check(np.arange(-50000, 50000, 1000, dtype="<i4")[::-1].copy(), "lower", True, what="sorted keys, descending edges")
    # float specials among keys and edges
    for tname, sp in (("f32", F32_SPECIALS), ("f64", F64_SPECIALS)):
        call = Call(torch, ctx, tname, make_keys(tname, S + 1, 3))
        for desc in (False, True):
            for mode in ("upper", "lower"):
                call.check(sort_edges(sp, tname, desc), mode, desc, what="specials as edges")
        call.keys_unchanged()


def test_unsorted_edges_stay_in_bounds(rs, torch, ctx):
    """The result is unspecified; the guards around the counts are not, and every key lands in one of the m + 1 bins."""
    S = rs.bin_caps(4)[2]
    rng = np.random.default_rng(2)
    call = Call(torch, ctx, "u32", rng.integers(0, 1 << 32, S + 1).astype("<u4"))
    for m in (1, 2, 63, 1000):
        got = call.run(rng.integers(0, 1 << 32, m).astype("<u4"), "upper")
        want_guards = with_guards(np.zeros((m + 1) * 8, dtype=np.uint8))
        assert np.array_equal(got[:64], want_guards[:64]) and np.array_equal(got[-64:], want_guards[-64:])
        assert int(got[64:-64].view("<i8").sum()) == S + 1


@pytest.mark.parametrize("cb", [4, 8])
def test_accumulate_and_overwrite(rs, torch, ctx, cb):
    S = rs.bin_caps(8)[2]
    n = 2 * S + 4
    call = Call(torch, ctx, "i64", make_keys("i64", n, 8))
    edges = make_edges("i64", 200, 3, False)
    whole = bin_reference(call.keys_raw, edges, "i64", "upper")
    start = np.arange(201, dtype=np.int64) * 3 + 1
    half = n // 2
    got = call.run(edges, "upper", cb=cb, initial=start, accumulate=True, n=half)
    first = got[64:-64].view("<i4" if cb == 4 else "<i8").astype(np.int64)
    assert same(got, with_guards(count_bytes_of(start + bin_reference(call.keys_raw[:half * 8], edges, "i64", "upper"), cb)), "first half")
    got = call.run(edges, "upper", cb=cb, initial=first, accumulate=True, n=n - half, key_offset=half)
    assert same(got, with_guards(count_bytes_of(start + whole, cb)), "two halves equal the whole")
    assert info(rs, ctx) == (16, 1, 0)  # no zeroing launch
    got = call.run(edges, "upper", cb=cb, initial=start)  # without the flag: overwritten
    assert same(got, with_guards(count_bytes_of(whole, cb)), "overwritten")
    got = call.run(edges, "upper", cb=cb, initial=start, accumulate=True, n=0)  # nothing to count, nothing zeroed
    assert same(got, with_guards(count_bytes_of(start, cb)), "n = 0, accumulating")
    call.keys_unchanged()


def test_num_on_the_device(rs, torch, ctx):
    S = rs.bin_caps(4)[2]
    n = 3 * S + 1
    call = Call(torch, ctx, "f32", make_keys("f32", n, 4), shift=4)
    edges = make_edges("f32", 64, 6, True)
    for num in (0, n // 2, n, n + 7):
        want = call.check(edges, "lower", True, num=num, what="num")
        assert int(want.sum()) == min(num, n)
    ids = Call(torch, ctx, "i32", np.random.default_rng(5).integers(-2, 300, n).astype("<i4"))
    for num in (0, n // 2, n, n + 7):
        ids.check(255, "index", num=num)
        ids.check(0, "index", num=num)  # m = 0: one bin holds N
        ids.check(make_edges("i32", 0, 0, False), "upper", num=num)


@pytest.mark.parametrize("tname", ["u8", "i8", "u16", "i32", "u32", "i64", "u64"])
def test_index_mode(rs, torch, ctx, tname):
    kb = util.TYPES[tname][2]
    _E, L, S = rs.bin_caps(kb)
    dt = np.dtype(INT_DTYPES[tname])
    lim = np.iinfo(dt)
    rng = np.random.default_rng(kb)
    n = 2 * S + 3
    for m in (1, 255, L - 1, L, L + 1, 16 * L, 16 * L + 1, 1 << 20):  # one window, two, sixteen (include/rsx.h), then the atomics
        v = rng.integers(max(lim.min, -5), min(lim.max, m + m // 8 + 5), n, endpoint=True).astype(dt)  # negative and too-large keys among them
        v[:5] = [lim.min, lim.max, 0, min(lim.max, m), min(lim.max, m - 1)]
        call = Call(torch, ctx, tname, v, shift=kb)
        want = call.check(m, "index", cb=8 if m != 255 else 4, what=("index", m))
        assert int(want.sum()) == n and (want[m] > 0 or (lim.min == 0 and lim.max < m))  # keys outside, where the type has any
        assert info(rs, ctx) == (16, 2, 0)
        call.keys_unchanged()
    for m in (L - 1, 3 * L, 1 << 20):  # all keys one value: one window, several, the atomics
        val = min(lim.max, m - 1, 77 if m < L else 2 * L + 77)
        want = Call(torch, ctx, tname, np.full(5 * S + 5, val, dtype=dt)).check(m, "index", cb=4, what="one value")
        assert want[val] == 5 * S + 5


def test_errors(rs, torch, ctx):
    E, _L, S = rs.bin_caps(4)
    ARG, UNS = rs._lib.ERR_ARG, rs._lib.ERR_UNSUPPORTED
    st = torch.cuda.current_stream().cuda_stream
    keys = torch.zeros(64, dtype=torch.int32, device="cuda")
    edges = torch.zeros(8, dtype=torch.int32, device="cuda")
    counts = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    k, e, c = keys.data_ptr(), edges.data_ptr(), counts.data_ptr()

    def refused(status, *args):
        with pytest.raises(rs.RsxError) as err:
            ctx.bin_count_device(*args)
        assert err.value.status == status, (args, err.value)

    #                 keys n  kb kind edges m mode counts cb desc num flags
    refused(ARG, k, 64, 3, 0, e, 8, 0, c, 8, False, 0, 0, st)               # a bad width
    refused(ARG, k, 64, 4, 3, e, 8, 0, c, 8, False, 0, 0, st)               # a bad kind
    refused(ARG, k, 64, 16, rs.KEY_FLOAT, e, 2, 0, c, 8, False, 0, 0, st)   # 16-byte floats
    refused(ARG, k, 64, 4, 0, e, 8, 3, c, 8, False, 0, 0, st)               # a bad mode
    refused(ARG, k, 64, 4, 0, e, 8, 0, c, 8, False, 0, 2, st)               # unknown flag bits
    refused(ARG, k, 64, 4, 0, e, 8, 0, c, 2, False, 0, 0, st)               # count_bytes
    refused(ARG, k, 64, 4, 0, e, 8, 0, c, 16, False, 0, 0, st)
    refused(ARG, k, 64, 4, 0, e, 8, 0, 0, 8, False, 0, 0, st)               # no counts
    refused(ARG, 0, 64, 4, 0, e, 8, 0, c, 8, False, 0, 0, st)               # no keys
    refused(ARG, k, 64, 4, 0, 0, 8, 0, c, 8, False, 0, 0, st)               # no edges
    refused(ARG, k + 2, 32, 4, 0, e, 8, 0, c, 8, False, 0, 0, st)           # misaligned keys, edges, counts, num
    refused(ARG, k, 64, 4, 0, e + 1, 4, 0, c, 8, False, 0, 0, st)
    refused(ARG, k, 64, 4, 0, e, 8, 0, c + 4, 8, False, 0, 0, st)
    refused(ARG, k, 64, 4, 0, e, 8, 0, c, 8, False, c + 4, 0, st)
    refused(ARG, k, 64, 4, 0, e, 8, 2, c, 8, False, 0, 0, st)               # the index mode with edges, with an order
    refused(ARG, k, 64, 4, 0, 0, 8, 2, c, 8, True, 0, 0, st)
    refused(ARG, k, 64, 4, 0, 0, (1 << 32) - 1, 2, c, 8, False, 0, 0, st)   # m + 1 does not fit
    refused(UNS, k, 64, 4, rs.KEY_FLOAT, 0, 8, 2, c, 8, False, 0, 0, st)    # the index mode on floats and on 128-bit keys
    refused(UNS, k, 4, 16, 0, 0, 8, 2, c, 8, False, 0, 0, st)
    refused(UNS, k, 64, 4, 0, e, E + 1, 0, c, 8, False, 0, 0, st)           # too many edges
    refused(UNS, k, 64, 4, 0, e, E + 1, 1, c, 8, True, 0, 0, st)
    refused(UNS, k, 1 << 32, 4, 0, e, 8, 0, c, 4, False, 0, 0, st)          # 2^32 keys into 4-byte counts
    with pytest.raises(rs.RsxError) as err:                                  # an order that is neither
        ctx._check(ctx._L.rsx_bin_count_device(ctx._h, k, 64, None, 4, 0, e, 8, 0, 2, c, 8, 0, st))
    assert err.value.status == ARG
    torch.cuda.synchronize()
    ctx.check()
    assert bool((counts == -1).all())  # nothing was enqueued


def test_python_layer(rs, torch, ctx):
    S = rs.bin_caps(4)[2]
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    x = torch.randn((3, S // 2 + 1, 2), device="cuda", generator=g)
    x[0, :4, 0] = torch.tensor([float("nan"), -0.0, float("inf"), -float("inf")], device="cuda")
    edges = torch.linspace(-3, 3, 64, device="cuda")
    raw, eraw = x.cpu().numpy().view(np.uint8).reshape(-1), edges.cpu().numpy().view(np.uint8)
    out = rs.radix_histogram(x, edges, ctx=ctx)
    ctx.check()
    assert out.dtype == torch.int64 and out.shape == (65,)
    assert np.array_equal(out.cpu().numpy(), bin_reference(raw, eraw, "f32", "upper"))
    finite = x[torch.isfinite(x)].cpu().numpy()
    hist = np.histogram(finite, edges.cpu().numpy())[0]  # the documented relation
    want = out[1:64].cpu().numpy().copy()
    want[-1] += int((finite == float(edges[-1])).sum())
    assert np.array_equal(hist, want)
    left = rs.radix_histogram(x, edges.flip(0).contiguous(), side="left", descending=True, count_dtype=torch.int32, ctx=ctx)
    ctx.check()
    assert left.dtype == torch.int32
    assert np.array_equal(left.cpu().numpy(), bin_reference(raw, eraw.reshape(-1, 4)[::-1].reshape(-1), "f32", "lower", True))
    buf = torch.full((65 + 2,), -7, dtype=torch.int32, device="cuda")
    num = torch.tensor([1000], dtype=torch.int64, device="cuda")
    got = rs.radix_histogram(x, edges, num=num, out=buf[1:66], ctx=ctx)
    assert got.data_ptr() == buf[1:66].data_ptr()
    rs.radix_histogram(x, edges, num=num, out=buf[1:66], accumulate=True, ctx=ctx)
    ctx.check()
    assert int(buf[0]) == -7 and int(buf[66]) == -7
    assert np.array_equal(buf[1:66].cpu().numpy(), 2 * bin_reference(raw, eraw, "f32", "upper", False, 1000))
    empty = rs.radix_histogram(x[:0], edges[:0], ctx=ctx)
    assert empty.tolist() == [0]
    # 128-bit keys
    k128 = make_keys("u128", 1000, 1)
    e128 = make_edges("u128", 20, 2, False)
    t = torch.from_numpy(k128.copy()).cuda().view(10, 100, 16)
    out = rs.radix_histogram(t, torch.from_numpy(e128.copy()).cuda().view(20, 16), ctx=ctx)
    ctx.check()
    assert np.array_equal(out.cpu().numpy(), bin_reference(k128, e128, "u128", "upper"))
    # radix_bincount
    ids = torch.randint(-3, 5000, (7, S // 4 + 3), dtype=torch.int64, device="cuda", generator=g)
    for bins, dt in ((4096, None), (1 << 17, torch.int32), (1 << 19, torch.int32), (0, None)):
        out = rs.radix_bincount(ids, bins, count_dtype=dt, ctx=ctx)
        ctx.check()
        assert out.dtype == (dt or torch.int64) and out.shape == (bins + 1,)
        inside = ids[(ids >= 0) & (ids < bins)]
        assert torch.equal(out[:bins].to(torch.int64), torch.bincount(inside, minlength=bins)) and int(out[bins]) == ids.numel() - inside.numel()
        assert np.array_equal(out.cpu().numpy(), bin_reference(ids.cpu().numpy().view(np.uint8), bins, "i64", "index"))
    acc = torch.ones(4097, dtype=torch.int64, device="cuda")
    assert rs.radix_bincount(ids, 4096, out=acc, accumulate=True, num=num, ctx=ctx) is acc
    ctx.check()
    assert np.array_equal(acc.cpu().numpy(), 1 + bin_reference(ids.cpu().numpy().view(np.uint8), 4096, "i64", "index", False, 1000))
    small = rs.radix_bincount(torch.tensor([[1, 1], [250, 255]], dtype=torch.uint8, device="cuda"), 251, ctx=ctx)
    assert small[1] == 2 and small[250] == 1 and small[251] == 1 and int(small.sum()) == 4


def test_graph_capture(rs, torch):
    """The call needs no reserve and allocates nothing: one capture on a fresh context into a preallocated out, replayed
    twice on changed keys.  The zeroing is inside the graph: the second replay does not add to the first."""
    S = rs.bin_caps(4)[2]
    n = 3 * S + 5
    c = rs.Context(torch.cuda.current_device())
    s = torch.cuda.Stream()
    keys = torch.zeros(n, dtype=torch.float32, device="cuda")
    edges = torch.linspace(-50, 50, 101, device="cuda")
    out = torch.full((102,), -1, dtype=torch.int64, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        got = rs.radix_histogram(keys, edges, out=out, ctx=c)
    assert got is out
    for seed in (1, 2):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        keys.copy_(torch.randint(-40 * seed, 40 * seed, (n,), device="cuda", generator=g).to(torch.float32))
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        want = bin_reference(keys.cpu().numpy().view(np.uint8), edges.cpu().numpy().view(np.uint8), "f32", "upper")
        assert np.array_equal(out.cpu().numpy(), want), seed
        assert info(rs, c) == (16, 2, 0)
    c.close()
