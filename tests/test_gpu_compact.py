"""GPU: rsx_compact_device / radix_compact / radix_nonzero against tests/compact_ref.py.

Every comparison is np.array_equal on all bytes of an allocation the test owns: 64 guard bytes of 0xA5, the column, 64 guard
bytes; every output is pre-filled with 0xA5 too, so a row that is written behind the kept ones (behind N under partition)
shows, and so does one that is not written.  The inputs are compared with their originals afterwards, and ctx.check() runs
after each call.  Sizes come from compact_caps: T = tile, S = scan_span."""
import itertools

import numpy as np
import pytest

import util
from compact_ref import compact_reference, expected_column, expected_index
from segment_pairs_gpu import guarded, same
from segment_pairs_ref import with_guards
from test_gpu_bin import F32_SPECIALS, F64_SPECIALS, info, make_keys

pytestmark = pytest.mark.gpu

KEY_TYPES = ["u8", "i16", "u32", "i32", "f32", "u64", "i64", "f64", "u128"]
MASKS = ["all", "none", "alternating", "last", "tile_ends", "half", "sparse", "bytes"]
PATH = 17


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


def make_mask(kind, n, tile, seed=0):
    rng = np.random.default_rng(seed)
    m = np.zeros(n, dtype=np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind == "last":
        m[n - 1:] = 1
    elif kind == "tile_ends":  # the first and the last row of every tile
        m[::tile] = 1
        m[tile - 1::tile] = 1
        m[n - 1:] = 1
    elif kind == "half":
        m[:] = rng.integers(0, 2, n)
    elif kind == "sparse":
        m[:] = rng.integers(0, 64, n) == 0
    elif kind == "bytes":  # any non-zero byte passes: 2 and 0x80 have their low bit clear
        m[:] = rng.choice(np.array([0, 0, 2, 0x80], dtype=np.uint8), n)
    else:
        assert kind == "none", kind
    return m


def make_values(n, vb, seed=1):
    return np.random.default_rng(seed).integers(0, 256, n * vb, dtype=np.uint8)


class Table:
    """The input columns of one call on the GPU (guarded; keys and mask `shift` bytes behind a 16-byte boundary) and the
    calls made on them through Context.compact_device on raw pointers."""

    def __init__(self, torch, c, n, tname=None, keys_raw=None, mask=None, values_raw=None, vb=0, key_shift=0, mask_shift=0):
        self.torch, self.c, self.n, self.tname, self.vb = torch, c, n, tname, vb
        self.kb, self.kind = (util.TYPES[tname][2], util.TYPES[tname][3]) if tname else (0, 0)
        self.keys_raw = np.ascontiguousarray(keys_raw).view(np.uint8).reshape(-1) if keys_raw is not None else None
        self.mask, self.values_raw = mask, values_raw
        self.shifts = (key_shift if n else 0, mask_shift if n else 0)  # (an empty view has no address to be aligned)
        self.kbuf, self.kmid = guarded(torch, self.keys_raw, self.shifts[0]) if keys_raw is not None else (None, None)
        self.mbuf, self.mmid = guarded(torch, mask, self.shifts[1]) if mask is not None else (None, None)
        self.vbuf, self.vmid = guarded(torch, values_raw) if values_raw is not None else (None, None)

    def run(self, lo=None, hi=None, desc=False, invert=False, partition=False, ib=8, num=None, outs=("keys", "values", "index"), what=None):
        """One call, every output in a guarded allocation of 0xA5 bytes, held against the reference -> (rows, m)."""
        torch, n = self.torch, self.n
        ptr = lambda mid: mid.data_ptr() if mid is not None and n else 0
        bounds = []
        for b in (lo, hi):
            bounds.append(guarded(torch, np.ascontiguousarray(b).view(np.uint8).reshape(-1)) if b is not None else (None, None))
        widths = {"keys": self.kb, "values": self.vb, "index": ib}
        outs = tuple(o for o in outs if widths[o])  # (a table without keys or values has no such output)
        out = {name: guarded(torch, np.full(n * widths[name], 0xA5, dtype=np.uint8)) for name in outs}
        nbuf, nmid = guarded(torch, np.full(8, 0xA5, dtype=np.uint8))
        dnum = torch.tensor([num], dtype=torch.int64, device="cuda") if num is not None else None
        optr = lambda name: out[name][1].data_ptr() if name in out and n else 0
        args = (ptr(self.kmid), n, self.kb, self.kind, ptr(self.mmid), bounds[0][1].data_ptr() if lo is not None else 0,
                bounds[1][1].data_ptr() if hi is not None else 0, ptr(self.vmid) if "values" in out else 0, self.vb if "values" in out else 0,
                optr("keys"), optr("values"), optr("index"), ib, nmid.data_ptr(), desc, dnum.data_ptr() if dnum is not None else 0,
                (1 if invert else 0) | (2 if partition else 0), torch.cuda.current_stream().cuda_stream)
        self.c.compact_device(*args)
        self.c.check()
        rows, m = compact_reference(n, self.tname, self.keys_raw, self.mask, lo, hi, desc, invert, partition, num)
        tag = (what, self.tname, n, desc, invert, partition, ib, num, outs)
        assert same(nbuf.cpu().numpy(), with_guards(np.array([m], dtype="<u8")), ("num",) + tag)
        if "keys" in out:
            assert same(out["keys"][0].cpu().numpy(), with_guards(expected_column(self.keys_raw, self.kb, n, rows)), ("keys",) + tag)
        if "values" in out:
            assert same(out["values"][0].cpu().numpy(), with_guards(expected_column(self.values_raw, self.vb, n, rows)), ("values",) + tag)
        if "index" in out:
            assert same(out["index"][0].cpu().numpy(), with_guards(expected_index(n, ib, rows)), ("index",) + tag)
        for (buf, _mid), raw in zip(bounds, (lo, hi)):
            if buf is not None:
                assert same(buf.cpu().numpy(), with_guards(raw), ("a bound",) + tag)
        return rows, m

    def unchanged(self):
        if self.kbuf is not None:
            assert same(self.kbuf.cpu().numpy(), with_guards(self.keys_raw, self.shifts[0]), ("the key column", self.tname))
        if self.mbuf is not None:
            assert same(self.mbuf.cpu().numpy(), with_guards(self.mask, self.shifts[1]), ("the mask", self.tname))
        if self.vbuf is not None:
            assert same(self.vbuf.cpu().numpy(), with_guards(self.values_raw), ("the values", self.tname))


def sizes(rs, kb=4, vb=4, ib=8):
    T, S = rs.compact_caps(kb, vb, ib)
    return T, S, [0, 1, T - 1, T, T + 1, 3 * T + 5, S * T + T + 3]


def ordered(tname, a, b, desc):
    """the raw keys a, b as (lower, upper) in the order of the call"""
    _rows, m = compact_reference(1, tname, a, lo=b, descending=desc)  # M(b) <= M(a)?
    return (b, a) if m else (a, b)


@pytest.mark.parametrize("partition", [False, True])
@pytest.mark.parametrize("which", range(7))
def test_sizes_and_masks(rs, torch, ctx, which, partition):
    """u32 keys, u32 values and 8-byte positions under every mask shape, at every size around a tile and past one sweep of
    the scan; the kept rows alone, then the stable partition."""
    T, _S, ns = sizes(rs)
    n = ns[which]
    keys = make_keys("u32", n, 3)
    vals = make_values(n, 4)
    for kind in MASKS:
        if n == 0 and kind != "all":
            continue
        t = Table(torch, ctx, n, "u32", keys, make_mask(kind, n, T, seed=which), vals, 4)
        rows, m = t.run(partition=partition, what=kind)
        assert rows.size == (n if partition else m)
        if kind in ("all", "none"):
            assert m == (n if kind == "all" else 0)
        t.unchanged()
    assert info(rs, ctx) == (PATH, 3 if n else 0, 0)


@pytest.mark.parametrize("tname", KEY_TYPES)
def test_key_types_and_bounds(rs, torch, ctx, tname):
    """Every key type under lo only, hi only, both, lo == hi and lo above hi -- each bound a key that occurs --, ascending and
    descending, with and without invert; floats with every special bit pattern as a key and as a bound."""
    kb = util.TYPES[tname][2]
    T = rs.compact_caps(kb, 0, 4)[0]
    n = 3 * T + 5
    keys = make_keys(tname, n, 11).reshape(n, kb)
    t = Table(torch, ctx, n, tname, keys)
    a, b = keys[n // 3].copy(), next(k for k in keys[n // 2:] if not np.array_equal(k, keys[n // 3])).copy()
    for desc, invert in itertools.product((False, True), repeat=2):
        low, up = ordered(tname, a, b, desc)
        kept = {}
        for what, lo, hi in (("lo", low, None), ("hi", None, up), ("both", low, up), ("equal", low, low), ("crossed", up, low)):
            _rows, kept[what] = t.run(lo, hi, desc, invert, ib=4, outs=("keys", "index"), what=what)
        assert kept["equal"] == kept["crossed"] == (n if invert else 0)
        assert 0 < kept["both"] < n  # the rows of `low` are in it, those of `up` are not (invert: the other way round)
    if tname in ("f32", "f64"):
        specials = F32_SPECIALS if kb == 4 else F64_SPECIALS
        for s, desc in itertools.product(specials, (False, True)):
            bound = np.array([s], dtype=specials.dtype).view(np.uint8)
            t.run(lo=bound, desc=desc, ib=4, outs=("keys",), what=("special lo", hex(int(s))))
            t.run(hi=bound, desc=desc, partition=True, ib=4, outs=("index",), what=("special hi", hex(int(s))))
    t.unchanged()


@pytest.mark.parametrize("tname,vb", [("u32", 4), ("i64", 16)])  # 16 and 8 rows per thread: one flag word of 16, of 8 bytes
def test_unaligned_bases(rs, torch, ctx, tname, vb):
    """The mask 1, 7 and 15 bytes behind a 16-byte boundary, the keys one and three keys behind one."""
    kb = util.TYPES[tname][2]
    T = rs.compact_caps(kb, vb, 8)[0]
    assert T == (4096 if vb == 4 else 2048)
    for n in (1, T - 1, 3 * T + 5):
        keys, vals = make_keys(tname, n, 5), make_values(n, vb)
        lo = keys.reshape(n, kb)[n // 2].copy()
        for mask_shift, key_shift in ((1, 0), (7, kb), (15, 3 * kb), (0, kb), (8, 0)):
            for kind in ("half", "tile_ends", "bytes"):
                t = Table(torch, ctx, n, tname, keys, make_mask(kind, n, T, seed=mask_shift), vals, vb, key_shift=key_shift, mask_shift=mask_shift)
                t.run(lo=lo, partition=(mask_shift == 7), what=(kind, mask_shift, key_shift))
                t.run(outs=("index",), ib=4, what=("mask only", kind, mask_shift, key_shift))
                t.unchanged()
    # one-byte keys: one and three bytes behind the boundary
    n = 3 * 4096 + 5
    keys = make_keys("u8", n, 6)
    for key_shift in (1, 3):
        t = Table(torch, ctx, n, "u8", keys, make_mask("half", n, 4096), key_shift=key_shift, mask_shift=key_shift)
        t.run(lo=keys[:1].copy(), hi=keys[7:8].copy(), outs=("keys", "index"), what=("u8", key_shift))
        t.unchanged()


def test_mask_and_range_together(rs, torch, ctx):
    T = rs.compact_caps(4, 0, 8)[0]
    n = 3 * T + 5
    keys = make_keys("f32", n, 8).reshape(n, 4)
    t = Table(torch, ctx, n, "f32", keys, make_mask("half", n, T))
    low, up = np.array([0xC0000000], dtype="<u4").view(np.uint8), np.array([0x3F800000], dtype="<u4").view(np.uint8)  # -2.0, 1.0
    for desc, invert, partition in itertools.product((False, True), repeat=3):
        lo, hi = (up, low) if desc else (low, up)
        _rows, m = t.run(lo, hi, desc, invert, partition, outs=("keys", "index"))
        _rows, range_only = Table(torch, ctx, n, "f32", keys).run(lo, hi, desc, invert, partition, outs=("keys",))
        assert (m > range_only) if invert else (0 < m < range_only)  # the mask took part
    t.unchanged()


@pytest.mark.parametrize("vb", [1, 2, 4, 8, 16, 12, 40])
def test_value_and_index_widths(rs, torch, ctx, vb):
    """Values the write kernel moves itself, and 12- and 40-byte rows behind positions: the caller's index when there is
    one, the workspace's otherwise; the gather stops at the device count (at N under partition)."""
    T = rs.compact_caps(4, vb, 8)[0]
    n = 3 * T + 5
    keys, vals = make_keys("i32", n, 4), make_values(n, vb)
    t = Table(torch, ctx, n, "i32", keys, make_mask("half", n, T), vals, vb)
    wide = vb in (12, 40)
    for partition in (False, True):
        for ib, outs in ((4, ("keys", "values", "index")), (8, ("keys", "values", "index")), (8, ("values",)), (4, ("values", "index"))):
            t.run(partition=partition, ib=ib, outs=outs, num=n - 7 if ib == 4 else None)
            assert info(rs, ctx) == (PATH, 4 if wide else 3, 0)
    t.unchanged()


@pytest.mark.parametrize("partition", [False, True])
def test_every_subset_of_outputs(rs, torch, ctx, partition):
    T = rs.compact_caps(8, 8, 8)[0]
    n = 2 * T + 77
    keys, vals = make_keys("u64", n, 2).reshape(n, 8), make_values(n, 8)
    t = Table(torch, ctx, n, "u64", keys, make_mask("half", n, T), vals, 8)
    counts = set()
    for k in range(4):
        for outs in itertools.combinations(("keys", "values", "index"), k):
            counts.add(t.run(lo=keys[5].copy(), partition=partition, outs=outs)[1])
    assert len(counts) == 1  # the number kept does not depend on what is asked for
    t.unchanged()


@pytest.mark.parametrize("partition", [False, True])
def test_device_count_bounds_the_rows(rs, torch, ctx, partition):
    """d_num in {0, 1, T + 3, n + 5}: rows behind N are neither counted nor written."""
    T = rs.compact_caps(4, 4, 8)[0]
    n = 3 * T + 5
    keys, vals = make_keys("u32", n, 9).reshape(n, 4), make_values(n, 4)
    t = Table(torch, ctx, n, "u32", keys, make_mask("half", n, T), vals, 4)
    for num in (0, 1, T + 3, n + 5):
        rows, m = t.run(partition=partition, num=num)
        assert rows.size == (min(num, n) if partition else m) and m <= min(num, n)
        t.run(lo=keys[3].copy(), invert=True, partition=partition, num=num, ib=4)
    # a mask whose rows behind N are all set, and keys behind N that would all pass
    rows, m = Table(torch, ctx, n, "u32", keys, make_mask("all", n, T), vals, 4).run(num=T + 3, partition=partition)
    assert m == T + 3
    t.unchanged()


def test_no_predicate_is_a_copy(rs, torch, ctx):
    T = rs.compact_caps(4, 4, 8)[0]
    n = 2 * T + 9
    keys, vals = make_keys("i32", n, 12), make_values(n, 4)
    t = Table(torch, ctx, n, "i32", keys, None, vals, 4)
    assert t.run()[1] == n
    assert t.run(num=T + 1)[1] == T + 1
    assert t.run(invert=True)[1] == 0
    rows, m = t.run(invert=True, partition=True)  # nothing kept, everything behind it: a copy again
    assert m == 0 and np.array_equal(rows, np.arange(n))
    t.unchanged()


@pytest.mark.parametrize("n_which", [0, 1, 5])
def test_nonzero(rs, torch, ctx, n_which):
    """radix_nonzero: a pure mask call with d_keys NULL equals torch.nonzero(mask).flatten()."""
    T, _S, ns = sizes(rs, 0, 0, 8)
    n = ns[n_which]
    for kind, dtype in (("half", torch.bool), ("bytes", torch.uint8), ("sparse", torch.bool), ("none", torch.uint8), ("all", torch.bool)):
        m = make_mask(kind, n, T, seed=n_which)
        mask = torch.from_numpy(m).cuda()
        mask = mask != 0 if dtype == torch.bool else mask
        want = torch.nonzero(mask).flatten()
        for idt in (None, torch.int32):
            index, num = rs.radix_nonzero(mask, index_dtype=idt, ctx=ctx)
            ctx.check()
            assert index.dtype == (idt or torch.int64) and index.shape == (n,) and num.dtype == torch.int64 and num.dim() == 0
            assert int(num) == want.numel() and torch.equal(index[:want.numel()].to(torch.int64), want)
        assert torch.equal(mask, torch.from_numpy(m).cuda() != 0 if dtype == torch.bool else torch.from_numpy(m).cuda())
    if n:
        out = (torch.full((n,), -1, dtype=torch.int64, device="cuda"), torch.full((1,), -1, dtype=torch.int64, device="cuda"))
        bound = torch.tensor([n // 2], dtype=torch.int64, device="cuda")
        index, num = rs.radix_nonzero(mask, num=bound, out=out, ctx=ctx)
        assert index is out[0] and num is out[1]
        want = torch.nonzero(mask[:n // 2]).flatten()
        assert int(num) == want.numel() and torch.equal(index[:want.numel()], want) and bool((index[want.numel():] == -1).all())
        assert info(rs, ctx)[0] == PATH


def test_python_layer(rs, torch, ctx):
    """radix_compact on tensors: scalar and tensor bounds, values with trailing dimensions, 128-bit keys, partition."""
    n = 3 * rs.compact_caps(4, 12, 8)[0] + 5
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    keys = torch.randint(-50, 50, (n,), device="cuda", generator=g, dtype=torch.int32)
    vals = torch.rand((n, 3), device="cuda", generator=g)
    mask = torch.rand(n, device="cuda", generator=g) < 0.5
    k0, v0, m0 = keys.clone(), vals.clone(), mask.clone()
    r = rs.radix_compact(keys, mask=mask, lo=-10, hi=torch.tensor([20], dtype=torch.int32, device="cuda"), values=vals, return_index=True, ctx=ctx)
    ctx.check()
    sel = mask & (keys >= -10) & (keys < 20)
    m = int(sel.sum())
    assert isinstance(r, rs.Compacted) and int(r.num) == m and r.num.dim() == 0 and r.keys.shape == (n,) and r.values.shape == (n, 3)
    assert torch.equal(r.keys[:m], keys[sel]) and torch.equal(r.values[:m], vals[sel]) and torch.equal(r.index[:m], torch.nonzero(sel).flatten())
    p = rs.radix_compact(keys, lo=20, descending=True, values=vals, partition=True, invert=True, index_dtype=torch.int32, return_index=True, ctx=ctx)
    sel = ~(keys <= 20)  # descending: lo is the largest key that passes
    m = int(sel.sum())
    assert int(p.num) == m and p.index.dtype == torch.int32
    assert torch.equal(p.keys, torch.cat((keys[sel], keys[~sel]))) and torch.equal(p.values, torch.cat((vals[sel], vals[~sel])))
    q = rs.radix_compact(None, mask=mask, values=vals, ctx=ctx)
    assert q.keys is None and q.index is None and torch.equal(q.values[:int(q.num)], vals[mask])
    wide = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
    wide[:, 15] = (keys & 7).to(torch.uint8)
    bound = torch.zeros(16, dtype=torch.uint8, device="cuda")
    bound[15] = 4
    w = rs.radix_compact(wide, hi=bound, ctx=ctx)
    sel = wide[:, 15] < 4
    assert int(w.num) == int(sel.sum()) and torch.equal(w.keys[:int(w.num)], wide[sel])
    e = rs.radix_compact(keys[:0], mask=mask[:0], values=vals[:0], return_index=True, ctx=ctx)
    assert int(e.num) == 0 and e.keys.shape == (0,) and e.values.shape == (0, 3)
    ctx.check()
    assert torch.equal(keys, k0) and torch.equal(vals, v0) and torch.equal(mask, m0)


def test_composes_with_quantile_and_group(rs, torch, ctx):
    """The cut of radix_quantile and the count of radix_group go into the call as device words: between the calls of a chain
    the host reads nothing (the test itself reads, to compare and to plant keys behind the count)."""
    n = 3 * rs.compact_caps(4, 8, 8)[0] + 5
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    score = torch.randn(n, device="cuda", generator=g)
    ids = torch.arange(n, device="cuda", dtype=torch.int64)
    cut = rs.radix_quantile(score, [0.9], ctx=ctx)
    top = rs.radix_compact(score, lo=cut[0:1], values=ids, ctx=ctx)
    ctx.check()
    raw = score.cpu().numpy().view(np.uint8)
    rows, m = compact_reference(n, "f32", raw, lo=cut[0:1].cpu().numpy().view(np.uint8))
    assert int(top.num) == m and 0 < m < n
    assert np.array_equal(top.values[:m].cpu().numpy(), rows) and np.array_equal(top.keys[:m].cpu().numpy().view(np.uint8), raw.reshape(n, 4)[rows].reshape(-1))
    labels = torch.randint(0, 100, (n,), device="cuda", generator=g, dtype=torch.int32)
    grp = rs.radix_group(labels, ctx=ctx)  # grp.keys has n rows, grp.num of them defined
    junk = grp.keys.clone()
    junk[int(grp.num):] = 50  # what lies behind the count would pass
    kept = rs.radix_compact(junk, lo=40, hi=60, num=grp.num, ctx=ctx)
    ctx.check()
    assert int(kept.num) == 20 and torch.equal(kept.keys[:20], torch.arange(40, 60, device="cuda", dtype=torch.int32))


def test_graph_capture(rs, torch):
    """out= after reserve_compact allocates nothing: one captured call, one linear chain, replayed once on changed inputs.
    Without the reserve on a fresh context: RSX_ERR_WORKSPACE, nothing enqueued."""
    n = 3 * rs.compact_caps(4, 4, 8)[0] + 5
    s = torch.cuda.Stream()
    keys = torch.zeros(n, dtype=torch.float32, device="cuda")
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    lo = torch.zeros(1, dtype=torch.float32, device="cuda")
    out = rs.Compacted(torch.full((n,), -1.0, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda"),
                       torch.full((n,), -1, dtype=torch.int64, device="cuda"), torch.full((1,), -1, dtype=torch.int64, device="cuda"))

    def enqueue(c):
        return rs.radix_compact(keys, mask=mask, lo=lo, values=vals, out=out, ctx=c)

    fresh = rs.Context(torch.cuda.current_device())
    g0 = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g0.capture_begin()
        try:
            enqueue(fresh)
        except rs.RsxError as e:
            err = e
        g0.capture_end()
    assert err is not None and err.status == rs._lib.ERR_WORKSPACE, err
    torch.cuda.synchronize()
    assert all(bool((t == -1).all()) for t in out)  # nothing was enqueued
    fresh.close()

    c = rs.Context(torch.cuda.current_device())
    c.reserve_compact(n, 4, 4, 8)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        got = enqueue(c)
    assert all(a is b for a, b in zip(got, out))
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    keys.copy_(torch.randn(n, device="cuda", generator=g))
    mask.copy_(torch.rand(n, device="cuda", generator=g) < 0.5)
    lo.fill_(-0.25)
    graph.replay()
    torch.cuda.synchronize()
    c.check()
    rows, m = compact_reference(n, "f32", keys.cpu().numpy().view(np.uint8), mask.cpu().numpy().view(np.uint8), lo=lo.cpu().numpy().view(np.uint8))
    assert int(out.num) == m and 0 < m < n
    want = np.concatenate([rows, np.full(n - m, -1, dtype=np.int64)])  # the rows behind the count keep their -1
    assert np.array_equal(out.index.cpu().numpy(), want) and np.array_equal(out.values.cpu().numpy(), want.astype(np.int32))
    assert torch.equal(out.keys[:m], keys[torch.from_numpy(rows).cuda()]) and bool((out.keys[m:] == -1.0).all())
    assert (c.get_info(rs.INFO_LAST_PASSES) >> 24) & 0x1F == PATH
    c.close()
