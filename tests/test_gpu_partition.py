"""GPU: rsx_multisplit_device / radix_partition against tests/partition_ref.py.

Every comparison is np.array_equal on all bytes of an allocation the test owns: 64 guard bytes of 0xA5, the array, 64
guard bytes; every output is pre-filled with 0xA5, so a row that is not written, or written where none belongs, shows.  The
key, value and edge columns are compared with their inputs afterwards, and ctx.check() runs after each call.  Sizes come
from partition_caps: S = share, T = tile, E = max_edges."""
import itertools

import numpy as np
import pytest

import util
from bin_ref import INT_DTYPES, bin_reference
from partition_ref import expected_index, expected_rows, partition_reference
from segment_pairs_gpu import guarded, key_tensor, same
from segment_pairs_ref import with_guards
from test_gpu_bin import KEY_TYPES, MODES, make_edges, make_keys

pytestmark = pytest.mark.gpu


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
def caps(rs):
    E, EI, T, S = rs.partition_caps(4)
    assert all(rs.partition_caps(kb) == (E, EI, T, S) for kb in (1, 2, 8, 16))  # one layout for every key width
    return E, EI, T, S


def make_values(n, vb, seed=5):
    return np.random.default_rng(seed).integers(0, 256, n * vb, dtype=np.uint8)


def filled(nbytes):
    return np.full(nbytes, 0xA5, dtype=np.uint8)


def info(rs, c):
    """(path, kernels launched, every other bit) of RSX_INFO_LAST_PASSES"""
    v = c.get_info(rs.INFO_LAST_PASSES)
    return (v >> 24) & 0x1F, v & 0xFF, v & ~((0x1F << 24) | 0xFF)


class Call:
    """One key column (and one value column) on the GPU, guarded, `shift` bytes behind a 16-byte boundary, and the calls
    made on it through Context.multisplit_device on raw pointers."""

    def __init__(self, torch, c, tname, keys_raw, values_raw=None, vb=0, shift=0):
        self.torch, self.c, self.tname = torch, c, tname
        self.kb, self.kind = util.TYPES[tname][2], util.TYPES[tname][3]
        self.keys_raw = np.ascontiguousarray(keys_raw).view(np.uint8).reshape(-1)
        self.n = self.keys_raw.size // self.kb
        self.shift = shift if self.n else 0  # (an empty view has no address to be aligned)
        self.kbuf, self.kmid = guarded(torch, self.keys_raw, self.shift)
        self.vb, self.values_raw = vb, values_raw
        if vb:
            self.vshift = (vb & -vb) if self.shift else 0  # one value's own alignment behind the boundary
            self.vbuf, self.vmid = guarded(torch, values_raw, self.vshift)

    def run(self, edges, mode, desc=False, outs="kvi", ib=8, num=None, status=None):
        """-> {"k" / "v" / "i" / "o": the whole allocation of that output as numpy bytes}.  edges: the raw edge bytes, or m
        itself in the index mode.  outs: the row outputs that are asked for."""
        torch, n = self.torch, self.n
        if mode == "index":
            m, emid, ebuf = int(edges), None, None
        else:
            edges = np.ascontiguousarray(edges).view(np.uint8).reshape(-1)
            m = edges.size // self.kb
            ebuf, emid = guarded(torch, edges)
        bufs, ptr = {}, {"k": 0, "v": 0, "i": 0}
        widths = {"k": self.kb, "v": self.vb, "i": ib}
        shifts = {"k": self.shift, "v": self.vshift if self.vb else 0, "i": ib if self.shift else 0}
        for o in outs:
            if widths[o] == 0:
                continue
            bufs[o], mid = guarded(torch, filled(n * widths[o]), shifts[o])
            ptr[o] = mid.data_ptr() if n else 0
        bufs["o"], omid = guarded(torch, filled((m + 2) * 8))
        dnum = torch.tensor([num], dtype=torch.int64, device="cuda") if num is not None else None
        want_v = self.vb and "v" in outs
        args = (self.kmid.data_ptr() if n else 0, n, self.kb, self.kind, emid.data_ptr() if emid is not None and m else 0, m, MODES[mode],
                self.vmid.data_ptr() if want_v and n else 0, self.vb if want_v and n else 0, ptr["k"], ptr["v"], ptr["i"], ib, omid.data_ptr(), desc,
                dnum.data_ptr() if dnum is not None else 0, torch.cuda.current_stream().cuda_stream)
        if status is None:
            self.c.multisplit_device(*args)
            self.c.check()
        else:
            import radix_sort_amd as rs
            with pytest.raises(rs.RsxError) as e:
                self.c.multisplit_device(*args)
            assert e.value.status == status, e.value
            torch.cuda.synchronize()
        if ebuf is not None:
            assert same(ebuf.cpu().numpy(), with_guards(edges), ("the edges", self.tname))
        self.shifts = shifts
        return {o: b.cpu().numpy() for o, b in bufs.items()}

    def expected(self, edges, mode, desc, outs, ib, num):
        perm, offsets = partition_reference(self.keys_raw, edges, self.tname, mode, desc, num)
        want = {"o": offsets.astype("<i8").view(np.uint8)}
        if "k" in outs:
            want["k"] = expected_rows(self.keys_raw, self.kb, perm, self.n)
        if "v" in outs and self.vb:
            want["v"] = expected_rows(self.values_raw, self.vb, perm, self.n)
        if "i" in outs:
            want["i"] = expected_index(perm, ib, self.n)
        return want

    def check(self, edges, mode, desc=False, outs="kvi", ib=8, num=None, what=None):
        want = self.expected(edges, mode, desc, outs, ib, num)
        got = self.run(edges, mode, desc, outs, ib, num)
        assert sorted(got) == sorted(want)
        for o in want:
            assert same(got[o], with_guards(want[o], self.shifts.get(o, 0)), (o, self.tname, what, mode, desc, outs, ib, num))
        return got

    def inputs_unchanged(self):
        assert same(self.kbuf.cpu().numpy(), with_guards(self.keys_raw, self.shift), ("the key column", self.tname))
        if self.vb:
            assert same(self.vbuf.cpu().numpy(), with_guards(self.values_raw, self.vshift), ("the value column", self.tname))


def test_sizes_around_the_tile_and_the_share(rs, torch, ctx, caps):
    E, _EI, T, S = caps
    for n in (0, 1, 15, 16, 17, T - 1, T, T + 1, S - 1, S, S + 1, 3 * S + 5):
        call = Call(torch, ctx, "u32", make_keys("u32", n, n), make_values(n, 4), 4)
        edges = make_edges("u32", 5, 3, False)
        call.check(edges, "upper", what=n)
        path, launched, rest = info(rs, ctx)
        assert (path, launched, rest) == (18, 4 if n else 3, 0), (n, path, launched, rest)
        call.check(edges, "lower", desc=False, outs="i", ib=4, what=n)
        call.inputs_unchanged()


def test_capped_grid_with_long_ragged_shares(rs, torch, ctx, caps):
    _E, _EI, T, S = caps
    n = 2 * ctx.get_info(rs._lib.INFO_NUM_CU) * S + T + 3  # the smallest size with a capped grid and shares longer than S
    call = Call(torch, ctx, "u32", make_keys("u32", n, 1), make_values(n, 4), 4)
    call.check(make_edges("u32", 64, 3, False), "upper", what="capped grid")
    call.inputs_unchanged()


@pytest.mark.parametrize("mode,desc", [("upper", False), ("lower", True)])
def test_numbers_of_edges(torch, ctx, caps, mode, desc):
    E, _EI, T, S = caps
    n = S + T + 17
    keys = make_keys("u32", n, 2, spread=600)
    call = Call(torch, ctx, "u32", keys, make_values(n, 8), 8)
    for m in (0, 1, 2, 63, 64, 65, E):
        edges = make_edges("u32", m, m, desc, spread=600).view("<u4").copy()
        if m >= 2:
            edges[1] = edges[0]  # duplicate edges (still sorted): an empty bin
        edges = edges.view(np.uint8)
        call.check(edges, mode, desc, what=m)
    call.inputs_unchanged()


@pytest.mark.parametrize("tname", KEY_TYPES)
def test_key_types(torch, ctx, caps, tname):
    _E, _EI, T, S = caps
    n = S + T + 5
    call = Call(torch, ctx, tname, make_keys(tname, n, 4), make_values(n, 4), 4)
    for mode, desc in (("upper", False), ("upper", True), ("lower", False), ("lower", True)):
        call.check(make_edges(tname, 7, 9, desc), mode, desc)
    if tname in INT_DTYPES:
        raw = np.random.default_rng(6).integers(-3, 12, n).astype(INT_DTYPES[tname])  # (unsigned: the negative ones wrap to large ids)
        icall = Call(torch, ctx, tname, raw.view(np.uint8), make_values(n, 4), 4)
        icall.check(8, "index")
        icall.inputs_unchanged()
    call.inputs_unchanged()


def test_index_mode_ids_outside(torch, ctx, caps):
    _E, EI, T, S = caps
    n = S + 77
    rng = np.random.default_rng(8)
    for tname, m in (("i32", 1), ("i64", 8), ("u32", 256), ("i32", EI), ("u8", 200), ("i16", EI)):
        dt = np.dtype(INT_DTYPES[tname])
        lo, hi = max(np.iinfo(dt).min, -m - 2), min(np.iinfo(dt).max, 2 * m + 2)
        v = rng.integers(lo, hi, n, endpoint=True).astype(dt)
        v[:3] = [np.iinfo(dt).min, np.iinfo(dt).max, 0]
        call = Call(torch, ctx, tname, v.view(np.uint8), make_values(n, 4), 4)
        call.check(m, "index", what=(tname, m))
        call.inputs_unchanged()
    v = np.full(n, -1, dtype="<i4")  # every id outside: the last bin holds all rows
    v[::2] = 1 << 20
    got = Call(torch, ctx, "i32", v.view(np.uint8)).check(64, "index", outs="ki")
    off = got["o"][64:-64].view("<i8")
    assert off[64] == 0 and off[65] == n
    # float and 128-bit keys have no index mode
    import radix_sort_amd as rs
    Call(torch, ctx, "f32", make_keys("f32", 40, 1)).run(4, "index", status=rs._lib.ERR_UNSUPPORTED)
    Call(torch, ctx, "u128", make_keys("u128", 40, 1)).run(4, "index", status=rs._lib.ERR_UNSUPPORTED)


def test_key_distributions(torch, ctx, caps):
    E, EI, T, S = caps
    n = S + T + 129
    i = np.arange(n)
    cases = {
        "one bin": np.full(n, 5),
        "cycling through 64 bins": i % 64,          # every wave round holds 64 different bins
        "cycling through all bins": i % (EI + 1),
        "sorted": np.sort(i * 7919 % 200),
        "reversed": np.sort(i * 7919 % 200)[::-1],
        "runs of 64": i // 64 % 50,                 # the wave-match edge: one bin per round ...
        "runs of 65": i // 65 % 50,                 # ... and a run that straddles two rounds
    }
    for what, ids in cases.items():
        m = EI if "all bins" in what else 63 if "64 bins" in what else 255
        call = Call(torch, ctx, "i32", ids.astype("<i4").view(np.uint8), make_values(n, 4), 4)
        call.check(m, "index", what=what)
        # the same bins through the edge search: with the edges 1 .. m, an id in 0 .. m has that many edges <= it
        edges = np.arange(1, m + 1, dtype="<i4").view(np.uint8)
        call.check(edges, "upper", what=what)
        call.inputs_unchanged()


@pytest.mark.parametrize("vb", [1, 2, 4, 8, 16, 3, 12, 24])
def test_value_widths(rs, torch, ctx, caps, vb):
    _E, _EI, T, S = caps
    n = S + T + 9
    call = Call(torch, ctx, "i32", make_keys("i32", n, 3), make_values(n, vb), vb)
    edges = make_edges("i32", 12, 3, False)
    fused = vb in (1, 2, 4, 8, 16)
    call.check(edges, "upper", outs="kvi", ib=8)
    assert info(rs, ctx) == (18, 4 if fused else 5, 0)
    call.check(edges, "upper", outs="kvi", ib=4)
    call.check(edges, "lower", outs="kv")          # the gather route: positions in the workspace
    assert info(rs, ctx) == (18, 4 if fused else 5, 0)
    call.check(edges, "upper", outs="v", num=n - 100)  # ... bounded by N on the device
    call.inputs_unchanged()


def test_every_subset_of_the_outputs(rs, torch, ctx, caps):
    _E, _EI, T, S = caps
    n = S + 3
    call = Call(torch, ctx, "f32", make_keys("f32", n, 3), make_values(n, 8), 8)
    edges = make_edges("f32", 9, 3, False)
    for r in range(4):
        for outs in itertools.combinations("kvi", r):
            call.check(edges, "upper", outs="".join(outs), ib=4 if r == 2 else 8)
            assert info(rs, ctx) == (18, 4 if outs else 3, 0)
    # no row output: the offsets are the exclusive sums of the bin counts
    got = call.run(edges, "lower", outs="")
    counts = bin_reference(call.keys_raw, edges, "f32", "lower")
    assert np.array_equal(np.diff(got["o"][64:-64].view("<i8")), counts)
    call.inputs_unchanged()


def test_device_row_count(torch, ctx, caps):
    _E, _EI, T, S = caps
    n = 2 * S + 11
    call = Call(torch, ctx, "i64", make_keys("i64", n, 3), make_values(n, 4), 4)
    edges = make_edges("i64", 20, 3, True)
    for num in (0, 1, T + 1, S, n - 1, n, n + 5, 1 << 40):
        got = call.check(edges, "upper", True, num=num, what=num)  # rows from N on stay 0xA5
        assert got["o"][64:-64].view("<i8")[-1] == min(n, num)
    call.inputs_unchanged()


@pytest.mark.parametrize("tname", ["u8", "i16", "u32", "f64", "u128"])
def test_bases_one_key_behind_a_boundary(torch, ctx, caps, tname):
    _E, _EI, T, S = caps
    n = S + T + 21
    kb = util.TYPES[tname][2]
    call = Call(torch, ctx, tname, make_keys(tname, n, 3), make_values(n, 4), 4, shift=kb)
    call.check(make_edges(tname, 6, 3, False), "upper", ib=4)
    call.check(make_edges(tname, 6, 3, False), "lower", ib=8)
    call.inputs_unchanged()


def test_unsorted_edges_still_permute_the_rows(torch, ctx, caps):
    E, _EI, T, S = caps
    n = S + T + 33
    keys = make_keys("u32", n, 3, spread=600)
    for m, num in ((9, None), (E, None), (200, n - 1000)):
        N = n if num is None else num
        edges = make_keys("u32", max(m, 16), 55, spread=600).view("<u4")[:m]  # as drawn: not sorted
        assert np.any(np.diff(edges.astype(np.int64)) < 0)
        call = Call(torch, ctx, "u32", keys, make_values(n, 4), 4)
        got = call.run(edges.view(np.uint8), "upper", num=num)
        off = got["o"][64:-64].view("<i8")
        assert off[0] == 0 and off[m + 1] == N and np.all(np.diff(off) >= 0)
        index = got["i"][64:-64].view("<i8")
        assert np.array_equal(np.sort(index[:N]), np.arange(N))  # every one of the N rows exactly once
        assert same(got["k"], with_guards(expected_rows(keys, 4, index[:N], n)), "keys follow the index")
        assert same(got["v"], with_guards(expected_rows(call.values_raw, 4, index[:N], n)), "values follow the index")
        assert same(got["i"], with_guards(expected_index(index[:N], 8, n)), "nothing behind N")
        call.inputs_unchanged()


def test_more_edges_than_the_caps(rs, torch, ctx, caps):
    E, EI, T, S = caps
    n = 5000
    keys = make_keys("i32", n, 3, spread=3000)
    vals = make_values(n, 12)
    edges = make_edges("i32", E + 1, 3, False, spread=3000)
    call = Call(torch, ctx, "i32", keys, vals, 12)
    got = call.run(edges, "upper", status=rs._lib.ERR_UNSUPPORTED)
    assert all(np.all(b == 0xA5) for b in got.values())  # nothing was enqueued
    ids = np.random.default_rng(3).integers(-5, EI + 40, n).astype("<i4")
    got = Call(torch, ctx, "i32", ids.view(np.uint8)).run(EI + 1, "index", status=rs._lib.ERR_UNSUPPORTED)
    assert all(np.all(b == 0xA5) for b in got.values())
    # radix_partition takes the chain through searchsorted, argsort and gathers: the same result
    k = torch.from_numpy(keys.view("<i4").copy()).cuda()
    v = torch.from_numpy(vals.reshape(n, 3, 4).copy()).cuda()
    e = torch.from_numpy(edges.view("<i4").copy()).cuda()
    for side, mode in (("right", "upper"), ("left", "lower")):
        out = rs.radix_partition(k, edges=e, values=v, side=side, return_index=True, ctx=ctx)
        ctx.check()
        perm, offsets = partition_reference(keys, edges, "i32", mode)
        assert np.array_equal(out.offsets.cpu().numpy(), offsets) and np.array_equal(out.index.cpu().numpy(), perm)
        assert np.array_equal(out.keys.cpu().numpy(), keys.view("<i4")[perm]) and np.array_equal(out.values.cpu().numpy().reshape(n, 12), vals.reshape(n, 12)[perm])
    t = torch.from_numpy(ids.copy()).cuda()
    num = torch.tensor([n - 700], dtype=torch.int64, device="cuda")
    pre = rs.Partitioned(torch.full((n,), -7, dtype=torch.int32, device="cuda"), None, torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                         torch.full((EI + 3,), -7, dtype=torch.int64, device="cuda"))
    out = rs.radix_partition(t, num_bins=EI + 1, num=num, out=pre, ctx=ctx)
    ctx.check()
    perm, offsets = partition_reference(ids.view(np.uint8), EI + 1, "i32", "index", num=n - 700)
    assert np.array_equal(out.offsets.cpu().numpy(), offsets)
    assert np.array_equal(out.index.cpu().numpy(), np.concatenate([perm, np.full(700, -7)]))
    assert np.array_equal(out.keys.cpu().numpy(), np.concatenate([ids[perm], np.full(700, -7)]))


def test_two_calls_give_equal_bytes(torch, ctx, caps):
    E, _EI, T, S = caps
    n = 3 * S + T + 1
    call = Call(torch, ctx, "u64", make_keys("u64", n, 3, spread=900), make_values(n, 16), 16)
    edges = make_edges("u64", E, 3, False, spread=900)
    a = call.check(edges, "upper")
    b = call.run(edges, "upper")
    assert all(np.array_equal(a[o], b[o]) for o in a)


def test_python_layer(rs, torch, ctx, caps):
    _E, _EI, T, S = caps
    n = S + T + 3
    keys_raw, vals = make_keys("f32", n, 3), make_values(n, 12)
    edges_raw = make_edges("f32", 11, 3, True)
    k = torch.from_numpy(keys_raw.view("<f4").copy()).cuda()
    e = torch.from_numpy(edges_raw.view("<f4").copy()).cuda()
    v = torch.from_numpy(vals.reshape(n, 3, 4).copy()).cuda()
    perm, offsets = partition_reference(keys_raw, edges_raw, "f32", "lower", True)
    out = rs.radix_partition(k, edges=e, values=v, side="left", descending=True, return_index=True, index_dtype=torch.int32, ctx=ctx)
    ctx.check()
    assert out.offsets.dtype == torch.int64 and out.index.dtype == torch.int32 and out.values.shape == v.shape
    assert np.array_equal(out.offsets.cpu().numpy(), offsets) and np.array_equal(out.index.cpu().numpy(), perm)
    assert np.array_equal(out.keys.cpu().numpy().view("<u4"), keys_raw.view("<u4")[perm])
    assert np.array_equal(out.values.cpu().numpy().reshape(n, 12), vals.reshape(n, 12)[perm])
    assert np.array_equal(k.cpu().numpy().view(np.uint8), keys_raw)
    plain = rs.radix_partition(k, edges=e, ctx=ctx)  # defaults: keys and offsets only
    assert plain.values is None and plain.index is None and plain.keys.shape == k.shape
    # out=: the given tensors come back; None fields are left out
    pre = rs.Partitioned(None, torch.empty_like(v), torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(13, dtype=torch.int64, device="cuda"))
    got = rs.radix_partition(k, edges=e, values=v, side="left", descending=True, out=pre, ctx=ctx)
    ctx.check()
    assert all(a is b for a, b in zip(got, pre))
    assert np.array_equal(got.index.cpu().numpy(), perm) and np.array_equal(got.values.cpu().numpy().reshape(n, 12), vals.reshape(n, 12)[perm])
    # the index mode, 128-bit keys, an empty input
    ids = torch.from_numpy(np.random.default_rng(1).integers(-2, 9, n).astype("<i8")).cuda()
    got = rs.radix_partition(ids, num_bins=8, return_index=True, ctx=ctx)
    perm, offsets = partition_reference(ids.cpu().numpy().view(np.uint8), 8, "i64", "index")
    assert np.array_equal(got.offsets.cpu().numpy(), offsets) and np.array_equal(got.index.cpu().numpy(), perm)
    wide = make_keys("u128", 300, 2)
    wedges = make_edges("u128", 5, 2, False)
    got = rs.radix_partition(torch.from_numpy(wide.reshape(-1, 16).copy()).cuda(), edges=torch.from_numpy(wedges.reshape(-1, 16).copy()).cuda(), ctx=ctx)
    perm, offsets = partition_reference(wide, wedges, "u128", "upper")
    assert np.array_equal(got.offsets.cpu().numpy(), offsets) and np.array_equal(got.keys.cpu().numpy(), wide.reshape(-1, 16)[perm])
    got = rs.radix_partition(k[:0], edges=e, return_index=True, ctx=ctx)
    assert got.keys.numel() == 0 and got.index.numel() == 0 and got.offsets.tolist() == [0] * 13
    ctx.check()
    # dtype and shape errors on device tensors
    with pytest.raises(TypeError, match="dtype"):
        rs.radix_partition(k, edges=e.double(), ctx=ctx)
    with pytest.raises(ValueError, match="out.offsets"):
        rs.radix_partition(k, edges=e, out=rs.Partitioned(None, None, None, torch.empty(12, dtype=torch.int64, device="cuda")), ctx=ctx)
    with pytest.raises(ValueError, match="shape"):
        rs.radix_partition(k, edges=e, out=rs.Partitioned(torch.empty(n + 1, device="cuda"), None, None, pre.offsets), ctx=ctx)
    with pytest.raises(ValueError, match="same device"):
        rs.radix_partition(k, edges=e.cpu(), ctx=ctx)
    with pytest.raises(rs.RsxError):  # an output that is an input
        rs.radix_partition(k, edges=e, out=rs.Partitioned(k, None, None, pre.offsets), ctx=ctx)
    ctx.check()


def test_composition_with_quantile_cuts_and_segment_sort(rs, torch, ctx, caps):
    _E, _EI, T, S = caps
    n = 4 * S + 77
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    keys = torch.randint(-(1 << 30), 1 << 30, (n,), dtype=torch.int32, device="cuda", generator=g)
    cuts = rs.radix_quantile(keys, [i / 16 for i in range(1, 16)], ctx=ctx).reshape(-1)  # 15 cuts, left on the device, sorted
    out = rs.radix_partition(keys, edges=cuts, ctx=ctx)
    assert torch.equal(out.offsets[1:] - out.offsets[:-1], rs.radix_histogram(keys, cuts, ctx=ctx))
    bucketed = out.keys.clone()
    rs.radix_sort_segments(bucketed, out.offsets, ctx=ctx)
    whole = keys.clone()
    rs.radix_sort(whole, ctx=ctx)
    ctx.check()
    assert torch.equal(bucketed, whole)  # the bucketing step of a sample sort


def test_graph_capture(rs, torch):
    """out= after reserve_multisplit allocates nothing: one captured call, one linear chain, replayed twice on changed
    inputs.  Without the reserve on a fresh context: RSX_ERR_WORKSPACE, nothing enqueued."""
    _E, _EI, T, S = rs.partition_caps(4)
    n = 3 * S + T + 5
    m = 40
    s = torch.cuda.Stream()
    keys = torch.zeros(n, dtype=torch.int32, device="cuda")
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    num = torch.full((1,), n, dtype=torch.int64, device="cuda")
    out = rs.Partitioned(torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda"),
                         torch.full((n,), -1, dtype=torch.int64, device="cuda"), torch.full((m + 2,), -1, dtype=torch.int64, device="cuda"))

    def enqueue(c):
        return rs.radix_partition(keys, num_bins=m, values=vals, num=num, out=out, ctx=c)

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
    c.reserve_multisplit(n, m, 4, 4, 8)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        got = enqueue(c)
    assert all(a is b for a, b in zip(got, out))
    g = torch.Generator(device="cuda")
    for seed, rows in ((1, n), (2, n - 999)):
        g.manual_seed(seed)
        keys.copy_(torch.randint(-3, m + 5, (n,), dtype=torch.int32, device="cuda", generator=g))
        num.fill_(rows)
        for t in out:
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        perm, offsets = partition_reference(keys.cpu().numpy().view(np.uint8), m, "i32", "index", num=rows)
        tail = np.full(n - rows, -1)
        assert np.array_equal(out.offsets.cpu().numpy(), offsets)
        assert np.array_equal(out.index.cpu().numpy(), np.concatenate([perm, tail]))
        assert np.array_equal(out.keys.cpu().numpy(), np.concatenate([keys.cpu().numpy()[perm], tail]))
        assert np.array_equal(out.values.cpu().numpy(), np.concatenate([perm, tail]))
    c.close()
