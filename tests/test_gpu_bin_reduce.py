"""GPU: rsx_bin_reduce_device / radix_bin_reduce against tests/bin_reduce_ref.py.

Every comparison is np.array_equal on all bytes of an allocation the test owns: 64 guard bytes of 0xA5, the array, 64
guard bytes; every output is pre-filled with 0xA5 unless a test accumulates, so an entry that is not written shows.  The
key, value and edge columns are compared with their inputs afterwards, and ctx.check() runs after each call.  Sizes come
from bin_reduce_caps: E = max_edges, EI = max_index_bins, T = tile, S = share.

The comparisons are exact because integer sums wrap, minima and maxima do not depend on an order, and the float sums of
these tests add values that are integers in [-8, 8]: with at most 2^20 rows (2^24 of f64) every partial sum is exactly
representable, so every association gives the same bytes.  General floats are held to the order-free bound."""
import numpy as np
import pytest

import util
from bin_reduce_ref import accumulate_reference, bin_reduce_reference, identity_bits
from reduce_ref import FLOAT, MAX, MIN, SIGNED, SUM, UNSIGNED, value_dtype
from segment_pairs_gpu import guarded, same
from segment_pairs_ref import with_guards
from test_gpu_bin import F32_SPECIALS, F64_SPECIALS, KEY_TYPES, MODES, count_bytes_of, make_edges, make_keys

pytestmark = pytest.mark.gpu

VALUE_TYPES = {"u32": (4, UNSIGNED), "i32": (4, SIGNED), "f32": (4, FLOAT), "u64": (8, UNSIGNED), "i64": (8, SIGNED), "f64": (8, FLOAT)}
OPS = {"sum": SUM, "min": MIN, "max": MAX}


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
    return rs.bin_reduce_caps(4, 4)  # (E, EI, T, S) of u32 keys with 4-byte values


def make_values(vname, n, seed=5, wide=False):
    """n values as raw bytes: integers in [-8, 8] (floats: exactly those; unsigned: 0 .. 16), or with `wide` integers over
    the whole width, so that sums wrap and the sign takes part."""
    vb, vkind = VALUE_TYPES[vname]
    rng = np.random.default_rng(seed)
    dt = value_dtype(vb, vkind)
    if wide and vkind != FLOAT:
        return rng.integers(0, 256, n * vb, dtype=np.uint8)
    lo, hi = (0, 17) if vkind == UNSIGNED else (-8, 9)
    return rng.integers(lo, hi, n).astype(dt).view(np.uint8)


def special_values(vname, n, seed=5):
    """float bit patterns with +-NaN, +-0.0, +-inf and denormals among ordinary values"""
    vb, _ = VALUE_TYPES[vname]
    rng = np.random.default_rng(seed)
    v = (rng.integers(-40, 41, n) / 4.0).astype("<f4" if vb == 4 else "<f8")
    raw = v.view("<u4" if vb == 4 else "<u8").copy()
    sp = F32_SPECIALS if vb == 4 else F64_SPECIALS
    where = rng.integers(0, n, max(n // 7, min(n, 2 * sp.size)))
    raw[where] = sp[rng.integers(0, sp.size, where.size)]
    return raw.view(np.uint8)


def filled(nbytes):
    return np.full(nbytes, 0xA5, dtype=np.uint8)


def info(rs, c):
    """(path, kernels launched, every other bit) of RSX_INFO_LAST_PASSES"""
    v = c.get_info(rs.INFO_LAST_PASSES)
    return (v >> 24) & 0x1F, v & 0xFF, v & ~((0x1F << 24) | 0xFF)


class Call:
    """One key column and one value column on the GPU, guarded, `shift` elements behind a 16-byte boundary, and the calls
    made on them through Context.bin_reduce_device on raw pointers."""

    def __init__(self, torch, c, tname, keys_raw, vname, values_raw, shift=0):
        self.torch, self.c, self.tname, self.vname = torch, c, tname, vname
        self.kb, self.kind = util.TYPES[tname][2], util.TYPES[tname][3]
        self.vb, self.vkind = VALUE_TYPES[vname]
        self.keys_raw = np.ascontiguousarray(keys_raw).view(np.uint8).reshape(-1)
        self.values_raw = np.ascontiguousarray(values_raw).view(np.uint8).reshape(-1)
        self.n = self.values_raw.size // self.vb
        assert self.keys_raw.size == self.n * self.kb
        self.kshift = shift * self.kb % 16 if self.n else 0  # (an empty view has no address to be aligned)
        self.vshift = shift * self.vb % 16 if self.n else 0
        self.kbuf, self.kmid = guarded(torch, self.keys_raw, self.kshift)
        self.vbuf, self.vmid = guarded(torch, self.values_raw, self.vshift)

    def run(self, edges, mode, op, desc=False, cb=8, num=None, initial=None, initial_counts=None, accumulate=False, status=None, c=None):
        """-> (the values allocation, the counts allocation or None) as numpy bytes.  edges: the raw edge bytes, or m
        itself in the index mode.  cb: 0 for no counts.  initial, initial_counts: the outputs before the call (default:
        0xA5 bytes)."""
        torch, n = self.torch, self.n
        c = self.c if c is None else c
        if mode == "index":
            m, emid, ebuf = int(edges), None, None
        else:
            edges = np.ascontiguousarray(edges).view(np.uint8).reshape(-1)
            m = edges.size // self.kb
            ebuf, emid = guarded(torch, edges)
        obuf, omid = guarded(torch, filled((m + 1) * self.vb) if initial is None else initial)
        cbuf = cmid = None
        if cb:
            cbuf, cmid = guarded(torch, filled((m + 1) * cb) if initial_counts is None else count_bytes_of(initial_counts, cb))
        dnum = torch.tensor([num], dtype=torch.int64, device="cuda") if num is not None else None
        args = (self.kmid.data_ptr() if n else 0, self.vmid.data_ptr() if n else 0, n, self.kb, self.kind,
                emid.data_ptr() if emid is not None and m else 0, m, MODES[mode], self.vb, self.vkind, OPS[op], omid.data_ptr(),
                cmid.data_ptr() if cb else 0, cb or 8, desc, dnum.data_ptr() if dnum is not None else 0, 1 if accumulate else 0,
                torch.cuda.current_stream().cuda_stream)
        if status is None:
            c.bin_reduce_device(*args)
            c.check()
        else:
            import radix_sort_amd as rs
            with pytest.raises(rs.RsxError) as e:
                c.bin_reduce_device(*args)
            assert e.value.status == status, e.value
            torch.cuda.synchronize()
        if ebuf is not None:
            assert same(ebuf.cpu().numpy(), with_guards(edges), ("the edges", self.tname))
        return obuf.cpu().numpy(), cbuf.cpu().numpy() if cb else None

    def reference(self, edges, mode, op, desc=False, num=None):
        r = bin_reduce_reference(self.keys_raw, edges, self.tname, mode, self.values_raw, self.vb, self.vkind, OPS[op], desc, num)
        return (r.exact if r.values is None else r.values), r.counts

    def check(self, edges, mode, op, desc=False, cb=8, num=None, what=None):
        want, counts = self.reference(edges, mode, op, desc, num)
        got, got_counts = self.run(edges, mode, op, desc, cb, num)
        tag = (self.tname, self.vname, what, mode, op, desc, cb, num)
        assert same(got, with_guards(want), ("values",) + tag)
        if cb:
            assert same(got_counts, with_guards(count_bytes_of(counts, cb)), ("counts",) + tag)
        return want, counts

    def inputs_unchanged(self):
        assert same(self.kbuf.cpu().numpy(), with_guards(self.keys_raw, self.kshift), ("the key column", self.tname))
        assert same(self.vbuf.cpu().numpy(), with_guards(self.values_raw, self.vshift), ("the value column", self.vname))


def test_sizes_around_the_tile_and_the_share(rs, torch, ctx, caps):
    _E, _EI, T, S = caps
    assert rs.bin_reduce_caps(4, 8)[2:] == (T, S)
    edges = make_edges("u32", 5, 3, False)
    for n in (0, 1, 63, 64, 65, T - 1, T, T + 1, S - 1, S, S + 1, 3 * S + 5):
        keys = make_keys("u32", n, n)
        for vname in ("f32", "i64"):
            call = Call(torch, ctx, "u32", keys, vname, make_values(vname, n, n + 1))
            call.check(edges, "upper", "sum", what=n)
            path, launched, rest = info(rs, ctx)
            assert (path, launched, rest) == (19, 2 if n else 1, 0), (n, path, launched, rest)
            call.check(edges, "lower", "sum", cb=0, what=n)
            call.check(edges, "upper", "sum", cb=4, what=n)
            call.check(edges, "lower", "max", cb=0, what=n)
            call.inputs_unchanged()


def test_capped_grid(rs, torch, ctx, caps):
    _E, _EI, T, S = caps
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    n = 2 * cus * S + T + 3  # more shares than workgroups: every workgroup walks more than S rows
    call = Call(torch, ctx, "u32", make_keys("u32", n, 1), "f64", make_values("f64", n, 2))
    call.check(make_edges("u32", 5, 3, False), "upper", "sum")
    call.inputs_unchanged()


def test_numbers_of_edges(rs, torch, ctx, caps):
    _E, _EI, T, S = caps
    n = S + T + 17
    keys = make_keys("u32", n, 9, spread=1500)
    for vname, op in (("f32", "sum"), ("i64", "min")):
        E = rs.bin_reduce_caps(4, VALUE_TYPES[vname][0])[0]  # (the cap depends on the value's width)
        call = Call(torch, ctx, "u32", keys, vname, make_values(vname, n, 4, wide=True))
        for m in (0, 1, 2, 63, 64, 65, E - 1, E):
            call.check(make_edges("u32", m, m, False, spread=1500), "upper", op, what=m)
            call.check(make_edges("u32", m, m + 1, True, spread=1500), "lower", op, desc=True, cb=4, what=m)
        equal = np.repeat(make_edges("u32", 4, 2, False, spread=1500).view("<u4"), 5).view(np.uint8)  # runs of equal edges: empty bins
        want, counts = call.check(equal, "upper", op, what="equal")
        assert (counts == 0).sum() >= 16
        call.inputs_unchanged()
    # unsorted edges: an unspecified grouping, but every row is counted once and nothing is written outside
    call = Call(torch, ctx, "u32", keys, "i32", make_values("i32", n, 4))
    unsorted = np.random.default_rng(3).permutation(make_edges("u32", 200, 5, False, spread=1500).view("<u4")).view(np.uint8)
    got, got_counts = call.run(unsorted, "upper", "sum")
    guard = filled(64)
    assert np.array_equal(got[:64], guard) and np.array_equal(got[-64:], guard)
    assert np.array_equal(got_counts[:64], guard) and np.array_equal(got_counts[-64:], guard)
    assert got_counts[64:-64].view("<i8").sum() == n and (got_counts[64:-64].view("<i8") >= 0).all()
    assert got[64:-64].view("<i4").sum() == call.values_raw.view("<i4").sum()
    call.inputs_unchanged()


@pytest.mark.parametrize("tname", KEY_TYPES)
def test_every_key_type(torch, ctx, caps, tname):
    _E, _EI, T, S = caps
    n = S + 333
    keys = make_keys(tname, n, 11)
    call = Call(torch, ctx, tname, keys, "f32", make_values("f32", n, 12))
    wide = Call(torch, ctx, tname, keys, "u64", make_values("u64", n, 13, wide=True))
    for desc in (False, True):
        edges = make_edges(tname, 9, 5, desc)
        call.check(edges, "upper", "sum", desc)
        call.check(edges, "lower", "min", desc, cb=4)
        wide.check(edges, "lower", "sum", desc)
        wide.check(edges, "upper", "max", desc, cb=0)
    if tname not in ("f32", "f64", "u128"):
        for m in (0, 1, 7, 50):
            call.check(m, "index", "sum", what=m)
            wide.check(m, "index", "min", cb=4, what=m)
    call.inputs_unchanged()
    wide.inputs_unchanged()


@pytest.mark.parametrize("vname", list(VALUE_TYPES))
@pytest.mark.parametrize("op", list(OPS))
def test_every_value_type_and_operator(torch, ctx, caps, vname, op):
    _E, _EI, T, S = caps
    n = S + T + 41
    vkind = VALUE_TYPES[vname][1]
    keys = make_keys("i32", n, 21)
    if vkind == FLOAT and op != "sum":
        values = special_values(vname, n)  # +-NaN, +-0.0, +-inf, denormals: the total order on bit patterns
    else:
        values = make_values(vname, n, 22, wide=vkind != FLOAT)
    call = Call(torch, ctx, "i32", keys, vname, values)
    call.check(make_edges("i32", 13, 5, False), "upper", op)
    call.check(make_edges("i32", 64, 6, True), "lower", op, desc=True, cb=4)
    call.check(0, "index", op)
    call.inputs_unchanged()


def test_index_mode_with_ids_outside(torch, ctx, caps):
    _E, EI, T, S = caps
    n = S + T + 5
    rng = np.random.default_rng(4)
    for tname, dt in (("i32", "<i4"), ("i64", "<i8"), ("u32", "<u4"), ("u8", "<u1")):
        lo = -20 if dt[1] == "i" else 0
        ids = rng.integers(lo, 120, n).astype(dt)
        if dt[1] == "i":
            ids[::97] = np.iinfo(dt).min
        ids[::89] = np.iinfo(dt).max
        call = Call(torch, ctx, tname, ids.view(np.uint8), "f32", make_values("f32", n, 6))
        for m in (1, 8, 64, 100, 119, 120, 121, EI):
            call.check(m, "index", "sum", what=m)
        call.check(100, "index", "max", cb=4)
        call.inputs_unchanged()


def test_distributions(torch, ctx, caps):
    E, EI, T, S = caps
    n = 2 * S + T + 29
    i = np.arange(n)
    shapes = {
        "one bin": np.full(n, 37),
        "every lane of a round in another bin": i % 64,
        "two bins alternating": (i & 1) * 40 + 3,
        "sorted": np.sort(np.random.default_rng(2).integers(0, 1000, n)),
        "runs that end inside a round": (i // 100) % 50,
        "spread over every bin": np.random.default_rng(3).integers(0, EI, n),
    }
    for what, ids in shapes.items():
        ids = ids.astype("<i4")
        for vname, op in (("f32", "sum"), ("i64", "sum"), ("f64", "max")):
            call = Call(torch, ctx, "i32", ids.view(np.uint8), vname, make_values(vname, n, 8))
            call.check(EI, "index", op, what=what)
            call.check(64, "index", op, cb=4, what=what)
            edges = (np.arange(0, 1000, 10)).astype("<i4").view(np.uint8)
            call.check(edges, "upper", op, what=what)
            call.inputs_unchanged()


@pytest.mark.parametrize("vname", list(VALUE_TYPES))
def test_empty_bins_hold_the_identity(torch, ctx, vname):
    vb, vkind = VALUE_TYPES[vname]
    n = 3000
    ids = (np.arange(n) % 3 * 4).astype("<i4")  # bins 0, 4 and 8 of 0 .. 10 hold rows
    call = Call(torch, ctx, "i32", ids.view(np.uint8), vname, make_values(vname, n, 3))
    for op in OPS:
        want, counts = call.check(10, "index", op)
        ident = np.array([identity_bits(vb, vkind, OPS[op])], dtype="<u" + str(vb))
        assert (want.view(ident.dtype)[counts == 0] == ident[0]).all() and (counts == 0).sum() == 8
    if vkind == FLOAT:  # a bin of -0.0 alone: a sum starts from +0.0
        values = np.zeros(n, dtype="<f" + str(vb))
        values[ids == 4] = -0.0
        values[ids == 8] = 1.0
        call = Call(torch, ctx, "i32", ids.view(np.uint8), vname, values.view(np.uint8))
        want, _ = call.check(10, "index", "sum")
        assert want.view("<u" + str(vb))[4] == 0 and want.view("<f" + str(vb))[8] == 1000.0
        want, _ = call.check(10, "index", "min")
        assert want.view("<u" + str(vb))[4] == 1 << (8 * vb - 1)  # (the minimum IS the -0.0)


@pytest.mark.parametrize("vname", list(VALUE_TYPES))
def test_accumulate(torch, ctx, caps, vname):
    _E, _EI, T, S = caps
    vb, vkind = VALUE_TYPES[vname]
    n = S + 77
    keys = make_keys("u32", n, 31)
    edges = make_edges("u32", 12, 5, False)
    call = Call(torch, ctx, "u32", keys, vname, make_values(vname, n, 32))
    initial = make_values(vname, 13, 33)
    counts0 = np.arange(13) * 1000 - 3000
    for op in OPS:
        r, counts = call.reference(edges, "upper", op)
        got, got_counts = call.run(edges, "upper", op, cb=4, initial=initial, initial_counts=counts0, accumulate=True)
        assert same(got, with_guards(accumulate_reference(initial, r, vb, vkind, OPS[op])), ("accumulated values", vname, op))
        assert same(got_counts, with_guards(count_bytes_of(counts0 + counts, 4)), ("accumulated counts", vname, op))
        # no rows: the outputs stay as they are, bit for bit (a -0.0 too)
        start = initial.copy()
        start[:vb] = np.array([1 << (8 * vb - 1)], dtype="<u" + str(vb)).view(np.uint8)
        got, got_counts = call.run(edges, "upper", op, cb=8, initial=start, initial_counts=counts0, accumulate=True, num=0)
        assert same(got, with_guards(start), ("no rows", vname, op)) and same(got_counts, with_guards(count_bytes_of(counts0, 8)), ("no rows", vname, op))
    empty = Call(torch, ctx, "u32", keys[:0], vname, initial[:0])
    got, got_counts = empty.run(edges, "upper", "sum", cb=8, initial=start, initial_counts=counts0, accumulate=True)
    assert same(got, with_guards(start), ("n == 0", vname)) and same(got_counts, with_guards(count_bytes_of(counts0, 8)), ("n == 0", vname))
    call.inputs_unchanged()


def test_device_row_count(torch, ctx, caps):
    _E, _EI, T, S = caps
    n = 2 * S + T + 9
    call = Call(torch, ctx, "i64", make_keys("i64", n, 41), "i32", make_values("i32", n, 42, wide=True))
    edges = make_edges("i64", 20, 5, False)
    for num in (0, 1, 63, S - 1, S + 1, n - 1, n, n + 1, 1 << 40):
        call.check(edges, "upper", "sum", num=num, what=num)
        call.check(edges, "lower", "max", num=num, cb=4, what=num)
    call.inputs_unchanged()


def test_alignment(torch, ctx, caps):
    _E, _EI, T, S = caps
    n = S + T + 3
    for tname, vname in (("u8", "f32"), ("i16", "i64"), ("u32", "f32"), ("f32", "f64"), ("u64", "i32"), ("i64", "f64")):
        call = Call(torch, ctx, tname, make_keys(tname, n, 51), vname, make_values(vname, n, 52), shift=1)  # one element behind a 16-byte boundary
        assert call.kshift == util.TYPES[tname][2] % 16 and call.vshift == VALUE_TYPES[vname][0]
        call.check(make_edges(tname, 9, 5, False), "upper", "sum")
        call.check(make_edges(tname, 9, 5, True), "lower", "min", desc=True, cb=4)
        call.inputs_unchanged()


def test_above_the_caps(rs, torch, ctx):
    n = 1000
    for tname, vname in (("u32", "f32"), ("u64", "f64"), ("u128", "i64")):
        E, EI, _T, _S = rs.bin_reduce_caps(util.TYPES[tname][2], VALUE_TYPES[vname][0])
        call = Call(torch, ctx, tname, make_keys(tname, n, 61), vname, make_values(vname, n, 62))
        call.check(make_edges(tname, E, 5, False, spread=3000), "upper", "sum")
        got, got_counts = call.run(make_edges(tname, E + 1, 5, False, spread=3000), "upper", "sum", status=rs._lib.ERR_UNSUPPORTED)
        assert (got == 0xA5).all() and (got_counts == 0xA5).all()  # nothing was enqueued
        if tname != "u128":
            call.check(EI, "index", "sum")
            got, got_counts = call.run(EI + 1, "index", "sum", status=rs._lib.ERR_UNSUPPORTED)
            assert (got == 0xA5).all() and (got_counts == 0xA5).all()
        call.inputs_unchanged()


@pytest.mark.parametrize("vname", ("f32", "f64"))
def test_general_float_sums_within_the_bound_and_the_same_on_every_call(rs, torch, ctx, caps, vname):
    """Every bin within g(c - 1) * sum|v| of the longdouble sum (reduce_ref's order-free bound); two calls on one context and
    one on a second context give equal bytes."""
    _E, _EI, T, S = caps
    vb = VALUE_TYPES[vname][0]
    n = 3 * S + 5
    rng = np.random.default_rng(71)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4")
    edges = np.sort(rng.integers(0, 1 << 32, 64, dtype=np.uint64)).astype("<u4")
    values = rng.standard_normal(n).astype("<f" + str(vb))
    call = Call(torch, ctx, "u32", keys.view(np.uint8), vname, values.view(np.uint8))
    ref = bin_reduce_reference(keys.view(np.uint8), edges.view(np.uint8), "u32", "upper", values.view(np.uint8), vb, FLOAT, SUM)
    a, counts = call.run(edges.view(np.uint8), "upper", "sum")
    assert same(counts, with_guards(count_bytes_of(ref.counts, 8)), ("counts", vname))
    got = a[64:-64].view("<f" + str(vb)).astype(np.longdouble)
    err = np.abs(got - ref.sums)
    print(vname, "largest error / bound:", float((err / np.maximum(ref.bound, np.finfo(np.longdouble).tiny)).max()), "largest error:", float(err.max()))
    assert (err <= ref.bound).all(), (vname, err, ref.bound)
    b, _ = call.run(edges.view(np.uint8), "upper", "sum")
    other = rs.Context(torch.cuda.current_device())
    c, _ = call.run(edges.view(np.uint8), "upper", "sum", c=other)
    other.close()
    assert np.array_equal(a, b) and np.array_equal(a, c)
    call.inputs_unchanged()


def test_python_layer(rs, torch, ctx, caps):
    _E, _EI, T, S = caps
    n = S + T + 3
    keys_raw, edges_raw = make_keys("f32", n, 3), make_edges("f32", 11, 3, True)
    vals = make_values("f32", n, 4)
    k = torch.from_numpy(keys_raw.view("<f4").copy()).cuda()
    e = torch.from_numpy(edges_raw.view("<f4").copy()).cuda()
    w = torch.from_numpy(vals.view("<f4").copy()).cuda()
    ref = bin_reduce_reference(keys_raw, edges_raw, "f32", "lower", vals, 4, FLOAT, SUM, True)
    got = rs.radix_bin_reduce(k, w, edges=e, side="left", descending=True, ctx=ctx)
    ctx.check()
    assert got.dtype == torch.float32 and got.shape == (12,)
    assert np.array_equal(got.cpu().numpy().view(np.uint8), ref.exact)
    assert np.array_equal(k.cpu().numpy().view(np.uint8), keys_raw) and np.array_equal(w.cpu().numpy().view(np.uint8), vals)
    # radix_histogram(weights=) is the same call; without weights nothing changes
    hist = rs.radix_histogram(k, e, side="left", descending=True, weights=w, ctx=ctx)
    assert np.array_equal(hist.cpu().numpy().view(np.uint8), ref.exact)
    plain = rs.radix_histogram(k, e, side="left", descending=True, ctx=ctx)
    assert plain.dtype == torch.int64 and np.array_equal(plain.cpu().numpy(), ref.counts)
    # return_counts=: the counts of radix_histogram; keys of any shape
    vals2, counts = rs.radix_bin_reduce(k[:n - n % 4].reshape(-1, 4), w[:n - n % 4].reshape(-1, 4), edges=e, op="max", return_counts=True,
                                        count_dtype=torch.int32, side="left", descending=True, ctx=ctx)
    m4 = n - n % 4
    ref4 = bin_reduce_reference(keys_raw[:m4 * 4], edges_raw, "f32", "lower", vals[:m4 * 4], 4, FLOAT, MAX, True)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), ref4.counts)
    assert torch.equal(counts.to(torch.int64), rs.radix_histogram(k[:m4], e, side="left", descending=True, ctx=ctx))
    assert np.array_equal(vals2.cpu().numpy().view(np.uint8), ref4.values)
    # num_bins=, int64 values, radix_bincount(weights=)
    ids_np = np.random.default_rng(1).integers(-2, 9, n).astype("<i8")
    ids = torch.from_numpy(ids_np).cuda()
    iv_np = make_values("i64", n, 5, wide=True)
    iv = torch.from_numpy(iv_np.view("<i8").copy()).cuda()
    refi = bin_reduce_reference(ids_np.view(np.uint8), 8, "i64", "index", iv_np, 8, SIGNED, SUM)
    got = rs.radix_bin_reduce(ids, iv, num_bins=8, ctx=ctx)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy().view(np.uint8), refi.values)
    assert torch.equal(rs.radix_bincount(ids, 8, weights=iv, ctx=ctx), got)
    assert np.array_equal(rs.radix_bincount(ids, 8, ctx=ctx).cpu().numpy(), refi.counts)
    # out= and accumulate=, values and counts; num=
    out = torch.full((9,), 5, dtype=torch.int64, device="cuda")
    cnt = torch.full((9,), 7, dtype=torch.int64, device="cuda")
    num = torch.tensor([n - 700], dtype=torch.int64, device="cuda")
    refn = bin_reduce_reference(ids_np.view(np.uint8), 8, "i64", "index", iv_np, 8, SIGNED, SUM, num=n - 700)
    back = rs.radix_bin_reduce(ids, iv, num_bins=8, num=num, out=(out, cnt), accumulate=True, return_counts=True, ctx=ctx)
    assert back[0] is out and back[1] is cnt
    assert np.array_equal(out.cpu().numpy(), refn.values.view("<i8") + 5) and np.array_equal(cnt.cpu().numpy(), refn.counts + 7)
    back = rs.radix_bincount(ids, 8, weights=iv, out=out, ctx=ctx)
    assert back is out and np.array_equal(out.cpu().numpy().view(np.uint8), refi.values)
    # 128-bit keys, an empty input
    wide = make_keys("u128", 300, 2)
    wedges = make_edges("u128", 5, 2, False)
    wv = make_values("f64", 300, 6)
    got = rs.radix_bin_reduce(torch.from_numpy(wide.reshape(-1, 16).copy()).cuda(), torch.from_numpy(wv.view("<f8").copy()).cuda(),
                              edges=torch.from_numpy(wedges.reshape(-1, 16).copy()).cuda(), op="min", ctx=ctx)
    refw = bin_reduce_reference(wide, wedges, "u128", "upper", wv, 8, FLOAT, MIN)
    assert np.array_equal(got.cpu().numpy().view(np.uint8), refw.values)
    got, counts = rs.radix_bin_reduce(k[:0], w[:0], edges=e, op="min", return_counts=True, ctx=ctx)
    assert got.cpu().numpy().view("<u4").tolist() == [0x7FFFFFFF] * 12 and counts.tolist() == [0] * 12
    ctx.check()
    # dtype, shape and device errors on device tensors
    with pytest.raises(TypeError, match="values must be"):
        rs.radix_bin_reduce(k, w.half(), edges=e, ctx=ctx)
    with pytest.raises(TypeError, match="dtype"):
        rs.radix_bin_reduce(k, w, edges=e.double(), ctx=ctx)
    with pytest.raises(ValueError, match="shape"):
        rs.radix_bin_reduce(k, w, edges=e, out=torch.empty(11, device="cuda"), ctx=ctx)
    with pytest.raises(ValueError, match="same device"):
        rs.radix_bin_reduce(k, w, edges=e.cpu(), ctx=ctx)
    with pytest.raises(ValueError, match="same device"):
        rs.radix_bin_reduce(k, w.cpu(), edges=e, ctx=ctx)
    with pytest.raises(rs.RsxError):  # an output that is an input
        rs.radix_bin_reduce(k[:12], w[:12], edges=e, out=w[:12], ctx=ctx)
    ctx.check()


def test_sorted_route_above_the_caps(rs, torch, ctx, caps):
    """m = E + 1 edges go through radix_searchsorted and radix_reduce_by_key; the first E edges are those of a kernel call,
    whose bins 0 .. E - 1 the two routes share, and bin E of the kernel call is bins E and E + 1 of the other."""
    E, EI, T, S = caps
    n = S + 17
    rng = np.random.default_rng(5)
    keys_np = rng.integers(0, 1 << 20, n).astype("<i4")
    edges_np = np.sort(rng.choice(1 << 20, E + 1, replace=False)).astype("<i4")
    iv_np = make_values("i64", n, 6, wide=True)
    k, e = torch.from_numpy(keys_np).cuda(), torch.from_numpy(edges_np).cuda()
    iv = torch.from_numpy(iv_np.view("<i8").copy()).cuda()
    E8 = rs.bin_reduce_caps(4, 8)[0]  # (the cap depends on the value's width)
    for op, code in OPS.items():
        ref = bin_reduce_reference(keys_np.view(np.uint8), edges_np[:E8 + 1].view(np.uint8), "i32", "upper", iv_np, 8, SIGNED, code)
        got, counts = rs.radix_bin_reduce(k, iv, edges=e[:E8 + 1], op=op, return_counts=True, ctx=ctx)
        assert info(rs, ctx)[0] != 19
        ctx.check()
        assert got.shape == (E8 + 2,) and np.array_equal(got.cpu().numpy().view(np.uint8), ref.values) and np.array_equal(counts.cpu().numpy(), ref.counts)
        kernel = rs.radix_bin_reduce(k, iv, edges=e[:E8], op=op, ctx=ctx)
        assert info(rs, ctx)[0] == 19
        assert torch.equal(kernel[:E8], got[:E8])
    # float sums of exactly representable values, accumulated onto an output; the index mode past its cap
    w_np = make_values("f32", n, 7)
    w = torch.from_numpy(w_np.view("<f4").copy()).cuda()
    ref = bin_reduce_reference(keys_np.view(np.uint8), edges_np.view(np.uint8), "i32", "lower", w_np, 4, FLOAT, SUM)
    out = torch.full((E + 2,), 2.0, dtype=torch.float32, device="cuda")
    rs.radix_bin_reduce(k, w, edges=e, side="left", out=out, accumulate=True, ctx=ctx)
    assert np.array_equal(out.cpu().numpy(), ref.exact.view("<f4") + np.float32(2.0))
    ids_np = rng.integers(-5, EI + 9, n).astype("<i4")
    ids = torch.from_numpy(ids_np).cuda()
    for op, code in OPS.items():
        ref = bin_reduce_reference(ids_np.view(np.uint8), EI + 1, "i32", "index", w_np, 4, FLOAT, code)
        got, counts = rs.radix_bin_reduce(ids, w, num_bins=EI + 1, op=op, return_counts=True, count_dtype=torch.int32, ctx=ctx)
        want = ref.exact if ref.values is None else ref.values
        assert np.array_equal(got.cpu().numpy().view(np.uint8), want) and np.array_equal(counts.cpu().numpy(), ref.counts)
    ctx.check()
    with pytest.raises(ValueError, match="bin_reduce_caps"):
        rs.radix_bin_reduce(k, iv, edges=e, num=torch.tensor([5], dtype=torch.int64, device="cuda"), ctx=ctx)


def test_graph_capture(rs, torch):
    """out= after reserve_bin_reduce allocates nothing: one captured call, replayed twice on changed inputs with equal
    bytes each time.  Without the reserve on a fresh context: RSX_ERR_WORKSPACE, nothing enqueued."""
    _E, _EI, T, S = rs.bin_reduce_caps(4, 4)
    n = 3 * S + T + 5
    m = 40
    s = torch.cuda.Stream()
    keys = torch.zeros(n, dtype=torch.int32, device="cuda")
    vals = torch.zeros(n, dtype=torch.float32, device="cuda")
    num = torch.full((1,), n, dtype=torch.int64, device="cuda")
    out = (torch.full((m + 1,), -1.0, dtype=torch.float32, device="cuda"), torch.full((m + 1,), -1, dtype=torch.int64, device="cuda"))

    def enqueue(c):
        return rs.radix_bin_reduce(keys, vals, num_bins=m, num=num, out=out, return_counts=True, ctx=c)

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
    c.reserve_bin_reduce(n, m, 4, 4)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        got = enqueue(c)
    assert got[0] is out[0] and got[1] is out[1]
    g = torch.Generator(device="cuda")
    for seed, rows in ((1, n), (2, n - 999)):
        g.manual_seed(seed)
        keys.copy_(torch.randint(-3, m + 5, (n,), dtype=torch.int32, device="cuda", generator=g))
        vals.copy_(torch.randint(-8, 9, (n,), device="cuda", generator=g).to(torch.float32))
        num.fill_(rows)
        seen = []
        for _ in range(2):
            for t in out:
                t.fill_(-1)
            graph.replay()
            torch.cuda.synchronize()
            c.check()
            seen.append((out[0].cpu().numpy().copy(), out[1].cpu().numpy().copy()))
        assert np.array_equal(seen[0][0].view(np.uint8), seen[1][0].view(np.uint8)) and np.array_equal(seen[0][1], seen[1][1])
        ref = bin_reduce_reference(keys.cpu().numpy().view(np.uint8), m, "i32", "index", vals.cpu().numpy().view(np.uint8), 4, FLOAT, SUM, num=rows)
        assert np.array_equal(seen[0][0].view(np.uint8), ref.exact) and np.array_equal(seen[0][1], ref.counts)
