"""GPU: rsx_topk_rows_device / radix_topk against tests/topk_ref.py -- the first k columns of the stable sort of every
row, byte for byte.

Every comparison is np.array_equal on all bytes of an allocation the test owns: 64 guard bytes of 0xA5, the array, 64
guard bytes -- for out_keys and out_index; the key column is compared with its input afterwards."""
import numpy as np
import pytest

import util
from segment_pairs_gpu import guarded, key_dtype, same
from segment_pairs_ref import with_guards
from topk_ref import first_k, index_bytes_of, rows_reference

pytestmark = pytest.mark.gpu

KEY_TYPES = ["u8", "i16", "u32", "i32", "f32", "u64", "i64", "f64", "u128"]
DISTS = ["uniform", "equal", "two", "highbyte"]
PATH = 7 << 24


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


class Call:
    """One key column on the GPU (guarded) and the calls made on it through Context.topk_rows_device on raw pointers."""

    def __init__(self, torch, c, tname, keys_raw, rows, row_len):
        self.torch, self.c, self.tname = torch, c, tname
        self.kb, self.kind = util.TYPES[tname][2], util.TYPES[tname][3]
        self.keys_raw, self.rows, self.row_len = keys_raw, rows, row_len
        self.kbuf, self.kmid = guarded(torch, keys_raw)
        self.full = {}

    def reference(self, desc):
        if desc not in self.full:
            self.full[desc] = rows_reference(self.keys_raw, self.kb, self.kind, self.rows, self.row_len, desc)
        return self.full[desc]

    def run(self, k, desc, ib=8, keys=True, index=True, status=None):
        """-> (out_keys allocation, out_index allocation) as numpy bytes, both pre-filled with 0xA5.  status: the call
        must fail with it (the allocations come back all the same)."""
        torch, n = self.torch, self.rows * k
        obuf, omid = guarded(torch, np.full(n * self.kb, 0xA5, dtype=np.uint8))
        ibuf, imid = guarded(torch, np.full(n * ib, 0xA5, dtype=np.uint8))
        args = (self.kmid.data_ptr(), omid.data_ptr() if keys else 0, imid.data_ptr() if index else 0, self.rows, self.row_len, k,
                self.kb, self.kind, ib, desc, torch.cuda.current_stream().cuda_stream)
        if status is None:
            self.c.topk_rows_device(*args)
            self.c.check()
        else:
            import radix_sort_amd as rs
            with pytest.raises(rs.RsxError) as e:
                self.c.topk_rows_device(*args)
            assert e.value.status == status, e.value
            torch.cuda.synchronize()
        return obuf.cpu().numpy(), ibuf.cpu().numpy()

    def check(self, k, desc, ib=8, what=None):
        wk, wi = first_k(self.reference(desc), k)
        gk, gi = self.run(k, desc, ib)
        assert same(gk, with_guards(wk), ("out_keys", self.tname, what, k, desc))
        assert same(gi, with_guards(index_bytes_of(wi, ib)), ("out_index", self.tname, what, k, desc, ib))
        return wi

    def keys_unchanged(self):
        assert same(self.kbuf.cpu().numpy(), with_guards(self.keys_raw), ("the key column", self.tname))


def ks_of(row_len):
    return sorted({min(max(k, 1), row_len) for k in (1, 2, row_len // 2, row_len - 1, row_len)})


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("tname", KEY_TYPES)
def test_every_key_type(rs, torch, ctx, tname, dist):
    """`equal`: every key ties, the indices are 0 .. k-1.  `two`: the threshold falls inside a run of ties."""
    rows = 37
    for row_len in (1, 2, 63, 64, 65, 1000):
        keys_raw = util.make_input(tname, rows * row_len, dist, seed=7 + row_len)
        call = Call(torch, ctx, tname, keys_raw, rows, row_len)
        for desc in (False, True):
            for k in ks_of(row_len):
                for ib in (4, 8):
                    wi = call.check(k, desc, ib, what=(dist, row_len))
                    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 1
                if dist == "equal":
                    assert np.array_equal(wi.reshape(rows, k), np.tile(np.arange(k), (rows, 1)))
        call.keys_unchanged()


@pytest.mark.parametrize("tname", ["f32", "u64"])
def test_class_edges(rs, torch, ctx, tname):
    """The longest row of the 256-thread class, the shortest and the longest of the 1024-thread class: one launch each."""
    caps, _ = rs.topk_caps(util.TYPES[tname][2])
    assert caps == rs.segment_pairs_caps(util.TYPES[tname][2], 4)
    for row_len in (caps[0], caps[0] + 1, caps[-1]):
        call = Call(torch, ctx, tname, util.make_input(tname, 3 * row_len, "uniform", seed=row_len), 3, row_len)
        for desc in (False, True):
            for k in (1, 64, 65, row_len // 2):
                call.check(k, desc, what=("edges", row_len))
                assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 1
        call.keys_unchanged()


@pytest.mark.parametrize("tname", ["f32", "u64"])
def test_two_rounds(rs, torch, ctx, tname):
    """Rows of two and three chunks whose candidates fit one chunk: two launches."""
    caps, _ = rs.topk_caps(util.TYPES[tname][2])
    L = caps[-1]
    for row_len in (L + 1, 2 * L + 5):
        for rows in (1, 3):
            for dist in ("uniform", "two"):
                call = Call(torch, ctx, tname, util.make_input(tname, rows * row_len, dist, seed=rows), rows, row_len)
                for desc in (False, True):
                    for k in (1, 100):
                        call.check(k, desc, ib=4 if desc else 8, what=("rounds", row_len, rows, dist))
                        assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 2
                call.keys_unchanged()


@pytest.mark.parametrize("dist", ["equal", "two"])
@pytest.mark.parametrize("tname", ["f32", "u64"])
def test_three_rounds_of_ties(rs, torch, ctx, tname, dist):
    """Four chunks of which each gives max_k candidates: 3 max_k + 7 > L, then max_k + max_k = L: three launches.  All
    keys (or half of them) tie: the order of every round's candidates is what carries the position rule through."""
    caps, max_k = rs.topk_caps(util.TYPES[tname][2])
    L = caps[-1]
    row_len = 3 * L + 7
    for rows in (1, 2):
        call = Call(torch, ctx, tname, util.make_input(tname, rows * row_len, dist, seed=3 + rows), rows, row_len)
        for desc in (False, True):
            wi = call.check(max_k, desc, what=("three rounds", rows, dist))
            assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 3
            if dist == "equal":
                assert np.array_equal(wi.reshape(rows, max_k), np.tile(np.arange(max_k), (rows, 1)))
        call.keys_unchanged()


@pytest.mark.parametrize("tname", ["f32", "u64"])
def test_k_above_max_k_on_a_long_row(rs, torch, ctx, tname):
    """The C call refuses and writes nothing; radix_topk sorts the row instead and returns the same definition."""
    kb, kind = util.TYPES[tname][2], util.TYPES[tname][3]
    caps, max_k = rs.topk_caps(kb)
    rows, row_len, k = 2, caps[-1] + 1, max_k + 1
    keys_raw = util.make_input(tname, rows * row_len, "two", seed=9)
    call = Call(torch, ctx, tname, keys_raw, rows, row_len)
    gk, gi = call.run(k, True, status=rs._lib.ERR_UNSUPPORTED)
    assert bool((gk == 0xA5).all()) and bool((gi == 0xA5).all())
    keys = call.kmid.view(key_dtype(torch, tname)).view(rows, row_len)
    for largest in (True, False):
        values, indices = rs.radix_topk(keys, k, largest=largest, ctx=ctx)
        ctx.check()
        wk, wi = first_k(call.reference(largest), k)
        assert values.shape == (rows, k) and values.dtype == keys.dtype and indices.dtype == torch.int64
        assert np.array_equal(values.cpu().view(torch.uint8).numpy().reshape(-1), wk)
        assert np.array_equal(indices.cpu().numpy().reshape(-1), wi)
    call.keys_unchanged()


def test_flat_array(rs, torch, ctx):
    """2^20 f32, k = 256 through radix_topk: the values are torch.topk's, the indices the reference's."""
    n, k = 1 << 20, 256
    g = torch.Generator(device="cuda")
    g.manual_seed(20)
    x = torch.randn(n, dtype=torch.float32, device="cuda", generator=g)
    x[::1000] = x[7]  # (ties, also inside the top)
    x[5::4001] = 9.0
    raw = x.cpu().numpy().view(np.uint8).reshape(-1)
    for largest in (True, False):
        values, indices = rs.radix_topk(x, k, largest=largest, ctx=ctx)
        ctx.check()
        assert (ctx.get_info(rs.INFO_LAST_PASSES) >> 24) & 0xF == 7 and ctx.get_info(rs.INFO_LAST_PASSES) & 0xFF >= 2
        assert values.shape == (k,) and indices.shape == (k,) and indices.dtype == torch.int64
        assert torch.equal(values, torch.topk(x, k, largest=largest, sorted=True).values)
        wk, wi = first_k(rows_reference(raw, 4, util.FLOAT, 1, n, largest), k)
        assert np.array_equal(indices.cpu().numpy(), wi)
        assert np.array_equal(values.cpu().numpy().view(np.uint8), wk)
    assert np.array_equal(x.cpu().numpy().view(np.uint8).reshape(-1), raw)


def test_python_shapes_and_dtypes(rs, torch, ctx):
    """radix_topk along the last dimension of a 3-D tensor, both index types, against torch's stable sort."""
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randint(-20, 20, (3, 5, 100), dtype=torch.int32, device="cuda", generator=g)
    for largest in (True, False):
        want = torch.sort(x, dim=-1, stable=True, descending=largest)
        for idt in (torch.int32, torch.int64):
            values, indices = rs.radix_topk(x, 7, largest=largest, index_dtype=idt, ctx=ctx)
            ctx.check()
            assert values.shape == (3, 5, 7) and indices.dtype == idt
            assert torch.equal(values, want.values[..., :7]) and torch.equal(indices.to(torch.int64), want.indices[..., :7])
    values, indices = rs.radix_topk(x, 0, ctx=ctx)
    assert values.shape == (3, 5, 0) and indices.shape == (3, 5, 0)


@pytest.mark.parametrize("shape", [(5, 700, 33), (2, 20000, 100)])
def test_only_one_output(rs, torch, ctx, shape):
    rows, row_len, k = shape
    call = Call(torch, ctx, "f32", util.make_input("f32", rows * row_len, "two", seed=4), rows, row_len)
    gk, gi = call.run(k, True, ib=4)
    wk, wi = first_k(call.reference(True), k)
    assert same(gk, with_guards(wk), "both: keys") and same(gi, with_guards(index_bytes_of(wi, 4)), "both: index")
    untouched_k, untouched_i = np.full_like(gk, 0xA5), np.full_like(gi, 0xA5)
    ok, oi = call.run(k, True, ib=4, keys=False)
    assert same(ok, untouched_k, "index only: keys") and same(oi, gi, "index only: index")
    ok, oi = call.run(k, True, ib=4, index=False)
    assert same(ok, gk, "keys only: keys") and same(oi, untouched_i, "keys only: index")
    call.keys_unchanged()


def test_errors(rs, torch, ctx):
    E = rs._lib
    call = Call(torch, ctx, "u32", util.make_input("u32", 4 * 50, "uniform", seed=2), 4, 50)
    for kwargs, k in ((dict(), 51), (dict(keys=False, index=False), 5), (dict(ib=3), 5)):
        gk, gi = call.run(k, False, status=E.ERR_ARG, **kwargs)
        assert bool((gk == 0xA5).all()) and bool((gi == 0xA5).all())  # nothing was enqueued
    gk, gi = call.run(0, False)  # k == 0: succeeds, the (empty) outputs' guards intact
    assert bool((gk == 0xA5).all()) and bool((gi == 0xA5).all())
    empty = Call(torch, ctx, "u32", np.zeros(0, dtype=np.uint8), 0, 50)
    gk, gi = empty.run(5, True)  # rows == 0
    assert bool((gk == 0xA5).all()) and bool((gi == 0xA5).all())
    L, h = ctx._L, ctx._h
    p = call.kmid.data_ptr()
    assert L.rsx_topk_rows_device(h, p, p, p, 4, 50, 5, 3, 0, 8, 0, None) == E.ERR_ARG       # key width
    assert L.rsx_topk_rows_device(h, p, p, p, 4, 50, 5, 16, 2, 8, 0, None) == E.ERR_ARG      # float keys of 16 bytes
    assert L.rsx_topk_rows_device(h, p, p, p, 4, 50, 5, 4, 0, 8, 2, None) == E.ERR_ARG       # order
    assert L.rsx_topk_rows_device(h, p, p, p, 2 ** 62, 2 ** 10, 5, 4, 0, 8, 0, None) == E.ERR_ARG  # rows * row_len overflows
    assert L.rsx_topk_rows_device(h, p + 2, p, p, 4, 50, 5, 4, 0, 8, 0, None) == E.ERR_ARG   # misaligned
    assert L.rsx_topk_rows_device(h, p, p, p, 1, 2 ** 32, 1, 4, 0, 8, 0, None) == E.ERR_UNSUPPORTED
    assert L.rsx_ctx_reserve_topk(h, 4, 50, 51, 4) == E.ERR_ARG
    torch.cuda.synchronize()
    call.check(5, True)  # the context works on
    call.keys_unchanged()


def test_graph_capture(rs, torch):
    """An LDS-class shape touches no workspace: after a warm-up call it captures on a context that reserved nothing.  A
    two-round shape needs reserve_topk first."""
    c = rs.Context(torch.cuda.current_device())
    rows, row_len, k = 64, 1000, 50
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, row_len), dtype=torch.int32, device="cuda")
    keys = torch.empty_like(src)
    values = torch.empty((rows, k), dtype=torch.int32, device="cuda")
    index = torch.empty((rows, k), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()

    def enqueue(kt, vt, it, k_):
        c.topk_rows_device(kt.data_ptr(), vt.data_ptr(), it.data_ptr(), kt.shape[0], kt.shape[1], k_, 4, rs.KEY_SIGNED, it.element_size(),
                           True, torch.cuda.current_stream().cuda_stream)

    with torch.cuda.stream(s):
        keys.copy_(src)
        enqueue(keys, values, index, k)  # warm-up outside capture
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        keys.copy_(src)
        enqueue(keys, values, index, k)
    for seed in (1, 2):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        src.copy_(torch.randint(-50 * seed, 50 * seed, (rows, row_len), dtype=torch.int32, device="cuda", generator=g))
        index.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        want = torch.sort(src, dim=-1, stable=True, descending=True)
        assert torch.equal(index, want.indices[:, :k]) and torch.equal(values, want.values[:, :k])
    # two rounds: RSX_ERR_WORKSPACE under capture without a reserve, nothing enqueued
    L = rs.topk_caps(4)[0][-1]
    rows = 3
    big = torch.randint(-1000, 1000, (rows, 2 * L + 5), dtype=torch.int32, device="cuda")
    bval = torch.full((rows, k), -1, dtype=torch.int32, device="cuda")
    bidx = torch.full((rows, k), -1, dtype=torch.int32, device="cuda")
    g2 = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g2.capture_begin()
        try:
            enqueue(big, bval, bidx, k)
        except rs.RsxError as e:
            err = e
        g2.capture_end()
    assert err is not None and err.status == rs._lib.ERR_WORKSPACE, err
    torch.cuda.synchronize()
    assert bool((bidx == -1).all()) and bool((bval == -1).all())  # nothing was enqueued
    c.reserve_topk(rows, 2 * L + 5, k, 4)
    g3 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g3, stream=s):
        enqueue(big, bval, bidx, k)
    g3.replay()
    torch.cuda.synchronize()
    c.check()
    assert (c.get_info(rs.INFO_LAST_PASSES)) == PATH | 2
    want = torch.sort(big, dim=-1, stable=True, descending=True)
    assert torch.equal(bidx.to(torch.int64), want.indices[:, :k]) and torch.equal(bval, want.values[:, :k])
    c.close()
