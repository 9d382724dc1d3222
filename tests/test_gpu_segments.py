"""GPU: radix_sort_segments / radix_sort_rows (rsx_sort_segments_device, rsx_sort_rows_device) against the CPU oracle
applied to each segment.  Every comparison is np.array_equal on all bytes of an allocation the test owns: 64 guard
bytes of 0xA5, the array (untouched head and tail included), 64 guard bytes -- for `x` and for `tmp`'s neighbours."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu
GUARD = 64


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
    return rs.default_context(torch.cuda.current_device())


def _digits(rs, t):
    return rs.RadixDigits(*util.TYPES[t])


def _expected(orc, raw, t, offs):
    """The oracle on every segment of `raw` (bytes), everything else as it was."""
    lay = orc.Layout(*util.TYPES[t])
    es = lay.elem_bytes
    out = raw.copy()
    for b, e in zip(offs[:-1], offs[1:]):
        b, e = int(b), int(e)
        if e - b > 1:
            out[b * es:e * es] = orc.sort0(raw[b * es:e * es], lay)
    return out


def _guarded(torch, raw):
    """(whole allocation, view of its middle) on the GPU, guards of 0xA5 around `raw`."""
    buf = torch.full((GUARD + raw.size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    mid = buf[GUARD:GUARD + raw.size]
    mid.copy_(torch.from_numpy(raw))
    return buf, mid


def _with_guards(raw):
    g = np.full(GUARD, 0xA5, dtype=np.uint8)
    return np.concatenate([g, raw, g])


def _segsort(rs, torch, ctx, t, raw, offs, max_seg_len=0, check=True):
    """Sorts the segments `offs` of `raw` on the GPU; returns the whole guarded allocation of x; asserts tmp's guards."""
    d = _digits(rs, t)
    xbuf, x = _guarded(torch, raw)
    tbuf, tmp = _guarded(torch, np.zeros(raw.size, dtype=np.uint8))
    o = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
    rs.radix_sort_segments(x, o, digits=d, tmp=tmp, ctx=ctx, max_seg_len=max_seg_len)
    if check:
        ctx.check()
    else:
        torch.cuda.synchronize()
    tb = tbuf.cpu().numpy()
    assert np.all(tb[:GUARD] == 0xA5) and np.all(tb[-GUARD:] == 0xA5), "tmp's neighbours were written"
    return xbuf.cpu().numpy()


def _same(got, exp, offs=None, es=1, base=GUARD):
    """np.array_equal with a report of where the first difference lies (byte, element, segment)."""
    if np.array_equal(got, exp):
        return True
    w = np.nonzero(got != exp)[0] if got.shape == exp.shape else np.zeros(1, dtype=np.int64)
    first, last = int(w[0]), int(w[-1])
    msg = f"{len(w)} bytes differ, first at byte {first} (element {(first - base) // es}), last at byte {last}"
    if offs is not None:
        o = np.asarray(offs, dtype=np.int64)
        k = int(np.searchsorted(o, (first - base) // es, side="right")) - 1
        if 0 <= k < len(o) - 1:
            msg += f"; segment {k} = [{int(o[k])}, {int(o[k + 1])}) of {len(o) - 1}"
    print(msg, "\n got", got[max(0, first - 4):first + 12].tolist(), "\n exp", exp[max(0, first - 4):first + 12].tolist())
    return False


def _ragged_offsets(rng, nseg, choices, head=0):
    lens = rng.choice(np.asarray(choices, dtype=np.int64), size=nseg)
    return np.concatenate([[head], head + np.cumsum(lens)]).astype(np.int64)


@pytest.mark.parametrize("dist", ["uniform", "equal", "two", "zipf", "highbyte"])
@pytest.mark.parametrize("t", list(util.TYPES))
def test_ragged_segments_every_type(rs, torch, ctx, orc, t, dist):
    rng = np.random.default_rng(sum(map(ord, t + dist)))
    offs = _ragged_offsets(rng, 3000, [0, 1, 2, 63, 64, 65, 1000], head=5)
    n = int(offs[-1]) + 7  # a head of 5 and a tail of 7 elements that no segment covers
    raw = util.make_input(t, n, dist, seed=11)
    got = _segsort(rs, torch, ctx, t, raw, offs)
    assert _same(got, _with_guards(_expected(orc, raw, t, offs)), offs, util.TYPES[t][0])


@pytest.mark.parametrize("t", ["u32", "f64", "(u64,u64)", "(u128,u128)", "u8", "i16"])
def test_class_edges(rs, torch, ctx, orc, t):
    """Lengths cap-1, cap, cap+1 of every class; above the last cap the segment goes through memory (key widths 1 and 2:
    odd and even pass counts; f64 and i16: raw signed / float keys on that form)."""
    caps = rs.segment_caps(_digits(rs, t))
    assert len(caps) >= 2 and caps == sorted(caps)
    lens = []
    for c in caps:
        lens += [c - 1, c, c + 1]
    lens += [3, 0, 1, 70]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1])
    for dist in ("uniform", "zipf"):
        raw = util.make_input(t, n, dist, seed=3)
        got = _segsort(rs, torch, ctx, t, raw, offs)
        assert np.array_equal(got, _with_guards(_expected(orc, raw, t, offs))), dist
    assert (ctx.get_info(rs.INFO_LAST_PASSES) >> 24) & 0xF == 6


@pytest.mark.parametrize("t", ["i32", "f32", "u64", "i64", "(f32,u32)", "(pay64+f64)", "u128", "(u8,[u8;7])", "(u32,[u8;8])", "(u64,[u64;2])"])
def test_through_memory_form_key_kinds(rs, torch, ctx, orc, t):
    """One segment above the largest LDS class for signed, float and unsigned keys of odd (1) and even widths."""
    caps = rs.segment_caps(_digits(rs, t))
    lens = [caps[-1] + 1234, 17, caps[-1] + 1]
    offs = np.concatenate([[2], 2 + np.cumsum(lens)]).astype(np.int64)
    raw = util.make_input(t, int(offs[-1]) + 3, "uniform", seed=8)
    got = _segsort(rs, torch, ctx, t, raw, offs)
    assert np.array_equal(got, _with_guards(_expected(orc, raw, t, offs)))


def test_one_long_segment_among_many_short(rs, torch, ctx, orc):
    t = "u64"
    lens = [100] * 5000 + [1 << 20] + [100] * 5000
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    raw = util.make_input(t, int(offs[-1]), "uniform", seed=21)
    exp = _with_guards(_expected(orc, raw, t, offs))
    got0 = _segsort(rs, torch, ctx, t, raw, offs, max_seg_len=0)
    assert np.array_equal(got0, exp)
    assert ctx.get_info(rs.INFO_LAST_PASSES) & 0xFF == 3  # every class was launched
    got1 = _segsort(rs, torch, ctx, t, raw, offs, max_seg_len=1 << 20)
    assert np.array_equal(got1, exp)


def test_vouched_bound_drops_classes(rs, torch, ctx, orc):
    t = "u32"
    rng = np.random.default_rng(2)
    offs = _ragged_offsets(rng, 20000, [0, 1, 5, 100, 1000])
    raw = util.make_input(t, int(offs[-1]), "uniform", seed=22)
    exp = _with_guards(_expected(orc, raw, t, offs))
    assert np.array_equal(_segsort(rs, torch, ctx, t, raw, offs, max_seg_len=0), exp)
    assert ctx.get_info(rs.INFO_LAST_PASSES) == (6 << 24) | 3
    assert np.array_equal(_segsort(rs, torch, ctx, t, raw, offs, max_seg_len=1000), exp)
    assert ctx.get_info(rs.INFO_LAST_PASSES) == (6 << 24) | 1


def test_empty_runs_single_segment_and_partial_cover(rs, torch, ctx, orc):
    t = "(u32,u32)"
    lay = orc.Layout(*util.TYPES[t])
    # empty segments in runs
    lens = [0] * 300 + [50] + [0] * 700 + [1, 0, 0, 9, 0] * 100 + [0] * 300
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    raw = util.make_input(t, int(offs[-1]), "two", seed=23)
    assert np.array_equal(_segsort(rs, torch, ctx, t, raw, offs), _with_guards(_expected(orc, raw, t, offs)))
    # nseg = 1 over a range that starts above 0 and ends below n: radix_sort of that range
    for n, b, e in ((5000, 100, 4900), (200000, 7, 199000)):
        raw = util.make_input(t, n, "uniform", seed=24)
        got = _segsort(rs, torch, ctx, t, raw, [b, e])
        exp = raw.copy()
        exp[b * 8:e * 8] = orc.sort_parallel(raw[b * 8:e * 8], lay, 4)
        assert np.array_equal(got, _with_guards(exp))
        x = torch.from_numpy(raw[b * 8:e * 8].copy()).cuda()
        rs.radix_sort(x, digits=_digits(rs, t), ctx=ctx)
        ctx.check()
        assert np.array_equal(got[GUARD + b * 8:GUARD + e * 8], x.cpu().numpy())
    # no segments at all
    raw = util.make_input(t, 100, "uniform", seed=25)
    assert np.array_equal(_segsort(rs, torch, ctx, t, raw, [40]), _with_guards(raw))


def _rows_case(rs, torch, ctx, orc, shape, dtype_name, seed):
    tname = {"int32": "i32", "float32": "f32", "int64": "i64", "uint8": "u8"}[dtype_name]
    dt = getattr(torch, dtype_name)
    numel = int(np.prod(shape))
    es = util.TYPES[tname][0]
    raw = util.make_input(tname, numel, "uniform", seed=seed)
    xbuf, xb = _guarded(torch, raw)
    tbuf, tb = _guarded(torch, np.zeros(raw.size, dtype=np.uint8))
    x = xb.view(dt).view(shape)
    tmp = tb.view(dt).view(shape)
    ref = None
    if dtype_name != "float32":
        ref = torch.sort(x.clone(), dim=-1, stable=True).values
    rs.radix_sort_rows(x, tmp=tmp, ctx=ctx)
    ctx.check()
    L = shape[-1]
    rows = numel // L if L else 0
    offs = np.arange(rows + 1, dtype=np.int64) * L
    exp = _expected(orc, raw, tname, offs) if L > 1 else raw
    assert np.array_equal(xbuf.cpu().numpy(), _with_guards(exp)), (shape, dtype_name)
    tg = tbuf.cpu().numpy()
    assert np.all(tg[:GUARD] == 0xA5) and np.all(tg[-GUARD:] == 0xA5)
    if ref is not None:
        assert torch.equal(x, ref), (shape, dtype_name)
    assert es * numel == raw.size


@pytest.mark.parametrize("dtype_name", ["int32", "float32", "int64", "uint8"])
@pytest.mark.parametrize("shape", [(1, 777), (300, 1), (300, 0), (3, 5, 257), (4096, 1024)])
def test_rows(rs, torch, ctx, orc, shape, dtype_name):
    _rows_case(rs, torch, ctx, orc, shape, dtype_name, seed=31)
    if shape[-1] > 1:
        assert (ctx.get_info(rs.INFO_LAST_PASSES)) == (6 << 24) | 1


@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_rows_above_the_largest_class(rs, torch, ctx, orc, dtype_name):
    caps = rs.segment_caps(rs.PRIMITIVES["i32" if dtype_name == "int32" else "i64"])
    _rows_case(rs, torch, ctx, orc, (3, caps[-1] + 1), dtype_name, seed=32)
    _rows_case(rs, torch, ctx, orc, (3, caps[-1]), dtype_name, seed=33)
    _rows_case(rs, torch, ctx, orc, (5, caps[0] + 1), dtype_name, seed=34)


def test_many_rows_just_above_the_largest_class(rs, torch, ctx, orc):
    """At least as many rows as the device has CUs, a little longer than the largest LDS class: one launch of the
    through-memory class (path 6) instead of a sort per row."""
    caps = rs.segment_caps(rs.PRIMITIVES["i32"])
    rows = ctx.get_info(rs._lib.INFO_NUM_CU) + 3
    _rows_case(rs, torch, ctx, orc, (rows, caps[-1] + 1), "int32", seed=36)
    assert ctx.get_info(rs.INFO_LAST_PASSES) == (6 << 24) | 1


def test_rows_of_packed_elements(rs, torch, ctx, orc):
    t = "(u64,u64)"
    d = _digits(rs, t)
    rows, L = 37, 301
    raw = util.make_input(t, rows * L, "two", seed=35)
    x = torch.from_numpy(raw.copy()).cuda().view(rows, L * 16)
    rs.radix_sort_rows(x, digits=d, ctx=ctx)
    ctx.check()
    offs = np.arange(rows + 1, dtype=np.int64) * L
    assert np.array_equal(x.cpu().numpy().reshape(-1), _expected(orc, raw, t, offs))


def test_ballot_ranks_give_the_same_bytes(rs, torch, orc):
    c = rs.Context(torch.cuda.current_device())
    c.set_option(rs.OPT_RANKING, 1)
    for t in ("u32", "(u64,u64)"):
        rng = np.random.default_rng(4)
        caps = rs.segment_caps(_digits(rs, t))
        offs = _ragged_offsets(rng, 2000, [0, 1, 2, 63, 64, 65, 1000, caps[0] + 1, caps[1] + 1])
        raw = util.make_input(t, int(offs[-1]), "zipf", seed=41)
        assert np.array_equal(_segsort(rs, torch, c, t, raw, offs), _with_guards(_expected(orc, raw, t, offs)))
    c.close()


def test_untrusted_offsets(rs, torch, orc):
    """A decreasing pair inside [0, n) and a last offset of n + 8, with x a view of a larger tensor the test owns (so that
    even a wrong implementation stays inside the test's memory): the other segments are sorted, the bad ones and
    everything outside [0, n) unchanged, check() raises once."""
    c = rs.Context(torch.cuda.current_device())
    t = "u32"
    d = _digits(rs, t)
    lay = orc.Layout(*util.TYPES[t])
    n, extra = 10000, 4096
    raw = util.make_input(t, n + extra, "uniform", seed=51)
    big = torch.from_numpy(raw.copy()).cuda()
    tbig = torch.full_like(big, 0xA5)
    x, tmp = big[:n * 4], tbig[:n * 4]
    # segments: [4000, 5000) good, [5000, 1000) decreasing, [1000, 3000) good, [3000, 3500) good, [3500, n + 8) ends behind n
    offs = [4000, 5000, 1000, 3000, 3500, n + 8]
    o = torch.tensor(offs, dtype=torch.int64, device="cuda")
    exp = raw.copy()
    for b, e_ in ((4000, 5000), (1000, 3000), (3000, 3500)):
        exp[b * 4:e_ * 4] = orc.sort0(raw[b * 4:e_ * 4], lay)
    for max_len in (0, 2000):
        big.copy_(torch.from_numpy(raw))
        rs.radix_sort_segments(x, o, digits=d, tmp=tmp, ctx=c, max_seg_len=max_len)
        with pytest.raises(rs.RsxError) as e:
            c.check()
        assert e.value.status == rs._lib.ERR_INTERNAL
        c.check()  # the condition was cleared
        assert np.array_equal(big.cpu().numpy(), exp)
        assert np.all(tbig[n * 4:].cpu().numpy() == 0xA5), "memory behind tmp was written"
    # a pending error fails the next call without a synchronisation of its own; check() clears it
    rs.radix_sort_segments(x, o, digits=d, tmp=tmp, ctx=c)
    torch.cuda.synchronize()
    with pytest.raises(rs.RsxError):
        rs.radix_sort_segments(x, o, digits=d, tmp=tmp, ctx=c)
    with pytest.raises(rs.RsxError):
        c.check()
    c.check()
    c.close()


def test_graph_capture_on_an_unreserved_context(rs, torch, orc):
    c = rs.Context(torch.cuda.current_device())  # never reserved
    t = "u32"
    d = _digits(rs, t)
    rng = np.random.default_rng(6)
    caps = rs.segment_caps(d)
    offs = _ragged_offsets(rng, 4000, [0, 1, 2, 63, 64, 65, 1000, caps[0] + 5])
    n = int(offs[-1])
    rows, L = 512, 300
    inputs = [(util.make_input(t, n, dist, seed=60 + i), util.make_input("f32", rows * L, dist, seed=70 + i))
              for i, dist in enumerate(("uniform", "zipf", "two"))]
    src = torch.from_numpy(inputs[0][0].copy()).cuda()
    work, tmp = torch.empty_like(src), torch.empty_like(src)
    src2 = torch.from_numpy(inputs[0][1].copy()).cuda().view(torch.float32).view(rows, L)
    work2, tmp2 = torch.empty_like(src2), torch.empty_like(src2)
    o = torch.from_numpy(offs).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside capture (a context's first call cannot be a captured one)
        work.copy_(src)
        rs.radix_sort_segments(work, o, digits=d, tmp=tmp, ctx=c)
        work2.copy_(src2)
        rs.radix_sort_rows(work2, tmp=tmp2, ctx=c)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        work.copy_(src)
        rs.radix_sort_segments(work, o, digits=d, tmp=tmp, ctx=c, max_seg_len=0)
        work2.copy_(src2)
        rs.radix_sort_rows(work2, tmp=tmp2, ctx=c)
    roffs = np.arange(rows + 1, dtype=np.int64) * L
    for raw, raw2 in inputs[1:]:
        src.copy_(torch.from_numpy(raw.copy()))
        src2.copy_(torch.from_numpy(raw2.copy()).view(torch.float32).view(rows, L))
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        assert _same(work.cpu().numpy(), _expected(orc, raw, t, offs), offs, 4, 0)
        assert _same(work2.cpu().numpy().view(np.uint8).reshape(-1), _expected(orc, raw2, "f32", roffs), roffs, 4, 0)
    c.close()


def test_reports_path_6(rs, torch, ctx):
    x = torch.randint(0, 1 << 30, (64, 100), dtype=torch.int32, device="cuda")
    rs.radix_sort_rows(x, ctx=ctx)
    ctx.check()
    info = ctx.get_info(rs.INFO_LAST_PASSES)
    assert (info >> 24) & 0xF == 6 and info & 0xFF == 1 and (info >> 28) & 3 == 0
    o = torch.tensor([0, 10, 6400], dtype=torch.int64, device="cuda")
    rs.radix_sort_segments(x.view(-1), o, ctx=ctx)
    ctx.check()
    info = ctx.get_info(rs.INFO_LAST_PASSES)
    assert (info >> 24) & 0xF == 6 and info & 0xFF == 3
    rs.radix_sort(x.view(-1), ctx=ctx)  # an ordinary sort reports its own path again
    ctx.check()
    assert (ctx.get_info(rs.INFO_LAST_PASSES) >> 24) & 0xF == 1
