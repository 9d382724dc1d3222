"""GPU: layouts without sort kernels of their own (any element size, integer keys of 1..16 bytes), sorted through the
packed re-layout (route 1) or the key-index proxy (route 2) of include/rsx.h, bit-exact with the CPU oracle."""
import ctypes

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

U, S, F = util.UNSIGNED, util.SIGNED, util.FLOAT
TILE_KEYS = {4: 28, 8: 14, 12: 10, 16: 5, 24: 5, 32: 3}  # keys per thread of the 512-thread one-launch tile
DIRECT_SIZES = (1, 2, 4, 8, 12, 16, 24, 32)


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


def canon(kb):
    return next(w for w in (1, 2, 4, 8, 16) if w >= kb)


def plan(es, ko, kb, kind):
    """(route, inner layout) as include/rsx.h describes the choice; route 0 = direct."""
    if es in DIRECT_SIZES and kb in (1, 2, 4, 8, 16):
        return 0, (es, ko, kb, kind)
    kw = canon(kb)
    c = kw + es - kb
    if c <= 16:
        sp = next(z for z in (4, 8, 12, 16) if z >= c and z % kw == 0)
        return 1, (sp, 0, kw, kind)
    return 2, ({1: 8, 2: 8, 4: 8, 8: 16, 16: 32}[kw], 0, kw, kind)


def make_raw(lay, n, dist, seed):
    """Key from util._key_ints, every other byte the element's index (little-endian, truncated)."""
    es, ko, kb, kind = lay
    rng = np.random.default_rng(seed)
    raw = np.zeros((n, es), dtype=np.uint8)
    if n == 0:
        return raw.reshape(-1)
    raw[:, ko:ko + kb] = util._key_ints(dist, n, kb, rng)
    idx = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8)
    pay = [b for b in range(es) if not ko <= b < ko + kb]
    for j, b in enumerate(pay[:8]):
        raw[:, b] = idx[:, j]
    return raw.reshape(-1)


def sort_gpu(rs, torch, c, raw, lay, offset=0, tmp_extra=0):
    """Sorts a copy of raw in a uint8 tensor at byte `offset`, with guard bytes around it; returns the sorted bytes."""
    guard = 64
    buf = torch.from_numpy(np.full(offset + raw.size + guard, 0xA5, dtype=np.uint8)).cuda()
    buf[offset:offset + raw.size] = torch.from_numpy(raw.copy()).cuda()
    x = buf[offset:offset + raw.size].view(-1, lay[0])  # (n, elem_bytes): the array states its element
    tmp = torch.empty(raw.size + tmp_extra, dtype=torch.uint8, device="cuda") if tmp_extra else None
    rs.radix_sort(x, digits=rs.RadixDigits(*lay), tmp=tmp, ctx=c)
    c.check()
    out = buf.cpu().numpy()
    assert (out[:offset] == 0xA5).all() and (out[offset + raw.size:] == 0xA5).all(), "guard bytes changed"
    return out[offset:offset + raw.size]


def route_of(c, rs):
    return (c.get_info(rs.INFO_LAST_PASSES) >> 28) & 3


def path_of(c, rs):
    return (c.get_info(rs.INFO_LAST_PASSES) >> 24) & 15


def _layouts(es):
    """(es, ko, kb, kind) for every key width of 1-8, 12, 16 that fits, unsigned and signed, f32 and f64; the key
    first, in the middle, last and at an odd offset in turn."""
    out = []
    widths = [kb for kb in (1, 2, 3, 4, 5, 6, 7, 8, 12, 16) if kb <= es]
    i = 0
    for kb in widths:
        kinds = [U, S] + ([F] if kb in (4, 8) else [])
        for kind in kinds:
            offs = [0, (es - kb) // 2, es - kb, 1 if es - kb >= 1 else 0]
            out.append((es, offs[i % 4], kb, kind))
            i += 1
    return [L for L in out if plan(*L)[0] != 0]


MATRIX_SIZES = [3, 5, 6, 7, 9, 10, 11, 13, 14, 15, 17, 20, 28, 31, 33, 40, 48, 64, 100, 257, 1024]


@pytest.mark.parametrize("es", MATRIX_SIZES)
def test_layout_matrix(rs, torch, ctx, orc, es):
    rng = np.random.default_rng(700 + es)
    for li, lay in enumerate(_layouts(es)):
        route, inner = plan(*lay)
        tile = 512 * TILE_KEYS[inner[0]]
        sizes = [0, 1, 2, 3, tile - 1, tile + 1, int(rng.integers(4, 3000))]
        if es <= 64 and li % 3 == 0:
            sizes.append(100003)
        for n in sizes:
            dist = util.DISTS[int(rng.integers(0, len(util.DISTS)))]
            raw = make_raw(lay, n, dist, seed=es * 1000 + li * 10 + n % 7)
            got = sort_gpu(rs, torch, ctx, raw, lay)
            assert np.array_equal(got, orc.sort_parallel(raw, orc.Layout(*lay), 4)), (lay, n, dist)
            if n > 1:
                assert route_of(ctx, rs) == route, (lay, n)


@pytest.mark.parametrize("lay,route", [((6, 0, 2, U), 1), ((7, 0, 6, S), 1), ((15, 0, 3, U), 1), ((12, 0, 12, S), 1),
                                       ((16, 0, 3, U), 2), ((20, 0, 4, U), 2), ((28, 0, 4, U), 2), ((33, 0, 1, U), 2),
                                       ((40, 0, 8, U), 2), ((36, 1, 16, S), 2), ((64, 8, 4, F), 2)])
def test_route_on_both_sides_of_the_rule(rs, torch, ctx, orc, lay, route):
    assert plan(*lay)[0] == route
    for n, path in ((1000, 1), (200003, None)):
        raw = make_raw(lay, n, "uniform", seed=n)
        assert np.array_equal(sort_gpu(rs, torch, ctx, raw, lay), orc.sort_parallel(raw, orc.Layout(*lay), 4))
        assert route_of(ctx, rs) == route
        if path is not None:
            assert path_of(ctx, rs) == path


def _device_check(rs, torch, c, lay, n, gen, param=0.0, need_stable=True):
    d = rs.RadixDigits(*lay)
    x = torch.empty(n * lay[0], dtype=torch.uint8, device="cuda")
    out = torch.zeros(3, dtype=torch.int64, device="cuda")
    c.generate_device(x.data_ptr(), n, d, gen, 0x5EED, param)
    c.verify_device(x.data_ptr(), n, d, out.data_ptr())
    before = out.cpu().numpy().astype(np.uint64)
    rs.radix_sort(x.view(n, lay[0]), digits=d, ctx=c)
    c.check()
    c.verify_device(x.data_ptr(), n, d, out.data_ptr())
    after = out.cpu().numpy().astype(np.uint64)
    assert after[0] == 0, f"{lay}: {after[0]} descents"
    assert after[1] == before[1], f"{lay}: multiset checksum changed"
    if need_stable:
        assert after[2] == 0, f"{lay}: {after[2]} stability violations"


def test_inner_paths(rs, torch, ctx, orc):
    """One tile, the middle-size bucket split, and the wide-key hybrid over 2^22 proxies with 8-byte keys."""
    lay = (40, 0, 8, U)
    raw = make_raw(lay, 512 * TILE_KEYS[16], "uniform", 1)  # one tile of 16-byte proxies
    assert np.array_equal(sort_gpu(rs, torch, ctx, raw, lay), orc.sort_parallel(raw, orc.Layout(*lay), 4))
    assert route_of(ctx, rs) == 2 and path_of(ctx, rs) == 1
    c = rs.Context(torch.cuda.current_device())
    lay = (10, 0, 4, U)  # route 1, 12-byte canonical elements
    raw = make_raw(lay, 300000, "uniform", 2)
    assert np.array_equal(sort_gpu(rs, torch, c, raw, lay), orc.sort_parallel(raw, orc.Layout(*lay), 8))
    assert route_of(c, rs) == 1 and path_of(c, rs) == 2
    _device_check(rs, torch, c, (40, 0, 8, U), (1 << 22) + 12345, rs.GEN_UNIFORM)
    assert route_of(c, rs) == 2 and path_of(c, rs) == 5
    c.close()


@pytest.mark.parametrize("lay", [(40, 0, 8, U), (20, 0, 4, U), (6, 0, 2, U), (7, 0, 6, U)])
def test_large_n_on_the_device(rs, torch, ctx, lay):
    for gen, param in ((rs.GEN_UNIFORM, 0.0), (rs.GEN_STEP, 16.0)):
        _device_check(rs, torch, ctx, lay, 1 << 24, gen, param, need_stable=lay[0] - lay[2] >= 3)


def test_route_1_past_2pow32_bytes(rs, torch):
    """The packed re-layout and its restore with byte offsets beyond 32 bits: 7-byte elements, 2^32 + 86415 bytes."""
    c = rs.Context(torch.cuda.current_device())
    lay, n = (7, 1, 6, S), 2 ** 32 // 7 + 12345
    assert n * 7 > 2 ** 32
    _device_check(rs, torch, c, lay, n, rs.GEN_UNIFORM, need_stable=False)  # (one payload byte: the index wraps)
    assert route_of(c, rs) == 1
    c.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("lay", [(40, 0, 8, U), (20, 0, 4, U), (6, 0, 2, U), (7, 0, 6, U), (7, 1, 6, S), (100, 36, 16, U),
                                 (48, 4, 4, F), (5, 0, 3, S)])
def test_stability(rs, torch, ctx, orc, lay):
    for dist in ("equal", "two", "step16"):
        raw = make_raw(lay, 50001, dist, 3)
        assert np.array_equal(sort_gpu(rs, torch, ctx, raw, lay), orc.sort_parallel(raw, orc.Layout(*lay), 4)), (lay, dist)


@pytest.mark.parametrize("lay", [(6, 0, 2, U), (20, 4, 4, F), (40, 0, 8, U), (100, 36, 16, U), (7, 3, 3, S)])
def test_unaligned_pointers_and_guards(rs, torch, ctx, orc, lay):
    raw = make_raw(lay, 40000, "uniform", 4)
    want = orc.sort_parallel(raw, orc.Layout(*lay), 4)
    for off in (1, 2, 4, 8):
        assert np.array_equal(sort_gpu(rs, torch, ctx, raw, lay, offset=off), want), (lay, off)
    assert np.array_equal(sort_gpu(rs, torch, ctx, raw, lay, offset=3, tmp_extra=4096), want)
    # d_tmp at an odd address too (route 2 gathers between the two with byte accesses)
    d = rs.RadixDigits(*lay)
    x = torch.from_numpy(raw.copy()).cuda()
    tb = torch.empty(raw.size + 1, dtype=torch.uint8, device="cuda")
    ctx.sort_device(x.data_ptr(), tb.data_ptr() + 1, len(raw) // lay[0], d, torch.cuda.current_stream().cuda_stream)
    ctx.check()
    assert np.array_equal(x.cpu().numpy(), want)


@pytest.mark.parametrize("fields", [[("k", "<u2"), ("v", "V4")], [("k", "<u4"), ("v", "V16")], [("k", "<u8"), ("v", "V32")]])
def test_host_path_structured(rs, orc, fields):
    dt = np.dtype(fields)
    n = 30011
    rng = np.random.default_rng(5)
    a = np.frombuffer(rng.integers(0, 256, size=n * dt.itemsize, dtype=np.uint8).tobytes(), dtype=dt).copy()
    d = rs.digits_of(dt)
    want = orc.sort_parallel(a.view(np.uint8).copy(), orc.Layout(d.elem_bytes, d.key_offset, d.key_bytes, d.key_kind), 4)
    rs.radix_sort(a)
    assert np.array_equal(a.view(np.uint8), want)


def test_graph_capture_and_context_reuse(rs, torch, orc):
    c = rs.Context(torch.cuda.current_device())
    la, lb = (6, 0, 2, U), (40, 0, 8, U)
    na, nb = 70001, 50021
    c.reserve(na, rs.RadixDigits(*la))
    c.reserve(nb, rs.RadixDigits(*lb))
    src_a = torch.from_numpy(make_raw(la, na, "uniform", 10)).cuda()
    src_b = torch.from_numpy(make_raw(lb, nb, "uniform", 11)).cuda()
    wa, ta, wb, tb = torch.empty_like(src_a), torch.empty_like(src_a), torch.empty_like(src_b), torch.empty_like(src_b)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        wa.copy_(src_a)
        c.sort_device(wa.data_ptr(), ta.data_ptr(), na, rs.RadixDigits(*la), s.cuda_stream)
        wb.copy_(src_b)
        c.sort_device(wb.data_ptr(), tb.data_ptr(), nb, rs.RadixDigits(*lb), s.cuda_stream)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        wa.copy_(src_a)
        c.sort_device(wa.data_ptr(), ta.data_ptr(), na, rs.RadixDigits(*la), st)
        wb.copy_(src_b)
        c.sort_device(wb.data_ptr(), tb.data_ptr(), nb, rs.RadixDigits(*lb), st)
    for i, dist in enumerate(("zipf", "uniform", "equal")):
        ra, rb = make_raw(la, na, dist, 20 + i), make_raw(lb, nb, dist, 30 + i)
        src_a.copy_(torch.from_numpy(ra))
        src_b.copy_(torch.from_numpy(rb))
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        assert np.array_equal(wa.cpu().numpy(), orc.sort_parallel(ra, orc.Layout(*la), 4)), dist
        assert np.array_equal(wb.cpu().numpy(), orc.sort_parallel(rb, orc.Layout(*lb), 4)), dist
    # direct, route 1 and route 2 sorts alternating on one context
    for i, lay in enumerate([(8, 0, 4, U), la, lb, (16, 0, 8, S), (9, 2, 5, S), (33, 0, 1, U), (4, 0, 4, F)] * 2):
        raw = make_raw(lay, 20000 + 97 * i, "uniform", 40 + i)
        assert np.array_equal(sort_gpu(rs, torch, c, raw, lay), orc.sort_parallel(raw, orc.Layout(*lay), 4)), lay
        assert route_of(c, rs) == plan(*lay)[0]
    c.close()


def _inner_layouts():
    """Every (element size, key width) the two routes hand to the existing kernels."""
    seen = set()
    for es in range(1, 300):
        for kb in range(1, 17):
            for ko in (0,):
                if kb > es:
                    continue
                r, inner = plan(es, ko, kb, U)
                if r:
                    seen.add(inner[:3])
    return sorted(seen)


@pytest.mark.parametrize("inner", _inner_layouts())
def test_direct_parity_of_the_inner_layouts(rs, torch, ctx, orc, inner):
    es, _, kw = inner
    kinds = [U, S] + ([F] if kw in (4, 8) else [])
    tile = 512 * TILE_KEYS[es]
    rng = np.random.default_rng(es * 100 + kw)
    for kind in kinds:
        lay = (es, 0, kw, kind)
        for n in (tile - 1, tile + 1, 3 * tile + 7, 100003):
            dist = util.DISTS[int(rng.integers(0, len(util.DISTS)))]
            raw = make_raw(lay, n, dist, seed=n + kind)
            assert np.array_equal(sort_gpu(rs, torch, ctx, raw, lay), orc.sort_parallel(raw, orc.Layout(*lay), 4)), (lay, n, dist)
            assert route_of(ctx, rs) == 0


def test_still_rejected(rs, torch, ctx):
    lib = ctx._L
    # descending bytes in the array and another fill in the scratch: a sort or a copy that did get enqueued shows
    x = (255 - torch.arange(4096, device="cuda") % 256).to(torch.uint8)
    t = torch.full((4096,), 0x3C, dtype=torch.uint8, device="cuda")
    x0, t0 = x.clone(), t.clone()
    p, q = x.data_ptr(), t.data_ptr()

    def sort(es, ko, kb, kind, n=100):
        lay = rs._lib.Layout(es, ko, kb, kind)
        return lib.rsx_sort_device(ctx._h, p, q, n, ctypes.byref(lay), None)

    assert sort(8, 0, 0, U) == rs._lib.ERR_ARG
    assert sort(20, 0, 17, U) == rs._lib.ERR_ARG
    assert sort(8, 0, 2, F) == rs._lib.ERR_ARG
    assert sort(6, 3, 4, U) == rs._lib.ERR_ARG
    assert sort(0, 0, 1, U) == rs._lib.ERR_ARG
    assert sort(40000, 0, 8, U, n=0) == rs._lib.ERR_UNSUPPORTED
    assert sort(32769, 0, 8, U, n=0) == rs._lib.ERR_UNSUPPORTED  # RSX_MAX_ELEM_BYTES + 1, with and without elements
    assert sort(32769, 32761, 8, S, n=1) == rs._lib.ERR_UNSUPPORTED
    assert b"RSX_MAX_ELEM_BYTES" in lib.rsx_last_error(ctx._h)
    lay = rs._lib.Layout(6, 0, 2, U)
    assert lib.rsx_ctx_reserve(ctx._h, 10, ctypes.byref(rs._lib.Layout(6, 0, 17, U))) == rs._lib.ERR_ARG
    assert lib.rsx_ctx_reserve(ctx._h, 10, ctypes.byref(rs._lib.Layout(32769, 0, 8, U))) == rs._lib.ERR_UNSUPPORTED
    assert lib.rsx_ctx_reserve(ctx._h, 2, ctypes.byref(rs._lib.Layout(32768, 0, 8, U))) == 0
    h = torch.zeros(256 * 8, dtype=torch.uint8, device="cuda")
    assert lib.rsx_histogram_device(ctx._h, p, 100, ctypes.byref(lay), 0, h.data_ptr(), None) == rs._lib.ERR_UNSUPPORTED
    assert lib.rsx_partition_device(ctx._h, p, q, 100, ctypes.byref(lay), 0, None, None) == rs._lib.ERR_UNSUPPORTED
    lay6 = rs._lib.Layout(8, 0, 6, U)
    assert lib.rsx_partition_device(ctx._h, p, q, 100, ctypes.byref(lay6), 0, None, None) == rs._lib.ERR_ARG
    with pytest.raises(rs.RsxError):
        rs.radix_sort_sharded([x[:600]], rs.RadixDigits(6, 0, 2, U), ctxs=[ctx])
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(t, t0)  # no refusal enqueued anything


def test_flat_byte_buffer_needs_the_element_shape(rs, torch, ctx, orc):
    """radix_sort on a flat byte tensor reads packed elements of the sizes with kernels only (what
    test_gpu_parity.py::test_errors pins for 3-byte elements); the same bytes as an (n, 3) tensor sort."""
    lay = (3, 0, 2, U)
    raw = make_raw(lay, 341, "uniform", 12)
    x = torch.from_numpy(raw.copy()).cuda()
    with pytest.raises(rs.RsxError) as e:
        rs.radix_sort(x, digits=rs.RadixDigits(*lay), ctx=ctx)
    assert e.value.status == rs._lib.ERR_UNSUPPORTED
    assert np.array_equal(x.cpu().numpy(), raw)  # untouched
    rs.radix_sort(x.view(-1, 3), digits=rs.RadixDigits(*lay), ctx=ctx)
    ctx.check()
    assert np.array_equal(x.cpu().numpy(), orc.sort_parallel(raw, orc.Layout(*lay), 4))
    assert route_of(ctx, rs) == 1
