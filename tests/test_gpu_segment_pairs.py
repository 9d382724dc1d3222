"""GPU: the segmented key / value calls (radix_sort_segments_pairs, radix_argsort_segments, radix_sort_rows_pairs,
radix_argsort_rows) against pairs_ref.pairs_reference applied to each segment (tests/segment_pairs_ref.py).

Every comparison is np.array_equal on all bytes of an allocation the test owns: 64 guard bytes of 0xA5, the array
(untouched heads, tails and bad segments included), 64 guard bytes -- for the keys, the values and the index."""
import numpy as np
import pytest

import util
from segment_pairs_gpu import check_all, expected_info, joined_elem, sort_pairs
from segment_pairs_ref import GUARD, expected_index, segments_reference

pytestmark = pytest.mark.gpu

U, S, F = util.UNSIGNED, util.SIGNED, util.FLOAT
KEY_TYPES = ["u8", "i16", "u32", "i32", "f32", "u64", "i64", "f64", "u128"]
DISTS = ["uniform", "equal", "two", "highbyte"]


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


def ragged_offsets(rng, nseg, choices, head=0):
    lens = rng.choice(np.asarray(choices, dtype=np.int64), size=nseg)
    return np.concatenate([[head], head + np.cumsum(lens)]).astype(np.int64)


def index_values(n):
    return np.arange(n, dtype="<u4").view(np.uint8)


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("tname", KEY_TYPES)
def test_ragged_segments_every_key_type(rs, torch, ctx, tname, dist):
    """u32 values = the element's position in the array: a tie out of input order shows.  A head of 5 and a tail of 7
    elements that no segment covers."""
    kb = util.TYPES[tname][2]
    rng = np.random.default_rng(sum(map(ord, tname + dist)))
    offs = ragged_offsets(rng, 3000, [0, 1, 2, 63, 64, 65, 1000], head=5)
    n = int(offs[-1]) + 7
    keys_raw = util.make_input(tname, n, dist, seed=11)
    for desc in (False, True):
        check_all(rs, torch, ctx, tname, keys_raw, index_values(n), 4, offs, desc, index_types=(torch.int32, torch.int64),
                  what=(tname, dist))
        assert ctx.get_info(rs.INFO_LAST_PAIRS) == expected_info(kb, 4)
        assert (ctx.get_info(rs.INFO_LAST_PASSES) >> 24) & 0xF == 6


@pytest.mark.parametrize("tname", ["u32", "u64"])
@pytest.mark.parametrize("vb", [1, 2, 4, 8, 16, 20, 100, None])
def test_value_widths(rs, torch, ctx, tname, vb):
    """Values of 1 .. 16 bytes ride in the joined element, 20 and 100 bytes behind positions and a gather; None: the keys
    alone (descending, which no other call gives per segment)."""
    kb = util.TYPES[tname][2]
    rng = np.random.default_rng(100 + (vb or 0))
    offs = ragged_offsets(rng, 600, [0, 1, 2, 63, 64, 65, 1000], head=3)
    n = int(offs[-1]) + 2
    keys_raw = util.make_input(tname, n, "two" if vb in (2, 20) else "uniform", seed=21)
    values_raw = None
    if vb:
        v = rng.integers(0, 256, size=(n, vb), dtype=np.uint8)
        v[:, 0] = np.arange(n) & 0xFF  # (neighbours differ: a tie out of order shows)
        values_raw = v.reshape(-1)
    for desc in (True, False):
        check_all(rs, torch, ctx, tname, keys_raw, values_raw, vb or 0, offs, desc, what=(tname, vb))
        assert ctx.get_info(rs.INFO_LAST_PAIRS) == expected_info(kb, vb or 0), (tname, vb)
        assert ctx.get_info(rs.INFO_LAST_PASSES) == (6 << 24) | 3


def _edge_values(rng, n, vb):
    v = rng.integers(0, 256, size=(n, vb), dtype=np.uint8)
    v[:, :4] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)
    return v.reshape(-1)


@pytest.mark.parametrize("tname,vb,es", [("u32", 4, 8), ("f32", 8, 12), ("u128", 16, 32)])
def test_class_edges(rs, torch, ctx, tname, vb, es):
    """Lengths around the two LDS caps of the JOINED element and one far above the last, in one call; then lengths up to
    the first cap with that cap vouched for: fewer launches."""
    kb = util.TYPES[tname][2]
    assert joined_elem(kb, vb) == es
    caps = rs.segment_pairs_caps(kb, vb)
    cap0, cap1 = caps
    lens = [cap0 - 1, cap0, cap0 + 1, cap1 - 1, cap1, cap1 + 1, 2 * cap1 + 3]
    offs = np.concatenate([[1], 1 + np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1]) + 1
    rng = np.random.default_rng(es)
    keys_raw = util.make_input(tname, n, "uniform", seed=3)
    values_raw = _edge_values(rng, n, vb)
    for desc in (False, True):
        check_all(rs, torch, ctx, tname, keys_raw, values_raw, vb, offs, desc, what=(tname, "edges"))
        assert ctx.get_info(rs.INFO_LAST_PASSES) == (6 << 24) | 3
        assert ctx.get_info(rs.INFO_LAST_PAIRS) == 3 | es << 8
    check_all(rs, torch, ctx, tname, keys_raw, None, 0, offs, True, index_types=(torch.int64,), what=(tname, "edges, argsort"))
    lens = [cap0 - 1, cap0, 3, 0, 1, 70]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1])
    check_all(rs, torch, ctx, tname, keys_raw[:n * kb], values_raw[:n * vb], vb, offs, True, max_seg_len=cap0, what=(tname, "vouched"))
    assert ctx.get_info(rs.INFO_LAST_PASSES) == (6 << 24) | 1


def test_keys_that_agree_on_their_high_bytes(rs, torch, ctx):
    """u64 keys below 2^16 in segments of 4000: the passes that start at a high digit find every neighbour tied and the
    workgroup falls back to every pass (and stays there)."""
    n, seg = 10 * 4000 + 9, 4000
    rng = np.random.default_rng(5)
    keys_raw = rng.integers(0, 1 << 16, size=n, dtype=np.uint64).astype("<u8").view(np.uint8)
    offs = np.concatenate([[9], 9 + np.cumsum([seg] * 10)]).astype(np.int64)
    for desc in (False, True):
        check_all(rs, torch, ctx, "u64", keys_raw, index_values(n), 4, offs, desc, index_types=(torch.int32,), what="small integers")
    # ... and a few ties among keys that the high digits do tell apart: the mending path
    keys = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    keys[1::97] = keys[0::97][:len(keys[1::97])]
    keys_raw = keys.astype("<u8").view(np.uint8)
    for desc in (False, True):
        check_all(rs, torch, ctx, "u64", keys_raw, index_values(n), 4, offs, desc, what="a few ties")


@pytest.mark.parametrize("tname", ["f32", "f64"])
def test_float_specials_follow_the_total_order(rs, torch, ctx, tname):
    kb = util.TYPES[tname][2]
    if kb == 4:
        bits = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x3F800000, 0xBF800000], dtype="<u4")
    else:
        bits = np.array([0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000000,
                         0x3FF0000000000000, 0xBFF0000000000000], dtype="<u8")
    row = np.tile(bits, 8)  # one row of 64: +-0, +-inf, both NaN signs, +-1, each eight times
    keys_raw = np.concatenate([row, row[::-1]]).view(np.uint8)
    offs = np.array([0, 64, 128], dtype=np.int64)
    for desc in (False, True):
        check_all(rs, torch, ctx, tname, keys_raw, index_values(128), 4, offs, desc, index_types=(torch.int64,), what=tname)
        gk, _gv = sort_pairs(rs, torch, ctx, tname, keys_raw, index_values(128), 4, offs, desc)
        first = gk[GUARD:GUARD + 64 * kb].view(bits.dtype)[::8]
        order = [5, 3, 7, 1, 0, 6, 2, 4]  # -NaN < -inf < -1 < -0 < +0 < 1 < +inf < +NaN
        assert list(first) == list(bits[order[::-1] if desc else order])


def _torch_sort(torch, keys, desc):
    return torch.sort(keys, dim=-1, stable=True, descending=desc)


def _rows_case(rs, torch, c, shape, dtype, seed, desc):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    hi = 50 if seed % 2 else 2 ** 31 - 1  # (odd seeds: many ties)
    keys = torch.randint(-hi, hi, shape, dtype=dtype, device="cuda", generator=g)
    want = _torch_sort(torch, keys, desc)
    idx = rs.radix_argsort_rows(keys, descending=desc, ctx=c)
    c.check()
    assert idx.dtype == torch.int64 and idx.shape == keys.shape
    assert torch.equal(idx, want.indices), ("indices", shape, dtype, desc)
    out32 = torch.empty(shape, dtype=torch.int32, device="cuda")
    assert rs.radix_argsort_rows(keys, descending=desc, out=out32, ctx=c) is out32
    c.check()
    assert torch.equal(out32.to(torch.int64), want.indices)
    k = keys.clone()
    payload = torch.arange(keys.numel(), dtype=torch.int64, device="cuda").reshape(shape) * 3 + 1
    v = payload.clone()
    rs.radix_sort_rows_pairs(k, v, descending=desc, ctx=c)
    c.check()
    assert torch.equal(k, want.values), ("values", shape, dtype, desc)
    assert torch.equal(v, payload.gather(-1, want.indices)), ("payload", shape, dtype, desc)
    k = keys.clone()
    rs.radix_sort_rows_pairs(k, None, descending=desc, ctx=c)
    c.check()
    assert torch.equal(k, want.values), ("keys only", shape, dtype, desc)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
@pytest.mark.parametrize("shape", [(37, 1000), (2, 3, 513)])
def test_rows_against_torch_sort(rs, torch, ctx, shape, dtype_name, desc):
    dtype = getattr(torch, dtype_name)
    _rows_case(rs, torch, ctx, shape, dtype, seed=len(shape) * 2, desc=desc)
    _rows_case(rs, torch, ctx, shape, dtype, seed=len(shape) * 2 + 1, desc=desc)
    assert ctx.get_info(rs.INFO_LAST_PASSES) == (6 << 24) | 1


def test_rows_of_values_with_trailing_dimensions(rs, torch, ctx):
    """One value is values[..., j, :]: 3 floats (12 bytes, gathered) and 2 int64 (16 bytes, fused)."""
    keys = torch.randint(0, 100, (5, 7, 301), dtype=torch.int32, device="cuda")
    want = _torch_sort(torch, keys, True)
    for vals in (torch.rand(5, 7, 301, 3, device="cuda"), torch.randint(0, 1 << 40, (5, 7, 301, 2), dtype=torch.int64, device="cuda")):
        k, v = keys.clone(), vals.clone()
        rs.radix_sort_rows_pairs(k, v, descending=True, ctx=ctx)
        ctx.check()
        assert torch.equal(k, want.values)
        assert torch.equal(v, vals.gather(-2, want.indices[..., None].expand(vals.shape)))


def test_rows_above_the_largest_class(rs, torch, ctx):
    """A few long rows: the whole-array call row by row.  At least as many rows as the device has CUs: one launch of the
    through-memory class."""
    cap1 = rs.segment_pairs_caps(4, 4)[-1]
    _rows_case(rs, torch, ctx, (3, cap1 + 1), torch.int32, seed=8, desc=True)
    keys = torch.randint(-99, 99, (3, cap1 + 1), dtype=torch.int32, device="cuda")
    rs.radix_argsort_rows(keys, ctx=ctx)
    assert ctx.get_info(rs.INFO_LAST_PAIRS) == 1 | 8 << 8  # (the last row's whole-array call)
    rows = ctx.get_info(rs._lib.INFO_NUM_CU)
    _rows_case(rs, torch, ctx, (rows, cap1 + 1), torch.int32, seed=9, desc=False)
    keys = torch.randint(-99, 99, (rows, cap1 + 1), dtype=torch.int32, device="cuda")
    idx = rs.radix_argsort_rows(keys, descending=True, ctx=ctx)
    ctx.check()
    assert ctx.get_info(rs.INFO_LAST_PASSES) == (6 << 24) | 1
    assert ctx.get_info(rs.INFO_LAST_PAIRS) == 3 | 8 << 8
    assert torch.equal(idx, _torch_sort(torch, keys, True).indices)


def test_rows_of_one_element_and_fresh_argsort_output(rs, torch, ctx):
    keys = torch.randint(0, 100, (9, 1), dtype=torch.int32, device="cuda")
    out = torch.full((9, 1), -7, dtype=torch.int64, device="cuda")
    assert rs.radix_argsort_rows(keys, out=out, ctx=ctx) is out
    ctx.check()
    assert torch.equal(out, torch.zeros_like(out))
    k1 = torch.randint(0, 100, (50,), dtype=torch.int32, device="cuda")
    o = torch.tensor([10, 10, 11, 30], dtype=torch.int64, device="cuda")
    got = rs.radix_argsort_segments(k1, o, ctx=ctx)  # a fresh out is zero-filled: the slots no segment covers are defined
    ctx.check()
    assert got.dtype == torch.int64 and got.shape == (50,)
    assert torch.equal(got[:11], torch.zeros(11, dtype=torch.int64, device="cuda")) and torch.equal(got[30:], torch.zeros(20, dtype=torch.int64, device="cuda"))
    assert torch.equal(got[11:30], torch.sort(k1[11:30], stable=True).indices)


@pytest.mark.parametrize("vb", [4, 20])
def test_untrusted_offsets(rs, torch, vb):
    """A decreasing pair inside [0, n) and a last offset of n + 8, with the columns views of larger tensors the test owns:
    the good neighbours are sorted, the bad segments' keys, values and index byte-identical to the input, check() raises
    once and the context works again."""
    c = rs.Context(torch.cuda.current_device())
    tname, kb, n, extra = "u32", 4, 10000, 4096
    keys_all = util.make_input(tname, n + extra, "uniform", seed=51)
    rng = np.random.default_rng(52)
    vals_all = rng.integers(0, 256, size=(n + extra) * vb, dtype=np.uint8)
    # segments: [4000, 5000) good, [5000, 1000) decreasing, [1000, 3000) good, [3000, 3500) good, [3500, n + 8) ends behind n
    offs = [4000, 5000, 1000, 3000, 3500, n + 8]
    o = torch.tensor(offs, dtype=torch.int64, device="cuda")
    for desc in (False, True):
        wk, wv, local = segments_reference(keys_all[:n * kb], vals_all[:n * vb], kb, U, vb, desc, offs)
        for max_len in (0, 2000):
            kbig = torch.from_numpy(keys_all.copy()).cuda()
            vbig = torch.from_numpy(vals_all.copy()).cuda()
            rs.radix_sort_segments_pairs(kbig[:n * kb].view(torch.uint32), vbig[:n * vb].view(n, vb), o, descending=desc, max_seg_len=max_len, ctx=c)
            with pytest.raises(rs.RsxError) as e:
                c.check()
            assert e.value.status == rs._lib.ERR_INTERNAL
            c.check()  # the condition was cleared
            assert np.array_equal(kbig.cpu().numpy(), np.concatenate([wk, keys_all[n * kb:]]))
            assert np.array_equal(vbig.cpu().numpy(), np.concatenate([wv, vals_all[n * vb:]]))
        kbig = torch.from_numpy(keys_all.copy()).cuda()
        ibig = torch.full(((n + extra) * 8,), 0xA5, dtype=torch.uint8, device="cuda")
        rs.radix_argsort_segments(kbig[:n * kb].view(torch.uint32), o, descending=desc, out=ibig[:n * 8].view(torch.int64), ctx=c)
        with pytest.raises(rs.RsxError):
            c.check()
        c.check()
        assert np.array_equal(kbig.cpu().numpy(), keys_all)
        assert np.array_equal(ibig.cpu().numpy(), np.concatenate([expected_index(local, 8), np.full(extra * 8, 0xA5, dtype=np.uint8)]))
    # the context works again
    check_all(rs, torch, c, tname, keys_all[:n * kb], vals_all[:n * vb], vb, [0, 5000, n], True, what="after the error")
    c.close()


def test_graph_capture(rs, torch):
    """The LDS classes touch no workspace: after one warm-up call radix_argsort_rows captures into a graph (one branch)
    on a context that never reserved anything.  A through-memory shape needs reserve_pairs first."""
    c = rs.Context(torch.cuda.current_device())
    rows, L = 64, 1000
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, L), dtype=torch.int32, device="cuda")
    keys = torch.empty_like(src)
    out = torch.empty((rows, L), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        keys.copy_(src)
        rs.radix_argsort_rows(keys, descending=True, out=out, ctx=c)  # warm-up outside capture
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        keys.copy_(src)
        rs.radix_argsort_rows(keys, descending=True, out=out, ctx=c)
    for seed in (1, 2):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        src.copy_(torch.randint(-50 * seed, 50 * seed, (rows, L), dtype=torch.int32, device="cuda", generator=g))
        out.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        assert torch.equal(out, torch.sort(src, dim=-1, stable=True, descending=True).indices)
    # a shape of the through-memory class: RSX_ERR_WORKSPACE under capture without a reserve, nothing enqueued
    cap1 = rs.segment_pairs_caps(4, 4)[-1]
    rows = c.get_info(rs._lib.INFO_NUM_CU)
    big = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, cap1 + 1), dtype=torch.int32, device="cuda")
    bout = torch.full((rows, cap1 + 1), -1, dtype=torch.int32, device="cuda")
    g2 = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g2.capture_begin()
        try:
            rs.radix_argsort_rows(big, out=bout, ctx=c)
        except rs.RsxError as e:
            err = e
        g2.capture_end()
    assert err is not None and err.status == rs._lib.ERR_WORKSPACE, err
    torch.cuda.synchronize()
    assert bool((bout == -1).all())  # nothing was enqueued
    c.reserve_pairs(big.numel(), 4, 4)
    g3 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g3, stream=s):
        rs.radix_argsort_rows(big, out=bout, ctx=c)
    g3.replay()
    torch.cuda.synchronize()
    c.check()
    assert torch.equal(bout.to(torch.int64), torch.sort(big, dim=-1, stable=True).indices)
    c.close()


@pytest.mark.parametrize("vb", [12, 3])
def test_reserve_pairs_then_captured_wide_values(rs, torch, vb):
    """reserve_pairs alone readies a fresh context for a CAPTURED call on values without a fused kernel (route 4: proxies,
    the copy of the values behind them, a gather): 12-byte values, and 3-byte ones, for which that route's workspace is
    the largest of the three sizes the reserve entry asks for.  Three segments of 4099 keys, a head and a tail outside."""
    from segment_pairs_gpu import guarded, key_tensor, same
    from segment_pairs_ref import with_guards
    n, offs = 4099, [3, 1400, 2801, 4090]
    rng = np.random.default_rng(vb)
    keys_raw = util.make_input("u32", n, "two", seed=5)
    v = rng.integers(0, 256, size=(n, vb), dtype=np.uint8)
    v[:, 0] = np.arange(n) & 0xFF  # (neighbours differ: a tie out of order shows)
    values_raw = v.reshape(-1)
    wk, wv, _local = segments_reference(keys_raw, values_raw, 4, U, vb, True, offs)
    c = rs.Context(torch.cuda.current_device())
    c.reserve_pairs(n, 4, vb)
    kbuf, kmid = guarded(torch, keys_raw)
    vbuf, vmid = guarded(torch, values_raw)
    o = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        rs.radix_sort_segments_pairs(key_tensor(torch, kmid, "u32"), vmid.view(n, vb), o, descending=True, ctx=c)
    graph.replay()
    torch.cuda.synchronize()
    c.check()
    assert c.get_info(rs.INFO_LAST_PAIRS) == expected_info(4, vb)
    assert same(kbuf.cpu().numpy(), with_guards(wk, 0), ("keys", vb))
    assert same(vbuf.cpu().numpy(), with_guards(wv, 0), ("values", vb))
    c.close()
