"""GPU: rsx_unique_device / radix_group / radix_unique against tests/unique_ref.py, byte for byte.

Every output sits in an allocation the test owns: 64 guard bytes of 0xA5, the array filled with 0xA5, 64 guard bytes.  What
comes back is compared whole: the entries the definition writes hold the reference's bytes, the entries of out_keys at m
and beyond, those of out_offsets beyond m and all guards still hold 0xA5; the key column is compared with its input.

The sizes come from rsx_unique_caps (T = tile, S = scan_span), so that they stay the edge cases of the kernels whatever
their constants are.  Keys of a shape are made from GROUP IDS, mapped to the key type by an increasing map (folded into
the type's range where it is too small for the ids: u8 and i16 then get other, still valid, groups)."""
import numpy as np
import pytest

import util
from segment_pairs_gpu import guarded, key_dtype, same
from segment_pairs_ref import segments_reference, with_guards
from unique_ref import unique_reference

pytestmark = pytest.mark.gpu

KEY_TYPES = ["u8", "i16", "u32", "i32", "f32", "i64", "f64", "u128", "i128"]
SHAPES = ["equal", "distinct", "runs_of_tile", "runs_shifted", "long_run", "seven", "third"]
PATH = 8 << 24
F32_SPECIALS = np.array([0xFFC00000, 0xFF800000, 0x80000000, 0x00000000, 0x7F800000, 0x7FC00000, 0x7FC00001], dtype="<u4")
F64_SPECIALS = np.array([0xFFF8000000000000, 0xFFF0000000000000, 0x8000000000000000, 0x0, 0x7FF0000000000000, 0x7FF8000000000000,
                         0x7FF8000000000001], dtype="<u8")  # -NaN, -inf, -0.0, +0.0, +inf, NaN, NaN of another payload


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


# ---- inputs ----
def group_ids(shape, n, T, rng):
    """n group ids (int64, in input order) whose sorted order has the runs the shape names."""
    if shape == "equal":  # m = 1: one run across every tile
        g = np.zeros(n, dtype=np.int64)
    elif shape == "distinct":  # m = n
        g = np.arange(n, dtype=np.int64)
    elif shape == "runs_of_tile":  # runs of exactly T from 0 on: every head is the first slot of a tile
        g = np.arange(n, dtype=np.int64) // T
    elif shape == "runs_shifted":  # a first run of T - 1: every later head is the last slot of a tile
        g = (np.arange(n, dtype=np.int64) + 1) // T
    elif shape == "long_run":  # runs of 1, a run over three whole tiles and parts of two more, runs of 1
        g = np.arange(n, dtype=np.int64)
        lo = min(5, n // 4)
        hi = min(n, lo + 3 * T + 7)
        g[lo:hi] = lo
    elif shape == "seven":
        g = rng.integers(0, 7, size=n, dtype=np.int64)
    elif shape == "third":
        g = rng.integers(0, max(1, n // 3), size=n, dtype=np.int64)
    else:
        raise ValueError(shape)
    return rng.permutation(g)


def keys_of(tname, g):
    """Raw key bytes for group ids g: an increasing map into the key type (both signs, floats of both signs)."""
    _es, _ko, kb, kind = util.TYPES[tname]
    n = g.size
    if kind == util.FLOAT:
        if int(g.max(initial=0)) < 7:  # the special values, in their order: -NaN -inf -0.0 +0.0 +inf NaN NaN'
            sp = F32_SPECIALS if kb == 4 else F64_SPECIALS
            return sp[g].view(np.uint8).reshape(-1).copy()
        v = (g - (int(g.max()) // 2)).astype("<f4" if kb == 4 else "<f8")  # exact below 2^24
        return v.view(np.uint8).reshape(-1).copy()
    if kb <= 8:
        span = 1 << (8 * kb)
        v = g % span if kb < 8 else g
        if kind == util.SIGNED:
            v = v - min(span // 2, max(1, int(v.max(initial=0)) // 2))
        return v.astype("<i8").view(np.uint8).reshape(n, 8)[:, :kb].reshape(-1).copy()
    # 128 bits: neighbouring ids differ in the low half only, every other pair in the high half
    hi = g // 2
    if kind == util.SIGNED:
        hi = hi - max(1, int(hi.max(initial=0)) // 2)
    out = np.zeros((n, 2), dtype="<u8")
    out[:, 0] = (g % 2).astype("<u8") << np.uint64(63)
    out[:, 1] = hi.astype("<i8").view("<u8")
    return out.view(np.uint8).reshape(-1).copy()


# ---- one call on guarded buffers ----
def canary(nbytes):
    return np.full(nbytes, 0xA5, dtype=np.uint8)


def first_then_canary(raw, nbytes):
    out = canary(nbytes)
    out[:raw.size] = raw
    return out


class Case:
    """One key column on the GPU (guarded) with its references per order, and unique_device calls on it."""

    def __init__(self, torch, c, tname, keys_raw):
        self.torch, self.c, self.tname = torch, c, tname
        self.kb, self.kind = util.TYPES[tname][2], util.TYPES[tname][3]
        self.keys_raw = keys_raw
        self.n = keys_raw.size // self.kb
        self.kbuf, self.kmid = guarded(torch, keys_raw)
        self.refs = {}

    def reference(self, desc):
        if desc not in self.refs:
            self.refs[desc] = unique_reference(self.keys_raw, self.kb, self.kind, desc)
        return self.refs[desc]

    def run(self, desc, keys=True, offsets=True, perm=False, inverse=False, ib=8, what=None):
        torch, n, kb = self.torch, self.n, self.kb
        bufs = {}
        for name, want, nbytes in (("keys", keys, n * kb), ("offsets", offsets, (n + 1) * 8), ("perm", perm, n * ib),
                                   ("inverse", inverse, n * ib), ("num", True, 8)):
            bufs[name] = guarded(torch, canary(nbytes)) if want else (None, None)
        ptr = {k: (v[1].data_ptr() if v[1] is not None else 0) for k, v in bufs.items()}
        if n == 0:  # (an empty view has no address of its own; the guards still do)
            ptr = {k: (bufs[k][0].data_ptr() + 64 if bufs[k][0] is not None else 0) for k in bufs}
        self.c.unique_device(self.kmid.data_ptr() if n else 0, n, kb, self.kind, ptr["keys"], ptr["offsets"], ptr["perm"], ptr["inverse"], ib,
                             ptr["num"], desc, torch.cuda.current_stream().cuda_stream)
        self.c.check()
        wk, wo, wp, wi, m = self.reference(desc)
        tag = (self.tname, n, what, "desc" if desc else "asc", ib)
        idt = "<i4" if ib == 4 else "<i8"
        assert same(bufs["num"][0].cpu().numpy(), with_guards(np.array([m], dtype="<u8")), ("num",) + tag)
        if keys:
            assert same(bufs["keys"][0].cpu().numpy(), with_guards(first_then_canary(wk, n * kb)), ("out_keys",) + tag)
        if offsets:
            assert same(bufs["offsets"][0].cpu().numpy(), with_guards(first_then_canary(wo.astype("<u8").view(np.uint8), (n + 1) * 8)),
                        ("out_offsets",) + tag)
        if perm:
            assert same(bufs["perm"][0].cpu().numpy(), with_guards(wp.astype(idt)), ("out_perm",) + tag)
        if inverse:
            assert same(bufs["inverse"][0].cpu().numpy(), with_guards(wi.astype(idt)), ("out_inverse",) + tag)
        return m

    def keys_unchanged(self):
        assert same(self.kbuf.cpu().numpy(), with_guards(self.keys_raw), ("the key column", self.tname, self.n))


def run_combinations(case, desc, what, rs, full):
    """keys only (the route without positions), all outputs, inverse without perm, perm without keys."""
    c = case.c
    case.run(desc, what=(what, "keys only"))
    assert c.get_info(rs.INFO_LAST_PASSES) == PATH | 3
    assert c.get_info(rs.INFO_LAST_PAIRS) == 1 | case.kb << 8
    case.run(desc, perm=True, inverse=True, ib=8, what=(what, "all"))
    assert c.get_info(rs.INFO_LAST_PASSES) == PATH | 3
    assert c.get_info(rs.INFO_LAST_PAIRS) == 1 | {1: 8, 2: 8, 4: 8, 8: 16, 16: 32}[case.kb] << 8
    if full:
        case.run(desc, inverse=True, ib=4, what=(what, "inverse without perm"))
        case.run(desc, keys=False, perm=True, ib=4, what=(what, "perm without keys"))
        case.run(desc, keys=False, offsets=False, perm=True, inverse=True, ib=4, what=(what, "perm and inverse alone"))


def sizes_for(rs, kb):
    """The small sizes, and those around one and two tiles of EITHER route."""
    ns = {1, 2, 63, 64, 65}
    for pos in (False, True):
        T, _S = rs.unique_caps(kb, pos)
        ns |= {T - 1, T, T + 1, 2 * T - 1, 2 * T + 1}
    return sorted(ns)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", KEY_TYPES)
def test_every_key_type_shape_and_small_size(rs, torch, ctx, tname, desc):
    kb = util.TYPES[tname][2]
    T = rs.unique_caps(kb, True)[0]
    rng = np.random.default_rng(kb * 2 + desc)
    for n in sizes_for(rs, kb):
        for si, shape in enumerate(SHAPES):
            case = Case(torch, ctx, tname, keys_of(tname, group_ids(shape, n, T, rng)))
            m = case.reference(desc)[4]
            if shape == "equal":
                assert m == 1
            if shape == "distinct" and kb >= 4:
                assert m == n
            run_combinations(case, desc, shape, rs, full=(n % 2 == 1 or si == 0))
            case.keys_unchanged()


@pytest.mark.parametrize("tname", ["f32", "f64"])
def test_float_specials(rs, torch, ctx, tname):
    """+-0.0, +-inf and NaNs of two payloads among ordinary values: the total order on bit patterns, bit-pattern equality."""
    kb = util.TYPES[tname][2]
    sp = (F32_SPECIALS if kb == 4 else F64_SPECIALS).view(np.uint8).reshape(7, kb)
    rng = np.random.default_rng(5)
    for n in (64, rs.unique_caps(kb, True)[0] + 1):
        raw = keys_of(tname, rng.integers(7, 40, size=n, dtype=np.int64)).reshape(n, kb)
        where = rng.random(n) < 0.5
        raw[where] = sp[rng.integers(0, 7, size=int(where.sum()))]
        case = Case(torch, ctx, tname, raw.reshape(-1).copy())
        for desc in (False, True):
            wk = case.reference(desc)[0].reshape(-1, kb)
            order = [bytes(r) for r in (sp[::-1] if desc else sp)]
            got = [bytes(r) for r in wk if bytes(r) in order]
            assert got[:2] == order[:2] and got[-2:] == order[-2:] and len(got) == 7  # -NaN first ... the NaNs last, all seven apart
            run_combinations(case, desc, "specials", rs, full=True)
        case.keys_unchanged()


def big_sizes(rs):
    out = []
    for pos in (False, True):
        T, S = rs.unique_caps(4, pos)
        out += [(pos, "S*T-1", S * T - 1), (pos, "S*T+1", S * T + 1), (pos, "(2S+1)*T+17", (2 * S + 1) * T + 17)]
    out.append((True, "2^22+3", (1 << 22) + 3))  # the sort's multi-launch path, a workspace of its size
    return out


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("which", range(7))
def test_scan_sweeps_and_the_large_sort(rs, torch, ctx, which, shape):
    """Around one sweep of the scan kernel's loop, over several sweeps, and behind the sort's multi-launch path: u32 keys,
    the route whose tile the size is made from, one order per case."""
    import radix_sort_amd
    pos, name, n = big_sizes(radix_sort_amd)[which]
    T = rs.unique_caps(4, pos)[0]
    desc = (which + SHAPES.index(shape)) % 2 == 1
    rng = np.random.default_rng(which)
    case = Case(torch, ctx, "u32", keys_of("u32", group_ids(shape, n, T, rng)))
    if pos:
        case.run(desc, perm=True, inverse=True, ib=4, what=(shape, name))
    else:
        case.run(desc, what=(shape, name))
    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 3
    case.keys_unchanged()


def test_num_alone_takes_two_kernels(rs, torch, ctx):
    case = Case(torch, ctx, "i32", util.make_input("i32", 10007, "step16", seed=3))
    assert case.run(False, keys=False, offsets=False) == 16
    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 2


def test_empty_and_single(rs, torch, ctx):
    empty = Case(torch, ctx, "u32", np.zeros(0, dtype=np.uint8))
    assert empty.run(False) == 0  # num == 0, offsets[0] == 0, nothing else
    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH
    assert empty.run(True, perm=True, inverse=True) == 0
    g = rs.radix_group(torch.zeros(0, dtype=torch.int32, device="cuda"), inverse=True, ctx=ctx)
    assert int(g.num) == 0 and int(g.offsets[0]) == 0 and g.keys.numel() == 0 and g.perm.numel() == 0 and g.inverse.numel() == 0
    for tname in ("u8", "f64", "u128"):
        one = Case(torch, ctx, tname, util.make_input(tname, 1, "uniform", seed=1))
        for desc in (False, True):
            run_combinations(one, desc, "n = 1", rs, full=True)
    g = rs.radix_group(torch.full((1,), -7, dtype=torch.int64, device="cuda"), inverse=True, ctx=ctx)
    assert int(g.num) == 1 and g.keys.tolist() == [-7] and g.offsets.tolist() == [0, 1] and g.perm.tolist() == [0] and g.inverse.tolist() == [0]


@pytest.mark.parametrize("tname", ["u8", "i16", "i32", "i64", "f32", "f64"])
def test_radix_unique_equals_torch_unique(rs, torch, ctx, tname):
    """Integer dtypes, and floats without NaN or -0.0 (where the two orders and the two equalities agree)."""
    dt = key_dtype(torch, tname)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    for n, span in ((1, 5), (1000, 7), (20011, 3000)):
        x = torch.randint(-span if tname != "u8" else 0, span, (n,), device="cuda", generator=gen).to(dt)
        if dt.is_floating_point:
            x = x * 0.5 + 0.25  # (no -0.0)
        want = torch.unique(x, sorted=True, return_inverse=True, return_counts=True)
        got = rs.radix_unique(x, return_inverse=True, return_counts=True, ctx=ctx)
        ctx.check()
        assert len(got) == 3
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w)
        assert torch.equal(rs.radix_unique(x, ctx=ctx), want[0])
        keys_d, counts_d = rs.radix_unique(x, return_counts=True, descending=True, ctx=ctx)
        assert torch.equal(keys_d, want[0].flip(0)) and torch.equal(counts_d, want[2].flip(0))


def test_group_fields_and_128_bit_keys(rs, torch, ctx):
    n = 5000
    raw = util.make_input("i128", n, "two", seed=4)
    keys = torch.from_numpy(raw.copy()).cuda().view(n, 16)
    wk, wo, wp, wi, m = unique_reference(raw, 16, util.SIGNED, True)
    g = rs.radix_group(keys, descending=True, inverse=True, index_dtype=torch.int32, ctx=ctx, key_kind=rs.KEY_SIGNED)
    ctx.check()
    assert isinstance(g, rs.Group) and g.num.dim() == 0 and g.num.dtype == torch.int64 and int(g.num) == m == 2
    assert g.keys.shape == (n, 16) and g.offsets.shape == (n + 1,) and g.offsets.dtype == torch.int64
    assert g.perm.dtype == torch.int32 and g.inverse.dtype == torch.int32
    assert np.array_equal(g.keys[:m].cpu().numpy().reshape(-1), wk)
    assert np.array_equal(g.offsets[:m + 1].cpu().numpy(), wo)
    assert np.array_equal(g.perm.cpu().numpy(), wp) and np.array_equal(g.inverse.cpu().numpy(), wi)
    g = rs.radix_group(keys, perm=False, ctx=ctx)  # unsigned by default, keys only
    assert g.perm is None and g.inverse is None
    wk, wo, _p, _i, m = unique_reference(raw, 16, util.UNSIGNED, False)
    assert int(g.num) == m and np.array_equal(g.keys[:m].cpu().numpy().reshape(-1), wk) and np.array_equal(g.offsets[:m + 1].cpu().numpy(), wo)
    assert np.array_equal(keys.cpu().numpy().reshape(-1), raw)


def test_offsets_feed_the_segmented_sort(rs, torch, ctx):
    """Group by a first key, then sort every group by a second key with radix_sort_segments_pairs: the offsets go from
    radix_group to the segmented call on the device, the host only slices them."""
    n = 30011
    rng = np.random.default_rng(8)
    a_raw = rng.integers(0, 97, size=n, dtype=np.int64).astype("<i4").view(np.uint8)
    b_raw = util.make_input("f32", n, "uniform", seed=9)
    a = torch.from_numpy(a_raw.copy()).cuda().view(torch.int32)
    b = torch.from_numpy(b_raw.copy()).cuda().view(torch.float32)
    g = rs.radix_group(a, ctx=ctx)
    m = int(g.num)
    keys2 = b[g.perm].contiguous()
    vals2 = g.perm.clone()
    rs.radix_sort_segments_pairs(keys2, vals2, g.offsets[:m + 1], ctx=ctx)
    ctx.check()
    _k, wo, wp, _i, wm = unique_reference(a_raw, 4, util.SIGNED, False)
    assert m == wm == 97
    gathered = b_raw.reshape(n, 4)[wp].reshape(-1)
    wk2, wv2, _local = segments_reference(gathered, wp.astype("<i8").view(np.uint8), 4, util.FLOAT, 8, False, wo)
    assert np.array_equal(keys2.view(torch.uint8).cpu().numpy().reshape(-1), wk2)
    assert np.array_equal(vals2.cpu().numpy().view(np.uint8).reshape(-1), wv2)


def test_capture_and_replay(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    n = 300001
    c.reserve_unique(n, 4, True)
    inputs = [util.make_input("u32", n, dist, seed=70 + i) for i, dist in enumerate(("step16", "highbyte"))]
    src = torch.from_numpy(inputs[0].copy()).cuda().view(torch.uint32)
    keys = torch.empty_like(src)
    out_keys = torch.empty_like(src)
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    inverse = torch.empty(n, dtype=torch.int32, device="cuda")
    num = torch.empty((), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()

    def enqueue():
        c.unique_device(keys.data_ptr(), n, 4, rs.KEY_UNSIGNED, out_keys.data_ptr(), offsets.data_ptr(), perm.data_ptr(), inverse.data_ptr(), 4,
                        num.data_ptr(), True, torch.cuda.current_stream().cuda_stream)

    with torch.cuda.stream(s):
        keys.copy_(src)
        enqueue()  # warm-up outside capture
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):  # one linear chain: the copy, then the call's launches
        keys.copy_(src)
        enqueue()
    for raw in inputs:
        src.view(torch.uint8).copy_(torch.from_numpy(raw.copy()))
        for t in (out_keys.view(torch.int32), offsets, perm, inverse):
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        wk, wo, wp, wi, m = unique_reference(raw, 4, util.UNSIGNED, True)
        assert int(num) == m
        assert np.array_equal(out_keys[:m].view(torch.uint8).cpu().numpy().reshape(-1), wk)
        assert np.array_equal(offsets[:m + 1].cpu().numpy(), wo) and bool((offsets[m + 1:] == -1).all())
        assert np.array_equal(perm.cpu().numpy(), wp) and np.array_equal(inverse.cpu().numpy(), wi)
    c.close()


def test_unreserved_call_under_capture_reports_workspace(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    x = torch.randint(0, 2 ** 31 - 1, (1000,), dtype=torch.int32, device="cuda")
    rs.radix_sort(x, ctx=c)  # one ordinary call: the context's error word and self-tests exist
    c.check()
    n = 1 << 16
    keys = torch.randint(0, 1000, (n,), dtype=torch.int32, device="cuda")
    before = keys.clone()
    outs = [torch.full((n + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(4)]
    num = torch.full((), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g.capture_begin()
        try:
            c.unique_device(keys.data_ptr(), n, 4, rs.KEY_SIGNED, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), 8,
                            num.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
        except rs.RsxError as e:
            err = e
        g.capture_end()
    assert err is not None and err.status == rs._lib.ERR_WORKSPACE, err
    torch.cuda.synchronize()
    assert torch.equal(keys, before) and int(num) == -1 and all(bool((o == -1).all()) for o in outs)  # nothing was enqueued
    c.close()


def test_errors(rs, torch, ctx):
    E = rs._lib
    case = Case(torch, ctx, "u32", util.make_input("u32", 200, "two", seed=2))
    L, h = ctx._L, ctx._h
    buf = torch.full((5 * 4096,), 0xA5, dtype=torch.uint8, device="cuda")  # a region of 4 KiB per output
    p = buf.data_ptr()
    k = case.kmid.data_ptr()
    assert p % 16 == 0 and k % 16 == 0
    ok = dict(keys=k, n=200, kb=4, kind=0, order=0, ok_=p, off=p + 4096, perm=p + 2 * 4096, inv=p + 3 * 4096, ib=8, num=p + 4 * 4096)

    def call(**kw):
        a = dict(ok, **kw)
        return L.rsx_unique_device(h, a["keys"] or None, a["n"], a["kb"], a["kind"], a["order"], a["ok_"] or None, a["off"] or None,
                                   a["perm"] or None, a["inv"] or None, a["ib"], a["num"] or None, None)

    assert call(kb=3) == E.ERR_ARG                      # key width
    assert call(kb=16, kind=2) == E.ERR_ARG             # float keys of 16 bytes
    assert call(order=2) == E.ERR_ARG
    assert call(num=0) == E.ERR_ARG                     # d_out_num is required
    assert call(ib=2) == E.ERR_ARG
    assert call(ib=2, perm=0, inv=0) == E.OK            # index_bytes is not looked at without perm and inverse
    ctx.check()
    assert call(keys=0) == E.ERR_ARG                    # null keys with n > 0
    assert call(keys=k + 2) == E.ERR_ARG                # misaligned, each pointer in turn
    assert call(ok_=p + 2) == E.ERR_ARG
    assert call(off=p + 4096 + 4) == E.ERR_ARG
    assert call(num=p + 4 * 4096 + 4) == E.ERR_ARG
    assert call(perm=p + 2 * 4096 + 4) == E.ERR_ARG
    assert call(inv=p + 3 * 4096 + 4, perm=0) == E.ERR_ARG
    assert call(perm=p + 2 * 4096 + 4, ib=4, inv=0) == E.OK        # naturally aligned is enough: the element-by-element form
    ctx.check()
    assert call(n=2 ** 32) == E.ERR_UNSUPPORTED         # dummy pointers, nothing launched
    assert L.rsx_ctx_reserve_unique(h, 2 ** 32, 4, 1) == E.ERR_UNSUPPORTED
    assert L.rsx_ctx_reserve_unique(h, 100, 3, 1) == E.ERR_ARG
    torch.cuda.synchronize()
    case.run(True, perm=True, inverse=True, ib=4)  # the context works on
    case.keys_unchanged()


def test_perm_at_natural_alignment(rs, torch, ctx):
    """An out_perm that is 4-byte but not 16-byte aligned takes the element-by-element stores: the same bytes."""
    n = rs.unique_caps(4, True)[0] * 2 + 5
    raw = util.make_input("i32", n, "step16", seed=12)
    keys = torch.from_numpy(raw.copy()).cuda().view(torch.int32)
    buf = torch.full((n + 8,), -1, dtype=torch.int32, device="cuda")
    perm = buf[1:1 + n]
    assert perm.data_ptr() % 16 == 4
    num = torch.zeros((), dtype=torch.int64, device="cuda")
    ctx.unique_device(keys.data_ptr(), n, 4, rs.KEY_SIGNED, 0, 0, perm.data_ptr(), 0, 4, num.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
    ctx.check()
    _k, _o, wp, _i, m = unique_reference(raw, 4, util.SIGNED, False)
    assert int(num) == m and np.array_equal(perm.cpu().numpy(), wp)
    assert int(buf[0]) == -1 and bool((buf[1 + n:] == -1).all())
