"""GPU: separate key and value arrays (radix_sort_pairs, radix_argsort; rsx_sort_pairs_device, rsx_argsort_device),
bit-exact against tests/pairs_ref.py: the stable permutation by mapped key, ascending and descending.

The permutation comes from the numpy reference; keys and indices are compared on the host, the value rows (up to
256 bytes each) on the device against values_in[perm], so that the large cases stay cheap."""
import numpy as np
import pytest

import util
from pairs_ref import pairs_reference

pytestmark = pytest.mark.gpu

U, S, F = util.UNSIGNED, util.SIGNED, util.FLOAT
KEY_TYPES = ["u8", "u16", "u32", "u64", "i8", "i16", "i32", "i64", "f32", "f64", "u128", "i128"]
VALUE_BYTES = [0, 1, 2, 4, 8, 16, 3, 12, 40, 256]  # none; typed; odd, joined; proxies and gather
TILE_KEYS = {1: 28, 2: 28, 4: 28, 8: 14, 12: 10, 16: 5, 24: 5, 32: 3}  # keys per thread of the 512-thread one-launch tile
GUARD = 256  # bytes of 0xA5 in front of and behind every array (a multiple of 16: the arrays stay 16-byte aligned)


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


# ---- include/rsx.h restated: where the value sits in the joined element and how large that element is ----
def voff(kb, vb):
    a = 1 if vb == 0 else 4 if vb % 4 == 0 else 2 if vb % 2 == 0 else 1
    return (kb + a - 1) // a * a


def joined_elem(kb, vb):
    need = voff(kb, vb) + vb
    return next((z for z in (1, 2, 4, 8, 12, 16, 24, 32) if z >= need and z % kb == 0), 0)


def expected_info(kb, vb):
    es = joined_elem(kb, vb)
    return (1 | es << 8) if es else (2 | joined_elem(kb, 4) << 8)


def sizes_for(kb, vb):
    tile = 512 * TILE_KEYS[joined_elem(kb, vb) or joined_elem(kb, 4)]
    return [0, 1, 2, 255, tile - 1, tile + 1, 200003, (1 << 22) + 5]


def key_dtype(torch, tname):
    return {"u8": torch.uint8, "i8": torch.int8, "i16": torch.int16, "i32": torch.int32, "i64": torch.int64, "f32": torch.float32,
            "f64": torch.float64, "u16": torch.uint16, "u32": torch.uint32, "u64": torch.uint64}.get(tname)


class Guarded:
    """A device array of `nbytes` bytes between two guards of 0xA5, `shift` bytes behind a 256-byte boundary."""

    def __init__(self, torch, nbytes, shift=0):
        self.torch, self.lo, self.nbytes = torch, GUARD + shift, nbytes
        self.buf = torch.full((self.lo + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    def bytes(self):
        return self.buf[self.lo:self.lo + self.nbytes]

    def intact(self):
        t = self.torch
        return bool(t.all(self.buf[:self.lo] == 0xA5)) and bool(t.all(self.buf[self.lo + self.nbytes:] == 0xA5))


def key_tensor(torch, g, tname, n):
    kb = util.TYPES[tname][2]
    if kb == 16:
        return g.bytes().view(n, 16)
    return g.bytes().view(key_dtype(torch, tname))


def make_values(torch, n, vb):
    """(n, vb) uint8 on the device: bytes 4g .. 4g+3 of row i hold i * M[g] mod 2^32, M[0] = 1 (the row's index)."""
    groups = (vb + 3) // 4
    mult = torch.tensor([1] + [2654435761 + 2 * 40503 * g for g in range(1, groups)], dtype=torch.int64, device="cuda")
    t = (torch.arange(n, dtype=torch.int64, device="cuda")[:, None] * mult[None, :]) & 0xFFFFFFFF
    t = (t - ((t >> 31) << 32)).to(torch.int32)  # the same 32 bits as a signed number
    return t.view(torch.uint8).reshape(n, groups * 4)[:, :vb].contiguous()


def dist_for(tname, i):
    kind = util.TYPES[tname][3]
    if kind == F and i % 2 == 0:
        return "uniform"  # util.make_input puts NaN of both signs, +-0, +-inf among them
    return util.DISTS[(KEY_TYPES.index(tname) * 3 + i) % len(util.DISTS)]


def run_pairs(rs, torch, c, tname, keys_raw, vb, desc, perm, want_keys, shift=0):
    _es, _ko, kb, kind = util.TYPES[tname]
    n = keys_raw.size // kb
    gk = Guarded(torch, n * kb, shift=(shift * kb) % 256)
    gk.bytes().copy_(torch.from_numpy(keys_raw))
    keys = key_tensor(torch, gk, tname, n)
    vals = gv = vin = None
    if vb:
        vin = make_values(torch, n, vb)
        va = next(a for a in (16, 8, 4, 2, 1) if vb % a == 0)
        gv = Guarded(torch, n * vb, shift=(shift * va) % 256)
        gv.bytes().copy_(vin.reshape(-1))
        vals = gv.bytes().view(n, vb)
    rs.radix_sort_pairs(keys, vals, descending=desc, ctx=c, key_kind=(kind if kb == 16 else None))
    c.check()
    what = (tname, vb, desc, n, shift)
    assert gk.intact(), ("key guards", what)
    assert np.array_equal(gk.bytes().cpu().numpy(), want_keys), ("keys", what)
    if vb:
        assert gv.intact(), ("value guards", what)
        p = torch.from_numpy(perm).cuda()
        assert torch.equal(vals, vin[p]), ("values", what)
    if n > 1:
        assert c.get_info(rs.INFO_LAST_PAIRS) == expected_info(kb, vb), what


@pytest.mark.parametrize("tname", KEY_TYPES)
def test_pairs_matrix(rs, torch, ctx, tname):
    _es, _ko, kb, kind = util.TYPES[tname]
    all_sizes = sorted({n for vb in VALUE_BYTES for n in sizes_for(kb, vb)})
    for i, n in enumerate(all_sizes):
        dists = [dist_for(tname, i)]
        if n == 200003:
            dists += [d for d in ("equal", "two", "lowbyte") if d not in dists]  # ties: the index values show the order kept
        for dist in dists:
            keys_raw = util.make_input(tname, n, dist, seed=1000 + 17 * i + KEY_TYPES.index(tname))
            for desc in (False, True):
                want_keys, _v, perm = pairs_reference(keys_raw, None, kb, kind, 0, desc)
                for vb in VALUE_BYTES:
                    if n in sizes_for(kb, vb):
                        run_pairs(rs, torch, ctx, tname, keys_raw, vb, desc, perm, want_keys)


@pytest.mark.parametrize("tname", ["u8", "i16", "f32", "u64", "i128"])
def test_pairs_naturally_aligned_arrays(rs, torch, ctx, tname):
    """Arrays that start one key (one value alignment unit) behind a 16-byte boundary take the element-by-element kernels."""
    _es, _ko, kb, kind = util.TYPES[tname]
    for n in (255, 200003):
        keys_raw = util.make_input(tname, n, "uniform" if kind == F else "two", seed=77 + n)
        for desc in (False, True):
            want_keys, _v, perm = pairs_reference(keys_raw, None, kb, kind, 0, desc)
            for vb in (0, 1, 4, 8, 12, 16, 40):
                run_pairs(rs, torch, ctx, tname, keys_raw, vb, desc, perm, want_keys, shift=1)


def _torch_order(torch, tname, keys, desc):
    """torch.sort(stable=True).indices of the keys; unsigned types torch cannot sort go through an order-preserving
    signed image."""
    if tname in ("u16", "u32"):
        keys = keys.to(torch.int64)
    elif tname == "u64":
        keys = keys.view(torch.int64) ^ torch.iinfo(torch.int64).min
    return torch.sort(keys, stable=True, descending=desc).indices


@pytest.mark.parametrize("tname", KEY_TYPES)
def test_argsort(rs, torch, ctx, tname):
    _es, _ko, kb, kind = util.TYPES[tname]
    for i, n in enumerate(sizes_for(kb, 4)):
        dist = dist_for(tname, i + 1)
        keys_raw = util.make_input(tname, n, dist, seed=500 + i)
        for desc in (False, True):
            _k, _v, perm = pairs_reference(keys_raw, None, kb, kind, 0, desc)
            for idt in (torch.int32, torch.int64):
                gk = Guarded(torch, n * kb)
                gk.bytes().copy_(torch.from_numpy(keys_raw))
                keys = key_tensor(torch, gk, tname, n)
                ib = 4 if idt == torch.int32 else 8
                gi = Guarded(torch, n * ib)
                out = gi.bytes().view(idt)
                got = rs.radix_argsort(keys, descending=desc, out=out, ctx=ctx, key_kind=(kind if kb == 16 else None))
                ctx.check()
                what = (tname, n, dist, desc, idt)
                assert got is out
                assert gk.intact() and gi.intact(), ("guards", what)
                assert np.array_equal(gk.bytes().cpu().numpy(), keys_raw), ("keys changed", what)
                assert np.array_equal(out.cpu().numpy().astype(np.int64), perm), what
                if n > 1:
                    assert ctx.get_info(rs.INFO_LAST_PAIRS) == expected_info(kb, 4), what
                if kind != F and kb <= 8:
                    assert torch.equal(out.to(torch.int64), _torch_order(torch, tname, keys, desc)), ("torch.sort", what)
    # without out=: a new int64 tensor, like torch.argsort
    keys_raw = util.make_input(tname, 4099, "two", seed=9)
    gk = Guarded(torch, 4099 * kb)
    gk.bytes().copy_(torch.from_numpy(keys_raw))
    r = rs.radix_argsort(key_tensor(torch, gk, tname, 4099), descending=True, ctx=ctx, key_kind=(kind if kb == 16 else None))
    ctx.check()
    assert r.dtype == torch.int64 and r.shape == (4099,)
    assert np.array_equal(r.cpu().numpy(), pairs_reference(keys_raw, None, kb, kind, 0, True)[2])


def test_bad_arguments_on_the_device(rs, torch, ctx):
    E = rs._lib.ERR_ARG
    k = torch.zeros(64, dtype=torch.int32, device="cuda")
    v = torch.zeros(64, dtype=torch.int64, device="cuda")
    L, h = ctx._L, ctx._h
    assert L.rsx_sort_pairs_device(h, k.data_ptr(), v.data_ptr(), 64, 3, 0, 8, 0, None) == E  # key width
    assert L.rsx_sort_pairs_device(h, k.data_ptr(), v.data_ptr(), 64, 4, 3, 8, 0, None) == E  # kind
    assert L.rsx_sort_pairs_device(h, k.data_ptr(), v.data_ptr(), 64, 2, 2, 8, 0, None) == E  # 2-byte float
    assert L.rsx_sort_pairs_device(h, k.data_ptr(), v.data_ptr(), 64, 4, 0, 8, 2, None) == E  # order
    assert L.rsx_sort_pairs_device(h, k.data_ptr(), v.data_ptr(), 64, 4, 0, 32769, 0, None) == E  # value width
    assert L.rsx_sort_pairs_device(h, k.data_ptr() + 2, v.data_ptr(), 32, 4, 0, 8, 0, None) == E  # key alignment
    assert L.rsx_sort_pairs_device(h, k.data_ptr(), v.data_ptr() + 4, 32, 4, 0, 8, 0, None) == E  # value alignment
    assert L.rsx_sort_pairs_device(h, None, v.data_ptr(), 64, 4, 0, 8, 0, None) == E
    assert L.rsx_sort_pairs_device(h, k.data_ptr(), None, 64, 4, 0, 8, 0, None) == E
    assert L.rsx_sort_pairs_device(h, k.data_ptr(), v.data_ptr(), 64, 4, 0, 0, 0, None) == E  # values without a width
    assert L.rsx_argsort_device(h, k.data_ptr(), v.data_ptr(), 64, 4, 0, 2, 0, None) == E  # index width
    assert L.rsx_argsort_device(h, k.data_ptr(), None, 64, 4, 0, 8, 0, None) == E
    assert L.rsx_argsort_device(h, k.data_ptr(), v.data_ptr() + 4, 32, 4, 0, 8, 0, None) == E
    assert L.rsx_ctx_reserve_pairs(h, 64, 5, 4) == E
    assert L.rsx_ctx_reserve_pairs(h, 64, 4, 32769) == E  # value width
    assert L.rsx_ctx_reserve_pairs(h, 2, 4, 32768) == 0
    assert L.rsx_sort_pairs_device(h, None, None, 0, 4, 0, 0, 0, None) == 0  # nothing to sort
    torch.cuda.synchronize()
    assert not k.any() and not v.any()


def test_large_u32_pairs_checked_on_the_device(rs, torch):
    """2^28 u32 keys with their u32 positions as values, both orders, checked without leaving the device."""
    c = rs.Context(torch.cuda.current_device())
    n = 1 << 28
    d = rs.PRIMITIVES["u32"]
    keys_in = torch.empty(n, dtype=torch.uint32, device="cuda")
    c.generate_device(keys_in.data_ptr(), n, d, rs.GEN_UNIFORM, 2024)
    ver = torch.zeros(3, dtype=torch.int64, device="cuda")
    c.verify_device(keys_in.data_ptr(), n, d, ver.data_ptr())
    c.check()
    sum_in = int(ver[1])
    bits_in = keys_in.view(torch.int32)  # (torch indexes and compares the signed view of the same bits)
    for desc in (False, True):
        keys = keys_in.clone()
        vals = torch.arange(n, dtype=torch.int32, device="cuda")
        rs.radix_sort_pairs(keys, vals, descending=desc, ctx=c)
        c.check()
        assert c.get_info(rs.INFO_LAST_PAIRS) == (1 | 8 << 8)
        c.verify_device(keys.data_ptr(), n, d, ver.data_ptr())
        c.check()
        assert int(ver[1]) == sum_in, "the key column is not a permutation of the input"
        bits = keys.view(torch.int32)
        ordered = ~bits if desc else bits  # descending: no inversions among the complemented keys
        c.verify_device(ordered.data_ptr(), n, d, ver.data_ptr())
        c.check()
        assert int(ver[0]) == 0, (desc, int(ver[0]))
        del ordered
        assert torch.equal(bits_in[vals.to(torch.int64)], bits), "keys_in[values_out] != keys_out"
        tie = bits[1:] == bits[:-1]
        assert int(tie.sum()) > 0
        assert not bool((tie & (vals[1:] <= vals[:-1])).any()), "equal keys out of input order"
        del keys, bits, vals, tie
    c.close()


def test_capture_and_replay(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    n = 300001
    c.reserve_pairs(n, 4, 4)
    inputs = [util.make_input("u32", n, dist, seed=60 + i) for i, dist in enumerate(("uniform", "two"))]
    src = torch.from_numpy(inputs[0].copy()).cuda().view(torch.uint32)
    keys = torch.empty_like(src)
    vals = torch.empty(n, dtype=torch.int32, device="cuda")
    index = torch.arange(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        keys.copy_(src)
        vals.copy_(index)
        rs.radix_sort_pairs(keys, vals, descending=True, ctx=c)  # warm-up outside capture
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        keys.copy_(src)
        vals.copy_(index)
        rs.radix_sort_pairs(keys, vals, descending=True, ctx=c)
    for raw in inputs:
        src.view(torch.uint8).copy_(torch.from_numpy(raw.copy()))
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        want_keys, want_vals, _p = pairs_reference(raw, np.arange(n, dtype="<u4").view(np.uint8), 4, U, 4, True)
        assert np.array_equal(keys.view(torch.uint8).cpu().numpy(), want_keys)
        assert np.array_equal(vals.cpu().numpy().view(np.uint8), want_vals)
    c.close()


def test_unreserved_pairs_under_capture_report_workspace(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    x = torch.randint(0, 2 ** 31 - 1, (1000,), dtype=torch.int32, device="cuda")
    rs.radix_sort(x, ctx=c)  # one ordinary call: the context's error word and self-tests exist
    c.check()
    n = 1 << 16
    keys = torch.randint(0, 2 ** 31 - 1, (n,), dtype=torch.int32, device="cuda")
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    before = keys.clone()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g.capture_begin()
        try:
            rs.radix_sort_pairs(keys, vals, ctx=c)
        except rs.RsxError as e:
            err = e
        g.capture_end()
    assert err is not None and err.status == rs._lib.ERR_WORKSPACE, err
    torch.cuda.synchronize()
    assert torch.equal(keys, before)  # nothing was enqueued
    c.close()


def test_any_layout_sort_after_a_pairs_call(rs, torch, orc):
    """radix_sort of a layout without kernels of its own shares the second workspace with the pairs calls."""
    c = rs.Context(torch.cuda.current_device())
    for lay in ((6, 0, 2, U), (40, 0, 8, U)):
        n = 100003
        keys_raw = util.make_input("i64", n, "uniform", seed=5)
        gk = Guarded(torch, n * 8)
        gk.bytes().copy_(torch.from_numpy(keys_raw))
        vals = make_values(torch, n, 40)
        vin = vals.clone()
        rs.radix_sort_pairs(gk.bytes().view(torch.int64), vals, descending=True, ctx=c)
        c.check()
        want_keys, _v, perm = pairs_reference(keys_raw, None, 8, S, 0, True)
        assert np.array_equal(gk.bytes().cpu().numpy(), want_keys)
        assert torch.equal(vals, vin[torch.from_numpy(perm).cuda()])
        raw = util.make_input_layout(lay, n, "uniform", seed=6)
        x = torch.from_numpy(raw.copy()).cuda().view(n, lay[0])
        rs.radix_sort(x, digits=rs.RadixDigits(*lay), ctx=c)
        c.check()
        assert np.array_equal(x.cpu().numpy().reshape(-1), orc.sort_parallel(raw, orc.Layout(*lay), 4)), lay
        # ... and a pairs call after it
        out = rs.radix_argsort(gk.bytes().view(torch.int64), ctx=c)
        c.check()
        assert np.array_equal(out.cpu().numpy(), pairs_reference(want_keys, None, 8, S, 0, False)[2])
    c.close()
