"""GPU: rsx_merge_device / radix_merge / radix_merge_pairs against tests/merge_ref.py, byte for byte.

Every output sits in an allocation the test owns: 64 guard bytes of 0xA5, the array filled with 0xA5, 64 guard bytes; what
comes back is compared whole, and both inputs are compared with their originals afterwards.

The sizes come from rsx_merge_caps (T = tile), so that they stay the edge cases of the kernel whatever its constants are.
Keys are made from ascending IDS, mapped to the key type by an increasing map (test_gpu_search.keys_from_ids); the values
of the matrix are u32 positions, with bit 31 set on b's side, so that a stability error shows in the bytes.  Each matrix
case asserts through merge_ref.tile_ranges that the shape it is named after occurs."""
import numpy as np
import pytest

import util
from merge_ref import merge_reference, tile_ranges
from segment_pairs_gpu import guarded, key_dtype, same
from segment_pairs_ref import with_guards
from test_gpu_search import F32_SPECIALS, F64_SPECIALS, canary, keys_from_ids

pytestmark = pytest.mark.gpu

PATH = 11 << 24
SHAPES = ["interleaved", "all_equal", "a_below_b", "b_below_a", "runs_of_tile", "blocks"]
FUSED = (1, 2, 4, 8, 16)


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
def shape_ids(shape, na, nb, T, rng):
    """(ids of a, ids of b): each ascending."""
    i, j = np.arange(na, dtype=np.int64), np.arange(nb, dtype=np.int64)
    if shape == "interleaved":
        return 2 * i, 2 * j + 1
    if shape == "all_equal":
        return np.full(na, 5, dtype=np.int64), np.full(nb, 5, dtype=np.int64)
    if shape == "a_below_b":
        return i, na + j
    if shape == "b_below_a":
        return nb + i, j
    if shape == "runs_of_tile":
        return i // T, j // T
    if shape == "blocks":  # blocks of 1 .. 2T equal keys, sides alternating; an a-block and the b-block behind it share their key
        a, b, k = [], [], 0
        left = [na, nb]
        while left[0] or left[1]:
            side = k % 2 if left[k % 2] else 1 - k % 2
            cnt = min(int(rng.integers(1, 2 * T + 1)), left[side])
            (a if side == 0 else b).append(np.full(cnt, k // 2, dtype=np.int64))
            left[side] -= cnt
            k += 1
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)  # noqa: E731
        return cat(a), cat(b)
    raise ValueError(shape)


def keys_of(tname, ia, ib, desc):
    """Raw key bytes of both arrays under ONE map, each sorted in the order asked for."""
    kb = util.TYPES[tname][2]
    both = keys_from_ids(tname, np.concatenate([ia, ib])).reshape(-1, kb)
    a, b = both[:ia.size], both[ia.size:]
    if desc:
        a, b = a[::-1], b[::-1]
    return np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)


def position_values(na, nb):
    return np.arange(na, dtype="<u4"), np.arange(nb, dtype="<u4") | np.uint32(1 << 31)


def row_values(n, vb, salt):
    """n rows of vb bytes that differ from row to row and from byte to byte."""
    r = np.arange(n, dtype=np.int64)[:, None] * 131 + np.arange(vb, dtype=np.int64)[None, :] * 7 + salt
    v = (r % 251).astype(np.uint8)
    v[:, :min(4, vb)] = (np.arange(n, dtype="<u4") * np.uint32(2) + np.uint32(salt & 1)).view(np.uint8).reshape(n, 4)[:, :min(4, vb)]
    return v


class Case:
    """Two sorted key arrays (and their values) on the GPU between guards, the reference computed once."""

    def __init__(self, torch, c, tname, a_raw, b_raw, desc, a_vals=None, b_vals=None, reference=True):
        self.torch, self.c, self.tname, self.desc = torch, c, tname, desc
        self.kb, self.kind = util.TYPES[tname][2], util.TYPES[tname][3]
        self.a_raw, self.b_raw = a_raw, b_raw
        self.na, self.nb = a_raw.size // self.kb, b_raw.size // self.kb
        self.n = self.na + self.nb
        self.abuf, self.amid = guarded(torch, a_raw)
        self.bbuf, self.bmid = guarded(torch, b_raw)
        self.vb = 0
        self.a_vals = self.b_vals = None
        if a_vals is not None:
            self.a_vals = np.ascontiguousarray(a_vals).view(np.uint8).reshape(-1)
            self.b_vals = np.ascontiguousarray(b_vals).view(np.uint8).reshape(-1)
            self.vb = (self.a_vals.size + self.b_vals.size) // self.n
            self.avbuf, self.avmid = guarded(torch, self.a_vals)
            self.bvbuf, self.bvmid = guarded(torch, self.b_vals)
        if reference:
            self.want = merge_reference(a_raw, b_raw, self.a_vals, self.b_vals, tname, desc)

    def call(self, out_keys, out_values, out_index, ib, stream=None):
        torch = self.torch
        ptr = lambda mid, cnt: mid.data_ptr() if cnt else 0  # noqa: E731 (an empty view has no address of its own)
        self.c.merge_device(ptr(self.amid, self.na), ptr(self.avmid, self.na) if self.vb else 0, self.na, ptr(self.bmid, self.nb),
                            ptr(self.bvmid, self.nb) if self.vb else 0, self.nb, self.kb, self.kind, self.vb, out_keys, out_values, out_index, ib,
                            self.desc, torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def run(self, rs, ib=8, keys=True, values=True, index=True, what=None):
        """One call with the outputs asked for -> compares each whole allocation with the reference."""
        torch, n = self.torch, self.n
        values = values and self.vb > 0
        ko = guarded(torch, canary(n * self.kb)) if keys else None
        vo = guarded(torch, canary(n * self.vb)) if values else None
        io = guarded(torch, canary(n * ib)) if index else None
        p = [(o[0].data_ptr() + 64 if o is not None else 0) for o in (ko, vo, io)]
        self.call(p[0], p[1], p[2], ib)
        self.c.check()
        wide = values and self.vb not in FUSED
        assert self.c.get_info(rs.INFO_LAST_PASSES) == PATH | (2 | 0x100 if wide else 1), (self.tname, self.vb, hex(self.c.get_info(rs.INFO_LAST_PASSES)))
        tag = (self.tname, self.na, self.nb, what, "desc" if self.desc else "asc", self.vb, ib)
        if keys:
            assert same(ko[0].cpu().numpy(), with_guards(self.want[0]), ("keys",) + tag)
        if values:
            assert same(vo[0].cpu().numpy(), with_guards(self.want[1]), ("values",) + tag)
        if index:
            assert same(io[0].cpu().numpy(), with_guards(self.want[2].astype("<i4" if ib == 4 else "<i8")), ("index",) + tag)

    def inputs_unchanged(self):
        assert same(self.abuf.cpu().numpy(), with_guards(self.a_raw), ("a", self.tname, self.na))
        assert same(self.bbuf.cpu().numpy(), with_guards(self.b_raw), ("b", self.tname, self.nb))
        if self.vb:
            assert same(self.avbuf.cpu().numpy(), with_guards(self.a_vals), ("a's values", self.tname, self.na))
            assert same(self.bvbuf.cpu().numpy(), with_guards(self.b_vals), ("b's values", self.tname, self.nb))


def pairs_of(T):
    return [(0, 1), (1, 0), (1, 1), (T, 0), (0, T + 1), (T - 1, 1), (T, T), (T + 1, T - 1), (1, 4 * T + 3), (4 * T + 3, 1), (3 * T + 7, 2 * T + 5)]


def seen_in(case, T):
    """What the tiles of a case look like: a set of "both", "a_only", "b_only", "ties"."""
    out = set()
    for _a0, acnt, _b0, bcnt, ties in tile_ranges(case.a_raw, case.b_raw, case.tname, case.desc, T):
        out.add("both" if acnt and bcnt else "a_only" if acnt else "b_only")
        if ties:
            out.add("ties")
    return out


NAMED = {"interleaved": {"both"}, "all_equal": {"a_only", "b_only", "ties"}, "a_below_b": {"a_only", "b_only"}, "b_below_a": {"a_only", "b_only"},
         "runs_of_tile": {"both", "ties"}, "blocks": {"both", "ties"}}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", ["u32", "i64"])
def test_full_cross(rs, torch, ctx, tname, desc, shape):
    kb = util.TYPES[tname][2]
    T = rs.merge_caps(kb, 4)
    rng = np.random.default_rng(kb + 2 * desc + 7 * SHAPES.index(shape))
    seen, v = set(), 0
    for na, nb in pairs_of(T):
        ia, ib_ = shape_ids(shape, na, nb, T, rng)
        a_raw, b_raw = keys_of(tname, ia, ib_, desc)
        case = Case(torch, ctx, tname, a_raw, b_raw, desc, *position_values(na, nb))
        seen |= seen_in(case, T)
        case.run(rs, ib=(4, 8)[v % 2], what=shape)  # the index widths take turns
        v += 1
        case.inputs_unchanged()
        if shape == "all_equal":  # one key: the output is a, then b
            assert np.array_equal(case.want[2], np.arange(na + nb))
    assert NAMED[shape] <= seen, (shape, NAMED[shape] - seen)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", ["u8", "i16", "i32", "f32", "f64", "u128", "i128"])
def test_other_key_types(rs, torch, ctx, tname, desc):
    kb = util.TYPES[tname][2]
    T = rs.merge_caps(kb, 4)
    rng = np.random.default_rng(kb + desc)
    seen, v = set(), 0
    for na, nb in ((1, 1), (T - 1, 1), (T + 1, T - 1), (3 * T + 7, 2 * T + 5)):
        for shape in ("interleaved", "runs_of_tile", "blocks", "a_below_b"):
            ia, ib_ = shape_ids(shape, na, nb, T, rng)
            if kb == 1:  # 256 keys: fewer, longer runs
                top = int(max(ia.max(initial=0), ib_.max(initial=0)))
                ia, ib_ = ia * 100 // (top + 1), ib_ * 100 // (top + 1)
            a_raw, b_raw = keys_of(tname, ia, ib_, desc)
            case = Case(torch, ctx, tname, a_raw, b_raw, desc, *position_values(na, nb))
            seen |= seen_in(case, T)
            case.run(rs, ib=(4, 8)[v % 2], what=shape)
            v += 1
            case.inputs_unchanged()
    assert {"both", "ties"} <= seen, seen


@pytest.mark.parametrize("tname", ["f32", "f64"])
def test_float_specials(rs, torch, ctx, tname):
    """The seven specials as runs in both arrays: seven different keys in the total order on bit patterns, -NaN first, -0.0
    before +0.0, the two NaNs last and apart."""
    kb = util.TYPES[tname][2]
    T = rs.merge_caps(kb, 4)
    sp = F32_SPECIALS if kb == 4 else F64_SPECIALS
    for ra, rb in ((1, 1), (3, 2), (T // 7 + 1, T // 5 + 1)):
        for desc in (False, True):
            order = sp[::-1] if desc else sp
            a, b = np.repeat(order, ra), np.repeat(order, rb)
            case = Case(torch, ctx, tname, a.view(np.uint8).reshape(-1).copy(), b.view(np.uint8).reshape(-1).copy(), desc, *position_values(a.size, b.size))
            want = np.concatenate([np.concatenate([s * ra + np.arange(ra), 7 * ra + s * rb + np.arange(rb)]) for s in range(7)])
            assert np.array_equal(case.want[2], want)  # run by run: a's, then b's
            case.run(rs, ib=4, what=("specials", ra, rb))
            case.run(rs, ib=8, values=False, what=("specials", ra, rb))
            case.inputs_unchanged()


@pytest.mark.parametrize("vb", [1, 2, 4, 8, 16, 3, 12, 32, 40])
def test_every_value_width(rs, torch, ctx, vb):
    """Every fused value width and one width per wide route (bytes: 3; 16-byte words: 32; neither: 12, 40), with the output
    combinations: all three, keys only, index only, values without keys."""
    rng = np.random.default_rng(vb)
    for tname, desc in (("u32", False), ("i64", True), ("u128", False)):
        kb = util.TYPES[tname][2]
        T = rs.merge_caps(kb, vb)
        for na, nb in ((T + 1, T - 1), (3 * T + 7, 2 * T + 5)):
            ia, ib_ = shape_ids("blocks", na, nb, T, rng)
            a_raw, b_raw = keys_of(tname, ia, ib_, desc)
            case = Case(torch, ctx, tname, a_raw, b_raw, desc, row_values(na, vb, 0), row_values(nb, vb, 1))
            assert case.vb == vb
            case.run(rs, ib=4, what="all three")
            case.run(rs, ib=8, values=False, index=False, what="keys only")
            case.run(rs, ib=8, keys=False, values=False, what="index only")
            case.run(rs, ib=8, keys=False, index=False, what="values without keys")
            case.run(rs, ib=8, keys=False, what="values and index")
            case.inputs_unchanged()


def test_values_of_32_kib(rs, torch, ctx):
    vb = 32768
    rng = np.random.default_rng(5)
    ia, ib_ = shape_ids("blocks", 23, 18, 4, rng)
    a_raw, b_raw = keys_of("i32", ia, ib_, False)
    case = Case(torch, ctx, "i32", a_raw, b_raw, False, row_values(23, vb, 0), row_values(18, vb, 1))
    case.run(rs, ib=4, what="32 KiB values")
    case.run(rs, ib=8, keys=False, index=False, what="32 KiB values alone")
    case.inputs_unchanged()


# ---- against what exists ----
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", ["i32", "i64", "f32", "u8"])
def test_merge_equals_sort_of_the_concatenation(rs, torch, ctx, tname, desc):
    """radix_merge_pairs = radix_sort_pairs of the concatenation, return_index = radix_argsort of it, and for ints and plain
    floats (no NaN, no -0.0) the keys = torch.sort(torch.cat(...), stable=True)."""
    dt = key_dtype(torch, tname)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    T = rs.merge_caps(util.TYPES[tname][2], 8)
    for na, nb, span in ((0, 5, 3), (7, 0, 3), (1000, 777, 50), (2 * T + 11, 3 * T + 5, 100)):
        a = torch.randint(0, span, (na,), device="cuda", generator=gen).to(dt)
        b = torch.randint(0, span, (nb,), device="cuda", generator=gen).to(dt)
        if dt.is_floating_point:
            a, b = a * 0.5 - 3.25, b * 0.5 - 3.25
        a, b = torch.sort(a, descending=desc).values, torch.sort(b, descending=desc).values
        av = torch.arange(na, device="cuda", dtype=torch.float64).reshape(na, 1).repeat(1, 3)  # 24-byte rows: the wide route
        bv = -torch.arange(nb, device="cuda", dtype=torch.float64).reshape(nb, 1).repeat(1, 3) - 1
        a0, b0 = a.clone(), b.clone()
        keys, vals = rs.radix_merge_pairs(a, av, b, bv, descending=desc, ctx=ctx)
        k2, v2 = rs.radix_merge_pairs(a, av[:, 0].contiguous(), b, bv[:, 0].contiguous(), descending=desc, ctx=ctx)  # 8-byte values: fused
        ck, cv = torch.cat((a, b)), torch.cat((av, bv))
        arg = rs.radix_argsort(ck, descending=desc, ctx=ctx)
        rs.radix_sort_pairs(ck, cv, descending=desc, ctx=ctx)
        ctx.check()
        assert keys.dtype == dt and keys.shape == (na + nb,) and vals.shape == (na + nb, 3)
        assert torch.equal(keys, ck) and torch.equal(vals, cv) and torch.equal(k2, ck) and torch.equal(v2, cv[:, 0])
        assert torch.equal(keys, torch.sort(torch.cat((a, b)), stable=True, descending=desc).values)
        k3, idx = rs.radix_merge(a, b, descending=desc, return_index=True, ctx=ctx)
        k4, idx32 = rs.radix_merge(a, b, descending=desc, return_index=True, index_dtype=torch.int32, ctx=ctx)
        ctx.check()
        assert idx.dtype == torch.int64 and idx32.dtype == torch.int32
        assert torch.equal(k3, ck) and torch.equal(k4, ck) and torch.equal(idx, arg) and torch.equal(idx32.long(), arg)
        out = torch.empty(na + nb, dtype=dt, device="cuda")
        assert rs.radix_merge(a, b, descending=desc, out=out, ctx=ctx) is out and torch.equal(out, ck)
        pair = (torch.empty(na + nb, dtype=dt, device="cuda"), torch.empty(na + nb, dtype=torch.int32, device="cuda"))
        got = rs.radix_merge(a, b, descending=desc, return_index=True, out=pair, ctx=ctx)
        assert got[0] is pair[0] and got[1] is pair[1] and torch.equal(pair[0], ck) and torch.equal(pair[1].long(), arg)
        assert torch.equal(a, a0) and torch.equal(b, b0)
    big = torch.empty(3 * (na + nb), dtype=dt, device="cuda")  # an output that begins inside an input
    big[:na] = a
    with pytest.raises(rs.RsxError) as e:
        rs.radix_merge(big[:na], b, descending=desc, out=big[na // 2:na // 2 + na + nb], ctx=ctx)
    assert e.value.status == rs._lib.ERR_ARG


def test_merge_of_two_groups_and_128_bit_keys(rs, torch, ctx):
    """README: merge the keys[:num] of two radix_group results; and (n, 16) uint8 keys with key_kind=."""
    rng = np.random.default_rng(23)
    a = rng.integers(-400, 400, size=30011).astype("<i4")
    b = rng.integers(-300, 500, size=20021).astype("<i4")
    ga = rs.radix_group(torch.from_numpy(a).cuda(), ctx=ctx)
    gb = rs.radix_group(torch.from_numpy(b).cuda(), ctx=ctx)
    ma, mb = int(ga.num), int(gb.num)
    keys, idx = rs.radix_merge(ga.keys[:ma], gb.keys[:mb], return_index=True, ctx=ctx)
    ctx.check()
    ua, ub = np.unique(a), np.unique(b)
    assert np.array_equal(keys.cpu().numpy(), np.sort(np.concatenate([ua, ub]), kind="stable"))
    assert np.array_equal(idx.cpu().numpy(), np.argsort(np.concatenate([ua, ub]), kind="stable"))
    from pairs_ref import pairs_reference
    ra = pairs_reference(util.make_input("i128", 3000, "two", seed=4), None, 16, util.SIGNED, 0, True)[0]
    rb = pairs_reference(util.make_input("i128", 2001, "uniform", seed=5), None, 16, util.SIGNED, 0, True)[0]
    want = merge_reference(ra, rb, None, None, "i128", True)
    got = rs.radix_merge(torch.from_numpy(ra.copy()).cuda().view(-1, 16), torch.from_numpy(rb.copy()).cuda().view(-1, 16), descending=True,
                         return_index=True, ctx=ctx, key_kind=rs.KEY_SIGNED)
    ctx.check()
    assert got[0].shape == (5001, 16) and np.array_equal(got[0].cpu().numpy().reshape(-1), want[0])
    assert np.array_equal(got[1].cpu().numpy(), want[2])


# ---- one larger case, and byte offsets past 2^32 ----
@pytest.fixture(scope="module")
def large():
    """na = 2^22 + 3 and nb = 2^21 + 1 u64 keys drawn from few enough values to tie, with u64 values; the reference computed once."""
    rng = np.random.default_rng(21)
    na, nb = (1 << 22) + 3, (1 << 21) + 1
    a = np.sort(rng.integers(0, 1 << 21, size=na, dtype=np.uint64) << np.uint64(40))
    b = np.sort(rng.integers(0, 1 << 21, size=nb, dtype=np.uint64) << np.uint64(40))
    av = np.arange(na, dtype="<u8")
    bv = np.arange(nb, dtype="<u8") | np.uint64(1 << 63)
    want = merge_reference(a.view(np.uint8), b.view(np.uint8), av, bv, "u64", False)
    assert np.array_equal(want[0].view("<u8"), np.sort(np.concatenate([a, b]), kind="stable"))
    return a, b, av, bv, want


def test_large_pair(rs, torch, ctx, large):
    a, b, av, bv, want = large
    case = Case(torch, ctx, "u64", a.view(np.uint8), b.view(np.uint8), False, av, bv, reference=False)
    case.want = want
    case.run(rs, ib=4, what="large")
    case.run(rs, ib=8, keys=False, values=False, what="large, index only")
    case.inputs_unchanged()


def test_u8_keys_past_two_to_the_32(rs, torch, ctx):
    """na = 2^32 + 4099 bytes in 256 filled runs merged with 4099 more: the output's runs end where the counts say.  Only fills,
    one merge and checks on the device."""
    na, nb = (1 << 32) + 4099, 4099
    base, extra = divmod(na, 256)
    cnt_a = np.array([base + (1 if v < extra else 0) for v in range(256)], dtype=np.int64)
    b_np = (np.arange(nb, dtype=np.int64) * 256 // nb).astype(np.uint8)
    cnt_b = np.bincount(b_np, minlength=256).astype(np.int64)
    ends_a = np.cumsum(cnt_a)
    ends = np.cumsum(cnt_a + cnt_b)
    starts = np.concatenate([[0], ends[:-1]])
    a = torch.empty(na, dtype=torch.uint8, device="cuda")
    for v in range(256):
        a[int(ends_a[v] - cnt_a[v]):int(ends_a[v])].fill_(v)
    b = torch.from_numpy(b_np).cuda()
    n = na + nb
    obuf = torch.full((64 + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = obuf[64:64 + n]
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(rs.RsxError) as e:  # 4-byte positions cannot count more than 2^32 keys
        ctx.merge_device(a.data_ptr(), 0, na, b.data_ptr(), 0, nb, 1, rs.KEY_UNSIGNED, 0, out.data_ptr(), 0, out.data_ptr(), 4, False, st)
    assert e.value.status == rs._lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((obuf[:4096] == 0xA5).all()) and bool((obuf[-4096:] == 0xA5).all())  # nothing was written by the refused call
    ctx.merge_device(a.data_ptr(), 0, na, b.data_ptr(), 0, nb, 1, rs.KEY_UNSIGNED, 0, out.data_ptr(), 0, 0, 8, False, st)
    ctx.check()
    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 1
    assert bool((obuf[:64] == 0xA5).all()) and bool((obuf[-64:] == 0xA5).all())
    first = out[torch.from_numpy(starts).cuda()].cpu().numpy()
    last = out[torch.from_numpy(ends - 1).cuda()].cpu().numpy()
    assert np.array_equal(first, np.arange(256)) and np.array_equal(last, np.arange(256))
    step = 1 << 30  # never descending, piece by piece: with the run ends above, every byte is what it must be
    for s in range(0, n - 1, step):
        e_ = min(s + step, n - 1)
        assert bool((out[s + 1:e_ + 1] >= out[s:e_]).all()), s
    with pytest.raises(ValueError, match="int64"):
        rs.radix_merge(a, b, return_index=True, index_dtype=torch.int32, ctx=ctx)
    del a, out, obuf


# ---- the precondition broken ----
@pytest.mark.parametrize("tname", ["u32", "i64", "u128"])
def test_unsorted_inputs_stay_in_bounds(rs, torch, ctx, tname):
    """Random unsorted a and b, both routes: the guards hold, the inputs are unchanged, every position is below n."""
    rng = np.random.default_rng(13)
    kb = util.TYPES[tname][2]
    for vb in (4, 12):
        T = rs.merge_caps(kb, vb)
        for na, nb in ((2, T + 1), (T + 1, T), (4 * T + 5, 3 * T + 7)):
            n = na + nb
            a_raw = keys_from_ids(tname, rng.integers(0, 4 * n, size=na))
            b_raw = keys_from_ids(tname, rng.integers(0, 4 * n, size=nb))
            case = Case(torch, ctx, tname, a_raw, b_raw, bool(vb == 12), row_values(na, vb, 0), row_values(nb, vb, 1), reference=False)
            for ib in (4, 8):
                ko, vo, io = (guarded(torch, canary(n * w)) for w in (kb, vb, ib))
                case.call(ko[1].data_ptr(), vo[1].data_ptr(), io[1].data_ptr(), ib)
                ctx.check()
                got = io[1].view(torch.int32 if ib == 4 else torch.int64)
                assert int(got.min()) >= 0 and int(got.max()) < n, (tname, na, nb, vb, ib)
                for buf, _mid in (ko, vo, io):
                    whole = buf.cpu().numpy()
                    assert (whole[:64] == 0xA5).all() and (whole[-64:] == 0xA5).all(), (tname, na, nb, vb, ib)
            case.inputs_unchanged()


# ---- empty sides, a side stream, capture ----
def test_empty_sides(rs, torch, ctx):
    E = rs._lib
    L, h = ctx._L, ctx._h
    # n == 0: nothing is launched and no pointer is looked at (dangling values here)
    assert L.rsx_merge_device(h, 8, 8, 0, 8, 8, 0, 4, 0, 4, 0, 8, 8, 8, 8, None) == E.OK
    assert L.rsx_merge_device(h, None, None, 0, None, None, 0, 4, 0, 0, 1, None, None, None, 3, None) == E.OK
    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH
    e = torch.zeros(0, dtype=torch.int32, device="cuda")
    x = torch.arange(5, dtype=torch.int32, device="cuda")
    assert rs.radix_merge(e, e, ctx=ctx).shape == (0,)
    assert rs.radix_merge(e, x, ctx=ctx).tolist() == [0, 1, 2, 3, 4] and rs.radix_merge(x, e, return_index=True, ctx=ctx)[1].tolist() == [0, 1, 2, 3, 4]
    k, v = rs.radix_merge_pairs(e, e.view(0, 1).float(), x, x.view(5, 1).float(), ctx=ctx)
    assert k.tolist() == [0, 1, 2, 3, 4] and v.shape == (5, 1) and v[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    ctx.check()


def test_a_side_stream(rs, torch, ctx):
    T = rs.merge_caps(8, 12)
    rng = np.random.default_rng(17)
    ia, ib_ = shape_ids("blocks", 2 * T + 3, 3 * T + 1, T, rng)
    a_raw, b_raw = keys_of("i64", ia, ib_, True)
    fused = Case(torch, ctx, "i64", a_raw, b_raw, True, *position_values(ia.size, ib_.size))
    wide = Case(torch, ctx, "i64", a_raw, b_raw, True, row_values(ia.size, 12, 0), row_values(ib_.size, 12, 1))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        fused.run(rs, 8, what="side stream")
        wide.run(rs, 4, what="side stream")
    s.synchronize()
    fused.inputs_unchanged()
    wide.inputs_unchanged()


def test_capture_and_replay_of_the_fused_route(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    T = rs.merge_caps(4, 4)
    na, nb = 2 * T + 9, 3 * T + 1
    n = na + nb
    src_a = torch.zeros(na, dtype=torch.int32, device="cuda")
    src_b = torch.zeros(nb, dtype=torch.int32, device="cuda")
    a, b = torch.empty_like(src_a), torch.empty_like(src_b)
    av = torch.arange(na, dtype=torch.int32, device="cuda")
    bv = torch.arange(nb, dtype=torch.int32, device="cuda") + (1 << 30)
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    vals = torch.empty(n, dtype=torch.int32, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()

    def enqueue():
        c.merge_device(a.data_ptr(), av.data_ptr(), na, b.data_ptr(), bv.data_ptr(), nb, 4, rs.KEY_SIGNED, 4, keys.data_ptr(), vals.data_ptr(),
                       idx.data_ptr(), 4, False, torch.cuda.current_stream().cuda_stream)

    with torch.cuda.stream(s):
        a.copy_(src_a)
        b.copy_(src_b)
        enqueue()  # the context's first call, outside the capture
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):  # one linear chain: the two copies, then the call's launch
        a.copy_(src_a)
        b.copy_(src_b)
        enqueue()
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        a_np = np.sort(rng.integers(-500, 500, size=na)).astype("<i4")
        b_np = np.sort(rng.integers(-500, 500, size=nb)).astype("<i4")
        src_a.copy_(torch.from_numpy(a_np))
        src_b.copy_(torch.from_numpy(b_np))
        keys.fill_(-1)
        vals.fill_(-1)
        idx.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        perm = np.argsort(np.concatenate([a_np, b_np]), kind="stable")
        assert np.array_equal(idx.cpu().numpy(), perm)
        assert np.array_equal(keys.cpu().numpy(), np.concatenate([a_np, b_np])[perm])
        assert np.array_equal(vals.cpu().numpy(), np.concatenate([av.cpu().numpy(), bv.cpu().numpy()])[perm])
    c.close()


def test_unreserved_wide_route_under_capture_reports_workspace(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    x = torch.randint(0, 2 ** 31 - 1, (1000,), dtype=torch.int32, device="cuda")
    rs.radix_sort(x, ctx=c)  # one ordinary call: the context's error word and self-tests exist
    c.check()
    na, nb = 1 << 15, 1 << 14
    a = torch.sort(torch.randint(0, 1000, (na,), dtype=torch.int32, device="cuda")).values
    b = torch.sort(torch.randint(0, 1000, (nb,), dtype=torch.int32, device="cuda")).values
    av = torch.arange(na, dtype=torch.int32, device="cuda").reshape(na, 1).repeat(1, 3).contiguous()  # 12-byte values
    bv = -torch.arange(nb, dtype=torch.int32, device="cuda").reshape(nb, 1).repeat(1, 3).contiguous() - 1
    keys = torch.full((na + nb,), -1, dtype=torch.int32, device="cuda")
    vals = torch.full((na + nb, 3), 77, dtype=torch.int32, device="cuda")

    def enqueue():
        c.merge_device(a.data_ptr(), av.data_ptr(), na, b.data_ptr(), bv.data_ptr(), nb, 4, rs.KEY_SIGNED, 12, keys.data_ptr(), vals.data_ptr(), 0, 8,
                       False, torch.cuda.current_stream().cuda_stream)

    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g.capture_begin()
        try:
            enqueue()
        except rs.RsxError as e:
            err = e
        g.capture_end()
    assert err is not None and err.status == rs._lib.ERR_WORKSPACE, err
    torch.cuda.synchronize()
    assert bool((keys == -1).all()) and bool((vals == 77).all())  # nothing was enqueued
    c.reserve_merge(na + nb, 4, 12)  # with the reserve the same call runs
    enqueue()
    c.check()
    assert c.get_info(rs.INFO_LAST_PASSES) == PATH | 2 | 0x100
    ck, cv = torch.cat((a, b)), torch.cat((av, bv))
    rs.radix_sort_pairs(ck, cv, ctx=c)
    assert torch.equal(keys, ck) and torch.equal(vals, cv)
    c.close()


def test_errors(rs, torch, ctx):
    E = rs._lib
    L, h = ctx._L, ctx._h
    P = 4096
    buf = torch.full((8 * P,), 0xA5, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert p % 16 == 0
    ok = dict(ak=p, av=p + P, na=100, bk=p + 2 * P, bv=p + 3 * P, nb=50, kb=4, kind=0, vb=8, order=0, ok=p + 4 * P, ov=p + 5 * P, oi=p + 7 * P, ib=8)

    def call(**kw):
        a = dict(ok, **kw)
        return L.rsx_merge_device(h, a["ak"] or None, a["av"] or None, a["na"], a["bk"] or None, a["bv"] or None, a["nb"], a["kb"], a["kind"], a["vb"],
                                  a["order"], a["ok"] or None, a["ov"] or None, a["oi"] or None, a["ib"], None)

    novals = dict(av=0, bv=0, ov=0, vb=0)
    assert call(kb=3) == E.ERR_ARG                        # key width
    assert call(kb=16, kind=2) == E.ERR_ARG               # float keys of 16 bytes
    assert call(kind=3) == E.ERR_ARG
    assert call(vb=32769) == E.ERR_ARG
    assert call(order=2) == E.ERR_ARG
    assert call(ib=2) == E.ERR_ARG and call(ib=0) == E.ERR_ARG
    assert call(ok=0, ov=0, oi=0) == E.ERR_ARG            # all outputs null
    assert call(ak=0) == E.ERR_ARG and call(bk=0) == E.ERR_ARG  # null inputs with a nonzero count
    assert call(av=0) == E.ERR_ARG and call(bv=0) == E.ERR_ARG  # values on one side only
    assert call(vb=0) == E.ERR_ARG and call(av=0, bv=0, vb=0) == E.ERR_ARG and call(ov=0, vb=0) == E.ERR_ARG  # vb == 0 <=> no value pointer
    for name in ("ak", "bk", "ok"):                      # misaligned, each pointer in turn
        assert call(**{name: ok[name] + 2}) == E.ERR_ARG, name
    for name in ("av", "bv", "ov", "oi"):
        assert call(**{name: ok[name] + 4}) == E.ERR_ARG, name
    assert call(**novals, na=2 ** 32, nb=1, ib=4, ok=0) == E.ERR_ARG   # 4-byte positions cannot count them
    assert call(**novals, na=2 ** 62, nb=0, ok=0) == E.ERR_UNSUPPORTED  # 2^31 tiles or more
    assert L.rsx_ctx_reserve_merge(h, 2 ** 62, 4, 0) == E.ERR_UNSUPPORTED
    assert L.rsx_ctx_reserve_merge(h, 100, 3, 0) == E.ERR_ARG and L.rsx_ctx_reserve_merge(h, 100, 4, 32769) == E.ERR_ARG
    # overlaps: every output against every input and against the other outputs, by one byte and by the whole range
    last = lambda base, cnt, w: base + cnt * w - w  # noqa: E731 (the range's last element)
    assert call(ok=ok["ak"]) == E.ERR_ARG and call(ok=last(ok["ak"], 100, 4)) == E.ERR_ARG
    assert call(ok=ok["bk"] - 150 * 4 + 4) == E.ERR_ARG   # the output's last key is b's first
    assert call(ok=ok["bk"]) == E.ERR_ARG and call(ok=ok["av"]) == E.ERR_ARG and call(ok=ok["bv"] + 392) == E.ERR_ARG
    assert call(ov=ok["ak"]) == E.ERR_ARG and call(ov=ok["bk"]) == E.ERR_ARG and call(ov=ok["av"]) == E.ERR_ARG and call(ov=last(ok["bv"], 50, 8)) == E.ERR_ARG
    assert call(oi=ok["ak"]) == E.ERR_ARG and call(oi=ok["bk"]) == E.ERR_ARG and call(oi=ok["av"]) == E.ERR_ARG and call(oi=ok["bv"]) == E.ERR_ARG
    assert call(ov=ok["ok"]) == E.ERR_ARG and call(oi=ok["ok"] + 592) == E.ERR_ARG and call(oi=ok["ov"] + 1192) == E.ERR_ARG
    assert call(ok=ok["oi"] + 1192) == E.ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())                     # no refused call wrote
    # what touches without sharing a byte is taken: an output that ends where an input begins, and the reverse
    assert call(ok=ok["bk"] - 150 * 4, **novals) == E.OK and call(ok=ok["ak"] + 100 * 4, **novals) == E.OK
    assert call(oi=ok["oi"] + 4, ib=4) == E.OK            # aligned to the index width is enough
    assert call(ok=0) == E.OK and call(ok=0, ov=0) == E.OK and call(oi=0, ib=3) == E.OK  # (index_bytes is looked at only with d_out_index)
    assert call(na=0, ak=0, av=0) == E.OK and call(nb=0, bk=0, bv=0) == E.OK  # an empty side needs no pointers
    ctx.check()
