"""GPU: rsx_setop_device / radix_set_op / radix_set_op_pairs against tests/setop_ref.py, byte for byte.

Every output sits in an allocation the test owns: 64 guard bytes of 0xA5, cap(op) rows filled with 0xA5, 64 guard bytes.
What comes back is compared whole: rows [0, num) with the reference, rows [num, cap) and the guards still 0xA5, the count
word exact, and both inputs compared with their originals afterwards.

The sizes come from rsx_setop_caps (T = tile), so that they stay the edge cases of the kernel whatever its constants are.
Keys are made from ascending IDS (test_gpu_merge.shape_ids and two shapes of this file), mapped to the key type by an
increasing map; the values of the matrix are u32 positions with bit 31 set on b's side, so that a wrong pick among equal
keys shows in the bytes.  Each shape asserts through setop_ref.tile_model that the condition it is named for occurs."""
import numpy as np
import pytest

import util
from segment_pairs_gpu import guarded, key_dtype, same
from segment_pairs_ref import with_guards
from setop_ref import OPS, capacity, setop_reference, tile_model
from test_gpu_merge import Case, keys_of, position_values, row_values, shape_ids
from test_gpu_search import F32_SPECIALS, F64_SPECIALS, canary, keys_from_ids

pytestmark = pytest.mark.gpu

PATH = 12 << 24
SHAPES = ["interleaved", "all_equal", "runs_of_tile", "blocks", "identical", "dup_mismatch"]
OP_NAMES = list(OPS)


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
def dup_cycle(T):
    return [(1, 1), (2, 1), (1, 2), (3, 0), (0, 3), (T + 1, 2), (2, T + 1)]


def setop_ids(shape, na, nb, T, rng):
    """(ids of a, ids of b): each ascending."""
    if shape == "identical":  # runs of three; a == b when na == nb
        return np.arange(na, dtype=np.int64) // 3, np.arange(nb, dtype=np.int64) // 3
    if shape == "dup_mismatch":  # key q occurs m times in a and n times in b, (m, n) cycling; what is left of one side goes on alone
        cyc = dup_cycle(T)
        a, b, q, left = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], 0, [na, nb]
        while left[0] or left[1]:
            m, n = cyc[q % len(cyc)]
            m, n = min(m, left[0]), min(n, left[1])
            if m + n == 0:  # the side this key belongs to is used up: one key of the other side
                m, n = (1, 0) if left[0] else (0, 1)
            a.append(np.full(m, q, dtype=np.int64))
            b.append(np.full(n, q, dtype=np.int64))
            left[0] -= m
            left[1] -= n
            q += 1
        return np.concatenate(a), np.concatenate(b)
    return shape_ids(shape, na, nb, T, rng)


def sizes_of(T):
    return [(0, 5), (5, 0), (1, 1), (T - 1, 1), (T, T), (T + 1, T - 1), (2 * T + 3, T - 1), (3 * T + 7, 3 * T - 5)]


class SetCase(Case):
    """test_gpu_merge.Case (two key arrays and their values on the GPU between guards) with the set-operation call."""

    def __init__(self, torch, c, tname, a_raw, b_raw, desc, a_vals=None, b_vals=None, n_a=None, n_b=None):
        super().__init__(torch, c, tname, a_raw, b_raw, desc, a_vals, b_vals, reference=False)
        self.n_a, self.n_b = n_a, n_b
        dev = lambda v: None if v is None else torch.tensor([v], dtype=torch.int64, device="cuda")  # noqa: E731
        self.a_num, self.b_num = dev(n_a), dev(n_b)
        self.refs = {}

    def reference(self, op):
        if op not in self.refs:  # computed once per operation, shared by every call
            self.refs[op] = setop_reference(self.a_raw, self.b_raw, self.a_vals, self.b_vals, self.tname, self.desc, op, self.n_a, self.n_b)
        return self.refs[op]

    def call(self, op, out_keys, out_values, out_index, ib, out_num, b_values=True, stream=None):
        torch = self.torch
        ptr = lambda mid, cnt: mid.data_ptr() if cnt else 0  # noqa: E731 (an empty view has no address of its own)
        self.c.setop_device(OPS[op], ptr(self.amid, self.na), ptr(self.avmid, self.na) if self.vb else 0, self.na,
                            self.a_num.data_ptr() if self.a_num is not None else 0, ptr(self.bmid, self.nb),
                            ptr(self.bvmid, self.nb) if self.vb and b_values else 0, self.nb, self.b_num.data_ptr() if self.b_num is not None else 0,
                            self.kb, self.kind, self.vb, out_keys, out_values, out_index, ib, out_num, self.desc,
                            torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def run(self, rs, op, ib=8, keys=True, values=True, index=True, b_values=True, what=None):
        """One call with the outputs asked for -> compares each whole allocation with the reference; returns the number kept."""
        torch = self.torch
        cap = capacity(op, self.na, self.nb)
        values = values and self.vb > 0
        ko = guarded(torch, canary(cap * self.kb)) if keys else None
        vo = guarded(torch, canary(cap * self.vb)) if values else None
        io = guarded(torch, canary(cap * ib)) if index else None
        no = guarded(torch, canary(8))
        p = [(o[0].data_ptr() + 64 if o is not None else 0) for o in (ko, vo, io)]
        self.call(op, p[0], p[1], p[2], ib, no[0].data_ptr() + 64, b_values=b_values)
        self.c.check()
        launched = 3 if self.na + self.nb else 0
        assert self.c.get_info(rs.INFO_LAST_PASSES) == PATH | launched, (self.tname, op, hex(self.c.get_info(rs.INFO_LAST_PASSES)))
        wk, wv, wi = self.reference(op)
        num = wi.size
        assert num <= cap
        tag = (self.tname, self.na, self.nb, op, what, "desc" if self.desc else "asc", self.vb, ib, self.n_a, self.n_b)

        def whole(rows, width):  # rows [0, num) exact, rows [num, cap) untouched
            exp = canary(cap * width)
            exp[:num * width] = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
            return with_guards(exp)

        assert same(no[0].cpu().numpy(), with_guards(np.array([num], dtype="<i8")), ("num",) + tag)
        if keys:
            assert same(ko[0].cpu().numpy(), whole(wk, self.kb), ("keys",) + tag)
        if values:
            assert same(vo[0].cpu().numpy(), whole(wv, self.vb), ("values",) + tag)
        if index:
            assert same(io[0].cpu().numpy(), whole(wi.astype("<i4" if ib == 4 else "<i8"), ib), ("index",) + tag)
        return num


def check_named(shape, case, T, kept):
    """The condition a shape is named for, on one case; kept: {op: number kept}."""
    na, nb = case.na, case.nb
    tiles = tile_model(case.a_raw, case.b_raw, case.tname, case.desc, T)
    if shape == "interleaved":
        assert kept["intersection"] == 0 and kept["union"] == na + nb and kept["difference"] == na
    if shape == "identical" and na == nb:
        assert kept["difference"] == 0 and kept["symmetric_difference"] == 0 and kept["intersection"] == na
    if shape == "all_equal" and na != nb and len(tiles) > 1:
        # one run spans every tile: every tile but the first looks its global lower bounds up, and probes leave the tiles
        assert all(t["front_a"] or t["front_b"] for t in tiles[1:]), tiles
        assert sum(t["outside"] for t in tiles) > 0
        assert kept["intersection"] == min(na, nb) and kept["union"] == max(na, nb) and kept["symmetric_difference"] == abs(na - nb)
    if shape == "runs_of_tile" and na > 3 * T and nb > 2 * T:
        # runs of T keys in both arrays: the merge's runs end on tile edges, so a tile whose first key is new skips both searches
        assert any(not t["front_a"] and not t["front_b"] for t in tiles[1:]), tiles
        assert any(t["front_a"] or t["front_b"] for t in tiles[1:]), tiles
    if shape == "dup_mismatch" and na + nb > 2 * T:
        assert any(t["ties"] for t in tiles) and sum(t["outside"] for t in tiles) > 0  # the long runs' probes leave their tiles
        assert 0 < kept["intersection"] < min(na, nb) and 0 < kept["difference"] < na


# ---- the matrix ----
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("tname", ["u32", "u64", "u128"])
def test_every_op_shape_and_size(rs, torch, ctx, tname, shape):
    kb = util.TYPES[tname][2]
    T = rs.setop_caps(kb)
    rng = np.random.default_rng(kb + 7 * SHAPES.index(shape))
    v = 0
    for na, nb in sizes_of(T):
        ia, ib_ = setop_ids(shape, na, nb, T, rng)
        assert ia.size == na and ib_.size == nb
        desc = v % 2 == 0  # the orders and the index widths take turns (the largest size ascending: runs_of_tile)
        a_raw, b_raw = keys_of(tname, ia, ib_, desc)
        case = SetCase(torch, ctx, tname, a_raw, b_raw, desc, *position_values(na, nb))
        kept = {}
        for op in OP_NAMES:
            kept[op] = case.run(rs, op, ib=(4, 8)[(v // 2) % 2], what=shape)
        v += 1
        case.inputs_unchanged()
        assert kept["union"] + kept["intersection"] == na + nb
        assert kept["intersection"] + kept["difference"] == na
        check_named(shape, case, T, kept)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", [t for t in util.PRIMS if t not in ("u32", "u64", "u128")])
def test_other_key_types(rs, torch, ctx, tname, desc):
    kb = util.TYPES[tname][2]
    T = rs.setop_caps(kb)
    rng = np.random.default_rng(kb + desc)
    na, nb = T + 1, T - 1
    for v, shape in enumerate(("dup_mismatch", "blocks")):
        ia, ib_ = setop_ids(shape, na, nb, T, rng)
        a_raw, b_raw = keys_of(tname, ia, ib_, desc)
        case = SetCase(torch, ctx, tname, a_raw, b_raw, desc, *position_values(na, nb))
        for op in OP_NAMES:
            case.run(rs, op, ib=(4, 8)[v % 2], what=shape)
        case.inputs_unchanged()


@pytest.mark.parametrize("tname", ["f32", "f64"])
def test_float_specials(rs, torch, ctx, tname):
    """The seven specials as runs in both arrays: seven different keys by bit pattern, -0.0 and +0.0 apart, the NaNs apart."""
    kb = util.TYPES[tname][2]
    T = rs.setop_caps(kb)
    sp = F32_SPECIALS if kb == 4 else F64_SPECIALS
    for ra, rb in ((1, 1), (3, 2), (T // 7 + 1, T // 5 + 1)):
        for desc in (False, True):
            order = sp[::-1] if desc else sp
            a, b = np.repeat(order, ra), np.repeat(order, rb)
            case = SetCase(torch, ctx, tname, a.view(np.uint8).reshape(-1).copy(), b.view(np.uint8).reshape(-1).copy(), desc,
                           *position_values(a.size, b.size))
            kept = {op: case.run(rs, op, ib=4, what=("specials", ra, rb)) for op in OP_NAMES}
            assert kept == {"union": 7 * max(ra, rb), "intersection": 7 * min(ra, rb), "difference": 7 * max(ra - rb, 0),
                            "symmetric_difference": 7 * abs(ra - rb)}
            case.inputs_unchanged()


@pytest.mark.parametrize("vb", [1, 2, 8, 16])
def test_the_other_value_widths(rs, torch, ctx, vb):
    """One case per fused width besides 4, with the output combinations; intersection and difference without b's values."""
    rng = np.random.default_rng(vb)
    tname, desc = (("u32", False), ("i64", True), ("u128", False), ("u8", True))[(1, 2, 8, 16).index(vb)]
    kb = util.TYPES[tname][2]
    T = rs.setop_caps(kb)
    na, nb = T + 1, T - 1
    ia, ib_ = setop_ids("dup_mismatch", na, nb, T, rng)
    a_raw, b_raw = keys_of(tname, ia, ib_, desc)
    case = SetCase(torch, ctx, tname, a_raw, b_raw, desc, row_values(na, vb, 0), row_values(nb, vb, 1))
    assert case.vb == vb
    for op in OP_NAMES:
        case.run(rs, op, ib=4, what="all three")
        case.run(rs, op, ib=8, keys=False, index=False, what="values without keys")
    case.run(rs, "union", ib=8, values=False, index=False, what="keys only")
    case.run(rs, "symmetric_difference", ib=8, keys=False, values=False, what="index only")
    case.run(rs, "intersection", ib=8, b_values=False, what="b's values not given")
    case.run(rs, "difference", ib=4, b_values=False, what="b's values not given")
    case.inputs_unchanged()


# ---- device counts ----
def test_device_counts(rs, torch, ctx):
    """Capacities (3T + 7, 3T - 5) with counts on the device: the rows beyond the counts hold descending garbage that must not
    reach the result, and a count above the capacity clamps."""
    tname = "u32"
    T = rs.setop_caps(4)
    na, nb = 3 * T + 7, 3 * T - 5
    rng = np.random.default_rng(3)
    ia, ib_ = setop_ids("dup_mismatch", na, nb, T, rng)
    top = int(max(ia.max(), ib_.max())) + 1
    for n_a, n_b in ((T + 1, 0), (T + 1, 2 * T), (na + 100, 2 * T), (0, 0), (na, nb + 1)):
        ga, gb = ia.copy(), ib_.copy()
        ca, cb = min(n_a, na), min(n_b, nb)
        ga[ca:] = top + np.arange(na - ca)[::-1]  # descending, and above every counted key
        gb[cb:] = top + np.arange(nb - cb)[::-1] // 2
        both = keys_from_ids(tname, np.concatenate([ga, gb])).reshape(-1, 4)
        a_raw, b_raw = both[:na].reshape(-1).copy(), both[na:].reshape(-1).copy()
        case = SetCase(torch, ctx, tname, a_raw, b_raw, False, *position_values(na, nb), n_a=n_a, n_b=n_b)
        for v, op in enumerate(OP_NAMES):
            num = case.run(rs, op, ib=(4, 8)[v % 2], what=("counts", n_a, n_b))
            wi = case.reference(op)[2]
            assert num <= ca + cb and bool(((wi < ca) | ((wi >= na) & (wi < na + cb))).all())  # nothing from beyond the counts
        case.inputs_unchanged()


def test_two_groups_combine_without_a_host_read(rs, torch, ctx):
    """README: the keys and num of two radix_group results go through radix_set_op(a_num=, b_num=); compared with numpy."""
    rng = np.random.default_rng(23)
    a = rng.integers(-400, 400, size=30011).astype("<i4")
    b = rng.integers(-300, 500, size=20021).astype("<i4")
    ga = rs.radix_group(torch.from_numpy(a).cuda(), perm=False, ctx=ctx)
    gb = rs.radix_group(torch.from_numpy(b).cuda(), perm=False, ctx=ctx)
    got = {op: rs.radix_set_op(ga.keys, gb.keys, op, a_num=ga.num, b_num=gb.num, ctx=ctx) for op in OP_NAMES}  # nothing read in between
    ctx.check()
    want = {"union": np.union1d(a, b), "intersection": np.intersect1d(a, b), "difference": np.setdiff1d(a, b),
            "symmetric_difference": np.setxor1d(a, b)}
    for op in OP_NAMES:
        r = got[op]
        assert r.num.shape == () and r.num.dtype == torch.int64 and r.index is None
        assert r.keys.shape == (capacity(op, a.size, b.size),)
        assert np.array_equal(r.keys[:int(r.num)].cpu().numpy(), want[op]), op


# ---- the Python calls ----
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", ["i32", "i64", "f32", "u8", "u128"])
def test_radix_set_op_and_pairs(rs, torch, ctx, tname, desc):
    kb = util.TYPES[tname][2]
    T = rs.setop_caps(kb)
    rng = np.random.default_rng(kb + 3 * desc)
    for na, nb in ((0, 5), (7, 0), (0, 0), (2 * T + 11, T + 5)):
        ia, ib_ = setop_ids("dup_mismatch", na, nb, T, rng)
        a_raw, b_raw = keys_of(tname, ia, ib_, desc)
        dt = key_dtype(torch, tname)

        def tens(raw):
            if raw.size == 0:  # (an empty byte tensor cannot be viewed as another dtype)
                return torch.empty((0, 16), dtype=torch.uint8, device="cuda") if kb == 16 else torch.empty(0, dtype=dt, device="cuda")
            t = torch.from_numpy(raw.copy()).cuda()
            return t.view(-1, 16) if kb == 16 else t.view(dt)

        a, b = tens(a_raw), tens(b_raw)
        av_np, bv_np = np.arange(na, dtype="<i8"), -np.arange(nb, dtype="<i8") - 1
        av, bv = torch.from_numpy(av_np).cuda(), torch.from_numpy(bv_np).cuda()
        kk = dict(key_kind=rs.KEY_UNSIGNED) if kb == 16 else {}
        for v, op in enumerate(OP_NAMES):
            wk, wv, wi = setop_reference(a_raw, b_raw, av_np, bv_np, tname, desc, op)
            cap = capacity(op, na, nb)
            idt = (torch.int64, torch.int32)[v % 2]
            r = rs.radix_set_op(a, b, op, descending=desc, return_index=True, index_dtype=idt, ctx=ctx, **kk)
            p = rs.radix_set_op_pairs(a, av, b, bv if v % 2 == 0 or op in ("union", "symmetric_difference") else None, op, descending=desc, ctx=ctx, **kk)
            ctx.check()
            assert int(r.num) == wi.size and int(p.num) == wi.size
            assert r.keys.shape[0] == cap and r.index.shape == (cap,) and r.index.dtype == idt and p.values.shape == (cap,)
            m = wi.size
            assert np.array_equal(r.keys[:m].cpu().numpy().view(np.uint8).reshape(-1), wk)
            assert np.array_equal(p.keys[:m].cpu().numpy().view(np.uint8).reshape(-1), wk)
            assert np.array_equal(r.index[:m].cpu().numpy(), wi)
            assert np.array_equal(p.values[:m].cpu().numpy().view(np.uint8).reshape(-1), wv)
            if cap:
                out = (torch.empty_like(r.keys), torch.empty(cap, dtype=torch.int32, device="cuda"))
                r2 = rs.radix_set_op(a, b, op, descending=desc, return_index=True, out=out, ctx=ctx, **kk)
                assert r2.keys is out[0] and r2.index is out[1] and int(r2.num) == m and np.array_equal(out[1][:m].cpu().numpy(), wi)
    with pytest.raises(ValueError, match="return_index"):
        rs.radix_set_op_pairs(a, av.view(-1, 1).repeat(1, 3).contiguous(), b, bv.view(-1, 1).repeat(1, 3).contiguous(), "union", ctx=ctx, **kk)
    big = torch.empty(4 * (na + nb), dtype=a.dtype, device="cuda") if kb != 16 else None  # an output that begins inside an input
    if big is not None:
        big[:na] = a
        with pytest.raises(rs.RsxError) as e:
            rs.radix_set_op(big[:na], b, "union", descending=desc, out=big[na // 2:na // 2 + na + nb], ctx=ctx)
        assert e.value.status == rs._lib.ERR_ARG


# ---- the precondition broken ----
@pytest.mark.parametrize("tname", ["u32", "i64", "u128"])
def test_unsorted_inputs_stay_in_bounds(rs, torch, ctx, tname):
    """Shuffled a and b: the guards hold, the inputs are unchanged, num <= cap and every position is below na + nb."""
    rng = np.random.default_rng(13)
    kb = util.TYPES[tname][2]
    T = rs.setop_caps(kb)
    for na, nb in ((T + 1, T), (4 * T + 5, 3 * T + 7)):
        n = na + nb
        a_raw = keys_from_ids(tname, rng.integers(0, n // 4, size=na))
        b_raw = keys_from_ids(tname, rng.integers(0, n // 4, size=nb))
        case = SetCase(torch, ctx, tname, a_raw, b_raw, False, *position_values(na, nb))
        for v, op in enumerate(OP_NAMES):
            ib = (4, 8)[v % 2]
            cap = capacity(op, na, nb)
            ko, vo, io = (guarded(torch, canary(cap * w)) for w in (kb, 4, ib))
            no = guarded(torch, canary(8))
            case.call(op, ko[1].data_ptr(), vo[1].data_ptr(), io[1].data_ptr(), ib, no[1].data_ptr())
            ctx.check()
            num = int(no[1].view(torch.int64)[0])
            assert 0 <= num <= cap, (tname, op, num, cap)
            got = io[1].view(torch.int32 if ib == 4 else torch.int64)[:num]
            assert num == 0 or (int(got.min()) >= 0 and int(got.max()) < n), (tname, na, nb, op)
            for buf, _mid in (ko, vo, io, no):
                whole = buf.cpu().numpy()
                assert (whole[:64] == 0xA5).all() and (whole[-64:] == 0xA5).all(), (tname, na, nb, op)
        case.inputs_unchanged()


# ---- empty inputs, capture, errors ----
def test_nothing_to_do(rs, torch, ctx):
    E = rs._lib
    L, h = ctx._L, ctx._h
    num = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    # na + nb == 0: the count is stored, nothing is launched and no other pointer is looked at (dangling values here)
    assert L.rsx_setop_device(h, 0, 8, 8, 0, None, 8, 8, 0, None, 4, 0, 4, 0, 8, 8, 8, 8, num.data_ptr(), None) == E.OK
    assert int(num) == 0 and ctx.get_info(rs.INFO_LAST_PASSES) == PATH
    e = torch.zeros(0, dtype=torch.int32, device="cuda")
    x = torch.arange(5, dtype=torch.int32, device="cuda")
    for op, ex, xe in (("union", [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]), ("intersection", [], []), ("difference", [], [0, 1, 2, 3, 4]),
                       ("symmetric_difference", [0, 1, 2, 3, 4], [0, 1, 2, 3, 4])):
        assert int(rs.radix_set_op(e, e, op, ctx=ctx).num) == 0
        r = rs.radix_set_op(e, x, op, ctx=ctx)
        assert r.keys[:int(r.num)].tolist() == ex
        r = rs.radix_set_op(x, e, op, return_index=True, ctx=ctx)
        assert r.keys[:int(r.num)].tolist() == xe and r.index[:int(r.num)].tolist() == xe
    ctx.check()


def test_capture_after_reserve_and_workspace_error_without(rs, torch):
    T = rs.setop_caps(4)
    na, nb = 2 * T + 9, 3 * T + 1
    src_a = torch.zeros(na, dtype=torch.int32, device="cuda")
    src_b = torch.zeros(nb, dtype=torch.int32, device="cuda")
    a, b = torch.empty_like(src_a), torch.empty_like(src_b)
    av = torch.arange(na, dtype=torch.int32, device="cuda")
    bv = torch.arange(nb, dtype=torch.int32, device="cuda") + (1 << 30)
    keys = torch.empty(na + nb, dtype=torch.int32, device="cuda")
    vals = torch.empty(na + nb, dtype=torch.int32, device="cuda")
    idx = torch.empty(na + nb, dtype=torch.int32, device="cuda")
    num = torch.empty((), dtype=torch.int64, device="cuda")

    def enqueue(c):
        c.setop_device(rs._lib.SETOP_SYMMETRIC_DIFFERENCE, a.data_ptr(), av.data_ptr(), na, 0, b.data_ptr(), bv.data_ptr(), nb, 0, 4, rs.KEY_SIGNED, 4,
                       keys.data_ptr(), vals.data_ptr(), idx.data_ptr(), 4, num.data_ptr(), False, torch.cuda.current_stream().cuda_stream)

    # without a reserve: the context has made an ordinary call (its error word and self-tests exist) but owns no workspace
    c0 = rs.Context(torch.cuda.current_device())
    x = torch.randint(0, 2 ** 31 - 1, (1000,), dtype=torch.int32, device="cuda")
    rs.radix_sort(x, ctx=c0)
    c0.check()
    keys.fill_(-1)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g.capture_begin()
        try:
            enqueue(c0)
        except rs.RsxError as e:
            err = e
        g.capture_end()
    assert err is not None and err.status == rs._lib.ERR_WORKSPACE, err
    torch.cuda.synchronize()
    assert bool((keys == -1).all())  # nothing was enqueued
    c0.close()

    c = rs.Context(torch.cuda.current_device())
    c.reserve_setop(na + nb, 4)
    graph = torch.cuda.CUDAGraph()
    s.synchronize()
    with torch.cuda.graph(graph, stream=s):  # one linear chain: the two copies, then the call's three launches
        a.copy_(src_a)
        b.copy_(src_b)
        enqueue(c)
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
        wk, wv, wi = setop_reference(a_np.view(np.uint8), b_np.view(np.uint8), av.cpu().numpy(), bv.cpu().numpy(), "i32", False, "symmetric_difference")
        m = wi.size
        assert int(num) == m
        assert np.array_equal(keys[:m].cpu().numpy().view(np.uint8), wk) and np.array_equal(vals[:m].cpu().numpy().view(np.uint8), wv)
        assert np.array_equal(idx[:m].cpu().numpy(), wi) and bool((keys[m:] == -1).all()) and bool((idx[m:] == -1).all())
    c.close()


def test_errors(rs, torch, ctx):
    E = rs._lib
    L, h = ctx._L, ctx._h
    P = 4096
    buf = torch.full((10 * P,), 0xA5, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert p % 16 == 0
    ok = dict(op=0, ak=p, av=p + P, na=100, an=0, bk=p + 2 * P, bv=p + 3 * P, nb=50, bn=0, kb=4, kind=0, vb=8, order=0, ok=p + 4 * P, ov=p + 5 * P,
              oi=p + 7 * P, ib=8, on=p + 9 * P)

    def call(**kw):
        a = dict(ok, **kw)
        return L.rsx_setop_device(h, a["op"], a["ak"] or None, a["av"] or None, a["na"], a["an"] or None, a["bk"] or None, a["bv"] or None, a["nb"],
                                  a["bn"] or None, a["kb"], a["kind"], a["vb"], a["order"], a["ok"] or None, a["ov"] or None, a["oi"] or None, a["ib"],
                                  a["on"] or None, None)

    novals = dict(av=0, bv=0, ov=0, vb=0)
    assert call(op=4) == E.ERR_ARG
    assert call(kb=3) == E.ERR_ARG and call(kb=16, kind=2) == E.ERR_ARG and call(kind=3) == E.ERR_ARG
    assert call(vb=32769) == E.ERR_ARG and call(vb=12) == E.ERR_UNSUPPORTED and call(vb=32) == E.ERR_UNSUPPORTED
    assert call(order=2) == E.ERR_ARG
    assert call(ib=2) == E.ERR_ARG and call(ib=0) == E.ERR_ARG
    assert call(on=0) == E.ERR_ARG and call(on=ok["on"] + 4) == E.ERR_ARG      # the count word: required, 8-byte aligned
    assert call(an=ok["on"] + 12) == E.ERR_ARG and call(bn=ok["on"] + 20) == E.ERR_ARG
    assert call(ok=0, ov=0, oi=0) == E.ERR_ARG                                # all outputs null
    assert call(ak=0) == E.ERR_ARG and call(bk=0) == E.ERR_ARG                 # null inputs with a nonzero count
    assert call(av=0) == E.ERR_ARG and call(bv=0) == E.ERR_ARG                 # a union emits from both sides
    assert call(op=3, bv=0) == E.ERR_ARG
    assert call(vb=0) == E.ERR_ARG and call(ov=0, vb=0) == E.ERR_ARG           # vb == 0 <=> no value pointer
    for name in ("ak", "bk", "ok"):
        assert call(**{name: ok[name] + 2}) == E.ERR_ARG, name
    for name in ("av", "bv", "ov", "oi"):
        assert call(**{name: ok[name] + 4}) == E.ERR_ARG, name
    assert call(**novals, na=2 ** 32, nb=1, ib=4, ok=0) == E.ERR_ARG           # 4-byte positions cannot count them
    assert call(**novals, na=2 ** 62, nb=0, ok=0) == E.ERR_UNSUPPORTED          # 2^31 tiles or more
    assert L.rsx_ctx_reserve_setop(h, 2 ** 62, 4) == E.ERR_UNSUPPORTED and L.rsx_ctx_reserve_setop(h, 100, 3) == E.ERR_ARG
    # overlaps: against cap(op) rows of every output
    last = lambda base, cnt, w: base + cnt * w - w  # noqa: E731
    assert call(ok=ok["ak"]) == E.ERR_ARG and call(ok=last(ok["ak"], 100, 4)) == E.ERR_ARG
    assert call(ok=ok["bk"] - 150 * 4 + 4) == E.ERR_ARG                        # union: the 150th row is b's first key
    assert call(op=1, ok=ok["bk"] - 50 * 4 + 4) == E.ERR_ARG                   # intersection: the 50th row is b's first key
    assert call(ov=ok["ak"]) == E.ERR_ARG and call(ov=last(ok["bv"], 50, 8)) == E.ERR_ARG and call(oi=ok["av"]) == E.ERR_ARG
    assert call(ov=ok["ok"]) == E.ERR_ARG and call(oi=ok["ok"] + 592) == E.ERR_ARG and call(ok=ok["oi"] + 1192) == E.ERR_ARG
    assert call(on=ok["ak"] + 8) == E.ERR_ARG and call(on=ok["ok"] + 8) == E.ERR_ARG and call(on=ok["oi"] + 1192) == E.ERR_ARG
    assert call(an=ok["on"]) == E.ERR_ARG and call(bn=ok["on"]) == E.ERR_ARG   # the count written over a count read
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())                                          # no refused call wrote
    # what is allowed: cap(op) rows that end in front of b (difference: 100, intersection: 50) where a union's 150 would not
    assert call(op=2, ok=ok["bk"] - 150 * 4 + 4, **novals) == E.OK and call(op=1, ok=ok["bk"] - 50 * 4, **novals) == E.OK
    assert call(op=1, bv=0) == E.OK and call(op=2, bv=0) == E.OK               # b's values are not looked at
    assert call(oi=ok["oi"] + 4, ib=4) == E.OK and call(oi=0, ib=3) == E.OK
    assert call(ok=0) == E.OK and call(ok=0, ov=0) == E.OK
    assert call(na=0, ak=0, av=0) == E.OK and call(nb=0, bk=0, bv=0) == E.OK   # an empty side needs no pointers
    ctx.check()
