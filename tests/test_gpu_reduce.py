"""GPU: rsx_reduce_by_key_device / radix_reduce_by_key against tests/reduce_ref.py.

Every array sits in an allocation the test owns: 64 guard bytes of 0xA5, the array (outputs filled with 0xA5), 64 guard
bytes.  What comes back is compared whole: the entries the definition writes hold the reference's bytes, the entries of
out_keys and out_values at m and beyond, those of out_offsets beyond m and all guards still hold 0xA5; both input columns
are compared with what was put in.

Sizes come from rsx_reduce_caps (T = tile, S = scan_span): 1, 2, T - 1, T, T + 1, 3T + 5 and S*T + T + 3 (the scan's
second sweep).  Shapes and keys are those of test_gpu_unique.py (group ids mapped into the key type).

Values.  Integers: uniform over the whole range of the type, so sums wrap.  Floats come in three forms:
  (a) nonzero integers in [-8, 8] as floats (one in eight negative), and now and then a -0.0 or +0.0: every partial sum
      is exact in any association, so sums are compared as BYTES -- except a group whose exact sum is zero and whose values
      are not all -0.0, which may come out as +0.0 or -0.0 and is compared as a number; the reference alone says which
      groups those are, and every case asserts that they are at most 1 in 20 of its groups;
  (b) standard normal values times 2^k, k uniform in [-20, 20]: |result - longdouble sum| <= g(c-1) * sum|v|;
  (c) specials, in tests of their own: +inf among finite values sums to +inf, a NaN sums to a NaN, +inf and -inf to a NaN,
      MIN and MAX over the seven special patterns of test_gpu_unique.py as bytes.
MIN and MAX of floats in the matrix use form (a): bytes.

The matrix.  Key types u8 i16 u32 f32 i64 u128 (index k), value types i32 u32 f32 i64 u64 f64 (index v), ops sum min max
(index o), orders ascending / descending (index d): the THINNING RULE keeps the combination when k + v + o + d is even --
108 of the 216, half.  Fixing any two of the four indices leaves both parities reachable through the other two, so every
(key width, value type), every (value type, op) and both orders of every key width are kept.  The 49 (size, shape)
pairs are numbered p = 7 * size index + shape index; the c-th kept combination OF ITS VALUE WIDTH (c = 0 .. 53) runs the
pairs with (p + c) % 16 == 0, three or four each: c takes every residue modulo 16, so every size with every shape runs
at least three times per value width.  A float SUM runs its pairs in forms (a) and (b)."""
import numpy as np
import pytest

import util
from reduce_ref import FLOAT, MAX, MIN, SIGNED, SUM, UNSIGNED, reduce_reference, value_dtype
from segment_pairs_gpu import guarded, joined_elem, same
from segment_pairs_ref import with_guards
from test_gpu_unique import F32_SPECIALS, F64_SPECIALS, SHAPES, canary, first_then_canary, group_ids, keys_of
from unique_ref import unique_reference

pytestmark = pytest.mark.gpu

KEY_TYPES = ["u8", "i16", "u32", "f32", "i64", "u128"]
VALUE_TYPES = {"i32": (4, SIGNED), "u32": (4, UNSIGNED), "f32": (4, FLOAT), "i64": (8, SIGNED), "u64": (8, UNSIGNED), "f64": (8, FLOAT)}
VALUE_NAMES = list(VALUE_TYPES)
OPS = [SUM, MIN, MAX]
OP_NAMES = {SUM: "sum", MIN: "min", MAX: "max"}
PATH = 9 << 24


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
def sizes_for(rs, kb, vb):
    T, S = rs.reduce_caps(kb, vb)
    return [1, 2, T - 1, T, T + 1, 3 * T + 5, S * T + T + 3]


def values_of(vname, n, rng, form):
    vb, vkind = VALUE_TYPES[vname]
    dt = value_dtype(vb, vkind)
    if vkind != FLOAT:
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, size=n, dtype=dt, endpoint=True)
    if form == "a":
        v = rng.integers(1, 9, size=n).astype(dt)
        v[rng.random(n) < 0.125] *= -1
        zero = rng.random(n) < 1.0 / 64
        v[zero] = np.where(rng.random(int(zero.sum())) < 0.5, dt.type(-0.0), dt.type(0.0))
        return v
    assert form == "b"
    return (rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, size=n))).astype(dt)


# ---- one call on guarded buffers ----
class Case:
    """One key column on the GPU (guarded) with its groups per order, and reduce_by_key_device calls on it."""

    def __init__(self, torch, c, tname, keys_raw):
        self.torch, self.c, self.tname = torch, c, tname
        self.kb, self.kind = util.TYPES[tname][2], util.TYPES[tname][3]
        self.keys_raw = keys_raw
        self.n = keys_raw.size // self.kb
        self.kbuf, self.kmid = guarded(torch, keys_raw)
        self.groups = {}

    def reference(self, vals, vname, op, desc):
        if desc not in self.groups:
            self.groups[desc] = unique_reference(self.keys_raw, self.kb, self.kind, desc)
        vb, vkind = VALUE_TYPES[vname]
        return reduce_reference(self.keys_raw, self.kb, self.kind, vals.view(np.uint8), vb, vkind, op, desc, groups=self.groups[desc])

    def call(self, vals, vname, op, desc, keys=True, values=True, offsets=True, c=None):
        """-> the whole allocations (numpy bytes) of out_keys, out_values, out_offsets, num and of the value column"""
        torch, n, kb = self.torch, self.n, self.kb
        c = c or self.c
        vb, vkind = VALUE_TYPES[vname]
        vbuf, vmid = guarded(torch, vals.view(np.uint8))
        bufs = {}
        for name, want, nbytes in (("keys", keys, n * kb), ("values", values, n * vb), ("offsets", offsets, (n + 1) * 8), ("num", True, 8)):
            bufs[name] = guarded(torch, canary(nbytes)) if want else (None, None)
        ptr = {k: (v[0].data_ptr() + 64 if v[0] is not None else 0) for k, v in bufs.items()}  # (an empty view has no address of its own)
        c.reduce_by_key_device(self.kmid.data_ptr() if n else 0, vmid.data_ptr() if n else 0, n, kb, self.kind, vb, vkind, op, ptr["keys"],
                               ptr["values"], ptr["offsets"], ptr["num"], desc, torch.cuda.current_stream().cuda_stream)
        c.check()
        out = {k: (v[0].cpu().numpy() if v[0] is not None else None) for k, v in bufs.items()}
        out["in_values"] = vbuf.cpu().numpy()
        return out

    def run(self, vals, vname, op, desc, form=None, what=None, **kw):
        n, kb = self.n, self.kb
        vb, vkind = VALUE_TYPES[vname]
        got = self.call(vals, vname, op, desc, **kw)
        ref = self.reference(vals, vname, op, desc)
        m = ref.m
        tag = (self.tname, vname, OP_NAMES[op], n, what, form, "desc" if desc else "asc")
        assert same(got["num"], with_guards(np.array([m], dtype="<u8")), ("num",) + tag)
        if got["keys"] is not None:
            assert same(got["keys"], with_guards(first_then_canary(ref.keys, n * kb)), ("out_keys",) + tag)
        if got["offsets"] is not None:
            assert same(got["offsets"], with_guards(first_then_canary(ref.offsets.astype("<u8").view(np.uint8), (n + 1) * 8)), ("out_offsets",) + tag)
        assert same(got["in_values"], with_guards(vals.view(np.uint8)), ("the value column",) + tag)
        assert same(self.kbuf.cpu().numpy(), with_guards(self.keys_raw), ("the key column",) + tag)
        if got["values"] is None:
            return ref
        if ref.values is not None:  # integers, float MIN and MAX: bytes
            assert same(got["values"], with_guards(first_then_canary(ref.values, n * vb)), ("out_values",) + tag)
            return ref
        dt = value_dtype(vb, vkind)
        mine = got["values"][64:64 + m * vb].copy()
        if form == "a":  # exact sums: bytes, but for the groups whose zero sum has no fixed sign
            starts = ref.offsets[:-1]
            g = vals[ref.perm]
            all_negative_zero = np.logical_and.reduceat((g == 0) & np.signbit(g), starts) if m else np.zeros(0, dtype=bool)
            free = (ref.exact.view(dt) == 0) & ~all_negative_zero
            print(tag, "groups", m, "with a zero sum of free sign", int(free.sum()))
            assert int(free.sum()) * 20 <= m, ("more than 1 in 20 groups have a zero sum of free sign", int(free.sum()), m) + tag
            assert np.all(mine.view(dt)[free] == 0), ("a zero sum is not zero",) + tag
            want = ref.exact.view(dt).copy()
            want[free] = mine.view(dt)[free]
            assert same(got["values"], with_guards(first_then_canary(want.view(np.uint8), n * vb)), ("out_values",) + tag)
        else:  # the order-free bound against the longdouble sums
            err = np.abs(mine.view(dt).astype(np.longdouble) - ref.sums)
            worst = int(np.argmax(err - ref.bound)) if m else 0
            print(tag, "groups", m, "largest error / bound", float(np.max(err / np.maximum(ref.bound, np.finfo(np.longdouble).tiny))) if m else 0.0)
            assert np.all(np.isfinite(mine.view(dt))) and np.all(err <= ref.bound), \
                ("outside g(c-1) * sum|v|", worst, float(err[worst]), float(ref.bound[worst])) + tag
            assert same(got["values"], with_guards(first_then_canary(mine, n * vb)), ("out_values behind m",) + tag)
        return ref


# ---- the matrix ----
def kept_combinations():
    out, per_width = [], {4: 0, 8: 0}
    for k, tname in enumerate(KEY_TYPES):
        for v, vname in enumerate(VALUE_NAMES):
            for o, op in enumerate(OPS):
                for d in (0, 1):
                    if (k + v + o + d) % 2:
                        continue
                    vb = VALUE_TYPES[vname][0]
                    out.append((tname, vname, op, bool(d), per_width[vb]))
                    per_width[vb] += 1
    return out


COMBINATIONS = kept_combinations()


def test_the_thinning_rule_covers_what_it_must():
    full = len(KEY_TYPES) * len(VALUE_NAMES) * len(OPS) * 2
    assert len(COMBINATIONS) * 2 >= full
    assert {(t, v) for t, v, _o, _d, _c in COMBINATIONS} == {(t, v) for t in KEY_TYPES for v in VALUE_NAMES}
    assert {(v, o) for _t, v, o, _d, _c in COMBINATIONS} == {(v, o) for v in VALUE_NAMES for o in OPS}
    assert {(t, d) for t, _v, _o, d, _c in COMBINATIONS} == {(t, d) for t in KEY_TYPES for d in (False, True)}
    for vb in (4, 8):
        pairs = set()
        for _t, v, _o, _d, c in COMBINATIONS:
            if VALUE_TYPES[v][0] == vb:
                pairs |= {p for p in range(49) if (p + c) % 16 == 0}
        assert pairs == set(range(49))


@pytest.mark.parametrize("tname,vname,op,desc,c", COMBINATIONS, ids=[f"{t}-{v}-{OP_NAMES[o]}-{'desc' if d else 'asc'}" for t, v, o, d, _c in COMBINATIONS])
def test_matrix(rs, torch, ctx, tname, vname, op, desc, c):
    kb = util.TYPES[tname][2]
    vb, vkind = VALUE_TYPES[vname]
    T = rs.reduce_caps(kb, vb)[0]
    sizes = sizes_for(rs, kb, vb)
    rng = np.random.default_rng(1000 + c * 2 + vb)
    for p in range(49):
        if (p + c) % 16:
            continue
        n, shape = sizes[p // 7], SHAPES[p % 7]
        case = Case(torch, ctx, tname, keys_of(tname, group_ids(shape, n, T, rng)))
        forms = ("a", "b") if (vkind == FLOAT and op == SUM) else ("a",) if vkind == FLOAT else (None,)
        for form in forms:
            ref = case.run(values_of(vname, n, rng, form), vname, op, desc, form=form, what=shape)
            if shape == "equal":
                assert ref.m == 1
            assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 3
            assert ctx.get_info(rs.INFO_LAST_PAIRS) == 1 | joined_elem(kb, vb) << 8


@pytest.mark.parametrize("vname", ["f32", "f64"])
@pytest.mark.parametrize("shape", ["equal", "long_run", "runs_of_tile", "runs_shifted"])
def test_the_carry_shapes_at_the_second_sweep(rs, torch, ctx, shape, vname):
    """One run through every tile and across the sweep boundary, whole tiles without a head, runs that end on the last slot
    of a tile (the carry must not leak into the next run) and one slot further: float sums in both forms, u32 keys."""
    vb = VALUE_TYPES[vname][0]
    T, S = rs.reduce_caps(4, vb)
    n = S * T + T + 3
    rng = np.random.default_rng(S + vb)
    case = Case(torch, ctx, "u32", keys_of("u32", group_ids(shape, n, T, rng)))
    for form in ("a", "b"):
        case.run(values_of(vname, n, rng, form), vname, SUM, shape == "runs_shifted", form=form, what=shape)


# ---- float specials ----
@pytest.mark.parametrize("vname", ["f32", "f64"])
def test_sums_of_infinities_and_nans(rs, torch, ctx, vname):
    vb, _vk = VALUE_TYPES[vname]
    dt = value_dtype(vb, FLOAT)
    T = rs.reduce_caps(4, vb)[0]
    rng = np.random.default_rng(3)
    for n in (64, 2 * T + 9):
        g = rng.integers(0, 4, size=n, dtype=np.int64)  # group 0: finite; 1: a +inf; 2: a NaN; 3: +inf and -inf
        vals = values_of(vname, n, rng, "a")
        for grp, specials in ((1, [np.inf]), (2, [np.nan]), (3, [np.inf, -np.inf])):
            where = np.nonzero(g == grp)[0]
            assert where.size > len(specials)
            vals[rng.choice(where, size=len(specials), replace=False)] = specials
        case = Case(torch, ctx, "u32", keys_of("u32", g))
        got = case.call(vals, vname, SUM, False)
        assert int(got["num"][64:72].view("<u8")[0]) == 4
        sums = got["values"][64:64 + 4 * vb].view(dt)
        exact = float(vals[g == 0].astype(np.float64).sum())
        assert sums[0] == exact and sums[1] == np.inf and np.isnan(sums[2]) and np.isnan(sums[3]), sums
        assert np.all(got["values"][64 + 4 * vb:] == 0xA5)


@pytest.mark.parametrize("vname", ["f32", "f64"])
def test_min_and_max_of_the_special_patterns(rs, torch, ctx, vname):
    vb, _vk = VALUE_TYPES[vname]
    sp = F32_SPECIALS if vb == 4 else F64_SPECIALS
    T = rs.reduce_caps(8, vb)[0]
    rng = np.random.default_rng(4)
    for n in (7, 64, 3 * T + 5):
        vals = sp[rng.integers(0, 7, size=n)].view(value_dtype(vb, FLOAT))
        ordinary = rng.random(n) < 0.3
        vals[ordinary] = values_of(vname, int(ordinary.sum()), rng, "b")
        for shape in ("seven", "third", "equal"):
            case = Case(torch, ctx, "i64", keys_of("i64", group_ids(shape, n, T, rng)))
            for op in (MIN, MAX):
                for desc in (False, True):
                    case.run(vals, vname, op, desc, what=("specials", shape))
    one = Case(torch, ctx, "u8", np.zeros(7, dtype=np.uint8))  # all seven in one group: -NaN is the minimum, the NaN of the larger payload the maximum
    all_seven = sp[rng.permutation(7)].view(value_dtype(vb, FLOAT))
    assert one.run(all_seven, vname, MIN, False).values.view(sp.dtype)[0] == sp[0]
    assert one.run(all_seven, vname, MAX, False).values.view(sp.dtype)[0] == sp[6]


# ---- the same bytes on every call ----
@pytest.mark.parametrize("vname", ["f32", "f64"])
def test_float_sums_are_the_same_bytes_on_every_call(rs, torch, ctx, vname):
    vb = VALUE_TYPES[vname][0]
    T, S = rs.reduce_caps(4, vb)
    fresh = rs.Context(torch.cuda.current_device())
    rng = np.random.default_rng(5)
    for n in (3 * T + 5, S * T + T + 3):
        for shape in ("seven", "long_run", "third"):
            case = Case(torch, ctx, "u32", keys_of("u32", group_ids(shape, n, T, rng)))
            vals = values_of(vname, n, rng, "b")
            first = case.call(vals, vname, SUM, False)
            again = case.call(vals, vname, SUM, False)
            other = case.call(vals, vname, SUM, False, c=fresh)
            for name in ("num", "keys", "values", "offsets"):
                assert np.array_equal(first[name], again[name]), (name, n, shape, "second call")
                assert np.array_equal(first[name], other[name]), (name, n, shape, "fresh context")
    fresh.close()


# ---- aliasing, agreement with the group call ----
@pytest.mark.parametrize("tname,vname,op", [("u32", "f32", SUM), ("i64", "i64", SUM), ("u8", "f64", MAX), ("u128", "u32", MIN), ("i16", "i32", SUM)])
def test_outputs_may_be_the_inputs(rs, torch, ctx, tname, vname, op):
    kb, kind = util.TYPES[tname][2], util.TYPES[tname][3]
    vb, vkind = VALUE_TYPES[vname]
    T = rs.reduce_caps(kb, vb)[0]
    rng = np.random.default_rng(6)
    for n in (1, T + 1, 3 * T + 5):
        keys_raw = keys_of(tname, group_ids("third", n, T, rng))
        vals = values_of(vname, n, rng, "a")
        for desc in (False, True):
            apart = Case(torch, ctx, tname, keys_raw).call(vals, vname, op, desc, offsets=False)
            m = int(apart["num"][64:72].view("<u8")[0])
            kbuf, kmid = guarded(torch, keys_raw)
            vbuf, vmid = guarded(torch, vals.view(np.uint8))
            num = torch.zeros((), dtype=torch.int64, device="cuda")
            ctx.reduce_by_key_device(kmid.data_ptr(), vmid.data_ptr(), n, kb, kind, vb, vkind, op, kmid.data_ptr(), vmid.data_ptr(), 0,
                                     num.data_ptr(), desc, torch.cuda.current_stream().cuda_stream)
            ctx.check()
            assert int(num) == m
            want_k = keys_raw.copy()
            want_k[:m * kb] = apart["keys"][64:64 + m * kb]
            want_v = vals.view(np.uint8).copy()
            want_v[:m * vb] = apart["values"][64:64 + m * vb]
            assert same(kbuf.cpu().numpy(), with_guards(want_k), ("keys in place", tname, vname, n, desc))
            assert same(vbuf.cpu().numpy(), with_guards(want_v), ("values in place", tname, vname, n, desc))


@pytest.mark.parametrize("tname", KEY_TYPES)
def test_groups_are_those_of_the_group_call(rs, torch, ctx, tname):
    kb, kind = util.TYPES[tname][2], util.TYPES[tname][3]
    T = rs.reduce_caps(kb, 4)[0]
    rng = np.random.default_rng(7)
    for n, shape in ((T + 1, "third"), (3 * T + 5, "seven"), (3 * T + 5, "runs_shifted")):
        keys_raw = keys_of(tname, group_ids(shape, n, T, rng))
        vals = values_of("i32", n, rng, None)
        for desc in (False, True):
            got = Case(torch, ctx, tname, keys_raw).call(vals, "i32", SUM, desc)
            kbuf, kmid = guarded(torch, keys_raw)
            outs = [guarded(torch, canary(nb)) for nb in (n * kb, (n + 1) * 8, 8)]
            ctx.unique_device(kmid.data_ptr(), n, kb, kind, outs[0][1].data_ptr(), outs[1][1].data_ptr(), 0, 0, 8, outs[2][1].data_ptr(), desc,
                              torch.cuda.current_stream().cuda_stream)
            ctx.check()
            for name, o in zip(("keys", "offsets", "num"), outs):
                assert same(got[name], o[0].cpu().numpy(), (name, tname, n, shape, desc))


def test_keys_alone_and_values_alone(rs, torch, ctx):
    T = rs.reduce_caps(4, 8)[0]
    rng = np.random.default_rng(8)
    n = 2 * T + 1
    case = Case(torch, ctx, "f32", keys_of("f32", group_ids("third", n, T, rng)))
    vals = values_of("u64", n, rng, None)
    case.run(vals, "u64", SUM, True, values=False, what="keys alone")
    case.run(vals, "u64", SUM, True, keys=False, offsets=False, what="values alone")
    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 3


def test_empty_and_single(rs, torch, ctx):
    empty = Case(torch, ctx, "u32", np.zeros(0, dtype=np.uint8))
    for vname in ("f32", "i64"):
        ref = empty.run(np.zeros(0, dtype=value_dtype(*VALUE_TYPES[vname])), vname, SUM, False)  # num == 0, offsets[0] == 0, nothing else
        assert ref.m == 0
        assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH
    r = rs.radix_reduce_by_key(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.float64, device="cuda"), offsets=True, ctx=ctx)
    assert int(r.num) == 0 and int(r.offsets[0]) == 0 and r.keys.numel() == 0 and r.values.numel() == 0
    rng = np.random.default_rng(9)
    for tname, vname in (("u8", "f64"), ("f32", "i32"), ("u128", "u64")):
        one = Case(torch, ctx, tname, util.make_input(tname, 1, "uniform", seed=1))
        for op in OPS:
            one.run(values_of(vname, 1, rng, "a"), vname, op, op == MIN, form="a", what="n = 1")
    z = np.array([-0.0], dtype="<f4")
    ref = Case(torch, ctx, "u32", np.zeros(4, dtype=np.uint8)).run(z, "f32", SUM, False, form="a", what="one -0.0")
    assert ref.exact.view("<u4")[0] == 0x80000000


# ---- stream capture ----
def test_capture_and_replay(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    n = 300001
    c.reserve_reduce(n, 4, 4)
    rng = np.random.default_rng(10)
    inputs = [(util.make_input("u32", n, dist, seed=80 + i), values_of("f32", n, rng, "a")) for i, dist in enumerate(("step16", "highbyte"))]
    ksrc = torch.from_numpy(inputs[0][0].copy()).cuda().view(torch.uint32)
    vsrc = torch.from_numpy(inputs[0][1].copy()).cuda()
    keys, vals = torch.empty_like(ksrc), torch.empty_like(vsrc)
    out_keys, out_vals = torch.empty_like(ksrc), torch.empty_like(vsrc)
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    num = torch.empty((), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()

    def enqueue():
        c.reduce_by_key_device(keys.data_ptr(), vals.data_ptr(), n, 4, rs.KEY_UNSIGNED, 4, rs.KEY_FLOAT, SUM, out_keys.data_ptr(), out_vals.data_ptr(),
                               offsets.data_ptr(), num.data_ptr(), True, torch.cuda.current_stream().cuda_stream)

    with torch.cuda.stream(s):
        keys.copy_(ksrc)
        vals.copy_(vsrc)
        enqueue()  # warm-up outside capture
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):  # one linear chain: the copies, then the call's launches
        keys.copy_(ksrc)
        vals.copy_(vsrc)
        enqueue()
    for kraw, v in inputs:
        ksrc.view(torch.uint8).copy_(torch.from_numpy(kraw.copy()))
        vsrc.copy_(torch.from_numpy(v.copy()))
        for t in (out_keys.view(torch.int32), offsets):
            t.fill_(-1)
        out_vals.fill_(-77.0)
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        ref = reduce_reference(kraw, 4, UNSIGNED, v.view(np.uint8), 4, FLOAT, SUM, True)
        m = ref.m
        assert int(num) == m
        assert np.array_equal(out_keys[:m].view(torch.uint8).cpu().numpy().reshape(-1), ref.keys)
        assert np.array_equal(offsets[:m + 1].cpu().numpy(), ref.offsets) and bool((offsets[m + 1:] == -1).all())
        assert np.array_equal(out_vals[:m].cpu().numpy(), ref.exact.view("<f4")) and bool((out_vals[m:] == -77.0).all())  # (groups of thousands: no zero sums)
    c.close()


def test_unreserved_call_under_capture_reports_workspace(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    x = torch.randint(0, 2 ** 31 - 1, (1000,), dtype=torch.int32, device="cuda")
    rs.radix_reduce_by_key(x, x.clone(), ctx=c)  # one ordinary call: the context's error word and self-tests exist
    c.check()
    n = 1 << 16  # more than the context has seen
    keys = torch.randint(0, 1000, (n,), dtype=torch.int32, device="cuda")
    vals = torch.randint(0, 1000, (n,), dtype=torch.int64, device="cuda")
    before = (keys.clone(), vals.clone())
    outs = [torch.full((n + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(3)]
    num = torch.full((), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g.capture_begin()
        try:
            c.reduce_by_key_device(keys.data_ptr(), vals.data_ptr(), n, 4, rs.KEY_SIGNED, 8, rs.KEY_SIGNED, SUM, outs[0].data_ptr(), outs[1].data_ptr(),
                                   outs[2].data_ptr(), num.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
        except rs.RsxError as e:
            err = e
        g.capture_end()
    assert err is not None and err.status == rs._lib.ERR_WORKSPACE, err
    torch.cuda.synchronize()
    assert torch.equal(keys, before[0]) and torch.equal(vals, before[1]) and int(num) == -1 and all(bool((o == -1).all()) for o in outs)  # nothing was enqueued
    c.close()


def test_errors(rs, torch, ctx):
    E = rs._lib
    rng = np.random.default_rng(11)
    case = Case(torch, ctx, "u32", util.make_input("u32", 200, "two", seed=2))
    L, h = ctx._L, ctx._h
    buf = torch.full((5 * 4096,), 0xA5, dtype=torch.uint8, device="cuda")  # a region of 4 KiB per array
    p = buf.data_ptr()
    k = case.kmid.data_ptr()
    assert p % 16 == 0 and k % 16 == 0
    ok = dict(keys=k, vals=p, n=200, kb=4, kind=0, vb=8, vkind=1, op=0, order=0, ok_=p + 4096, ov=p + 2 * 4096, off=p + 3 * 4096, num=p + 4 * 4096)

    def call(**kw):
        a = dict(ok, **kw)
        return L.rsx_reduce_by_key_device(h, a["keys"] or None, a["vals"] or None, a["n"], a["kb"], a["kind"], a["vb"], a["vkind"], a["op"],
                                          a["order"], a["ok_"] or None, a["ov"] or None, a["off"] or None, a["num"] or None, None)

    assert call() == E.OK
    ctx.check()
    assert call(kb=3) == E.ERR_ARG                      # key width
    assert call(kb=16, kind=2) == E.ERR_ARG             # float keys of 16 bytes
    for vb in (0, 1, 2, 3, 12, 16):
        assert call(vb=vb) == E.ERR_ARG                 # value width
    assert call(vkind=3) == E.ERR_ARG
    assert call(op=3) == E.ERR_ARG and call(op=-1) == E.ERR_ARG
    assert call(order=2) == E.ERR_ARG
    assert call(num=0) == E.ERR_ARG                     # d_out_num is required
    assert call(ok_=0, ov=0) == E.ERR_ARG               # one of keys and values is required
    assert call(ok_=0) == E.OK and call(ov=0) == E.OK and call(off=0) == E.OK
    ctx.check()
    assert call(keys=0) == E.ERR_ARG and call(vals=0) == E.ERR_ARG  # null inputs with n > 0
    assert call(keys=k + 2) == E.ERR_ARG                # misaligned, each pointer in turn
    assert call(vals=p + 4) == E.ERR_ARG
    assert call(ok_=p + 4096 + 2) == E.ERR_ARG
    assert call(ov=p + 2 * 4096 + 4) == E.ERR_ARG
    assert call(off=p + 3 * 4096 + 4) == E.ERR_ARG
    assert call(num=p + 4 * 4096 + 4) == E.ERR_ARG
    assert call(vals=p + 4, ov=p + 2 * 4096 + 4, vb=4) == E.OK and call(keys=k + 4, ok_=p + 4096 + 4) == E.OK  # naturally aligned is enough
    ctx.check()
    assert call(n=2 ** 32) == E.ERR_UNSUPPORTED         # dummy pointers, nothing launched
    assert L.rsx_ctx_reserve_reduce(h, 2 ** 32, 4, 4) == E.ERR_UNSUPPORTED
    assert L.rsx_ctx_reserve_reduce(h, 100, 3, 4) == E.ERR_ARG and L.rsx_ctx_reserve_reduce(h, 100, 4, 2) == E.ERR_ARG
    torch.cuda.synchronize()
    case.run(values_of("i64", 200, rng, None), "i64", MAX, True)  # the context works on


def test_values_at_natural_alignment(rs, torch, ctx):
    """Columns that are 4- or 8-byte but not 16-byte aligned take the element-by-element join: the same bytes."""
    T = rs.reduce_caps(4, 8)[0]
    n = 2 * T + 5
    rng = np.random.default_rng(12)
    kraw = keys_of("u32", group_ids("third", n, T, rng))
    v = values_of("f64", n, rng, "a")
    kb_, vb_ = torch.zeros(n + 8, dtype=torch.int32, device="cuda"), torch.zeros(n + 8, dtype=torch.float64, device="cuda")
    keys, vals = kb_[1:1 + n], vb_[1:1 + n]
    assert keys.data_ptr() % 16 == 4 and vals.data_ptr() % 16 == 8
    keys.view(torch.uint8).copy_(torch.from_numpy(kraw.copy()))
    vals.copy_(torch.from_numpy(v.copy()))
    r = rs.radix_reduce_by_key(keys.view(torch.uint32), vals, op="max", ctx=ctx)
    ctx.check()
    ref = reduce_reference(kraw, 4, UNSIGNED, v.view(np.uint8), 8, FLOAT, MAX, False)
    m = int(r.num)
    assert m == ref.m and np.array_equal(r.keys[:m].view(torch.uint8).cpu().numpy().reshape(-1), ref.keys)
    assert np.array_equal(r.values[:m].view(torch.uint8).cpu().numpy().reshape(-1), ref.values)


# ---- the Python call against torch ----
def test_python_sum_equals_index_add(rs, torch, ctx):
    rng = np.random.default_rng(13)
    for n, span in ((1, 5), (1000, 7), (40013, 3000)):
        keys = torch.from_numpy(rng.integers(-span, span, size=n, dtype=np.int64)).cuda()
        vals = torch.from_numpy(values_of("f32", n, rng, "a")).cuda()
        uniq, inverse = torch.unique(keys, sorted=True, return_inverse=True)
        want = torch.zeros(uniq.numel(), dtype=torch.float32, device="cuda").index_add_(0, inverse, vals)  # (exact sums: any order)
        for desc in (False, True):
            r = rs.radix_reduce_by_key(keys, vals, descending=desc, offsets=True, ctx=ctx)
            ctx.check()
            assert isinstance(r, rs.Reduced) and r.num.dim() == 0 and r.num.dtype == torch.int64
            m = int(r.num)
            assert m == uniq.numel() and r.keys.shape == keys.shape and r.values.shape == vals.shape and r.offsets.shape == (n + 1,)
            assert r.values.dtype == torch.float32 and r.offsets.dtype == torch.int64
            assert torch.equal(r.keys[:m], uniq.flip(0) if desc else uniq)
            assert torch.equal(r.values[:m], want.flip(0) if desc else want)  # (as numbers: a zero sum equals a zero of either sign)
            counts = torch.bincount(inverse, minlength=m)
            assert torch.equal(r.offsets[1:m + 1] - r.offsets[:m], counts.flip(0) if desc else counts)
        assert rs.radix_reduce_by_key(keys, vals, ctx=ctx).offsets is None


def test_python_min_and_max_equal_scatter_reduce(rs, torch, ctx):
    rng = np.random.default_rng(14)
    n = 30011
    keys = torch.from_numpy(rng.integers(0, 977, size=n).astype(np.int16)).cuda()
    vals = torch.from_numpy(values_of("i32", n, rng, None)).cuda()
    uniq, inverse = torch.unique(keys, sorted=True, return_inverse=True)
    for op, torch_op in (("min", "amin"), ("max", "amax")):
        want = torch.zeros(uniq.numel(), dtype=torch.int32, device="cuda").scatter_reduce(0, inverse, vals, torch_op, include_self=False)
        r = rs.radix_reduce_by_key(keys, vals, op=op, ctx=ctx)
        ctx.check()
        m = int(r.num)
        assert m == uniq.numel() and torch.equal(r.keys[:m], uniq) and torch.equal(r.values[:m], want)


def test_python_unsigned_values_and_128_bit_keys(rs, torch, ctx):
    rng = np.random.default_rng(15)
    n = 5000
    raw = util.make_input("i128", n, "two", seed=4)
    keys = torch.from_numpy(raw.copy()).cuda().view(n, 16)
    v = values_of("u64", n, rng, None)
    vals = torch.from_numpy(v.view("<i8").copy()).cuda().view(torch.uint64)
    r = rs.radix_reduce_by_key(keys, vals, op="max", descending=True, ctx=ctx, key_kind=rs.KEY_SIGNED)
    ctx.check()
    ref = reduce_reference(raw, 16, SIGNED, v.view(np.uint8), 8, UNSIGNED, MAX, True)
    m = int(r.num)
    assert m == ref.m == 2 and r.keys.shape == (n, 16) and r.values.dtype == torch.uint64
    assert np.array_equal(r.keys[:m].cpu().numpy().reshape(-1), ref.keys)
    assert np.array_equal(r.values[:m].view(torch.uint8).cpu().numpy().reshape(-1), ref.values)
    assert np.array_equal(keys.cpu().numpy().reshape(-1), raw)
