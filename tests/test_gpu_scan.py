"""GPU: rsx_scan_by_key_device / radix_scan_by_key against tests/scan_ref.py.

Every array sits in an allocation the test owns: 64 guard bytes of 0xA5, the array (outputs filled with 0xA5), 64 guard
bytes.  What comes back is compared whole, and both input columns are compared with what was put in after every call.
Sizes, shapes, values and the thinned matrix are those of tests/scan_cases.py (its docstring has the rules; test_scan_ref.py
asserts on the CPU what the thinning rule still covers and that the float inputs meet the 1-in-20 condition).

Float sums: form (a) as bytes, but for the entries the reference marks `free` (an exact prefix of zero whose values are not
all -0.0), which are compared as numbers; form (b) inside |result - longdouble prefix| <= g(c-1) * sum|v|, c the 1-based
rank; in both forms every output is finite where the inputs are.  Everything else is compared as bytes.  Exclusive calls
store FIRST, 0x5A repeated, at the heads: no operator's identity, so a `first` that was combined shows."""
import numpy as np
import pytest

import util
from reduce_ref import FLOAT, MAX, MIN, SIGNED, SUM, UNSIGNED, value_dtype
from scan_cases import COMBINATIONS, FIRST, OP_NAMES, OPS, VALUE_TYPES, combination_id, ids_for, matrix_inputs, values_of
from scan_ref import scan_reference
from segment_pairs_gpu import guarded, joined_elem, same
from segment_pairs_ref import with_guards
from test_gpu_unique import F32_SPECIALS, F64_SPECIALS, canary, keys_of
from unique_ref import unique_reference

pytestmark = pytest.mark.gpu

PATH = 14 << 24
RUNS_BIT = 0x100


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


def flags_of(rs, exclusive, runs):
    return (rs.SCAN_EXCLUSIVE if exclusive else 0) | (rs.SCAN_RUNS if runs else 0)


# ---- one call on guarded buffers ----
class Case:
    """One key column on the GPU (guarded) with its groups, and scan_by_key_device calls on it."""

    def __init__(self, torch, rs, c, tname, keys_raw, shift=0):
        self.torch, self.rs, self.c, self.tname = torch, rs, c, tname
        self.kb, self.kind = util.TYPES[tname][2], util.TYPES[tname][3]
        self.keys_raw = keys_raw
        self.n = keys_raw.size // self.kb
        self.shift = shift
        self.kbuf, self.kmid = guarded(torch, keys_raw, shift)
        self.groups = None

    def reference(self, vals, vname, op, exclusive, runs, first=FIRST):
        if not runs and self.groups is None:
            self.groups = unique_reference(self.keys_raw, self.kb, self.kind, False)
        vb, vkind = VALUE_TYPES[vname]
        return scan_reference(self.keys_raw, self.kb, self.kind, None if vals is None else vals.view(np.uint8), vb, vkind, op, exclusive, first, runs,
                              groups=self.groups)

    def call(self, vals, vname, op, exclusive, runs, first=FIRST, num=True, c=None, shifts=(0, 0)):
        """vals None: the count form (d_values 0).  -> the whole allocations (numpy bytes) of out, num and the value column"""
        torch, n, kb = self.torch, self.n, self.kb
        c = c or self.c
        vb, vkind = VALUE_TYPES[vname]
        vbuf = guarded(torch, vals.view(np.uint8), shifts[0])[0] if vals is not None else None
        obuf = guarded(torch, canary(n * vb), shifts[1])[0]
        nbuf, nmid = guarded(torch, canary(8)) if num else (None, None)
        # (an empty view has no address of its own: every pointer is taken from its allocation)
        c.scan_by_key_device(self.kbuf.data_ptr() + 64 + self.shift, vbuf.data_ptr() + 64 + shifts[0] if vals is not None else 0, n, kb, self.kind, vb,
                             vkind, op, flags_of(self.rs, exclusive, runs), first, obuf.data_ptr() + 64 + shifts[1], nmid.data_ptr() if num else 0,
                             torch.cuda.current_stream().cuda_stream)
        c.check()
        return {"out": obuf.cpu().numpy(), "num": nbuf.cpu().numpy() if num else None, "in_values": vbuf.cpu().numpy() if vbuf is not None else None}

    def run(self, vals, vname, op, exclusive, runs, form=None, what=None, **kw):
        n = self.n
        vb, vkind = VALUE_TYPES[vname]
        shifts = kw.get("shifts", (0, 0))
        got = self.call(vals, vname, op, exclusive, runs, **kw)
        ref = self.reference(vals, vname, op, exclusive, runs, kw.get("first", FIRST))
        tag = (self.tname, vname, OP_NAMES[op], n, what, form, "excl" if exclusive else "incl", "runs" if runs else "grouped")
        if got["num"] is not None:
            assert same(got["num"], with_guards(np.array([ref.num], dtype="<u8")), ("num",) + tag)
        if vals is not None:
            assert same(got["in_values"], with_guards(vals.view(np.uint8), shifts[0]), ("the value column",) + tag)
        assert same(self.kbuf.cpu().numpy(), with_guards(self.keys_raw, self.shift), ("the key column",) + tag)
        if ref.values is not None:  # integers, float MIN and MAX: bytes
            assert same(got["out"], with_guards(ref.values, shifts[1]), ("out",) + tag)
            return ref
        dt = value_dtype(vb, vkind)
        lo = 64 + shifts[1]
        mine = got["out"][lo:lo + n * vb].copy()
        assert np.all(np.isfinite(mine.view(dt))) or not np.all(np.isfinite(vals)), ("an output is not finite",) + tag
        if form == "a":  # exact prefixes: bytes, but for the entries whose zero has no fixed sign
            free = ref.free
            print(tag, "entries", n, "with a zero of free sign", int(free.sum()))
            assert int(free.sum()) * 20 <= n, ("more than 1 in 20 entries have a zero of free sign", int(free.sum()), n) + tag
            assert np.all(mine.view(dt)[free] == 0), ("a zero prefix is not zero",) + tag
            want = ref.exact.view(dt).copy()
            want[free] = mine.view(dt)[free]
            assert same(got["out"], with_guards(want.view(np.uint8), shifts[1]), ("out",) + tag)
        else:  # the order-free bound against the longdouble prefixes; the heads of an exclusive call as bytes
            err = np.abs(mine.view(dt).astype(np.longdouble) - ref.sums)
            worst = int(np.argmax(err - ref.bound)) if n else 0
            print(tag, "largest error / bound", float(np.max(err / np.maximum(ref.bound, np.finfo(np.longdouble).tiny))) if n else 0.0)
            assert np.all(err <= ref.bound), ("outside g(c-1) * sum|v|", worst, float(err[worst]), float(ref.bound[worst])) + tag
            if exclusive:
                u = "<u" + str(vb)
                assert np.array_equal(mine.view(u)[ref.heads], ref.exact.view(u)[ref.heads]), ("first at the heads",) + tag
            assert same(got["out"], with_guards(mine, shifts[1]), ("the guards of out",) + tag)
        return ref


# ---- the matrix ----
@pytest.mark.parametrize("tname,vname,op,exclusive,runs,c", COMBINATIONS, ids=[combination_id(*cmb) for cmb in COMBINATIONS])
def test_matrix(rs, torch, ctx, tname, vname, op, exclusive, runs, c):
    kb = util.TYPES[tname][2]
    for n, shape, _T, keys_raw, vals in matrix_inputs(rs, tname, vname, op, runs, c):
        case = Case(torch, rs, ctx, tname, keys_raw)
        for form, v in vals.items():
            ref = case.run(v, vname, op, exclusive, runs, form=form, what=shape)
            if shape == "equal":
                assert ref.num == 1
            assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 3 | (RUNS_BIT if runs else 0)
            if not runs:
                assert ctx.get_info(rs.INFO_LAST_PAIRS) == 1 | joined_elem(kb, 4) << 8


@pytest.mark.parametrize("runs", [False, True], ids=["grouped", "runs"])
@pytest.mark.parametrize("vname", ["f32", "f64"])
@pytest.mark.parametrize("shape", ["equal", "long_run", "runs_of_tile", "runs_shifted"])
def test_the_carry_shapes_at_the_second_sweep(rs, torch, ctx, shape, vname, runs):
    """One run through every tile and across the sweep boundary, whole tiles without a head, runs that end on the last slot
    of a tile (the carry must not leak past the head into the next run) and one slot further, and the exclusive value of a
    tile's first slot (the carry itself): float sums in both forms, u32 keys."""
    vb = VALUE_TYPES[vname][0]
    T, S = rs.scan_by_key_caps(4, vb, runs)
    n = S * T + T + 3
    rng = np.random.default_rng(S + vb + (1 if runs else 0))
    case = Case(torch, rs, ctx, "u32", keys_of("u32", ids_for(shape, n, T, rng, runs)))
    for form in ("a", "b"):
        v = values_of(vname, n, rng, form)
        for exclusive in (False, True):
            case.run(v, vname, SUM, exclusive, runs, form=form, what=shape)


# ---- float specials ----
@pytest.mark.parametrize("runs", [False, True], ids=["grouped", "runs"])
@pytest.mark.parametrize("vname", ["f32", "f64"])
def test_running_sums_through_infinities_and_nans(rs, torch, ctx, vname, runs):
    """A prefix that has met +inf is +inf, one that has met a NaN, or +inf and -inf, is a NaN, and the prefixes in front
    of them are the finite ones (form (a): exact)."""
    vb, _vk = VALUE_TYPES[vname]
    dt = value_dtype(vb, FLOAT)
    T = rs.scan_by_key_caps(4, vb, runs)[0]
    rng = np.random.default_rng(3)
    for n in (64, 2 * T + 9):
        g = np.sort(rng.integers(0, 4, size=n, dtype=np.int64)) if runs else rng.integers(0, 4, size=n, dtype=np.int64)
        vals = values_of(vname, n, rng, "a")
        for grp, specials in ((1, [np.inf]), (2, [np.nan]), (3, [np.inf, -np.inf])):  # group 0 stays finite
            where = np.nonzero(g == grp)[0]
            assert where.size > len(specials)
            vals[rng.choice(where, size=len(specials), replace=False)] = specials
        case = Case(torch, rs, ctx, "u32", keys_of("u32", g))
        for exclusive in (False, True):
            got = case.call(vals, vname, SUM, exclusive, runs, first=0)
            ref = case.reference(vals, vname, SUM, exclusive, runs, first=0)
            assert int(got["num"][64:72].view("<u8")[0]) == ref.num == 4
            mine, want = got["out"][64:64 + n * vb].view(dt), ref.exact.view(dt)
            assert np.array_equal(np.isnan(mine), np.isnan(want)), (vname, n, exclusive)
            ok = ~np.isnan(want)
            assert np.array_equal(mine[ok], want[ok]), (vname, n, exclusive)  # (as numbers: infinities included)
            assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want[g == 0]).all()


@pytest.mark.parametrize("vname", ["f32", "f64"])
def test_running_min_and_max_of_the_special_patterns(rs, torch, ctx, vname):
    vb, _vk = VALUE_TYPES[vname]
    sp = F32_SPECIALS if vb == 4 else F64_SPECIALS
    rng = np.random.default_rng(4)
    for runs in (False, True):
        T = rs.scan_by_key_caps(8, vb, runs)[0]
        for n in (7, 64, 3 * T + 5):
            vals = sp[rng.integers(0, 7, size=n)].view(value_dtype(vb, FLOAT))
            ordinary = rng.random(n) < 0.3
            vals[ordinary] = values_of(vname, int(ordinary.sum()), rng, "b")
            for shape in ("seven", "third", "equal"):
                case = Case(torch, rs, ctx, "i64", keys_of("i64", ids_for(shape, n, T, rng, runs)))
                for op in (MIN, MAX):
                    for exclusive in (False, True):
                        case.run(vals, vname, op, exclusive, runs, what=("specials", shape))
    one = Case(torch, rs, ctx, "u8", np.zeros(7, dtype=np.uint8))  # all seven in one group, in their order
    in_order = sp.copy().view(value_dtype(vb, FLOAT))
    low = one.run(in_order, vname, MIN, False, True).values.view(sp.dtype)
    high = one.run(in_order, vname, MAX, False, False).values.view(sp.dtype)
    assert np.all(low == sp[0]) and np.array_equal(high, sp)  # -NaN is the minimum from the start; the maximum climbs


# ---- the count form ----
@pytest.mark.parametrize("vname", ["i32", "u32", "i64", "u64"])
def test_the_count_form_ranks_every_group(rs, torch, ctx, vname):
    vb = VALUE_TYPES[vname][0]
    dt = value_dtype(*VALUE_TYPES[vname])
    rng = np.random.default_rng(16)
    for runs in (False, True):
        T, S = rs.scan_by_key_caps(2, vb, runs)
        for n, shape in ((1, "equal"), (T + 1, "seven"), (3 * T + 5, "third"), (3 * T + 5, "long_run"), (S * T + T + 3, "equal")):
            case = Case(torch, rs, ctx, "i16", keys_of("i16", ids_for(shape, n, T, rng, runs)))
            for exclusive in (False, True):
                ref = case.run(None, vname, SUM, exclusive, runs, first=0, what=("count form", shape))  # (d_values is 0: never dereferenced)
                assert np.array_equal(ref.values.view(dt), (ref.rank + (0 if exclusive else 1)).astype(dt))  # arange inside every group
                assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 3 | (RUNS_BIT if runs else 0)
        case.run(None, vname, SUM, True, runs, first=FIRST, what="count form, first stored as it is")


def test_num_is_optional(rs, torch, ctx):
    rng = np.random.default_rng(17)
    for runs in (False, True):
        T = rs.scan_by_key_caps(4, 4, runs)[0]
        n = 2 * T + 1
        case = Case(torch, rs, ctx, "f32", keys_of("f32", ids_for("third", n, T, rng, runs)))
        v = values_of("i32", n, rng, None)
        with_num = case.run(v, "i32", MAX, False, runs)
        case.run(v, "i32", MAX, False, runs, num=False)
        if runs:  # "third" as it lies: far more runs than distinct keys
            assert with_num.num > unique_reference(case.keys_raw, 4, util.FLOAT, False)[4]


# ---- in place, the same bytes on every call ----
@pytest.mark.parametrize("runs", [False, True], ids=["grouped", "runs"])
@pytest.mark.parametrize("tname,vname,op", [("u32", "f32", SUM), ("i64", "i64", SUM), ("u8", "f64", MAX), ("u128", "u32", MIN), ("i16", "i32", SUM)])
def test_out_may_be_the_values(rs, torch, ctx, tname, vname, op, runs):
    kb, kind = util.TYPES[tname][2], util.TYPES[tname][3]
    vb, vkind = VALUE_TYPES[vname]
    T = rs.scan_by_key_caps(kb, vb, runs)[0]
    rng = np.random.default_rng(6)
    for n in (1, T + 1, 3 * T + 5):
        keys_raw = keys_of(tname, ids_for("third", n, T, rng, runs))
        vals = values_of(vname, n, rng, "b")
        for exclusive in (False, True):
            apart = Case(torch, rs, ctx, tname, keys_raw).call(vals, vname, op, exclusive, runs)
            kbuf, kmid = guarded(torch, keys_raw)
            vbuf, vmid = guarded(torch, vals.view(np.uint8))
            ctx.scan_by_key_device(kmid.data_ptr(), vmid.data_ptr(), n, kb, kind, vb, vkind, op, flags_of(rs, exclusive, runs), FIRST, vmid.data_ptr(), 0,
                                   torch.cuda.current_stream().cuda_stream)
            ctx.check()
            assert same(vbuf.cpu().numpy(), apart["out"], ("values in place", tname, vname, n, exclusive, runs))
            assert same(kbuf.cpu().numpy(), with_guards(keys_raw), ("the key column", tname, vname, n, exclusive, runs))


@pytest.mark.parametrize("vname", ["f32", "f64"])
def test_float_sums_are_the_same_bytes_on_every_call(rs, torch, ctx, vname):
    vb = VALUE_TYPES[vname][0]
    fresh = rs.Context(torch.cuda.current_device())
    rng = np.random.default_rng(5)
    for runs in (False, True):
        T, S = rs.scan_by_key_caps(4, vb, runs)
        for n in (3 * T + 5, S * T + T + 3):
            for shape in ("seven", "long_run", "third"):
                case = Case(torch, rs, ctx, "u32", keys_of("u32", ids_for(shape, n, T, rng, runs)))
                vals = values_of(vname, n, rng, "b")
                first = case.call(vals, vname, SUM, False, runs)
                again = case.call(vals, vname, SUM, False, runs)
                other = case.call(vals, vname, SUM, False, runs, c=fresh)
                for name in ("num", "out"):
                    assert np.array_equal(first[name], again[name]), (name, n, shape, runs, "second call")
                    assert np.array_equal(first[name], other[name]), (name, n, shape, runs, "fresh context")
    fresh.close()


# ---- agreement with the other calls ----
@pytest.mark.parametrize("tname,vname,op", [("u32", "i32", SUM), ("i64", "u64", SUM), ("f32", "i64", MIN), ("u8", "f32", MAX), ("u128", "f64", MIN),
                                            ("i16", "u32", MAX)])
def test_the_last_of_every_group_is_the_reduced_value(rs, torch, ctx, tname, vname, op):
    kb, kind = util.TYPES[tname][2], util.TYPES[tname][3]
    vb, vkind = VALUE_TYPES[vname]
    T = rs.scan_by_key_caps(kb, vb, False)[0]
    rng = np.random.default_rng(7)
    for n, shape in ((T + 1, "third"), (3 * T + 5, "seven")):
        keys_raw = keys_of(tname, ids_for(shape, n, T, rng, False))
        vals = values_of(vname, n, rng, "a")
        got = Case(torch, rs, ctx, tname, keys_raw).call(vals, vname, op, False, False)
        kbuf, kmid = guarded(torch, keys_raw)
        vbuf, vmid = guarded(torch, vals.view(np.uint8))
        outs = [guarded(torch, canary(nb)) for nb in (n * vb, (n + 1) * 8, 8)]
        ctx.reduce_by_key_device(kmid.data_ptr(), vmid.data_ptr(), n, kb, kind, vb, vkind, op, 0, outs[0][1].data_ptr(), outs[1][1].data_ptr(),
                                 outs[2][1].data_ptr(), False, torch.cuda.current_stream().cuda_stream)
        ctx.check()
        m = int(outs[2][1].cpu().numpy().view("<u8")[0])
        assert m == int(got["num"][64:72].view("<u8")[0])
        offsets = outs[1][1].cpu().numpy().view("<u8")[:m + 1].astype(np.int64)
        perm = unique_reference(keys_raw, kb, kind, False)[2]
        last = perm[offsets[1:] - 1]  # the last input position of every group
        u = "<u" + str(vb)
        assert np.array_equal(got["out"][64:64 + n * vb].view(u)[last], outs[0][1].cpu().numpy().view(u)[:m]), (tname, vname, n, shape)


@pytest.mark.parametrize("tname,vname", [("u32", "i32"), ("i64", "u64"), ("u8", "i64")])
def test_runs_of_the_sorted_keys_are_the_groups(rs, torch, ctx, tname, vname):
    """A runs call on the keys sorted by radix_sort_pairs (with their values) gives the grouped call's results gathered
    through radix_argsort."""
    from segment_pairs_gpu import key_dtype
    vb, vkind = VALUE_TYPES[vname]
    rng = np.random.default_rng(18)
    n = 40013
    keys_raw = keys_of(tname, ids_for("third", n, 1024, rng, False))
    v = values_of(vname, n, rng, None)
    keys = torch.from_numpy(keys_raw.copy()).cuda().view(key_dtype(torch, tname))
    vals = torch.from_numpy(v.view("<i" + str(vb)).copy()).cuda()
    for op in ("sum", "min", "max"):
        if vkind == UNSIGNED and op != "sum":
            continue  # (the tensors here are signed views of the unsigned bytes: sums agree, orders do not)
        for exclusive in (False, True):
            grouped = rs.radix_scan_by_key(keys, vals, op=op, exclusive=exclusive, first=7, ctx=ctx)
            perm = rs.radix_argsort(keys, ctx=ctx)
            sk, sv = keys.clone(), vals.clone()
            rs.radix_sort_pairs(sk, sv, ctx=ctx)
            lying = rs.radix_scan_by_key(sk, sv, op=op, exclusive=exclusive, first=7, runs=True, ctx=ctx)
            ctx.check()
            assert torch.equal(lying, grouped[perm]), (tname, vname, op, exclusive)


# ---- alignment ----
@pytest.mark.parametrize("runs", [False, True], ids=["grouped", "runs"])
def test_columns_at_natural_alignment_give_the_same_bytes(rs, torch, ctx, runs):
    rng = np.random.default_rng(12)
    for tname, vname, op in (("u32", "f64", SUM), ("i64", "f32", SUM), ("u8", "i64", MAX), ("i16", "u32", MIN)):
        kb = util.TYPES[tname][2]
        vb = VALUE_TYPES[vname][0]
        T = rs.scan_by_key_caps(kb, vb, runs)[0]
        n = 2 * T + 5
        keys_raw = keys_of(tname, ids_for("third", n, T, rng, runs))
        vals = values_of(vname, n, rng, "b")
        for exclusive in (False, True):
            at16 = Case(torch, rs, ctx, tname, keys_raw).call(vals, vname, op, exclusive, runs)
            for ks, vs, os_ in ((max(kb, 4) % 16, 0, 0), (0, 4 if vb == 4 else 8, 0), (0, 0, 4 if vb == 4 else 8), (8, 8, 8), (4 if kb <= 4 else 8, vb, vb)):
                case = Case(torch, rs, ctx, tname, keys_raw, shift=ks)
                assert (case.kmid.data_ptr() % 16) == ks
                got = case.call(vals, vname, op, exclusive, runs, shifts=(vs, os_))
                lo = 64 + os_
                assert same(got["out"][lo:lo + n * vb], at16["out"][64:64 + n * vb], ("out", tname, vname, ks, vs, os_, exclusive))
                assert same(got["out"], with_guards(got["out"][lo:lo + n * vb], os_), ("the guards of out", tname, vname, ks, vs, os_))
                assert same(got["in_values"], with_guards(vals.view(np.uint8), vs), ("the value column",))
                assert same(case.kbuf.cpu().numpy(), with_guards(keys_raw, ks), ("the key column",))


# ---- n = 0 and n = 1, what the context reports ----
def test_empty_and_single(rs, torch, ctx):
    empty = Case(torch, rs, ctx, "u32", np.zeros(0, dtype=np.uint8))
    for runs in (False, True):
        for vname in ("f32", "i64"):
            ref = empty.run(np.zeros(0, dtype=value_dtype(*VALUE_TYPES[vname])), vname, SUM, True, runs)  # num == 0, nothing else
            assert ref.num == 0
            assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | (RUNS_BIT if runs else 0)
            empty.run(None, vname if vname != "f32" else "u32", SUM, False, runs, num=False)
        out, num = rs.radix_scan_by_key(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.float64, device="cuda"), runs=runs,
                                        return_num=True, ctx=ctx)
        assert int(num) == 0 and out.numel() == 0 and out.dtype == torch.float64
    rng = np.random.default_rng(9)
    for tname, vname in (("u8", "f64"), ("f32", "i32"), ("u128", "u64")):
        one = Case(torch, rs, ctx, tname, util.make_input(tname, 1, "uniform", seed=1))
        for op in OPS:
            for exclusive in (False, True):
                for runs in (False, True):
                    ref = one.run(values_of(vname, 1, rng, "a"), vname, op, exclusive, runs, form="a", what="n = 1")
                    assert ref.num == 1
    z = np.array([-0.0, -0.0], dtype="<f4")
    ref = Case(torch, rs, ctx, "u32", np.zeros(8, dtype=np.uint8)).run(z, "f32", SUM, False, True, form="a", what="-0.0 and -0.0")
    assert list(ref.exact.view("<u4")) == [0x80000000, 0x80000000]  # no +0.0 identity was added


def test_what_the_context_reports(rs, torch, ctx):
    rng = np.random.default_rng(19)
    n = 5000
    keys_raw = keys_of("i64", ids_for("third", n, 1024, rng, False))
    case = Case(torch, rs, ctx, "i64", keys_raw)
    v = values_of("f32", n, rng, "a")
    case.call(v, "f32", SUM, False, False)
    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 3
    assert ctx.get_info(rs.INFO_LAST_PAIRS) == 1 | joined_elem(8, 4) << 8 == 1 | 16 << 8
    x = torch.randint(0, 100, (1000,), dtype=torch.int32, device="cuda")
    rs.radix_sort_pairs(x, x.clone().to(torch.int64), ctx=ctx)  # another joined element: 12 bytes
    pairs = ctx.get_info(rs.INFO_LAST_PAIRS)
    assert pairs == 1 | joined_elem(4, 8) << 8
    case.call(v, "f32", SUM, True, True)
    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 3 | RUNS_BIT
    assert ctx.get_info(rs.INFO_LAST_PAIRS) == pairs  # untouched: nothing was joined
    case.call(None, "u32", SUM, True, False, first=0)
    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 3
    assert ctx.get_info(rs.INFO_LAST_PAIRS) == 1 | 16 << 8
    assert rs._lib.load().rsx_version() == ctx._L.rsx_version()


# ---- stream capture ----
@pytest.mark.parametrize("runs", [False, True], ids=["grouped", "runs"])
def test_capture_and_replay(rs, torch, runs):
    c = rs.Context(torch.cuda.current_device())
    n = 300001
    c.reserve_scan_by_key(n, 4, 4, runs)
    rng = np.random.default_rng(10)
    inputs = []
    for i, dist in enumerate(("step16", "highbyte")):
        kraw = util.make_input("u32", n, dist, seed=80 + i)
        if runs:
            kraw = np.sort(kraw.view("<u4") >> np.uint32(12 * i)).view(np.uint8)  # long runs, then shorter ones
        inputs.append((kraw, values_of("f32", n, rng, "a")))
    ksrc = torch.from_numpy(inputs[0][0].copy()).cuda().view(torch.uint32)
    vsrc = torch.from_numpy(inputs[0][1].copy()).cuda()
    keys, vals = torch.empty_like(ksrc), torch.empty_like(vsrc)
    out = torch.empty_like(vsrc)
    num = torch.empty((), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    first = int(np.array([-3.5], dtype="<f4").view("<u4")[0])

    def enqueue():
        c.scan_by_key_device(keys.data_ptr(), vals.data_ptr(), n, 4, rs.KEY_UNSIGNED, 4, rs.KEY_FLOAT, SUM, flags_of(rs, True, runs), first,
                             out.data_ptr(), num.data_ptr(), torch.cuda.current_stream().cuda_stream)

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
        out.fill_(-77.0)
        num.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        ref = scan_reference(kraw, 4, UNSIGNED, v.view(np.uint8), 4, FLOAT, SUM, True, first, runs)
        assert int(num) == ref.num
        mine, want = out.cpu().numpy(), ref.exact.view("<f4")
        assert np.array_equal(mine[~ref.free], want[~ref.free]) and np.all(mine[ref.free] == 0)
        assert np.array_equal(mine[ref.heads].view("<u4"), np.full(ref.num, first, dtype="<u4"))
    c.close()


@pytest.mark.parametrize("runs", [False, True], ids=["grouped", "runs"])
def test_unreserved_call_under_capture_reports_workspace(rs, torch, runs):
    c = rs.Context(torch.cuda.current_device())
    x = torch.randint(0, 2 ** 31 - 1, (1000,), dtype=torch.int32, device="cuda")
    rs.radix_scan_by_key(x, x.clone(), runs=runs, ctx=c)  # one ordinary call: the context's error word and self-tests exist
    c.check()
    n = 1 << 20  # more than the context has seen
    keys = torch.randint(0, 1000, (n,), dtype=torch.int32, device="cuda")
    vals = torch.randint(0, 1000, (n,), dtype=torch.int64, device="cuda")
    before = (keys.clone(), vals.clone())
    out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    num = torch.full((), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g.capture_begin()
        try:
            c.scan_by_key_device(keys.data_ptr(), vals.data_ptr(), n, 4, rs.KEY_SIGNED, 8, rs.KEY_SIGNED, SUM, flags_of(rs, False, runs), 0,
                                 out.data_ptr(), num.data_ptr(), torch.cuda.current_stream().cuda_stream)
        except rs.RsxError as e:
            err = e
        g.capture_end()
    assert err is not None and err.status == rs._lib.ERR_WORKSPACE, err
    torch.cuda.synchronize()
    assert torch.equal(keys, before[0]) and torch.equal(vals, before[1]) and int(num) == -1 and bool((out == -1).all())  # nothing was enqueued
    c.close()


# ---- errors ----
def test_errors(rs, torch, ctx):
    E = rs._lib
    rng = np.random.default_rng(11)
    case = Case(torch, rs, ctx, "u32", util.make_input("u32", 200, "two", seed=2))
    L, h = ctx._L, ctx._h
    buf = torch.full((3 * 4096,), 0xA5, dtype=torch.uint8, device="cuda")  # a region of 4 KiB per array
    p = buf.data_ptr()
    k = case.kmid.data_ptr()
    assert p % 16 == 0 and k % 16 == 0
    ok = dict(keys=k, vals=p, n=200, kb=4, kind=0, vb=8, vkind=1, op=0, flags=0, first=0, out=p + 4096, num=p + 2 * 4096)

    def call(**kw):
        a = dict(ok, **kw)
        return L.rsx_scan_by_key_device(h, a["keys"] or None, a["vals"] or None, a["n"], a["kb"], a["kind"], a["vb"], a["vkind"], a["op"], a["flags"],
                                        a["first"], a["out"] or None, a["num"] or None, None)

    for flags in (0, 1, 2, 3):
        assert call(flags=flags) == E.OK
    ctx.check()
    assert call(kb=3) == E.ERR_ARG                      # key width
    assert call(kb=16, kind=2) == E.ERR_ARG             # float keys of 16 bytes
    for vb in (0, 1, 2, 3, 12, 16):
        assert call(vb=vb) == E.ERR_ARG                 # value width
    assert call(vkind=3) == E.ERR_ARG
    assert call(op=3) == E.ERR_ARG and call(op=-1) == E.ERR_ARG
    assert call(flags=4) == E.ERR_ARG and call(flags=0x80000001) == E.ERR_ARG  # unknown flag bits
    assert call(out=0) == E.ERR_ARG                     # d_out is required
    assert call(keys=0) == E.ERR_ARG                    # null keys with n > 0
    assert call(num=0) == E.OK                          # d_out_num is optional
    assert call(vals=0) == E.OK and call(vals=0, flags=3, vkind=0, vb=4) == E.OK  # the count form
    assert call(vals=0, op=1) == E.ERR_ARG and call(vals=0, op=2) == E.ERR_ARG    # ... takes SUM
    assert call(vals=0, vkind=2) == E.ERR_ARG                                     # ... and an integer kind
    ctx.check()
    assert call(out=k, vb=4) == E.ERR_ARG and call(out=k + 400, vb=4) == E.ERR_ARG  # d_out on the keys
    assert call(num=k + 8) == E.ERR_ARG and call(num=p + 4096 + 8) == E.ERR_ARG     # d_out_num in the keys, in d_out
    assert call(out=p) == E.OK                          # d_out may be d_values
    assert call(keys=k + 2) == E.ERR_ARG                # misaligned, each pointer in turn
    assert call(vals=p + 4) == E.ERR_ARG
    assert call(out=p + 4096 + 4) == E.ERR_ARG
    assert call(num=p + 2 * 4096 + 4) == E.ERR_ARG
    for flags in (0, 2):
        assert call(vals=p + 4, out=p + 4096 + 4, vb=4, flags=flags) == E.OK and call(keys=k + 4, n=199, flags=flags) == E.OK  # naturally aligned is enough
    ctx.check()
    assert call(n=2 ** 32) == E.ERR_UNSUPPORTED         # dummy pointers, nothing launched
    assert L.rsx_ctx_reserve_scan_by_key(h, 2 ** 32, 4, 4, 0) == E.ERR_UNSUPPORTED
    assert L.rsx_ctx_reserve_scan_by_key(h, 100, 3, 4, 0) == E.ERR_ARG and L.rsx_ctx_reserve_scan_by_key(h, 100, 4, 2, 2) == E.ERR_ARG
    assert L.rsx_ctx_reserve_scan_by_key(h, 100, 4, 4, 8) == E.ERR_ARG
    torch.cuda.synchronize()
    for runs in (False, True):
        case.run(values_of("i64", 200, rng, None), "i64", MAX, True, runs)  # the context works on


# ---- the Python call against torch ----
def test_python_runs_of_one_key_equal_cumsum(rs, torch, ctx):
    rng = np.random.default_rng(13)
    for n in (1, 1000, 40013):
        for dtype in (torch.int32, torch.int64):
            keys = torch.full((n,), 42, dtype=torch.int16, device="cuda")
            v = torch.from_numpy(rng.integers(-1000, 1000, size=n)).to(dtype).cuda()
            got = rs.radix_scan_by_key(keys, v, runs=True, ctx=ctx)
            ctx.check()
            assert got.dtype == dtype and got.shape == v.shape and torch.equal(got, torch.cumsum(v, 0).to(dtype))
            out = torch.empty_like(v)
            got, num = rs.radix_scan_by_key(keys, v, exclusive=True, runs=True, out=out, return_num=True, ctx=ctx)
            ctx.check()
            assert got is out and num.dim() == 0 and num.dtype == torch.int64 and int(num) == 1
            assert torch.equal(out, (torch.cumsum(v, 0) - v).to(dtype))  # first=None is 0 for "sum"


def cpu_groups(keys):
    """{key: its input positions in order} on the CPU."""
    groups = {}
    for i, k in enumerate(keys.tolist()):
        groups.setdefault(k, []).append(i)
    return groups


def test_python_grouped_sum_equals_cumsum_per_group(rs, torch, ctx):
    rng = np.random.default_rng(14)
    n = 40013
    keys = torch.from_numpy(rng.integers(-3000, 3000, size=n, dtype=np.int64))
    vals = torch.from_numpy(rng.integers(-2 ** 40, 2 ** 40, size=n, dtype=np.int64))
    want = torch.empty_like(vals)
    for pos in cpu_groups(keys).values():
        idx = torch.tensor(pos)
        want[idx] = torch.cumsum(vals[idx], 0)
    v = vals.cuda()
    got = rs.radix_scan_by_key(keys.cuda(), v, ctx=ctx)
    ctx.check()
    assert torch.equal(got.cpu(), want)
    assert rs.radix_scan_by_key(keys.cuda(), v, out=v, ctx=ctx) is v  # in place
    ctx.check()
    assert torch.equal(v.cpu(), want)
    for op, fn in (("min", torch.cummin), ("max", torch.cummax)):
        want = torch.empty_like(vals)
        for pos in cpu_groups(keys).values():
            idx = torch.tensor(pos)
            want[idx] = fn(vals[idx], 0).values
        assert torch.equal(rs.radix_scan_by_key(keys.cuda(), vals.cuda(), op=op, ctx=ctx).cpu(), want)
        excl = rs.radix_scan_by_key(keys.cuda(), vals.cuda(), op=op, exclusive=True, ctx=ctx).cpu()  # first=None: the type's end
        heads = torch.tensor([pos[0] for pos in cpu_groups(keys).values()])
        assert bool((excl[heads] == (2 ** 63 - 1 if op == "min" else -2 ** 63)).all())


def test_python_cumcount(rs, torch, ctx):
    rng = np.random.default_rng(15)
    n = 30011
    keys = torch.from_numpy(rng.integers(0, 977, size=n).astype(np.int16))
    want = torch.empty(n, dtype=torch.int64)
    for pos in cpu_groups(keys).values():
        want[torch.tensor(pos)] = torch.arange(len(pos))
    got, num = rs.radix_scan_by_key(keys.cuda(), None, exclusive=True, return_num=True, ctx=ctx)
    ctx.check()
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want) and int(num) == len(cpu_groups(keys))
    got = rs.radix_scan_by_key(keys.cuda(), None, index_dtype=torch.int32, ctx=ctx)  # row_number(): 1-based
    ctx.check()
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), (want + 1).to(torch.int32))
    raw = util.make_input("i128", 5000, "two", seed=4)
    wide = torch.from_numpy(raw.copy()).cuda().view(5000, 16)
    got, num = rs.radix_scan_by_key(wide, None, exclusive=True, return_num=True, ctx=ctx, key_kind=rs.KEY_SIGNED)
    ctx.check()
    ref = scan_reference(raw, 16, SIGNED, None, 8, SIGNED, SUM, True, 0, False)
    assert int(num) == ref.num == 2 and np.array_equal(got.cpu().numpy(), ref.rank)
