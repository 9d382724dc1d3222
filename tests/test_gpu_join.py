"""GPU: rsx_join_device / radix_join against tests/join_ref.py, byte for byte (the method of tests/test_gpu_setop.py).

Every output sits in an allocation the test owns: 64 guard bytes of 0xA5, `capacity` rows filled with 0xA5, 64 guard bytes.
What comes back is compared whole: rows [0, min(T, capacity)) with the reference, the rest and the guards still 0xA5, the
count word exact (the FULL number of rows), the inputs and index arrays compared with their originals afterwards.

The sizes come from rsx_join_caps (A = the keys of a per count tile, WIN = the keys of b a count tile stages at most, R =
the rows per write tile), so that they stay the edge cases of the kernels whatever their constants are; every case keeps
T <= 2^18 rows.  Keys are made from ascending IDS mapped to the key type by an increasing map.  Each shape asserts through
join_ref.tile_model that the condition it is named for occurs."""
import numpy as np
import pytest

import util
from join_ref import HOWS, bound, join_reference, tile_model
from segment_pairs_gpu import guarded, key_dtype, same
from segment_pairs_ref import with_guards
from test_gpu_merge import keys_of, shape_ids
from test_gpu_search import F32_SPECIALS, F64_SPECIALS, canary, keys_from_ids

pytestmark = pytest.mark.gpu

PATH = 13 << 24
SHAPES = ["pairs", "all_equal", "dup_cycle", "sparse", "a_below_b", "b_below_a", "wide_window"]
HOW_NAMES = list(HOWS)
MAX_ROWS = 1 << 18


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
def dup_cycle(A, WIN):
    return [(1, 1), (2, 1), (1, 2), (3, 0), (0, 3), (A + 1, 2), (2, WIN + 1)]


def cycle_ids(cyc, na, nb):
    """Key q occurs m times in a and n times in b, (m, n) cycling; what is left of one side goes on alone."""
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


def sizes_of(shape, A, WIN, R):
    if shape == "all_equal":
        return [(A + 1, 37), (3, 3 * R + 5), (1, R), (R, 1)]
    if shape == "sparse":  # (the second: more keys between two rows than the write kernel stages, four tiles of rows)
        return [(5 * A + 3, R + 3), (4 * R + 2 * A + 3, 2)]
    if shape == "wide_window":
        return [(A, WIN + A + 1)]
    sizes = [(0, 5), (5, 0), (1, 1), (A - 1, 1), (A, A), (A + 1, A - 1), (2 * A + 3, R + 5), (3 * A + 7, 3 * A - 5)]
    if shape == "dup_cycle":
        sizes.append((A + 20, WIN + 30))  # room for the run of WIN + 1 keys of b whatever the window is
    return sizes


def join_ids(shape, na, nb, A, WIN, R):
    """(ids of a, ids of b): each ascending."""
    i, j = np.arange(na, dtype=np.int64), np.arange(nb, dtype=np.int64)
    if shape == "pairs":  # distinct keys; every second key of a occurs once in b
        return i, 2 * j
    if shape == "all_equal":
        return np.full(na, 5, dtype=np.int64), np.full(nb, 5, dtype=np.int64)
    if shape == "dup_cycle":
        return cycle_ids(dup_cycle(A, WIN), na, nb)
    if shape == "sparse":  # b holds a's first key, its key 2A + 1 over and over, and its last key
        return i, np.concatenate([[0], np.full(nb - 2, 2 * A + 1, dtype=np.int64), [na - 1]])
    if shape == "wide_window":  # a's keys are spread over all of b's, which are distinct
        return i * (nb // na), j
    return shape_ids(shape, na, nb, A, None)


class JoinCase:
    """Two sorted key arrays on the GPU between guards, optional index arrays and device counts, the references computed
    once per kind of join."""

    def __init__(self, torch, c, tname, a_raw, b_raw, desc, n_a=None, n_b=None, a_index=None, b_index=None):
        self.torch, self.c, self.tname, self.desc = torch, c, tname, desc
        self.kb, self.kind = util.TYPES[tname][2], util.TYPES[tname][3]
        self.a_raw, self.b_raw = a_raw, b_raw
        self.na, self.nb = a_raw.size // self.kb, b_raw.size // self.kb
        self.abuf, self.amid = guarded(torch, a_raw)
        self.bbuf, self.bmid = guarded(torch, b_raw)
        self.n_a, self.n_b = n_a, n_b
        dev = lambda v: None if v is None else torch.tensor([v], dtype=torch.int64, device="cuda")  # noqa: E731
        self.a_num, self.b_num = dev(n_a), dev(n_b)
        self.a_index, self.b_index = a_index, b_index  # numpy arrays of the call's index width, or None
        self.aibuf = guarded(torch, a_index) if a_index is not None else None
        self.bibuf = guarded(torch, b_index) if b_index is not None else None
        self.refs = {}

    def reference(self, how):
        if how not in self.refs:  # computed once per kind of join, shared by every call
            self.refs[how] = join_reference(self.a_raw, self.b_raw, self.tname, self.desc, how, self.n_a, self.n_b, self.a_index,
                                            self.b_index if how in ("inner", "left") else None)
            assert self.refs[how][2] <= MAX_ROWS
        return self.refs[how]

    def model(self, rs, how, capacity=None):
        A, WIN, R = rs.join_caps(self.kb)
        return tile_model(self.a_raw, self.b_raw, self.tname, self.desc, how, A, WIN, R, self.n_a, self.n_b, capacity)

    def call(self, how, out_a, out_b, ib, capacity, out_num, stream=None):
        torch = self.torch
        ptr = lambda mid, cnt: mid.data_ptr() if cnt else 0  # noqa: E731 (an empty view has no address of its own)
        pairs = how in ("inner", "left")
        self.c.join_device(HOWS[how], ptr(self.amid, self.na), self.na, self.a_num.data_ptr() if self.a_num is not None else 0,
                           self.aibuf[1].data_ptr() if self.aibuf is not None and self.na else 0, ptr(self.bmid, self.nb), self.nb,
                           self.b_num.data_ptr() if self.b_num is not None else 0,
                           self.bibuf[1].data_ptr() if self.bibuf is not None and self.nb and pairs else 0, self.kb, self.kind, out_a, out_b, ib,
                           capacity, out_num, self.desc, torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def run(self, rs, how, ib=8, capacity=None, what=None):
        """One call -> compares each whole allocation with the reference; returns T.  capacity None: T + 5 rows; 0: the
        count-only form, both outputs null."""
        torch = self.torch
        wl, wr, T = self.reference(how)
        cap = T + 5 if capacity is None else capacity
        pairs = how in ("inner", "left")
        ao = guarded(torch, canary(cap * ib))
        bo = guarded(torch, canary(cap * ib)) if pairs else None
        no = guarded(torch, canary(8))
        self.call(how, ao[1].data_ptr() if cap else 0, bo[1].data_ptr() if pairs and cap else 0, ib, cap, no[1].data_ptr())
        self.c.check()
        launched = 0 if self.na == 0 else 2 if cap == 0 else 3
        assert self.c.get_info(rs.INFO_LAST_PASSES) == PATH | launched, (self.tname, how, hex(self.c.get_info(rs.INFO_LAST_PASSES)))
        tag = (self.tname, self.na, self.nb, how, what, "desc" if self.desc else "asc", ib, cap, self.n_a, self.n_b)
        m = min(T, cap)
        dt = "<i4" if ib == 4 else "<i8"

        def whole(rows):  # rows [0, m) exact, rows [m, cap) untouched
            exp = canary(cap * ib)
            exp[:m * ib] = np.ascontiguousarray(rows[:m].astype(dt)).view(np.uint8).reshape(-1)
            return with_guards(exp)

        assert same(no[0].cpu().numpy(), with_guards(np.array([T], dtype="<i8")), ("num",) + tag)
        assert same(ao[0].cpu().numpy(), whole(wl), ("left",) + tag)
        if pairs:
            assert same(bo[0].cpu().numpy(), whole(wr), ("right",) + tag)
        return T

    def inputs_unchanged(self):
        assert same(self.abuf.cpu().numpy(), with_guards(self.a_raw), ("a", self.tname, self.na))
        assert same(self.bbuf.cpu().numpy(), with_guards(self.b_raw), ("b", self.tname, self.nb))
        if self.aibuf is not None:
            assert same(self.aibuf[0].cpu().numpy(), with_guards(self.a_index), ("a_index", self.tname, self.na))
        if self.bibuf is not None:
            assert same(self.bibuf[0].cpu().numpy(), with_guards(self.b_index), ("b_index", self.tname, self.nb))


def check_named(shape, case, rs, rows):
    """The condition a shape is named for, on one case; rows: {how: T}."""
    na, nb = case.na, case.nb
    A, WIN, R = rs.join_caps(case.kb)
    assert rows["semi"] + rows["anti"] == na and rows["left"] == rows["inner"] + rows["anti"]
    if shape == "pairs":
        count, _w = case.model(rs, "inner")
        assert rows["inner"] == rows["semi"] == min(nb, (na + 1) // 2) and all(t["total"] <= A for t in count)
    if shape == "all_equal":
        assert rows["inner"] == na * nb and rows["anti"] == 0
        _c, write = case.model(rs, "inner")
        if nb > 3 * R:  # one key's rows span more than three write tiles
            assert sum(w["keys"] == 1 for w in write) > 3
        if (na, nb) == (A + 1, 37):  # one write tile holds the rows of many keys, of both count tiles at the end
            assert all(w["keys"] > 1 for w in write) and write[-1]["tiles"] == 2
    if shape == "dup_cycle" and na > A + 8:
        ia = join_ids(shape, na, nb, A, WIN, R)[0]
        assert ia[A - 1] == ia[A]  # a run of a across the count-tile boundary
        count, _w = case.model(rs, "inner")
        if nb > WIN + 10:  # the run of b longer than the window: the global route
            assert not all(t["staged"] for t in count) and any(t["staged"] for t in count)
    if shape == "sparse":
        count, write = case.model(rs, "inner")
        totals = [t["total"] for t in count]
        assert totals[0] == 1 and totals[-1] == 1 and sum(totals) == nb  # count tiles with no row in between
        if nb > 2:
            assert max(totals) == nb - 2 and totals.count(0) == len(totals) - 3
            assert write[-1]["tiles"] >= 3 and write[-1]["keys"] > R  # more keys than rows: most of them contribute nothing
            _c, write = case.model(rs, "semi")
            assert rows["semi"] == 3
        else:
            assert totals.count(0) == len(totals) - 2 and write[0]["keys"] == na > 4 * R  # the searches in global memory
        assert write[0]["tiles"] == len(count)  # one write tile from the first and the last count tile
    if shape in ("a_below_b", "b_below_a") and na and nb:
        assert rows["inner"] == 0 and rows["semi"] == 0 and rows["left"] == na and rows["anti"] == na
    if shape == "wide_window":
        count, _w = case.model(rs, "inner")
        assert len(count) == 1 and not count[0]["staged"] and rows["inner"] == na


# ---- the matrix ----
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("tname", ["u32", "i64"])
def test_every_how_shape_and_size(rs, torch, ctx, tname, shape):
    kb = util.TYPES[tname][2]
    A, WIN, R = rs.join_caps(kb)
    v = 0
    for na, nb in sizes_of(shape, A, WIN, R):
        ia, ib_ = join_ids(shape, na, nb, A, WIN, R)
        assert ia.size == na and ib_.size == nb
        desc = v % 2 == 0  # the orders and the index widths take turns
        a_raw, b_raw = keys_of(tname, ia, ib_, desc)
        case = JoinCase(torch, ctx, tname, a_raw, b_raw, desc)
        rows = {}
        for h, how in enumerate(HOW_NAMES):
            rows[how] = case.run(rs, how, ib=(4, 8)[(v + h) % 2], what=shape)
        v += 1
        case.inputs_unchanged()
        check_named(shape, case, rs, rows)


def test_capacity(rs, torch, ctx):
    """Every capacity around the write tile and around T, and the count-only form: num is T every time."""
    A, WIN, R = rs.join_caps(4)
    ia, ib_ = join_ids("dup_cycle", 2 * A + 3, R + 5, A, WIN, R)
    a_raw, b_raw = keys_of("u32", ia, ib_, False)
    case = JoinCase(torch, ctx, "u32", a_raw, b_raw, False)
    for how in ("inner", "left"):
        T = case.reference(how)[2]
        assert T > R + 1
        for v, cap in enumerate((0, 1, R, R + 1, T - 1, T, T + 3 * R)):
            assert case.run(rs, how, ib=(8, 4)[v % 2], capacity=cap, what="capacity") == T
    case.inputs_unchanged()


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", ["u8", "u16", "i32", "f32", "f64", "u128", "i128"])
def test_other_key_types(rs, torch, ctx, tname, desc):
    kb = util.TYPES[tname][2]
    A, WIN, R = rs.join_caps(kb)
    na, nb = A + 1, A - 1
    ia, ib_ = join_ids("dup_cycle", na, nb, A, WIN, R)
    a_raw, b_raw = keys_of(tname, ia, ib_, desc)
    case = JoinCase(torch, ctx, tname, a_raw, b_raw, desc)
    for h, how in enumerate(HOW_NAMES):
        case.run(rs, how, ib=(4, 8)[(h + desc) % 2], what="dup_cycle")
    case.inputs_unchanged()


@pytest.mark.parametrize("tname", ["f32", "f64"])
def test_float_specials(rs, torch, ctx, tname):
    """The seven specials as runs in both arrays: seven different keys by bit pattern.  -0.0 and +0.0 do not match, a NaN
    matches only the NaN of its own bits: with one special left out of b, exactly its run is unmatched."""
    kb = util.TYPES[tname][2]
    sp = F32_SPECIALS if kb == 4 else F64_SPECIALS
    for ra, rb in ((1, 1), (3, 2), (150, 201)):
        for desc in (False, True):
            order = sp[::-1] if desc else sp
            for gone in (None, 2, 3, 5, 6):  # -0.0, +0.0 and two NaNs, one at a time
                a = np.repeat(order, ra)
                b = np.repeat(order if gone is None else np.delete(order, list(order).index(sp[gone])), rb)
                case = JoinCase(torch, ctx, tname, a.view(np.uint8).reshape(-1).copy(), b.view(np.uint8).reshape(-1).copy(), desc)
                rows = {how: case.run(rs, how, ib=4, what=("specials", ra, rb, gone)) for how in HOW_NAMES}
                hit = 7 if gone is None else 6
                assert rows == {"inner": hit * ra * rb, "left": hit * ra * rb + (7 - hit) * ra, "semi": hit * ra, "anti": (7 - hit) * ra}
                case.inputs_unchanged()


# ---- device counts ----
def test_device_counts(rs, torch, ctx):
    """Capacities (3A + 7, 3A - 5) with counts on the device -- 0, mid-tile, exactly a tile, above the length: the keys
    beyond the counts hold descending garbage that must not reach the result."""
    tname = "u32"
    A, WIN, R = rs.join_caps(4)
    na, nb = 3 * A + 7, 3 * A - 5
    ia, ib_ = join_ids("dup_cycle", na, nb, A, WIN, R)
    top = int(max(ia.max(), ib_.max())) + 1
    for n_a, n_b in ((A + 1, 0), (A + 301, 2 * A), (A, A), (2 * A, nb + 1), (na + 100, A + 7), (0, 0), (0, nb)):
        ga, gb = ia.copy(), ib_.copy()
        ca, cb = min(n_a, na), min(n_b, nb)
        ga[ca:] = top + np.arange(na - ca)[::-1]  # descending, and above every counted key
        gb[cb:] = top + np.arange(nb - cb)[::-1] // 2
        both = keys_from_ids(tname, np.concatenate([ga, gb])).reshape(-1, 4)
        a_raw, b_raw = both[:na].reshape(-1).copy(), both[na:].reshape(-1).copy()
        case = JoinCase(torch, ctx, tname, a_raw, b_raw, False, n_a=n_a, n_b=n_b)
        for v, how in enumerate(HOW_NAMES):
            case.run(rs, how, ib=(4, 8)[v % 2], what=("counts", n_a, n_b))
            wl, wr, T = case.reference(how)
            assert T <= bound(how, ca, cb) and bool((wl < ca).all()) and (wr is None or bool((wr < cb).all()))  # nothing from beyond the counts
        case.inputs_unchanged()


# ---- index arrays ----
@pytest.mark.parametrize("ib", [4, 8])
def test_index_arrays(rs, torch, ctx, ib):
    """Random permutations (offset, so that they cannot pass for positions) in place of the positions of a, of b, of both."""
    rng = np.random.default_rng(ib)
    A, WIN, R = rs.join_caps(8)
    na, nb = 2 * A + 3, R + 5
    ia, ib_ = join_ids("dup_cycle", na, nb, A, WIN, R)
    a_raw, b_raw = keys_of("i64", ia, ib_, ib == 4)
    dt = "<i4" if ib == 4 else "<i8"
    pa = (rng.permutation(na) + 7 * na).astype(dt)
    pb = (rng.permutation(nb) + (1 << 20 if ib == 4 else 1 << 40)).astype(dt)
    for ai, bi in ((pa, pb), (pa, None), (None, pb)):
        case = JoinCase(torch, ctx, "i64", a_raw, b_raw, ib == 4, a_index=ai, b_index=bi)
        for how in ("inner", "left") + (("semi", "anti") if bi is None else ()):
            case.run(rs, how, ib=ib, what="index arrays")
        case.inputs_unchanged()


# ---- the Python call ----
def _tensor(torch, raw, tname):
    kb = util.TYPES[tname][2]
    dt = key_dtype(torch, tname)
    if raw.size == 0:  # (an empty byte tensor cannot be viewed as another dtype)
        return torch.empty((0, 16), dtype=torch.uint8, device="cuda") if kb == 16 else torch.empty(0, dtype=dt, device="cuda")
    t = torch.from_numpy(raw.copy()).cuda()
    return t.view(-1, 16) if kb == 16 else t.view(dt)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", ["u32", "i64", "f32"])
def test_radix_join(rs, torch, ctx, tname, desc):
    kb = util.TYPES[tname][2]
    A, WIN, R = rs.join_caps(kb)
    rng = np.random.default_rng(kb + 3 * desc)
    for na, nb in ((0, 5), (7, 0), (A + 11, A + 5)):
        ia, ib_ = join_ids("dup_cycle", na, nb, A, WIN, R)
        a_raw, b_raw = keys_of(tname, ia, ib_, desc)
        a, b = _tensor(torch, a_raw, tname), _tensor(torch, b_raw, tname)
        # the same keys shuffled: the tables a user has
        sa, sb = rng.permutation(na), rng.permutation(nb)
        ua_raw = a_raw.reshape(-1, kb)[sa].reshape(-1).copy()
        ub_raw = b_raw.reshape(-1, kb)[sb].reshape(-1).copy()
        ua, ub = _tensor(torch, ua_raw, tname), _tensor(torch, ub_raw, tname)
        pa = rs.radix_argsort(ua, descending=desc, ctx=ctx).cpu().numpy() if na else np.zeros(0, dtype=np.int64)
        pb = rs.radix_argsort(ub, descending=desc, ctx=ctx).cpu().numpy() if nb else np.zeros(0, dtype=np.int64)
        for v, how in enumerate(HOW_NAMES):
            wl, wr, T = join_reference(a_raw, b_raw, tname, desc, how)
            pairs = wr is not None
            idt = (torch.int64, torch.int32)[v % 2]
            # sorted inputs: the exact allocation (one host read), a capacity, out=
            r = rs.radix_join(a, b, how, assume_sorted=True, descending=desc, index_dtype=idt, ctx=ctx)
            assert r.num.shape == () and r.num.dtype == torch.int64 and int(r.num) == T
            assert r.left.shape == (T,) and r.left.dtype == idt and np.array_equal(r.left.cpu().numpy(), wl)
            assert (r.right is None) == (not pairs) and (not pairs or (r.right.shape == (T,) and np.array_equal(r.right.cpu().numpy(), wr)))
            cap = T // 2 + 3
            r = rs.radix_join(a, b, how, assume_sorted=True, capacity=cap, descending=desc, ctx=ctx)
            m = min(T, cap)
            assert int(r.num) == T and r.left.shape == (cap,) and r.left.dtype == torch.int64 and np.array_equal(r.left[:m].cpu().numpy(), wl[:m])
            assert not pairs or np.array_equal(r.right[:m].cpu().numpy(), wr[:m])
            out = (torch.full((T + 2,), -7, dtype=torch.int32, device="cuda"), torch.full((T + 2,), -7, dtype=torch.int32, device="cuda") if pairs else None)
            r = rs.radix_join(a, b, how, assume_sorted=True, descending=desc, out=out, ctx=ctx)
            assert r.left is out[0] and r.right is out[1] and int(r.num) == T
            assert np.array_equal(out[0].cpu().numpy(), np.concatenate([wl, [-7, -7]]))
            assert not pairs or np.array_equal(out[1].cpu().numpy(), np.concatenate([wr, [-7, -7]]))
            # unsorted inputs: exactly (pa[L], pb[R]); the inputs stay as they were
            r = rs.radix_join(ua, ub, how, descending=desc, index_dtype=idt, ctx=ctx)
            assert int(r.num) == T and r.left.dtype == idt and np.array_equal(r.left.cpu().numpy(), pa[wl])
            assert (r.right is None) == (not pairs)
            if pairs:
                assert np.array_equal(r.right.cpu().numpy(), np.where(wr < 0, -1, pb[np.maximum(wr, 0)] if nb else -1))
            r = rs.radix_join(ua, ub, how, descending=desc, capacity=T + 1, ctx=ctx)
            assert int(r.num) == T and np.array_equal(r.left[:T].cpu().numpy(), pa[wl])
            assert np.array_equal(ua.cpu().numpy().view(np.uint8).reshape(-1), ua_raw) and np.array_equal(ub.cpu().numpy().view(np.uint8).reshape(-1), ub_raw)
        ctx.check()
    with pytest.raises(ValueError, match="assume_sorted"):
        rs.radix_join(ua, ub, "inner", a_num=torch.zeros((), dtype=torch.int64, device="cuda"), ctx=ctx)


def test_two_groups_join_without_a_host_read(rs, torch, ctx):
    """Two radix_group results joined on their distinct keys through a_num= / b_num=; the result is read only at the end."""
    rng = np.random.default_rng(23)
    a = rng.integers(-400, 400, size=30011).astype("<i4")
    b = rng.integers(-300, 500, size=20021).astype("<i4")
    ga = rs.radix_group(torch.from_numpy(a).cuda(), perm=False, ctx=ctx)
    gb = rs.radix_group(torch.from_numpy(b).cuda(), perm=False, ctx=ctx)
    cap = min(a.size, b.size)
    r = rs.radix_join(ga.keys, gb.keys, assume_sorted=True, a_num=ga.num, b_num=gb.num, capacity=cap, ctx=ctx)  # nothing read in between
    s = rs.radix_join(ga.keys, gb.keys, "anti", assume_sorted=True, a_num=ga.num, b_num=gb.num, capacity=cap, ctx=ctx)
    ctx.check()
    ua, ub = np.unique(a), np.unique(b)
    common, ia, ib_ = np.intersect1d(ua, ub, return_indices=True)
    T = int(r.num)
    assert T == common.size and r.left.shape == (cap,) and r.right.shape == (cap,)
    assert np.array_equal(r.left[:T].cpu().numpy(), ia) and np.array_equal(r.right[:T].cpu().numpy(), ib_)
    assert np.array_equal(ga.keys[r.left[:T]].cpu().numpy(), common) and np.array_equal(gb.keys[r.right[:T]].cpu().numpy(), common)
    assert s.right is None and np.array_equal(ga.keys[s.left[:int(s.num)]].cpu().numpy(), np.setdiff1d(ua, ub))


# ---- the precondition broken ----
@pytest.mark.parametrize("tname", ["u32", "i64", "u128"])
def test_unsorted_inputs_stay_in_bounds(rs, torch, ctx, tname):
    """Shuffled a and b: the guards hold, the inputs are unchanged, num <= bound and every index is a position or NONE."""
    rng = np.random.default_rng(13)
    kb = util.TYPES[tname][2]
    A, WIN, R = rs.join_caps(kb)
    cap = 4 * R
    for na, nb in ((A + 1, A), (4 * A + 5, 3 * A + 7)):
        n = na + nb
        a_raw = keys_from_ids(tname, rng.integers(0, n // 4, size=na))
        b_raw = keys_from_ids(tname, rng.integers(0, n // 4, size=nb))
        case = JoinCase(torch, ctx, tname, a_raw, b_raw, False)
        for v, how in enumerate(HOW_NAMES):
            ib = (4, 8)[v % 2]
            pairs = how in ("inner", "left")
            ao, bo, no = guarded(torch, canary(cap * ib)), guarded(torch, canary(cap * ib)), guarded(torch, canary(8))
            case.call(how, ao[1].data_ptr(), bo[1].data_ptr() if pairs else 0, ib, cap, no[1].data_ptr())
            ctx.check()
            num = int(no[1].view(torch.int64)[0])
            assert 0 <= num <= bound(how, na, nb), (tname, how, num)
            m = min(num, cap)
            idt = torch.int32 if ib == 4 else torch.int64
            left = ao[1].view(idt)[:m]
            assert m == 0 or (int(left.min()) >= 0 and int(left.max()) < na), (tname, na, nb, how)
            if pairs:
                right = bo[1].view(idt)[:m]
                assert m == 0 or (int(right.min()) >= -1 and int(right.max()) < nb), (tname, na, nb, how)
                assert how == "left" or m == 0 or int(right.min()) >= 0
            for buf, mid in (ao, bo, no):
                whole = buf.cpu().numpy()
                assert (whole[:64] == 0xA5).all() and (whole[-64:] == 0xA5).all(), (tname, na, nb, how)
            assert bool((ao[1][m * ib:] == 0xA5).all()) and bool((bo[1][(m if pairs else 0) * ib:] == 0xA5).all())
        case.inputs_unchanged()


# ---- empty inputs, capture, errors ----
def test_nothing_to_do(rs, torch, ctx):
    E = rs._lib
    L, h = ctx._L, ctx._h
    num = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    # na == 0: the count is stored, nothing is launched and no other pointer is looked at (dangling ones here)
    assert L.rsx_join_device(h, 0, 8, 0, None, 8, 8, 5, None, 8, 4, 0, 0, 8, 8, 8, 100, num.data_ptr(), None) == E.OK
    assert int(num) == 0 and ctx.get_info(rs.INFO_LAST_PASSES) == PATH
    e = torch.zeros(0, dtype=torch.int32, device="cuda")
    x = torch.arange(5, dtype=torch.int32, device="cuda")
    for how, rows, right in (("inner", [], []), ("left", [0, 1, 2, 3, 4], [-1] * 5), ("semi", [], None), ("anti", [0, 1, 2, 3, 4], None)):
        for sorted_ in (True, False):
            r = rs.radix_join(e, x, how, assume_sorted=sorted_, ctx=ctx)
            assert int(r.num) == 0 and r.left.shape == (0,) and (r.right is None) == (right is None)
            assert int(rs.radix_join(e, e, how, assume_sorted=sorted_, capacity=3, ctx=ctx).num) == 0
            r = rs.radix_join(x, e, how, assume_sorted=sorted_, ctx=ctx)  # nb == 0 goes through the kernels
            assert int(r.num) == len(rows) and r.left.tolist() == rows and (right is None or r.right.tolist() == right)
            assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | (3 if rows else 2)
    ctx.check()


def test_capture_after_reserve_and_workspace_error_without(rs, torch):
    A, WIN, R = rs.join_caps(4)
    na, nb = 2 * A + 9, 3 * A + 1
    cap = 8 * R
    src_a = torch.zeros(na, dtype=torch.int32, device="cuda")
    src_b = torch.zeros(nb, dtype=torch.int32, device="cuda")
    a, b = torch.empty_like(src_a), torch.empty_like(src_b)
    left = torch.empty(cap, dtype=torch.int32, device="cuda")
    right = torch.empty(cap, dtype=torch.int32, device="cuda")
    num = torch.empty((), dtype=torch.int64, device="cuda")

    def enqueue(c):
        c.join_device(rs.JOIN_LEFT, a.data_ptr(), na, 0, 0, b.data_ptr(), nb, 0, 0, 4, rs.KEY_SIGNED, left.data_ptr(), right.data_ptr(), 4, cap,
                      num.data_ptr(), False, torch.cuda.current_stream().cuda_stream)

    # without a reserve: the context has made an ordinary call (its error word and self-tests exist) but owns no workspace
    c0 = rs.Context(torch.cuda.current_device())
    x = torch.randint(0, 2 ** 31 - 1, (1000,), dtype=torch.int32, device="cuda")
    rs.radix_sort(x, ctx=c0)
    c0.check()
    left.fill_(-7)
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
    assert bool((left == -7).all())  # nothing was enqueued
    c0.close()

    c = rs.Context(torch.cuda.current_device())
    c.reserve_join(na, 4)
    graph = torch.cuda.CUDAGraph()
    s.synchronize()
    with torch.cuda.graph(graph, stream=s):  # one linear chain: the two copies, then the call's three launches
        a.copy_(src_a)
        b.copy_(src_b)
        enqueue(c)
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        a_np = np.sort(rng.integers(-700, 700, size=na)).astype("<i4")
        b_np = np.sort(rng.integers(-700, 700, size=nb)).astype("<i4")
        src_a.copy_(torch.from_numpy(a_np))
        src_b.copy_(torch.from_numpy(b_np))
        left.fill_(-7)
        right.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        wl, wr, T = join_reference(a_np.view(np.uint8), b_np.view(np.uint8), "i32", False, "left")
        assert int(num) == T and T <= cap
        assert np.array_equal(left[:T].cpu().numpy(), wl) and np.array_equal(right[:T].cpu().numpy(), wr)
        assert bool((left[T:] == -7).all()) and bool((right[T:] == -7).all())
    c.close()


def test_errors(rs, torch, ctx):
    E = rs._lib
    L, h = ctx._L, ctx._h
    P = 4096
    buf = torch.full((12 * P,), 0xA5, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert p % 16 == 0
    ok = dict(how=0, ak=p, na=100, an=0, ai=p + P, bk=p + 2 * P, nb=50, bn=0, bi=p + 3 * P, kb=4, kind=0, order=0, oa=p + 4 * P, ob=p + 6 * P, ib=8,
              cap=200, on=p + 8 * P)

    def call(**kw):
        a = dict(ok, **kw)
        return L.rsx_join_device(h, a["how"], a["ak"] or None, a["na"], a["an"] or None, a["ai"] or None, a["bk"] or None, a["nb"], a["bn"] or None,
                                 a["bi"] or None, a["kb"], a["kind"], a["order"], a["oa"] or None, a["ob"] or None, a["ib"], a["cap"], a["on"] or None, None)

    assert call(how=4) == E.ERR_ARG
    assert call(kb=3) == E.ERR_ARG and call(kb=16, kind=2) == E.ERR_ARG and call(kind=3) == E.ERR_ARG
    assert call(order=2) == E.ERR_ARG
    assert call(ib=2) == E.ERR_ARG and call(ib=0) == E.ERR_ARG
    assert call(on=0) == E.ERR_ARG and call(on=ok["on"] + 4) == E.ERR_ARG      # the count word: required, 8-byte aligned
    assert call(an=ok["on"] + 12) == E.ERR_ARG and call(bn=ok["on"] + 20) == E.ERR_ARG
    assert call(ak=0) == E.ERR_ARG and call(bk=0) == E.ERR_ARG                 # null inputs with a nonzero count
    assert call(oa=0) == E.ERR_ARG and call(ob=0) == E.ERR_ARG and call(oa=0, ob=0) == E.ERR_ARG  # null outputs with a capacity
    assert call(oa=0, cap=0) == E.ERR_ARG and call(ob=0, cap=0) == E.ERR_ARG   # the count-only form has no output at all
    for how in (2, 3):                                                        # semi and anti have no right-hand side
        assert call(how=how) == E.ERR_ARG and call(how=how, ob=0) == E.ERR_ARG and call(how=how, bi=0) == E.ERR_ARG
        assert call(how=how, ob=0, bi=0, oa=0) == E.ERR_ARG
    for name in ("ak", "bk"):
        assert call(**{name: ok[name] + 2}) == E.ERR_ARG, name
    for name in ("ai", "bi", "oa", "ob"):
        assert call(**{name: ok[name] + 4}) == E.ERR_ARG, name
    assert call(na=2 ** 32) == E.ERR_UNSUPPORTED and call(nb=2 ** 32) == E.ERR_UNSUPPORTED and call(na=2 ** 40, how=3, ob=0, bi=0) == E.ERR_UNSUPPORTED
    R = rs.join_caps(4)[2]
    assert call(na=2 ** 32 - 1, nb=2 ** 32 - 1, cap=2 ** 31 * R + 1) == E.ERR_UNSUPPORTED  # more than 2^31 write workgroups
    assert L.rsx_ctx_reserve_join(h, 2 ** 32, 4) == E.ERR_UNSUPPORTED and L.rsx_ctx_reserve_join(h, 100, 3) == E.ERR_ARG
    # overlaps: against min(capacity, bound) rows of every output
    last = lambda base, cnt, w: base + cnt * w - w  # noqa: E731
    assert call(oa=ok["ak"]) == E.ERR_ARG and call(oa=ok["ak"] + 392) == E.ERR_ARG and call(ob=ok["bk"]) == E.ERR_ARG
    assert call(oa=ok["ai"]) == E.ERR_ARG and call(ob=last(ok["bi"], 50, 8)) == E.ERR_ARG
    assert call(oa=ok["bk"] - 200 * 8 + 8) == E.ERR_ARG                        # the 200th row is b's first key
    assert call(ob=ok["oa"]) == E.ERR_ARG and call(ob=ok["oa"] + 199 * 8) == E.ERR_ARG
    assert call(on=ok["ak"] + 8) == E.ERR_ARG and call(on=ok["oa"] + 8) == E.ERR_ARG and call(on=ok["ob"] + 199 * 8) == E.ERR_ARG
    assert call(on=ok["ai"]) == E.ERR_ARG and call(an=ok["on"]) == E.ERR_ARG and call(bn=ok["on"]) == E.ERR_ARG
    assert call(an=ok["oa"] + 16) == E.ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())                                          # no refused call wrote
    # what is allowed: min(capacity, bound) rows that end in front of b where the capacity's would not
    assert call(how=2, ob=0, bi=0, oa=ok["bk"] - 100 * 8, cap=10 ** 6) == E.OK  # a semi join writes at most na rows
    assert call(oa=ok["bk"] - 150 * 8, cap=150) == E.OK and call(oa=ok["oa"] + 4, ob=ok["ob"] + 4, ai=0, bi=0, ib=4) == E.OK
    assert call(ai=0) == E.OK and call(bi=0) == E.OK and call(oa=0, ob=0, cap=0) == E.OK
    assert call(nb=0, bk=0, bi=0) == E.OK and call(how=1, nb=0, bk=0, bi=0) == E.OK  # an empty b needs no pointers
    assert call(na=10, nb=10, cap=2 ** 63) == E.OK                                        # a generous capacity: the grid follows the bound
    ctx.check()
