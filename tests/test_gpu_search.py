"""GPU: rsx_search_sorted_device / radix_searchsorted against tests/search_ref.py, byte for byte.

Every output sits in an allocation the test owns: 64 guard bytes of 0xA5, the array filled with 0xA5, 64 guard bytes; what
comes back is compared whole, and both inputs are compared with their originals afterwards.

The sizes come from rsx_search_caps (T = tile, W = window), so that they stay the edge cases of the kernel whatever its
constants are.  Keys are made from IDS, mapped to the key type by an increasing map: the haystack holds even ids from 2
on, so that odd ids (and 0) are keys absent from it, between its keys, below its first and above its last.  Each
matrix case asserts through search_ref.tile_routes that the route a needle kind is named after occurs."""
import numpy as np
import pytest

import util
from search_ref import search_reference, tile_routes
from segment_pairs_gpu import guarded, key_dtype, same
from segment_pairs_ref import with_guards

pytestmark = pytest.mark.gpu

PATH = 10 << 24
HAY_KINDS = ["distinct", "runs_of_3", "runs_of_tile", "equal"]
NEEDLE_KINDS = ["members", "shuffled", "absent", "cluster_w", "cluster_w1", "every_kth"]
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
def keys_from_ids(tname, ids):
    """Raw key bytes for ids >= 0: an increasing map into the key type (both signs, floats of both signs; 128-bit keys whose
    neighbours differ in the low half only)."""
    _es, _ko, kb, kind = util.TYPES[tname]
    ids = np.asarray(ids, dtype=np.int64)
    n = ids.size
    top = int(ids.max(initial=0))
    if kind == util.FLOAT:
        assert top < 1 << 24
        return (ids - top // 2).astype("<f4" if kb == 4 else "<f8").view(np.uint8).reshape(-1).copy()
    if kb <= 8:
        span = 1 << (8 * kb)
        assert kb == 8 or top < span, (tname, top)
        v = ids - (min(span // 2, max(1, top // 2)) if kind == util.SIGNED else 0)
        return v.astype("<i8").view(np.uint8).reshape(n, 8)[:, :kb].reshape(-1).copy()
    hi = ids // 4
    if kind == util.SIGNED:
        hi = hi - max(1, top // 8)
    out = np.zeros((n, 2), dtype="<u8")
    out[:, 0] = (ids % 4).astype("<u8") << np.uint64(62)
    out[:, 1] = hi.astype("<i8").view("<u8")
    return out.view(np.uint8).reshape(-1).copy()


def hay_ids(kind, N, T, groups=None):
    """N ascending even ids >= 2.  groups: at most that many distinct keys (types too narrow for the shape)."""
    i = np.arange(N, dtype=np.int64)
    if kind == "distinct":
        g = i
    elif kind == "runs_of_3":
        g = i // 3
    elif kind == "runs_of_tile":
        g = i // T
    elif kind == "equal":
        g = np.zeros(N, dtype=np.int64)
    else:
        raise ValueError(kind)
    if groups is not None and N and int(g[-1]) >= groups:
        g = i * groups // N
    return 2 * (1 + g)


def needle_ids(kind, h, m, T, W, rng):
    """m needle ids for the ascending haystack ids h."""
    N = h.size
    top = int(h[-1]) if N else 2
    absent = np.concatenate([np.array([0, 1, top + 1, top + 3], dtype=np.int64), 2 * rng.integers(0, top // 2 + 1, size=max(0, m - 4)) + 1])
    if N == 0 or kind == "absent":
        return rng.permutation(absent)[:m] if m < 4 else rng.permutation(absent)
    if kind in ("members", "shuffled"):  # a stretch of the haystack itself (all of it, repeated in place, when m > N)
        idx = (N - m) // 2 + np.arange(m) if m <= N else np.arange(m, dtype=np.int64) * N // m
        ids = h[idx]
        return ids if kind == "members" else rng.permutation(ids)
    if kind in ("cluster_w", "cluster_w1"):  # every tile: its smallest and largest needle span haystack elements apart
        span = min(N, W if kind == "cluster_w" else W + 1)
        ids = np.empty(m, dtype=np.int64)
        for t0 in range(0, m, T):
            cnt = min(T, m - t0)
            s = int(rng.integers(0, N - span + 1))
            pick = s + rng.integers(0, span, size=cnt)
            pick[0] = s
            pick[cnt - 1] = s + span - 1 if cnt > 1 else s
            ids[t0:t0 + cnt] = h[rng.permutation(pick)] if cnt > 2 else h[pick]
        return ids
    if kind == "every_kth":  # ordered, every tile wider than the window
        k = W // T + 1
        return h[np.sort(np.arange(m, dtype=np.int64) * k % N)]
    raise ValueError(kind)


# ---- one haystack and one needle array on the GPU, and calls on them ----
def canary(nbytes):
    return np.full(nbytes, 0xA5, dtype=np.uint8)


class Case:
    def __init__(self, torch, c, tname, hay_raw, ndl_raw, desc, num=None):
        self.torch, self.c, self.tname, self.desc = torch, c, tname, desc
        self.kb, self.kind = util.TYPES[tname][2], util.TYPES[tname][3]
        self.hay_raw, self.ndl_raw = hay_raw, ndl_raw
        self.n, self.m = hay_raw.size // self.kb, ndl_raw.size // self.kb
        self.hbuf, self.hmid = guarded(torch, hay_raw)
        self.nbuf, self.nmid = guarded(torch, ndl_raw)
        self.num = num
        self.numt = None if num is None else torch.tensor([num], dtype=torch.int64, device="cuda")
        self.want = search_reference(hay_raw, ndl_raw, tname, desc, num=num)  # computed once, shared by every call

    def routes(self, rs, presorted):
        T, W = rs.search_caps(self.kb, presorted)
        return tile_routes(self.hay_raw, self.ndl_raw, self.tname, self.desc, T, W, presorted, num=self.num)

    def run(self, rs, ib=8, lower=True, upper=True, presort=False, what=None):
        torch, m = self.torch, self.m
        lo = guarded(torch, canary(m * ib)) if lower else (None, None)
        up = guarded(torch, canary(m * ib)) if upper else (None, None)
        ptr = [(b[0].data_ptr() + 64 if b[0] is not None else 0) for b in (lo, up)]  # (an empty view has no address of its own)
        self.c.search_sorted_device(self.hmid.data_ptr() if self.n else 0, self.n, self.nbuf.data_ptr() + 64, m, self.kb, self.kind, ptr[0], ptr[1],
                                    ib, self.desc, self.numt.data_ptr() if self.numt is not None else 0, rs.SEARCH_PRESORT if presort else 0,
                                    torch.cuda.current_stream().cuda_stream)
        self.c.check()
        if m:
            assert self.c.get_info(rs.INFO_LAST_PASSES) == PATH | (1 if self.n else 0) | (0x100 if presort and self.n else 0)
        tag = (self.tname, self.n, m, what, "desc" if self.desc else "asc", ib, "presort" if presort else "as given")
        idt = "<i4" if ib == 4 else "<i8"
        if lower:
            assert same(lo[0].cpu().numpy(), with_guards(self.want[0].astype(idt)), ("lower",) + tag)
        if upper:
            assert same(up[0].cpu().numpy(), with_guards(self.want[1].astype(idt)), ("upper",) + tag)

    def inputs_unchanged(self):
        assert same(self.hbuf.cpu().numpy(), with_guards(self.hay_raw), ("the haystack", self.tname, self.n))
        assert same(self.nbuf.cpu().numpy(), with_guards(self.ndl_raw), ("the needles", self.tname, self.m))


def needle_counts(nkind, N, ms):
    """The needle counts of a case; the haystack ITSELF (m = N) too where the needles are its members."""
    return list(ms) + ([N] if nkind in ("members", "shuffled") and N > 0 and N not in ms else [])


VARIANTS = [(ib, lower, upper) for ib in (4, 8) for lower, upper in ((True, True), (True, False), (False, True))]


def make_case(torch, ctx, tname, desc, hkind, nkind, N, m, T, W, rng, groups=None):
    h = hay_ids(hkind, N, T, groups)
    q = needle_ids(nkind, h, m, T, W, rng)
    both = keys_from_ids(tname, np.concatenate([h, q]))  # one map for both arrays
    kb = util.TYPES[tname][2]
    hay, ndl = both[:N * kb].reshape(N, kb), both[N * kb:]
    if desc:
        hay = hay[::-1]
    return Case(torch, ctx, tname, np.ascontiguousarray(hay).reshape(-1), ndl.copy(), desc)


def check_named_route(case, rs, hkind, nkind, N, m, T, W):
    """The route a needle kind is named after, where the haystack's shape lets it be reached: -> the name of what was seen."""
    as_given, presorted = case.routes(rs, False), case.routes(rs, True)
    if N == 0:
        assert as_given.all() and presorted.all()  # an empty window
        return None
    if nkind == "members" and hkind != "equal" and m <= N:
        assert as_given.all(), (hkind, N, m)  # every tile in LDS
        return "members: every tile in LDS"
    if nkind == "shuffled" and hkind == "distinct" and N >= 4 * W and m == N:
        assert not as_given[:m // T].any() and presorted.all(), (N, m)  # (every full tile)
        return "shuffled: global as given, LDS after the sort"
    if nkind == "cluster_w" and hkind == "distinct" and N >= W:
        assert as_given.all(), (N, m)
        return "cluster of W: LDS"
    if nkind == "cluster_w1" and hkind == "distinct" and N >= W + 1 and m >= 2:
        assert not as_given[:-1].any() and (m % T == 1 or not as_given[-1]), (N, m)
        return "cluster of W + 1: global"
    if nkind == "every_kth" and hkind == "distinct" and m >= T and m * (W // T + 1) < N:
        assert not as_given[0] and not presorted[0], (N, m)
        return "every k-th: global"
    if hkind == "equal" and N > W and nkind in ("members", "shuffled"):
        assert not as_given.any() and not presorted.any()  # the documented weak spot: one run longer than the window
        return "a long run: global"
    return None


@pytest.mark.parametrize("hkind", HAY_KINDS)
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", ["u32", "i64"])
def test_full_cross(rs, torch, ctx, tname, desc, hkind):
    kb = util.TYPES[tname][2]
    T, W = rs.search_caps(kb)
    rng = np.random.default_rng(kb + 2 * desc + 7 * HAY_KINDS.index(hkind))
    seen, v = set(), 0
    for N in (0, 1, 2, W, W + 1, 4 * W + 5):
        for nkind in NEEDLE_KINDS:
            for m in needle_counts(nkind, N, (1, T, T + 1, 3 * T + 7)):
                case = make_case(torch, ctx, tname, desc, hkind, nkind, N, m, T, W, rng)
                seen.add(check_named_route(case, rs, hkind, nkind, N, m, T, W))
                for presort in (False, True):  # both routes; the index width and the outputs take turns
                    ib, lower, upper = VARIANTS[v % len(VARIANTS)]
                    v += 1
                    case.run(rs, ib, lower, upper, presort, what=(hkind, nkind))
                case.inputs_unchanged()
    want = {"members: every tile in LDS"} if hkind != "equal" else {"a long run: global"}
    if hkind == "distinct":
        want |= {"shuffled: global as given, LDS after the sort", "cluster of W: LDS", "cluster of W + 1: global", "every k-th: global"}
    assert want <= seen, (want - seen)
    assert v >= 2 * len(VARIANTS)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tname", ["u8", "i16", "i32", "f32", "f64", "u128", "i128"])
def test_other_key_types(rs, torch, ctx, tname, desc):
    kb = util.TYPES[tname][2]
    T, W = rs.search_caps(kb)
    groups = {1: 100, 2: 20000}.get(kb)  # (odd ids between them: 2 * groups + 4 ids in all)
    rng = np.random.default_rng(kb + desc)
    seen, v = set(), 0
    for N, m, hkind in ((1, T + 1, "distinct"), (W + 1, T + 1, "distinct"), (4 * W + 5, 3 * T + 7, "distinct"), (4 * W + 5, T, "runs_of_3"),
                        (W, 1, "equal")):
        for nkind in NEEDLE_KINDS:
            for mm in needle_counts(nkind, N, (m,)):
                case = make_case(torch, ctx, tname, desc, hkind, nkind, N, mm, T, W, rng, groups)
                if groups is None:
                    seen.add(check_named_route(case, rs, hkind, nkind, N, mm, T, W))
                else:
                    seen.add(bool(case.routes(rs, False).all()))
                for presort in (False, True):
                    ib, lower, upper = VARIANTS[v % len(VARIANTS)]
                    v += 1
                    case.run(rs, ib, lower, upper, presort, what=(hkind, nkind))
                case.inputs_unchanged()
    if groups is None:
        assert {"members: every tile in LDS", "shuffled: global as given, LDS after the sort", "cluster of W + 1: global"} <= seen, seen
    else:
        assert seen == {True, False}, seen  # both routes were reached


@pytest.mark.parametrize("tname", ["f32", "f64"])
def test_float_specials(rs, torch, ctx, tname):
    """The seven specials as haystack (runs of each) and as needles: seven different keys in the total order on bit patterns."""
    kb = util.TYPES[tname][2]
    T, W = rs.search_caps(kb)
    sp = F32_SPECIALS if kb == 4 else F64_SPECIALS
    rng = np.random.default_rng(3)
    for reps, m in ((1, 7), (3, T + 1), (W // 7 + 1, 3 * T + 7)):
        for desc in (False, True):
            hay = np.repeat(sp[::-1] if desc else sp, reps)
            ndl = sp[rng.integers(0, 7, size=m)]
            ndl[:7] = sp
            case = Case(torch, ctx, tname, hay.view(np.uint8).reshape(-1).copy(), ndl.view(np.uint8).reshape(-1).copy(), desc)
            first = case.want[0][:7].tolist()
            assert first == [(6 - i if desc else i) * reps for i in range(7)]  # -NaN first ... the two NaNs last and apart
            assert (case.want[1] - case.want[0] == reps).all()
            for presort in (False, True):
                case.run(rs, 8, True, True, presort, what=("specials", reps))
                case.run(rs, 4, False, True, presort, what=("specials", reps))
            case.inputs_unchanged()


def test_sorted_num_hides_the_tail(rs, torch, ctx):
    """d_sorted_num smaller than n: behind N the array holds SMALLER keys, which must not be read as data."""
    T, W = rs.search_caps(4)
    rng = np.random.default_rng(11)
    for N, tail in ((0, 5), (1, 1), (W + 1, W), (3 * W, T + 3)):
        h = np.concatenate([hay_ids("runs_of_3", N, T), np.zeros(tail, dtype=np.int64)])
        for nkind, m in (("members", T + 1), ("shuffled", 2 * T + 1), ("absent", 9)):
            q = needle_ids(nkind, h[:N], m, T, W, rng)
            q[0] = 0  # the tail's own key too: nothing orders before it, it is absent from the first N
            both = keys_from_ids("i32", np.concatenate([h, q]))
            case = Case(torch, ctx, "i32", both[:h.size * 4].copy(), both[h.size * 4:].copy(), False, num=N)
            assert case.want[0][0] == 0 and case.want[1][0] == 0
            for presort in (False, True):
                case.run(rs, 8, True, True, presort, what=("num", N, tail))
            case.inputs_unchanged()
    # a count larger than n is cut to n
    h = hay_ids("distinct", 100, T)
    both = keys_from_ids("u32", np.concatenate([h, h[::3]]))
    case = Case(torch, ctx, "u32", both[:400].copy(), both[400:].copy(), False, num=10 ** 12)
    case.run(rs, 4, True, True, False)


@pytest.fixture(scope="module")
def large(torch):
    """N = 2^22 + 3 u64 keys and m = 2^17 + 1 ordered needles, half of them members; the reference computed once."""
    rng = np.random.default_rng(21)
    N, m = (1 << 22) + 3, (1 << 17) + 1
    hay = np.sort(rng.integers(0, 1 << 63, size=N, dtype=np.uint64) << np.uint64(1))
    ndl = np.sort(np.concatenate([hay[rng.integers(0, N, size=m // 2)], rng.integers(0, 1 << 63, size=m - m // 2, dtype=np.uint64) * np.uint64(2) + np.uint64(1)]))
    want = search_reference(hay.view(np.uint8), ndl.view(np.uint8), "u64", False)
    assert np.array_equal(want[0], np.searchsorted(hay, ndl, side="left")) and np.array_equal(want[1], np.searchsorted(hay, ndl, side="right"))
    return hay, ndl, want, rng.permutation(m)


@pytest.mark.parametrize("presort", [False, True])
@pytest.mark.parametrize("order", ["ordered", "shuffled"])
def test_large_pair(rs, torch, ctx, large, order, presort):
    hay, ndl, want, perm = large
    if order == "shuffled":
        ndl, want = ndl[perm], (want[0][perm], want[1][perm])
    h = torch.from_numpy(hay.view(np.int64)).cuda()
    q = torch.from_numpy(ndl.view(np.int64).copy()).cuda()
    lo, lmid = guarded(torch, canary(ndl.size * 8))
    up, umid = guarded(torch, canary(ndl.size * 4))
    ctx.search_sorted_device(h.data_ptr(), hay.size, q.data_ptr(), ndl.size, 8, rs.KEY_UNSIGNED, lmid.data_ptr(), 0, 8, False, 0,
                             rs.SEARCH_PRESORT if presort else 0, torch.cuda.current_stream().cuda_stream)
    ctx.search_sorted_device(h.data_ptr(), hay.size, q.data_ptr(), ndl.size, 8, rs.KEY_UNSIGNED, 0, umid.data_ptr(), 4, False, 0,
                             rs.SEARCH_PRESORT if presort else 0, torch.cuda.current_stream().cuda_stream)
    ctx.check()
    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH | 1 | (0x100 if presort else 0)
    assert same(lo.cpu().numpy(), with_guards(want[0].astype("<i8")), ("lower", order, presort))
    assert same(up.cpu().numpy(), with_guards(want[1].astype("<i4")), ("upper", order, presort))
    assert np.array_equal(h.cpu().numpy(), hay.view(np.int64)) and np.array_equal(q.cpu().numpy(), ndl.view(np.int64))


def test_u8_haystack_past_two_to_the_32(rs, torch, ctx):
    """2^32 + 4099 bytes in 256 filled runs, all 256 values as needles: the counts are the runs' ends.  Only fills and one search."""
    N = (1 << 32) + 4099
    base, extra = divmod(N, 256)
    ends = np.cumsum([base + (1 if v < extra else 0) for v in range(256)], dtype=np.int64)
    starts = np.concatenate([[0], ends[:-1]])
    hay = torch.empty(N, dtype=torch.uint8, device="cuda")
    for v in range(256):
        hay[int(starts[v]):int(ends[v])].fill_(v)
    order = np.random.default_rng(5).permutation(256)
    q = torch.from_numpy(order.astype(np.uint8)).cuda()
    lo, lmid = guarded(torch, canary(256 * 8))
    up, umid = guarded(torch, canary(256 * 8))
    st = torch.cuda.current_stream().cuda_stream
    for presort in (False, True):
        lmid.fill_(0xA5)
        umid.fill_(0xA5)
        ctx.search_sorted_device(hay.data_ptr(), N, q.data_ptr(), 256, 1, rs.KEY_UNSIGNED, lmid.data_ptr(), umid.data_ptr(), 8, False, 0,
                                 rs.SEARCH_PRESORT if presort else 0, st)
        ctx.check()
        assert same(lo.cpu().numpy(), with_guards(starts[order].astype("<i8")), ("lower", presort))
        assert same(up.cpu().numpy(), with_guards(ends[order].astype("<i8")), ("upper", presort))
    with pytest.raises(rs.RsxError) as e:  # 4-byte indices cannot count 2^32 keys
        ctx.search_sorted_device(hay.data_ptr(), N, q.data_ptr(), 256, 1, rs.KEY_UNSIGNED, lmid.data_ptr(), umid.data_ptr(), 4, False, 0, 0, st)
    assert e.value.status == rs._lib.ERR_ARG
    torch.cuda.synchronize()
    assert same(lo.cpu().numpy(), with_guards(starts[order].astype("<i8")), "nothing was written by the refused call")
    with pytest.raises(ValueError, match="int64"):
        rs.radix_searchsorted(hay, q, index_dtype=torch.int32, ctx=ctx)
    del hay


def test_u32_haystack_of_four_gib(rs, torch, ctx):
    """arange(2^30 + 5) as u32: byte offsets past 2^32, 4-byte indices, positions known in closed form."""
    N = (1 << 30) + 5
    hay = torch.arange(N, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(9)
    vals = np.concatenate([np.array([0, 1, (1 << 30) - 1, 1 << 30, N - 1, N, N + 7, (1 << 31) + 3, (1 << 32) - 1], dtype=np.int64),
                           rng.integers(0, 1 << 32, size=2100)])
    q = torch.from_numpy(vals.astype("<u4").view("<i4")).cuda()
    m = vals.size
    wl, wu = np.minimum(vals, N), np.minimum(vals + 1, N)
    st = torch.cuda.current_stream().cuda_stream
    for presort in (False, True):
        lo, lmid = guarded(torch, canary(m * 4))
        up, umid = guarded(torch, canary(m * 4))
        ctx.search_sorted_device(hay.data_ptr(), N, q.data_ptr(), m, 4, rs.KEY_UNSIGNED, lmid.data_ptr(), umid.data_ptr(), 4, False, 0,
                                 rs.SEARCH_PRESORT if presort else 0, st)
        ctx.check()
        assert same(lo.cpu().numpy(), with_guards(wl.astype("<u4")), ("lower", presort))
        assert same(up.cpu().numpy(), with_guards(wu.astype("<u4")), ("upper", presort))
    del hay


def test_an_unsorted_haystack_stays_in_bounds(rs, torch, ctx):
    """The precondition broken: every output still lies in [0, N], the guards hold, nothing faults."""
    rng = np.random.default_rng(13)
    for tname in ("u32", "i64", "u128"):
        kb, kind = util.TYPES[tname][2], util.TYPES[tname][3]
        T, W = rs.search_caps(kb)
        for N, m in ((2, T + 1), (W + 1, T), (4 * W + 5, 3 * T + 7)):
            hay_raw = keys_from_ids(tname, rng.integers(0, 4 * N, size=N))
            ndl_raw = keys_from_ids(tname, rng.integers(0, 4 * N, size=m))
            hbuf, hmid = guarded(torch, hay_raw)
            nbuf, nmid = guarded(torch, ndl_raw)
            for presort in (False, True):
                for ib in (4, 8):
                    desc = ib == 8
                    lo, lmid = guarded(torch, canary(m * ib))
                    up, umid = guarded(torch, canary(m * ib))
                    ctx.search_sorted_device(hmid.data_ptr(), N, nmid.data_ptr(), m, kb, kind, lmid.data_ptr(), umid.data_ptr(), ib, desc, 0,
                                             rs.SEARCH_PRESORT if presort else 0, torch.cuda.current_stream().cuda_stream)
                    ctx.check()
                    idt = torch.int32 if ib == 4 else torch.int64
                    for buf, mid in ((lo, lmid), (up, umid)):
                        got = mid.view(idt)
                        assert int(got.min()) >= 0 and int(got.max()) <= N, (tname, N, m, presort, ib)
                        whole = buf.cpu().numpy()
                        assert (whole[:64] == 0xA5).all() and (whole[-64:] == 0xA5).all()
            assert same(hbuf.cpu().numpy(), with_guards(hay_raw), "the haystack") and same(nbuf.cpu().numpy(), with_guards(ndl_raw), "the needles")


def test_empty_sides(rs, torch, ctx):
    T, W = rs.search_caps(4)
    E = rs._lib
    L, h = ctx._L, ctx._h
    # m == 0: nothing is launched and no pointer is looked at (dangling values here)
    assert L.rsx_search_sorted_device(h, 8, 100, 8, 8, 0, 4, 0, 0, None, None, 8, 0, None) == E.OK
    assert L.rsx_search_sorted_device(h, 8, 100, 8, 8, 0, 4, 0, 0, 8, 8, 8, 1, None) == E.OK
    assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH
    # n == 0: memsets, also with a null haystack
    q = torch.arange(T + 5, dtype=torch.int32, device="cuda")
    for presort in (False, True):
        for ib in (4, 8):
            lo, lmid = guarded(torch, canary((T + 5) * ib))
            ctx.search_sorted_device(0, 0, q.data_ptr(), T + 5, 4, rs.KEY_SIGNED, lmid.data_ptr(), 0, ib, False, 0, rs.SEARCH_PRESORT if presort else 0,
                                     torch.cuda.current_stream().cuda_stream)
            ctx.check()
            assert ctx.get_info(rs.INFO_LAST_PASSES) == PATH
            assert same(lo.cpu().numpy(), with_guards(np.zeros((T + 5) * ib, dtype=np.uint8)), ("n = 0", presort, ib))
    e = torch.zeros(0, dtype=torch.int32, device="cuda")
    assert rs.radix_searchsorted(e, q, ctx=ctx).tolist() == [0] * (T + 5)
    both = rs.radix_searchsorted(q, e.view(0, 3), side="both", ctx=ctx)
    assert both[0].shape == (0, 3) and both[1].shape == (0, 3)


def test_a_side_stream(rs, torch, ctx):
    T, W = rs.search_caps(8)
    rng = np.random.default_rng(17)
    case = make_case(torch, ctx, "i64", True, "runs_of_3", "shuffled", 2 * W + 1, 2 * T + 3, T, W, rng)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for presort in (False, True):
            case.run(rs, 8, True, True, presort, what="side stream")
    s.synchronize()
    case.inputs_unchanged()


def test_capture_and_replay_of_the_as_given_route(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    T, W = rs.search_caps(4)
    N, m = 3 * W + 1, 2 * T + 9
    rng = np.random.default_rng(19)
    hay_np = np.sort(rng.integers(-5000, 5000, size=N)).astype("<i4")
    hay = torch.from_numpy(hay_np).cuda()
    src = torch.zeros(m, dtype=torch.int32, device="cuda")
    q = torch.empty_like(src)
    lower = torch.empty(m, dtype=torch.int32, device="cuda")
    upper = torch.empty(m, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()

    def enqueue():
        c.search_sorted_device(hay.data_ptr(), N, q.data_ptr(), m, 4, rs.KEY_SIGNED, lower.data_ptr(), upper.data_ptr(), 4, False, 0, 0,
                               torch.cuda.current_stream().cuda_stream)

    with torch.cuda.stream(s):
        q.copy_(src)
        enqueue()  # the context's first call, outside the capture
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):  # one linear chain: the copy, then the call's launch
        q.copy_(src)
        enqueue()
    for seed in (1, 2):
        ndl = np.random.default_rng(seed).integers(-6000, 6000, size=m).astype("<i4")
        src.copy_(torch.from_numpy(ndl))
        lower.fill_(-1)
        upper.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        assert np.array_equal(lower.cpu().numpy(), np.searchsorted(hay_np, ndl, side="left"))
        assert np.array_equal(upper.cpu().numpy(), np.searchsorted(hay_np, ndl, side="right"))
    c.close()


def test_unreserved_presort_under_capture_reports_workspace(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    x = torch.randint(0, 2 ** 31 - 1, (1000,), dtype=torch.int32, device="cuda")
    rs.radix_sort(x, ctx=c)  # one ordinary call: the context's error word and self-tests exist
    c.check()
    m = 1 << 16
    q = torch.randint(0, 2 ** 31 - 1, (m,), dtype=torch.int32, device="cuda")
    out = torch.full((m,), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g.capture_begin()
        try:
            c.search_sorted_device(x.data_ptr(), 1000, q.data_ptr(), m, 4, rs.KEY_SIGNED, out.data_ptr(), 0, 8, False, 0, rs.SEARCH_PRESORT,
                                   torch.cuda.current_stream().cuda_stream)
        except rs.RsxError as e:
            err = e
        g.capture_end()
    assert err is not None and err.status == rs._lib.ERR_WORKSPACE, err
    torch.cuda.synchronize()
    assert bool((out == -1).all())  # nothing was enqueued
    c.reserve_search(m, 4)  # with the reserve the same call runs
    c.search_sorted_device(x.data_ptr(), 1000, q.data_ptr(), m, 4, rs.KEY_SIGNED, out.data_ptr(), 0, 8, False, 0, rs.SEARCH_PRESORT,
                           torch.cuda.current_stream().cuda_stream)
    c.check()
    assert torch.equal(out, torch.searchsorted(x, q))
    c.close()


def test_errors(rs, torch, ctx):
    E = rs._lib
    L, h = ctx._L, ctx._h
    buf = torch.full((4 * 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert p % 16 == 0
    ok = dict(hay=p, n=100, num=0, ndl=p + 4096, m=50, kb=4, kind=0, order=0, lo=p + 2 * 4096, up=p + 3 * 4096, ib=8, flags=0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.rsx_search_sorted_device(h, a["hay"] or None, a["n"], a["num"] or None, a["ndl"] or None, a["m"], a["kb"], a["kind"], a["order"],
                                          a["lo"] or None, a["up"] or None, a["ib"], a["flags"], None)

    assert call(kb=3) == E.ERR_ARG                       # key width
    assert call(kb=16, kind=2) == E.ERR_ARG              # float keys of 16 bytes
    assert call(order=2) == E.ERR_ARG
    assert call(ib=2) == E.ERR_ARG
    assert call(flags=2) == E.ERR_ARG and call(flags=3) == E.ERR_ARG   # unknown flag bits
    assert call(lo=0, up=0) == E.ERR_ARG                 # both outputs null
    assert call(hay=0) == E.ERR_ARG and call(ndl=0) == E.ERR_ARG       # null inputs
    assert call(hay=p + 2) == E.ERR_ARG and call(ndl=p + 4096 + 2) == E.ERR_ARG       # misaligned, each pointer in turn
    assert call(lo=p + 2 * 4096 + 4) == E.ERR_ARG and call(up=p + 3 * 4096 + 4) == E.ERR_ARG
    assert call(num=p + 4) == E.ERR_ARG
    assert call(n=2 ** 32, ib=4) == E.ERR_ARG            # 4-byte indices cannot count them
    assert call(m=2 ** 32, flags=1) == E.ERR_UNSUPPORTED
    assert L.rsx_ctx_reserve_search(h, 2 ** 32, 4) == E.ERR_UNSUPPORTED
    assert L.rsx_ctx_reserve_search(h, 100, 3) == E.ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf[2 * 4096:] == 0xA5).all())          # no refused call wrote
    assert call(lo=p + 2 * 4096 + 4, ib=4, up=0) == E.OK  # aligned to the index width is enough
    assert call(up=0) == E.OK and call(lo=0, flags=1) == E.OK
    ctx.check()


@pytest.mark.parametrize("tname", ["i32", "i64", "f32"])
def test_radix_searchsorted_equals_torch_searchsorted(rs, torch, ctx, tname):
    """Integer dtypes, and floats without NaN or -0.0 (where the two orders agree)."""
    dt = key_dtype(torch, tname)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    for n, shape, span in ((1, (5,), 3), (1000, (7, 11), 50), (20011, (3, 5, 301), 3000)):
        hay = torch.randint(-span, span, (n,), device="cuda", generator=gen).to(dt)
        q = torch.randint(-span - 2, span + 2, shape, device="cuda", generator=gen).to(dt)
        if dt.is_floating_point:
            hay, q = hay * 0.5 + 0.25, q * 0.5 + 0.25  # (no -0.0)
        hay = torch.sort(hay).values
        for presort in (None, False, True):
            left = rs.radix_searchsorted(hay, q, ctx=ctx, presort=presort)
            right = rs.radix_searchsorted(hay, q, side="right", index_dtype=torch.int32, ctx=ctx, presort=presort)
            ctx.check()
            assert left.dtype == torch.int64 and left.shape == q.shape and torch.equal(left, torch.searchsorted(hay, q))
            assert right.dtype == torch.int32 and torch.equal(right, torch.searchsorted(hay, q, right=True, out_int32=True))
        out = torch.full(shape, -1, dtype=torch.int32, device="cuda")
        assert rs.radix_searchsorted(hay, q, side="right", out=out, ctx=ctx) is out
        assert torch.equal(out, right)
        pair = (torch.empty(shape, dtype=torch.int64, device="cuda"), torch.empty(shape, dtype=torch.int64, device="cuda"))
        got = rs.radix_searchsorted(hay, q, side="both", out=pair, ctx=ctx)
        assert got[0] is pair[0] and got[1] is pair[1] and torch.equal(pair[0], left) and torch.equal(pair[1], right.long())
        desc = hay.flip(0).contiguous()
        lo_d, up_d = rs.radix_searchsorted(desc, q, side="both", descending=True, ctx=ctx)
        assert torch.equal(lo_d, n - right.long()) and torch.equal(up_d, n - left)
    with pytest.raises(ValueError, match="same device"):
        rs.radix_searchsorted(hay, q.cpu(), ctx=ctx)


def test_bucketize_and_128_bit_keys(rs, torch, ctx):
    edges = torch.tensor([0.0, 1.0, 2.5, 10.0], device="cuda")
    x = torch.tensor([[-1.0, 0.0, 0.5], [2.5, 9.0, 11.0]], device="cuda")
    assert torch.equal(rs.radix_searchsorted(edges, x, side="right", ctx=ctx), torch.bucketize(x, edges, right=True))
    n, m = 3000, 700
    raw = util.make_input("i128", n, "two", seed=4)
    ndl = np.concatenate([raw[:16 * (m - 2)], util.make_input("i128", 2, "uniform", seed=5)])
    from pairs_ref import pairs_reference
    hay = pairs_reference(raw, None, 16, util.SIGNED, 0, True)[0]
    want = search_reference(hay, ndl, "i128", True)
    got = rs.radix_searchsorted(torch.from_numpy(hay.copy()).cuda().view(n, 16), torch.from_numpy(ndl.copy()).cuda().view(m // 7, 7, 16), side="both",
                                descending=True, ctx=ctx, key_kind=rs.KEY_SIGNED)
    ctx.check()
    assert got[0].shape == (m // 7, 7)
    assert np.array_equal(got[0].cpu().numpy().reshape(-1), want[0]) and np.array_equal(got[1].cpu().numpy().reshape(-1), want[1])


def test_the_join_probe_of_two_groups(rs, torch, ctx):
    """README: lo, hi = radix_searchsorted(gb.keys, ga.keys, side="both", sorted_num=gb.num) over two radix_group results;
    behind gb.num the key array is unwritten memory, which the device-side count keeps out of the search."""
    rng = np.random.default_rng(23)
    a = rng.integers(-400, 400, size=30011).astype("<i4")
    b = rng.integers(-300, 500, size=20021).astype("<i4")
    ga = rs.radix_group(torch.from_numpy(a).cuda(), ctx=ctx)
    gb = rs.radix_group(torch.from_numpy(b).cuda(), ctx=ctx)
    gb.keys[int(gb.num):] = -2 ** 31  # (the test's canary tail: smaller than every key)
    lo, hi = rs.radix_searchsorted(gb.keys, ga.keys, side="both", sorted_num=gb.num, ctx=ctx)
    ctx.check()
    ma, mb = int(ga.num), int(gb.num)
    ua, ub = np.unique(a), np.unique(b)
    assert ma == ua.size and mb == ub.size
    found = (hi > lo)[:ma].cpu().numpy()
    assert np.array_equal(found, np.isin(ua, ub))
    assert bool(((hi - lo)[:ma] <= 1).all())
    hit = lo[:ma][torch.from_numpy(found).cuda()]
    assert torch.equal(gb.keys[hit], ga.keys[:ma][torch.from_numpy(found).cuda()])
