"""GPU: rsx_select_device / radix_select, radix_kthvalue, radix_median, radix_quantile against tests/select_ref.py -- column
r of the full stable sort, byte for byte.

Every comparison is np.array_equal on all bytes of an allocation the test owns: 64 guard bytes of 0xA5, the array, 64
guard bytes -- for out_keys and out_index; the key column is compared with its input afterwards, and ctx.check() runs
after each call.  Sizes come from select_caps: T = tile, B = digit_bits, cap(n) = n // cand_div + cand_floor."""
import numpy as np
import pytest

import util
from pairs_ref import mapped_columns, stable_perm
from segment_pairs_gpu import guarded, key_tensor, same
from segment_pairs_ref import with_guards
from select_ref import quantile_ranks, select_reference

pytestmark = pytest.mark.gpu

KEY_TYPES = ["u8", "i16", "u32", "i32", "f32", "u64", "i64", "f64", "u128"]
PATH = 15 << 24


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


@pytest.fixture(scope="module")
def caps(rs):
    return rs.select_caps(4)  # (max_ranks, digit_bits, tile, cand_div, cand_floor): the same for every width


def levels_of(kb, bits):
    return (8 * kb + bits - 1) // bits


def launches(kb, bits, index):
    """zero + (count, pick) per level + a compact launch behind every level but the last + the index launches or the write"""
    lv = levels_of(kb, bits)
    return 1 + 2 * lv + (lv - 1) + (3 if index else 1)


def index_bytes_of(pos, ib):
    return np.asarray(pos, dtype="<i4" if ib == 4 else "<i8").view(np.uint8).reshape(-1)


class Call:
    """One key column on the GPU (guarded, `shift` bytes behind a 16-byte boundary) and the calls made on it through
    Context.select_device on raw pointers; the stable permutation of each order is computed once."""

    def __init__(self, torch, c, tname, keys_raw, shift=0):
        self.torch, self.c, self.tname = torch, c, tname
        self.kb, self.kind = util.TYPES[tname][2], util.TYPES[tname][3]
        self.keys_raw = np.ascontiguousarray(keys_raw).view(np.uint8).reshape(-1)
        self.n = self.keys_raw.size // self.kb
        self.shift = shift
        self.kbuf, self.kmid = guarded(torch, self.keys_raw, shift)
        self.perm = {}

    def reference(self, ranks, desc):
        if desc not in self.perm:
            self.perm[desc] = stable_perm(mapped_columns(self.keys_raw, self.kb, self.kind, desc))
        pos = self.perm[desc][np.asarray(list(ranks), dtype=np.int64)]
        return self.keys_raw.reshape(self.n, self.kb)[pos].reshape(-1), pos

    def run(self, ranks, desc, ib=8, keys=True, index=True, status=None):
        """-> (out_keys allocation, out_index allocation) as numpy bytes, both pre-filled with 0xA5.  status: the call
        must fail with it (the allocations come back all the same)."""
        torch, m = self.torch, len(ranks)
        obuf, omid = guarded(torch, np.full(m * self.kb, 0xA5, dtype=np.uint8))
        ibuf, imid = guarded(torch, np.full(m * max(ib, 1), 0xA5, dtype=np.uint8))
        args = (self.kmid.data_ptr(), self.n, self.kb, self.kind, list(ranks), omid.data_ptr() if keys else 0, imid.data_ptr() if index else 0,
                ib, desc, torch.cuda.current_stream().cuda_stream)
        if status is None:
            self.c.select_device(*args)
            self.c.check()
        else:
            import radix_sort_amd as rs
            with pytest.raises(rs.RsxError) as e:
                self.c.select_device(*args)
            assert e.value.status == status, e.value
            torch.cuda.synchronize()
        return obuf.cpu().numpy(), ibuf.cpu().numpy()

    def check(self, ranks, desc, ib=8, what=None):
        wk, wi = self.reference(ranks, desc)
        gk, gi = self.run(ranks, desc, ib)
        assert same(gk, with_guards(wk), ("out_keys", self.tname, what, list(ranks), desc))
        assert same(gi, with_guards(index_bytes_of(wi, ib)), ("out_index", self.tname, what, list(ranks), desc, ib))
        return wi

    def keys_unchanged(self):
        assert same(self.kbuf.cpu().numpy(), with_guards(self.keys_raw, self.shift), ("the key column", self.tname))


def info(rs, c):
    """(path bits, compacted, kernels launched, bits 12-23) of RSX_INFO_LAST_PASSES"""
    v = c.get_info(rs.INFO_LAST_PASSES)
    return v & (0xF << 24), (v >> 8) & 0xF, v & 0xFF, (v >> 12) & 0xFFF


def many_ranks(n, m):
    """m ranks below n, out of order and with a repeat"""
    r = [n - 1, 0, n // 2, n // 3, n // 2, (2 * n) // 3, 1 % n, n // 5, n - 1 - n // 7, n // 11, n // 2, n // 13]
    return [r[i % len(r)] for i in range(m)]


def sizes_of(T):
    return [1, 2, 255, T - 1, T, T + 1, 3 * T + 5, (1 << 20) + 3]


@pytest.mark.parametrize("tname", KEY_TYPES)
def test_every_key_type_and_size(rs, torch, ctx, caps, tname):
    """Both orders, both index widths; `two`: every rank falls inside a long run of ties."""
    max_ranks, bits, T, _div, _floor = caps
    kb = util.TYPES[tname][2]
    for n in sizes_of(T):
        for dist in (("uniform", "two") if n <= 3 * T + 5 else ("uniform",)):
            call = Call(torch, ctx, tname, util.make_input(tname, n, dist, seed=11 + n))
            for desc in (False, True):
                for ib in (4, 8):
                    call.check(sorted({0, n - 1, n // 2}), desc, ib, what=(dist, n))
                    path, _compacted, launched, zero = info(rs, ctx)
                    assert path == PATH and launched == launches(kb, bits, True) and zero == 0
                call.check(many_ranks(n, max_ranks), desc, 4 if desc else 8, what=(dist, n, "many"))
            call.keys_unchanged()


@pytest.mark.parametrize("tname", KEY_TYPES)
def test_only_one_output(rs, torch, ctx, caps, tname):
    max_ranks, bits, T, _div, _floor = caps
    kb = util.TYPES[tname][2]
    n = 3 * T + 5
    call = Call(torch, ctx, tname, util.make_input(tname, n, "two", seed=4))
    ranks = many_ranks(n, max_ranks)
    for desc in (False, True):
        wk, wi = call.reference(ranks, desc)
        gk, gi = call.run(ranks, desc, ib=4)
        assert same(gk, with_guards(wk), "both: keys") and same(gi, with_guards(index_bytes_of(wi, 4)), "both: index")
        untouched_k, untouched_i = np.full_like(gk, 0xA5), np.full_like(gi, 0xA5)
        ok, oi = call.run(ranks, desc, ib=4, keys=False)
        assert same(ok, untouched_k, "index only: keys") and same(oi, gi, "index only: index")
        assert info(rs, ctx)[2] == launches(kb, bits, True)
        ok, oi = call.run(ranks, desc, ib=4, index=False)
        assert same(ok, gk, "keys only: keys") and same(oi, untouched_i, "keys only: index")
        assert info(rs, ctx)[2] == launches(kb, bits, False)
        ok, oi = call.run(ranks, desc, ib=0, index=False)  # no index: its width is not looked at
        assert same(ok, gk, "keys only, no index width: keys")
    call.keys_unchanged()


# ---- shapes that pick a route: bits 8-11 of RSX_INFO_LAST_PASSES say after which level the candidates were compacted ----
def _uint_keys(values, kb):
    return np.ascontiguousarray(np.asarray(values, dtype=np.uint64).astype({4: "<u4", 8: "<u8"}[kb])).view(np.uint8)


@pytest.mark.parametrize("tname", ["u32", "i32", "f32", "u64", "f64"])
def test_route_spread(rs, torch, ctx, caps, tname):
    """Keys that differ in the top digit: the gate opens behind level 0."""
    n = (1 << 16) + 7
    call = Call(torch, ctx, tname, util.make_input(tname, n, "uniform", seed=3))
    for desc in (False, True):
        call.check(many_ranks(n, caps[0]), desc)
        assert info(rs, ctx)[:2] == (PATH, 1)
    call.keys_unchanged()


@pytest.mark.parametrize("kb", [4, 8])
def test_route_low(rs, torch, ctx, caps, kb):
    """Keys that differ only in the lowest digit, everything above constant: never compacted.  In the two lowest digits:
    compacted behind the last level but one."""
    max_ranks, bits, T, div, floor = caps
    n = (1 << 16) + 7
    lv = levels_of(kb, bits)
    last_width = 8 * kb - bits * (lv - 1)
    rng = np.random.default_rng(kb)
    top = (0x5A5A5A5A5A5A5A5A >> (64 - 8 * kb)) & ~((1 << (last_width + bits)) - 1)
    tname = {4: "u32", 8: "u64"}[kb]
    low = rng.integers(0, 1 << last_width, size=n, dtype=np.uint64) | np.uint64(top)
    call = Call(torch, ctx, tname, _uint_keys(low, kb))
    for desc in (False, True):
        call.check(many_ranks(n, max_ranks), desc)
        assert info(rs, ctx)[:2] == (PATH, 0)
    call.keys_unchanged()
    low2 = rng.integers(0, 1 << (last_width + bits), size=n, dtype=np.uint64) | np.uint64(top)
    call = Call(torch, ctx, tname, _uint_keys(low2, kb))
    for desc in (False, True):
        call.check(many_ranks(n, max_ranks), desc)
        assert info(rs, ctx)[:2] == (PATH, lv - 1)  # 1 + level lv - 2
    call.keys_unchanged()


@pytest.mark.parametrize("tname", ["u8", "i16", "f32", "i64", "u128"])
def test_route_all_keys_equal(rs, torch, ctx, caps, tname):
    """Never compacted (n candidates at every level); the element at rank r is the one at position r."""
    n = 3 * caps[2] + 5
    call = Call(torch, ctx, tname, util.make_input(tname, n, "equal", seed=8))
    for desc in (False, True):
        ranks = many_ranks(n, caps[0])
        wi = call.check(ranks, desc, ib=4)
        assert wi.tolist() == ranks
        assert info(rs, ctx)[:2] == (PATH, 0)
    call.keys_unchanged()


@pytest.mark.parametrize("tname", ["u32", "f64"])
def test_runs_longer_than_a_tile(rs, torch, ctx, caps, tname):
    """Two values in runs longer than T: the wanted occurrence lies in a later tile than the value's first."""
    T = caps[2]
    kb = util.TYPES[tname][2]
    pats = util.make_input(tname, 2, "uniform", seed=2).reshape(2, kb)
    which = np.concatenate([np.zeros(T + 9, int), np.ones(2 * T + 1, int), np.zeros(T + 3, int), np.ones(5, int), np.zeros(3 * T, int)])
    n = which.size
    call = Call(torch, ctx, tname, pats[which].reshape(-1))
    zeros = int((which == 0).sum())
    for desc in (False, True):
        ranks = [0, T + 8, T + 9, T + 10, zeros - 1, zeros, n - 1, n // 2]
        wi = call.check(ranks, desc)
        assert len({int(p) // T for p in wi}) >= 4  # the answers lie in several tiles
    call.keys_unchanged()


@pytest.mark.parametrize("kb", [4, 8])
def test_route_crowded_bucket_at_the_gate(rs, torch, ctx, caps, kb):
    """A top-digit bucket of exactly cap(n) keys holds the rank: compacted behind level 0.  cap(n) + 1: behind level 1."""
    max_ranks, bits, T, div, floor = caps
    n = 1 << 16
    cap = n // div + floor
    tname = {4: "u32", 8: "u64"}[kb]
    shift = 8 * kb - bits
    rng = np.random.default_rng(5)
    for crowd in (cap, cap + 1):
        vals = rng.integers(0, 1 << shift, size=n, dtype=np.uint64)  # top digit 0 ...
        where = rng.permutation(n)[:crowd]
        vals[where] |= np.uint64(1000 << shift)  # ... and `crowd` keys of top digit 1000, the largest
        call = Call(torch, ctx, tname, _uint_keys(vals, kb))
        call.check([n - 1 - crowd // 2], False)  # inside the crowd
        assert info(rs, ctx)[:2] == (PATH, 1 if crowd == cap else 2), crowd
        call.check([crowd // 2], True)
        assert info(rs, ctx)[:2] == (PATH, 1 if crowd == cap else 2), crowd
        call.check([0, n - 1], False)  # two slots: the other bucket alone is above the capacity
        assert info(rs, ctx)[:2] == (PATH, 2)
        call.keys_unchanged()


def test_route_128_bit_halves(rs, torch, ctx, caps):
    """128-bit keys that differ only in the high half (the gate opens behind level 0) and only in the low half (behind the
    first level that lies wholly inside it)."""
    max_ranks, bits, T, div, floor = caps
    n = 1 << 16
    rng = np.random.default_rng(16)
    half = rng.integers(0, 256, size=(n, 8), dtype=np.uint8)
    const = np.tile(np.arange(1, 9, dtype=np.uint8), (n, 1))
    high = Call(torch, ctx, "u128", np.concatenate([const, half], axis=1).reshape(-1))
    low = Call(torch, ctx, "i128", np.concatenate([half, const], axis=1).reshape(-1))
    first_inside = next(lv for lv in range(levels_of(16, bits)) if 128 - bits * lv <= 64)  # level 6 of 12
    for desc in (False, True):
        high.check(many_ranks(n, max_ranks), desc)
        assert info(rs, ctx)[:2] == (PATH, 1)
        low.check(many_ranks(n, max_ranks), desc)
        assert info(rs, ctx)[:2] == (PATH, 1 + first_inside)
    high.keys_unchanged()
    low.keys_unchanged()


@pytest.mark.parametrize("tname", ["f32", "f64"])
def test_float_specials_and_both_zeros(rs, torch, ctx, caps, tname):
    """-NaN < -inf < negatives < -0 < +0 < positives < +inf < +NaN by bit pattern; every rank of a small array."""
    kb = util.TYPES[tname][2]
    if kb == 4:
        sp = np.array([0x00000000, 0x80000000, 0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x3F800000, 0xBF800000, 0x00000001,
                       0x80000001, 0x7FFFFFFF, 0xFFFFFFFF], dtype="<u4")
    else:
        sp = np.array([0x0, 0x8000000000000000, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                       0x3FF0000000000000, 0xBFF0000000000000, 0x1, 0x8000000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF], dtype="<u8")
    rng = np.random.default_rng(1)
    keys = sp[rng.integers(0, len(sp), size=61)]
    call = Call(torch, ctx, tname, keys.view(np.uint8))
    for desc in (False, True):
        for b in range(0, 61, caps[0]):
            call.check(list(range(b, min(61, b + caps[0]))), desc, ib=4)
    call.keys_unchanged()
    big = np.concatenate([sp[rng.integers(0, 2, size=3 * caps[2])], sp])  # both zeros around the rank, in long runs
    call = Call(torch, ctx, tname, big.view(np.uint8))
    zeros = int((big == sp[1]).sum())  # the negative zeros come first in ascending order
    negatives = 5  # -NaN (two patterns), -inf, -1, the negative denormal
    for desc in (False, True):
        at = negatives + zeros if not desc else big.size - negatives - zeros
        call.check([at - 1, at, at + 1, 0, big.size - 1], desc)
    call.keys_unchanged()


@pytest.mark.parametrize("tname", ["u32", "f32", "u64", "f64"])
def test_keys_one_width_behind_a_16_byte_boundary(rs, torch, ctx, caps, tname):
    """The head and the tail of the 16-byte loads: the key column starts one key behind a 16-byte boundary."""
    kb = util.TYPES[tname][2]
    n = 3 * caps[2] + 5
    for dist in ("uniform", "two"):
        call = Call(torch, ctx, tname, util.make_input(tname, n, dist, seed=6), shift=kb)
        assert call.kmid.data_ptr() % 16 == kb
        for desc in (False, True):
            call.check(many_ranks(n, caps[0]), desc, what=("shifted", dist))
            call.check([0, n - 1], desc, ib=4, what=("shifted", dist))
        call.keys_unchanged()


def test_errors(rs, torch, ctx, caps):
    E = rs._lib
    max_ranks = caps[0]
    call = Call(torch, ctx, "u32", util.make_input("u32", 200, "uniform", seed=2))
    for kwargs, ranks in ((dict(), [200]), (dict(), [0, 1 << 40]), (dict(keys=False, index=False), [5]), (dict(ib=3), [5]),
                          (dict(), list(range(max_ranks + 1)))):
        gk, gi = call.run(ranks, False, status=E.ERR_ARG, **kwargs)
        assert bool((gk == 0xA5).all()) and bool((gi == 0xA5).all())  # nothing was enqueued
    gk, gi = call.run([], False)  # no rank: succeeds, the (empty) outputs' guards intact
    assert bool((gk == 0xA5).all()) and bool((gi == 0xA5).all())
    assert info(rs, ctx) == (PATH, 0, 0, 0)
    L, h = ctx._L, ctx._h
    p = call.kmid.data_ptr()
    import ctypes
    r = (ctypes.c_uint64 * 2)(0, 1)
    assert L.rsx_select_device(h, None, 0, 4, 0, None, 0, None, None, 0, 0, None) == E.OK         # nranks == 0 looks at no pointer
    assert L.rsx_select_device(h, p, 200, 3, 0, r, 2, p, p, 8, 0, None) == E.ERR_ARG              # key width
    assert L.rsx_select_device(h, p, 200, 16, 2, r, 2, p, p, 8, 0, None) == E.ERR_ARG             # float keys of 16 bytes
    assert L.rsx_select_device(h, p, 200, 4, 0, r, 2, p, p, 8, 2, None) == E.ERR_ARG              # order
    assert L.rsx_select_device(h, p + 2, 200, 4, 0, r, 2, p, p, 8, 0, None) == E.ERR_ARG          # misaligned keys
    assert L.rsx_select_device(h, p, 200, 4, 0, r, 2, p, p + 4, 8, 0, None) == E.ERR_ARG          # misaligned index
    assert L.rsx_select_device(h, p, 200, 4, 0, None, 2, p, p, 8, 0, None) == E.ERR_ARG           # no ranks
    assert L.rsx_select_device(h, None, 200, 4, 0, r, 2, p, p, 8, 0, None) == E.ERR_ARG           # no keys
    assert L.rsx_select_device(h, p, 0, 4, 0, r, 2, p, p, 8, 0, None) == E.ERR_ARG                # no rank is below n == 0
    assert L.rsx_select_device(h, p, 1 << 32, 1, 0, r, 2, p, p, 4, 0, None) == E.ERR_UNSUPPORTED  # 4-byte indices of 2^32 keys
    assert L.rsx_ctx_reserve_select(h, 100, 5) == E.ERR_ARG
    torch.cuda.synchronize()
    call.check([5, 0], True)  # the context works on
    call.keys_unchanged()


# ---- the Python calls ----
def _raw(t):
    """the bytes of a tensor of any shape (0-d too)"""
    import torch
    return t.cpu().reshape(-1).view(torch.uint8).numpy()


@pytest.mark.parametrize("tname", ["i16", "f32", "u64", "u128"])
def test_radix_select(rs, torch, ctx, caps, tname):
    """An int gives 0-d results, a sequence 1-D ones; negative ranks count from the end; more than max_ranks go in batches."""
    _es, _ko, kb, kind = util.TYPES[tname]
    n = 2 * caps[2] + 77
    raw = util.make_input(tname, n, "two" if tname == "i16" else "uniform", seed=12)
    _buf, mid = guarded(torch, raw)
    keys = key_tensor(torch, mid, tname)
    for desc in (False, True):
        v = rs.radix_select(keys, -1, descending=desc, ctx=ctx)
        ctx.check()
        wk, wi = select_reference(raw, kb, kind, [n - 1], desc)
        assert v.shape == (() if kb < 16 else (16,)) and v.dtype == keys.dtype and np.array_equal(_raw(v), wk.reshape(-1))
        ranks = [((7919 * i) % (2 * n)) - n for i in range(3 * caps[0] + 1)]  # both signs
        for idt in (None, torch.int32):
            v, i = rs.radix_select(keys, ranks, descending=desc, return_index=True, index_dtype=idt, ctx=ctx)
            ctx.check()
            wk, wi = select_reference(raw, kb, kind, [r % n for r in ranks], desc)
            assert i.dtype == (idt or torch.int64) and i.shape == (len(ranks),) and v.shape[0] == len(ranks)
            assert np.array_equal(i.cpu().numpy().astype(np.int64), wi) and np.array_equal(_raw(v), wk.reshape(-1))
        v, i = rs.radix_select(keys, 3, descending=desc, return_index=True, ctx=ctx)
        ctx.check()
        wk, wi = select_reference(raw, kb, kind, [3], desc)
        assert i.shape == () and int(i) == int(wi[0]) and np.array_equal(_raw(v), wk.reshape(-1))
    v = rs.radix_select(keys, [], ctx=ctx)
    assert v.shape[0] == 0
    assert np.array_equal(mid.cpu().numpy(), raw)


@pytest.mark.parametrize("tname", ["u32", "f32", "i64"])
def test_agreement_with_radix_topk(rs, torch, ctx, tname):
    """The last column of radix_topk(keys, k) of a flat array is radix_select(keys, k - 1, descending=True)."""
    kb = util.TYPES[tname][2]
    n = min(rs.topk_caps(kb)[0][-1], 10007)
    raw = util.make_input(tname, n, "two", seed=21)
    _buf, mid = guarded(torch, raw)
    keys = key_tensor(torch, mid, tname)
    for k in (1, 2, n // 2, n):
        for largest in (True, False):
            tv, ti = rs.radix_topk(keys, k, largest=largest, ctx=ctx)
            sv, si = rs.radix_select(keys, k - 1, descending=largest, return_index=True, ctx=ctx)
            ctx.check()
            assert int(ti[-1]) == int(si) and np.array_equal(_raw(tv[-1]), _raw(sv)), (k, largest)


def test_radix_kthvalue_both_routes(rs, torch, ctx):
    """Short rows through radix_topk, one launch; a row longer than the top-k's largest LDS class through the flat call."""
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    x = torch.randint(-30, 30, (3, 5, 200), dtype=torch.int32, device="cuda", generator=g)
    for largest in (False, True):
        want = torch.sort(x, dim=-1, stable=True, descending=largest)
        for k in (1, 77, 200):
            v, i = rs.radix_kthvalue(x, k, largest=largest, ctx=ctx)
            ctx.check()
            assert (ctx.get_info(rs.INFO_LAST_PASSES) >> 24) & 0xF == 7
            assert v.shape == (3, 5) and i.shape == (3, 5) and i.dtype == torch.int64
            assert torch.equal(v, want.values[..., k - 1]) and torch.equal(i, want.indices[..., k - 1])
    L = rs.topk_caps(4)[0][-1]
    y = torch.randint(-1000, 1000, (2, L + 1), dtype=torch.int32, device="cuda", generator=g)
    for largest in (False, True):
        want = torch.sort(y, dim=-1, stable=True, descending=largest)
        for k in (1, L // 2, L + 1):
            v, i = rs.radix_kthvalue(y, k, largest=largest, index_dtype=torch.int32, ctx=ctx)
            ctx.check()
            assert (ctx.get_info(rs.INFO_LAST_PASSES) >> 24) & 0xF == 15
            assert v.shape == (2,) and i.dtype == torch.int32
            assert torch.equal(v, want.values[..., k - 1]) and torch.equal(i.to(torch.int64), want.indices[..., k - 1])


@pytest.mark.parametrize("tname", ["i32", "f64"])
def test_radix_median_and_quantile(rs, torch, ctx, caps, tname):
    _es, _ko, kb, kind = util.TYPES[tname]
    for n in (1, 2, 1000, 2 * caps[2] + 1):
        raw = util.make_input(tname, n, "uniform", seed=n)
        _buf, mid = guarded(torch, raw)
        keys = key_tensor(torch, mid, tname)
        v, i = rs.radix_median(keys, ctx=ctx)
        ctx.check()
        wk, wi = select_reference(raw, kb, kind, [(n - 1) // 2], False)
        assert int(i) == int(wi[0]) and np.array_equal(_raw(v), wk.reshape(-1))
        q = [0.0, 1.0, 0.5, 0.25, 0.999, 0.3333, 0.75, 0.1, 0.9, 0.0625, 0.51]  # more than max_ranks: in batches
        assert len(q) > caps[0]
        for method in ("lower", "higher", "nearest"):
            got = rs.radix_quantile(keys, q, method=method, ctx=ctx)
            ctx.check()
            wk, _wi = select_reference(raw, kb, kind, quantile_ranks(n, q, method), False)
            assert got.shape == (len(q),) and np.array_equal(_raw(got), wk.reshape(-1)), (n, method)
        one = rs.radix_quantile(keys, 0.5, ctx=ctx)
        ctx.check()
        wk, _wi = select_reference(raw, kb, kind, quantile_ranks(n, [0.5], "lower"), False)
        assert one.shape == () and np.array_equal(_raw(one), wk.reshape(-1))
        assert np.array_equal(mid.cpu().numpy(), raw)


def test_graph_capture(rs, torch, caps):
    """After reserve_select the call allocates nothing: one captured call, replayed twice on changed keys.  Without the
    reserve on a fresh context: RSX_ERR_WORKSPACE, nothing enqueued."""
    n, ranks = 3 * caps[2] + 5, [7, 3 * caps[2], 100, 7]
    s = torch.cuda.Stream()
    keys = torch.zeros(n, dtype=torch.float32, device="cuda")
    values = torch.full((len(ranks),), -1.0, dtype=torch.float32, device="cuda")
    index = torch.full((len(ranks),), -1, dtype=torch.int64, device="cuda")

    def enqueue(c):
        c.select_device(keys.data_ptr(), n, 4, rs.KEY_FLOAT, ranks, values.data_ptr(), index.data_ptr(), 8, True,
                        torch.cuda.current_stream().cuda_stream)

    fresh = rs.Context(torch.cuda.current_device())
    g0 = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g0.capture_begin()
        try:
            enqueue(fresh)
        except rs.RsxError as e:
            err = e
        g0.capture_end()
    assert err is not None and err.status == rs._lib.ERR_WORKSPACE, err
    torch.cuda.synchronize()
    assert bool((index == -1).all()) and bool((values == -1.0).all())  # nothing was enqueued
    fresh.close()

    c = rs.Context(torch.cuda.current_device())
    c.reserve_select(n, 4)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        enqueue(c)
    for seed in (1, 2):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        keys.copy_(torch.randint(-40 * seed, 40 * seed, (n,), device="cuda", generator=g).to(torch.float32))
        index.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        c.check()
        wk, wi = select_reference(keys.cpu().numpy().view(np.uint8), 4, util.FLOAT, ranks, True)
        assert np.array_equal(index.cpu().numpy(), wi) and np.array_equal(values.cpu().numpy().view(np.uint8).reshape(-1), wk.reshape(-1))
        assert c.get_info(rs.INFO_LAST_PASSES) & (0xF << 24) == PATH
    c.close()
