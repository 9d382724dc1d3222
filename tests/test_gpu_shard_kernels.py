"""GPU: the building blocks of the multi-GPU schedules called directly, each against plain CPU code (as
test_gpu_parity.py::test_histogram_and_partition_pass does for the histogram and the partition pass):
rsx_bounds_device, rsx_bounds_ranges_device, rsx_splitter_count_device, rsx_splitter_pick_device,
rsx_partition_count_device, rsx_partition_scatter_device.  The end-to-end sharded sorts reach them with two ranks (one
boundary) and keys of at most 8 bytes; here: many boundaries, 16-byte keys (the high query word, digits 8..15), more
queries than one workgroup, empty and clamped ranges, sub-ranges that do not divide n.  References: mapped keys from
oracle.numpy_mapped_key_columns as python ints + bisect; orc.partition_pass per sub-range.  Exact (==)."""
import bisect
import ctypes

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

U, S, F = util.UNSIGNED, util.SIGNED, util.FLOAT
KERNEL_TYPES = ["u8", "i16", "f32", "u64", "i64", "i128", "(u128,u128)", "(pay64+f64)", "(u64,[u64;2])", "(u32,[u8;8])"]
M64 = (1 << 64) - 1
GUARD = 64


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
    c = rs.Context(torch.cuda.current_device())
    yield c
    c.close()


def _input(lay_or_name, n, dist, seed):
    if isinstance(lay_or_name, str):
        return util.make_input(lay_or_name, n, dist, seed), util.TYPES[lay_or_name]
    return util.make_input_layout(lay_or_name, n, dist, seed), lay_or_name


def _key_ints(orc, raw, lay):
    """Mapped keys of the elements in raw as python ints (unsigned order == sort order)."""
    k = orc.numpy_mapped_key_columns(raw, orc.Layout(*lay))
    return [int.from_bytes(row.tobytes(), "little") for row in k]


def _sorted_with_keys(orc, t, n, dist, seed):
    raw, lay = _input(t, n, dist, seed)
    srt = orc.sort_parallel(raw, orc.Layout(*lay), 4)
    keys = _key_ints(orc, srt, lay)
    assert all(a <= b for a, b in zip(keys, keys[1:]))
    return srt, lay, keys


def _dev_u64(torch, values):
    """python ints (unsigned, < 2^64) -> int64 tensor on the device holding the same bits."""
    a = np.array([v & M64 for v in values], dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64).copy()).cuda()


def _host_u64(t):
    return [int(v) for v in t.cpu().numpy().view(np.uint64)]


def _pairs(keys):
    """128-bit keys -> [lo0, hi0, lo1, hi1, ...]"""
    out = []
    for k in keys:
        out += [k & M64, k >> 64]
    return out


def _query_pool(keys, kb, rng, count):
    top = (1 << (8 * kb)) - 1
    pool = [0, (1 << 128) - 1, top, keys[0], keys[-1], max(keys[0] - 1, 0), min(keys[-1] + 1, (1 << 128) - 1)]
    for i in rng.integers(0, len(keys), size=count):
        k = keys[int(i)]
        pool += [k, max(k - 1, 0), min(k + 1, (1 << 128) - 1)]
    return pool


def _longest_run(keys):
    best, start = (0, 0), 0
    for i in range(1, len(keys) + 1):
        if i == len(keys) or keys[i] != keys[start]:
            if i - start > best[1] - best[0]:
                best = (start, i)
            start = i
    return best


@pytest.mark.parametrize("t", KERNEL_TYPES)
def test_bounds_whole_array(rs, torch, ctx, orc, t):
    d = rs.RadixDigits(*util.TYPES[t])
    n = 100003
    for si, dist in enumerate(("two", "step16", "zipf", "uniform")):
        srt, lay, keys = _sorted_with_keys(orc, t, n, dist, seed=70 + si)
        x = torch.from_numpy(srt).cuda()
        rng = np.random.default_rng(700 + si)
        pool = _query_pool(keys, lay[2], rng, 400)
        for nq in (1, 256, 257, 1000):
            qs = pool[:nq] if nq >= 7 else [keys[n // 2]]
            qs = qs + [pool[int(i)] for i in rng.integers(0, len(pool), size=nq - len(qs))]
            dq = _dev_u64(torch, _pairs(qs))
            out = torch.full((2 * nq,), -1, dtype=torch.int64, device="cuda")
            ctx.bounds_device(x.data_ptr(), n, d, dq.data_ptr(), nq, out.data_ptr())
            ctx.check()
            got = _host_u64(out)
            assert got[:nq] == [bisect.bisect_left(keys, q) for q in qs], (t, dist, nq, "keys below")
            assert got[nq:] == [bisect.bisect_right(keys, q) for q in qs], (t, dist, nq, "keys at or below")


def _random_ranges(keys, n, nr, rng):
    """nr ranges (beg, end) as the callers may pass them: proper, empty, reversed, clamped, inside a run of equal keys."""
    r0, r1 = _longest_run(keys)
    special = [(0, n), (0, 0), (n, n), (5, 5), (n // 2, n // 3), (n, 0), (n - 7, n + 12345), (0, 1 << 40), (n, n + 1),
               (n + 5, n + 9), (r0, r1), (r0 + (r1 - r0) // 4, r1 - (r1 - r0) // 4), (n - 1, n), (0, 1)]
    out = special[:nr]
    while len(out) < nr:
        a, b = sorted(int(v) for v in rng.integers(0, n + 1, size=2))
        out.append((a, b))
    return out


def _clamp(beg, end, n):
    e = min(end, n)
    return min(beg, e), e


@pytest.mark.parametrize("t", KERNEL_TYPES)
def test_bounds_with_ranges(rs, torch, ctx, orc, t):
    """out[qi] = keys of the range below the query, out[nq + qi] = at or below, both relative to the range's start;
    beg > end answers 0 and 0; end > n is clamped to n."""
    d = rs.RadixDigits(*util.TYPES[t])
    n = 100003
    for si, dist in enumerate(("two", "zipf", "uniform")):
        srt, lay, keys = _sorted_with_keys(orc, t, n, dist, seed=80 + si)
        x = torch.from_numpy(srt).cuda()
        rng = np.random.default_rng(800 + si)
        pool = _query_pool(keys, lay[2], rng, 400)
        for nq in (1, 256, 257, 1000):
            ranges = _random_ranges(keys, n, nq, rng) if nq > 1 else [(n // 4, n // 2)]
            qs = []
            for (b, e) in ranges:  # half of the queries from inside their own range, the rest from the pool
                b2, e2 = _clamp(b, e, n)
                qs.append(keys[int(rng.integers(b2, e2))] if e2 > b2 and rng.random() < 0.5 else pool[int(rng.integers(0, len(pool)))])
            dq = _dev_u64(torch, _pairs(qs))
            dr = _dev_u64(torch, [v for r in ranges for v in r])
            out = torch.full((2 * nq,), -1, dtype=torch.int64, device="cuda")
            ctx.bounds_ranges_device(x.data_ptr(), n, d, dq.data_ptr(), dr.data_ptr(), nq, out.data_ptr())
            ctx.check()
            got = _host_u64(out)
            for qi, ((b, e), q) in enumerate(zip(ranges, qs)):
                b2, e2 = _clamp(b, e, n)
                want = (bisect.bisect_left(keys, q, b2, e2) - b2, bisect.bisect_right(keys, q, b2, e2) - b2)
                assert (got[qi], got[nq + qi]) == want, (t, dist, nq, qi, (b, e), hex(q))
                if b > e:
                    assert want == (0, 0)


@pytest.mark.parametrize("t", KERNEL_TYPES)
def test_splitter_count_every_digit(rs, torch, ctx, orc, t):
    """less[b * 256 + j] = elements of range b below prefix_b | j << 8 * digit, for 1, 7 and 300 boundaries with ranges
    and prefixes of their own, every digit from the top down."""
    d = rs.RadixDigits(*util.TYPES[t])
    n = 50021
    for si, dist in enumerate(("zipf", "uniform", "two")):
        srt, lay, keys = _sorted_with_keys(orc, t, n, dist, seed=90 + si)
        kb = lay[2]
        x = torch.from_numpy(srt).cuda()
        rng = np.random.default_rng(900 + si)
        for nb in (1, 7, 300):
            ranges = _random_ranges(keys, n, nb, rng)
            dr = _dev_u64(torch, [v for r in ranges for v in r])
            for digit in range(kb - 1, -1, -1):
                low = (1 << (8 * (digit + 1))) - 1
                prefixes = [keys[int(i)] & ~low for i in rng.integers(0, n, size=nb)]  # digits above `digit` of a present key
                dp = _dev_u64(torch, _pairs(prefixes))
                less = torch.full((nb * 256,), -1, dtype=torch.int64, device="cuda")
                ctx.splitter_count_device(x.data_ptr(), n, d, dr.data_ptr(), dp.data_ptr(), nb, digit, less.data_ptr())
                ctx.check()
                got = _host_u64(less)
                for b, ((beg, end), p) in enumerate(zip(ranges, prefixes)):
                    b2, e2 = _clamp(beg, end, n)
                    want = [bisect.bisect_left(keys, p | (j << (8 * digit)), b2, e2) - b2 for j in range(256)]
                    assert got[b * 256:(b + 1) * 256] == want, (t, dist, nb, digit, b, (beg, end), hex(p))
                assert _host_u64(dp) == _pairs(prefixes)  # the count leaves the prefix alone


def _pick_reference(total, rank):
    below = sum(1 for v in total if v <= rank)
    return below - 1 if below else 0


def test_splitter_pick(rs, torch, ctx):
    """prefix |= pick << 8 * digit with pick = the largest j whose total does not exceed the rank, on hand-made
    monotone totals; the prefix word that the digit does not address stays as it was."""
    big = 1 << 40
    step = [j * 10 for j in range(256)]                       # 0, 10, 20, ...
    runs = [(j // 16) * 100 for j in range(256)]              # runs of 16 equal totals
    flat = [0] * 256                                          # everything equal
    late = [0] * 200 + [big + j for j in range(56)]           # a long run of zeros, then values beyond 2^32
    cases = []
    for total in (step, runs, flat, late):
        for rank in (0, 5, 10, 15, total[1], max(total[1] - 1, 0), total[128], total[128] + 1, max(total[255] - 1, 0),
                     total[255], total[255] + 1, big * 4, (1 << 63) + 5, 99, 100, 1500, 1599, 1600):
            cases.append((total, rank))
    nb = len(cases)
    total = _dev_u64(torch, [v for c in cases for v in c[0]])
    rank = _dev_u64(torch, [c[1] for c in cases])
    rng = np.random.default_rng(5)
    for digit in (0, 7, 8, 15, 3, 12):
        word, shift = (0, 8 * digit) if digit < 8 else (1, 8 * (digit - 8))
        before = []
        for b in range(nb):  # digits above `digit` fixed (random), `digit` and below zero, as the search leaves them
            v = int.from_bytes(rng.bytes(16), "little") >> (8 * (digit + 1)) << (8 * (digit + 1))
            before += [v & M64, v >> 64]
        prefix = _dev_u64(torch, before)
        ctx.splitter_pick_device(total.data_ptr(), rank.data_ptr(), prefix.data_ptr(), nb, digit)
        ctx.check()
        got = _host_u64(prefix)
        for b, (tot, r) in enumerate(cases):
            pick = _pick_reference(tot, r)
            want = list(before[2 * b:2 * b + 2])
            want[word] |= pick << shift
            assert got[2 * b:2 * b + 2] == want, (digit, b, r, pick, [hex(v) for v in got[2 * b:2 * b + 2]])
    assert _pick_reference(step, 15) == 1 and _pick_reference(runs, 100) == 31 and _pick_reference(flat, 0) == 255
    assert _pick_reference(late, 5) == 199 and _pick_reference(step, 1 << 63) == 255


@pytest.mark.parametrize("t", KERNEL_TYPES)
@pytest.mark.parametrize("R", [3, 8])
def test_splitter_search_as_the_sharded_sort_drives_it(rs, torch, ctx, orc, t, R):
    """R sorted arrays of unequal lengths (one empty) stand for R ranks.  For a list of global ranks: count on every
    array -> sum over the arrays (the all-reduce) -> pick, digit by digit from the top; the prefix ends as the key at
    that rank of the oracle's sort of the concatenation, and the final bounds cut the arrays so that the cuts add up
    to the rank."""
    lay = util.TYPES[t]
    d = rs.RadixDigits(*lay)
    es, _ko, kb, _kind = lay
    lens = [(7919 * (r + 2)) % 30011 + 100 for r in range(R)]
    lens[1] = 0
    total_n = sum(lens)
    for si, dist in enumerate(("two", "zipf", "uniform")):
        raw, _ = _input(t, total_n, dist, seed=110 + si)
        whole = orc.sort_parallel(raw, orc.Layout(*lay), 4)  # the oracle's sort of the concatenation
        all_keys = _key_ints(orc, whole, lay)
        offs = np.concatenate(([0], np.cumsum(lens))) * es
        parts = [orc.sort_parallel(raw[offs[r]:offs[r + 1]], orc.Layout(*lay), 2) for r in range(R)]
        pkeys = [_key_ints(orc, p, lay) for p in parts]
        xs = [torch.from_numpy(p.copy()).cuda() for p in parts]
        r0, r1 = _longest_run(all_keys)
        ranks = sorted({0, total_n - 1, total_n // 2, r0, (r0 + r1) // 2, r1 - 1, min(r1, total_n - 1), total_n // 3, 1})
        nb = len(ranks)
        drank = _dev_u64(torch, ranks)
        prefix = torch.zeros(2 * nb, dtype=torch.int64, device="cuda")
        dranges = [_dev_u64(torch, [0, lens[r]] * nb) for r in range(R)]
        less = torch.empty(nb * 256, dtype=torch.int64, device="cuda")
        for digit in range(kb - 1, -1, -1):
            summed = torch.zeros(nb * 256, dtype=torch.int64, device="cuda")
            for r in range(R):
                ctx.splitter_count_device(xs[r].data_ptr(), lens[r], d, dranges[r].data_ptr(), prefix.data_ptr(), nb, digit,
                                          less.data_ptr())
                summed += less
            ctx.splitter_pick_device(summed.data_ptr(), drank.data_ptr(), prefix.data_ptr(), nb, digit)
        ctx.check()
        got = _host_u64(prefix)
        found = [got[2 * b] | (got[2 * b + 1] << 64) for b in range(nb)]
        assert found == [all_keys[r] for r in ranks], (t, R, dist)
        below, upto = np.zeros((R, nb), dtype=np.int64), np.zeros((R, nb), dtype=np.int64)
        out = torch.empty(2 * nb, dtype=torch.int64, device="cuda")
        for r in range(R):
            ctx.bounds_ranges_device(xs[r].data_ptr(), lens[r], d, prefix.data_ptr(), dranges[r].data_ptr(), nb, out.data_ptr())
            o = out.cpu().numpy()
            below[r], upto[r] = o[:nb], o[nb:]
            assert list(below[r]) == [bisect.bisect_left(pkeys[r], k) for k in found], (t, R, dist, r)
            assert list(upto[r]) == [bisect.bisect_right(pkeys[r], k) for k in found], (t, R, dist, r)
        for b, rank in enumerate(ranks):  # the cut: everything below the key, then equal keys in rank order
            assert below[:, b].sum() <= rank < upto[:, b].sum(), (t, R, dist, rank)
            left, cuts = rank - int(below[:, b].sum()), []
            for r in range(R):
                take = min(int(upto[r, b] - below[r, b]), left)
                cuts.append(int(below[r, b]) + take)
                left -= take
            assert sum(cuts) == rank and all(0 <= c <= lens[r] for r, c in enumerate(cuts))


def _sub(n, nsub, k):
    return n * k // nsub


def _reference_partition(orc, raw, lay, n, digit, nsub):
    """orc.partition_pass on every sub-range [n k / nsub, n (k+1) / nsub): (bytes, nsub x 256 counts)."""
    es = lay[0]
    out = np.empty_like(raw)
    hist = np.zeros((nsub, 256), dtype=np.uint64)
    L = orc.Layout(*lay)
    for k in range(nsub):
        b, e = _sub(n, nsub, k) * es, _sub(n, nsub, k + 1) * es
        if e > b:
            out[b:e], hist[k] = orc.partition_pass(np.ascontiguousarray(raw[b:e]), L, digit)
    return out, hist


def _guarded(torch, nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


@pytest.mark.parametrize("t", KERNEL_TYPES)
def test_partition_count_and_scatter(rs, torch, ctx, orc, t):
    """nsub sub-ranges of n elements, n not divisible by nsub and n below nsub (empty sub-ranges) included, every digit:
    the nsub x 256 counts and the scattered bytes against the oracle's pass on each sub-range."""
    lay = util.TYPES[t]
    d = rs.RadixDigits(*lay)
    es, _ko, kb, _kind = lay
    for n in (0, 5, 15, 70001, 3000001):
        raw = util.make_input(t, n, "zipf" if n % 2 else "uniform", seed=120 + n % 97)
        src = torch.from_numpy(raw.copy()).cuda()
        for nsub in (1, 2, 3, 7, 16):
            for digit in range(kb):
                want, want_hist = _reference_partition(orc, raw, lay, n, digit, nsub)
                hist = torch.full((nsub * 256,), -1, dtype=torch.int64, device="cuda")
                buf, dst = _guarded(torch, n * es)
                ctx.partition_count_device(src.data_ptr(), n, d, digit, nsub, hist.data_ptr())
                for k in range(nsub):
                    ctx.partition_scatter_device(src.data_ptr(), dst.data_ptr(), n, d, digit, nsub, k)
                ctx.check()
                assert np.array_equal(hist.cpu().numpy().view(np.uint64).reshape(nsub, 256), want_hist), (t, n, nsub, digit)
                got = buf.cpu().numpy()
                assert np.array_equal(got[GUARD:GUARD + n * es], want), (t, n, nsub, digit)
                assert (got[:GUARD] == 0xA5).all() and (got[GUARD + n * es:] == 0xA5).all(), (t, n, nsub, digit)
        assert np.array_equal(src.cpu().numpy(), raw)  # the source is read only


@pytest.mark.parametrize("t", ["u8", "u64", "i128", "(u128,u128)", "(u32,[u8;8])"])
def test_partition_scatter_touches_its_sub_range_only(rs, torch, ctx, orc, t):
    lay = util.TYPES[t]
    d = rs.RadixDigits(*lay)
    es, _ko, kb, _kind = lay
    for n, nsub, some in ((70001, 3, (1,)), (70001, 7, (0, 3, 6)), (70001, 16, (15, 2)), (10, 16, (0, 7, 15)),
                          (300007, 2, (1,))):
        raw = util.make_input(t, n, "uniform", seed=130)
        src = torch.from_numpy(raw.copy()).cuda()
        for digit in (kb - 1, 0):
            want, _ = _reference_partition(orc, raw, lay, n, digit, nsub)
            expect = np.full(n * es + 2 * GUARD, 0xA5, dtype=np.uint8)
            for k in some:
                b, e = _sub(n, nsub, k) * es, _sub(n, nsub, k + 1) * es
                expect[GUARD + b:GUARD + e] = want[b:e]
            hist = torch.zeros(nsub * 256, dtype=torch.int64, device="cuda")
            buf, dst = _guarded(torch, n * es)
            ctx.partition_count_device(src.data_ptr(), n, d, digit, nsub, hist.data_ptr())
            for k in some:
                ctx.partition_scatter_device(src.data_ptr(), dst.data_ptr(), n, d, digit, nsub, k)
            ctx.check()
            assert np.array_equal(buf.cpu().numpy(), expect), (t, n, nsub, some, digit)


@pytest.mark.parametrize("t", ["u64", "(u128,u128)", "f32"])
def test_partition_counts_survive_a_sort_in_between(rs, torch, orc, t):
    """count, then an ordinary sort of another array on the same context, then the scatters: what the overlapped
    schedule does.  The sub-range count matrices are the context's own and the sort must leave them alone."""
    lay = util.TYPES[t]
    d = rs.RadixDigits(*lay)
    es, _ko, kb, _kind = lay
    c = rs.Context(torch.cuda.current_device())
    for n, m, nsub in ((70001, 3000001, 3), (3000001, 70001, 16), (3000001, 5000003, 7), (70001, 1000, 2)):
        raw = util.make_input(t, n, "zipf", seed=140)
        other = util.make_input(t, m, "uniform", seed=141)
        src = torch.from_numpy(raw.copy()).cuda()
        y = torch.from_numpy(other.copy()).cuda()
        digit = kb - 1
        want, want_hist = _reference_partition(orc, raw, lay, n, digit, nsub)
        hist = torch.zeros(nsub * 256, dtype=torch.int64, device="cuda")
        buf, dst = _guarded(torch, n * es)
        c.partition_count_device(src.data_ptr(), n, d, digit, nsub, hist.data_ptr())
        rs.radix_sort(y, digits=d, ctx=c)
        for k in range(nsub - 1, -1, -1):
            c.partition_scatter_device(src.data_ptr(), dst.data_ptr(), n, d, digit, nsub, k)
        c.check()
        assert np.array_equal(y.cpu().numpy(), orc.sort_parallel(other, orc.Layout(*lay), 8)), (t, n, m, "the sort")
        assert np.array_equal(hist.cpu().numpy().view(np.uint64).reshape(nsub, 256), want_hist), (t, n, m)
        got = buf.cpu().numpy()
        assert np.array_equal(got[GUARD:GUARD + n * es], want), (t, n, m, nsub)
        assert (got[:GUARD] == 0xA5).all() and (got[GUARD + n * es:] == 0xA5).all()
    c.close()


def test_partition_sub_range_argument_errors(rs, torch):
    d = rs.PRIMITIVES["u32"]
    n = 1000
    src = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(16 * 256, dtype=torch.int64, device="cuda")
    fresh = rs.Context(torch.cuda.current_device())

    def status(fn, *a):
        with pytest.raises(rs.RsxError) as e:
            fn(*a)
        return e.value.status

    ARG = rs._lib.ERR_ARG
    assert status(fresh.partition_scatter_device, src.data_ptr(), dst.data_ptr(), n, d, 0, 2, 0) == ARG  # no count ran
    for nsub in (0, 17):
        assert status(fresh.partition_count_device, src.data_ptr(), n, d, 0, nsub, hist.data_ptr()) == ARG
        assert status(fresh.partition_scatter_device, src.data_ptr(), dst.data_ptr(), n, d, 0, nsub, 0) == ARG
    assert status(fresh.partition_count_device, src.data_ptr(), n, d, 4, 2, hist.data_ptr()) == ARG  # digit out of range
    assert status(fresh.partition_count_device, src.data_ptr(), n, d, 0, 2, 0) == ARG  # null histogram
    fresh.partition_count_device(src.data_ptr(), n, d, 0, 2, hist.data_ptr())
    assert status(fresh.partition_scatter_device, src.data_ptr(), dst.data_ptr(), n, d, 0, 2, 2) == ARG  # k >= nsub
    assert status(fresh.partition_scatter_device, src.data_ptr(), dst.data_ptr(), n, d, 4, 2, 0) == ARG
    fresh.partition_scatter_device(src.data_ptr(), dst.data_ptr(), n, d, 0, 2, 1)
    fresh.check()
    fresh.close()


def test_bounds_and_splitter_take_any_element_size(rs, torch, ctx, orc):
    """include/rsx.h: the bounds and splitter entry points read the key in place, so they take elements of ANY size
    whose key is 1, 2, 4, 8 or 16 bytes wide; other key widths are refused with RSX_ERR_ARG."""
    for lay in ((40, 0, 8, U), (100, 36, 16, U), (6, 0, 2, U), (13, 5, 4, S)):
        d = rs.RadixDigits(*lay)
        n = 20011
        srt, _, keys = _sorted_with_keys(orc, lay, n, "zipf", seed=150)
        kb = lay[2]
        x = torch.from_numpy(srt).cuda()
        rng = np.random.default_rng(15)
        qs = _query_pool(keys, kb, rng, 100)[:300]
        nq = len(qs)
        ranges = _random_ranges(keys, n, nq, rng)
        dq, dr = _dev_u64(torch, _pairs(qs)), _dev_u64(torch, [v for r in ranges for v in r])
        out = torch.full((2 * nq,), -1, dtype=torch.int64, device="cuda")
        ctx.bounds_device(x.data_ptr(), n, d, dq.data_ptr(), nq, out.data_ptr())
        got = _host_u64(out)
        assert got == [bisect.bisect_left(keys, q) for q in qs] + [bisect.bisect_right(keys, q) for q in qs], lay
        ctx.bounds_ranges_device(x.data_ptr(), n, d, dq.data_ptr(), dr.data_ptr(), nq, out.data_ptr())
        got = _host_u64(out)
        for qi, ((b, e), q) in enumerate(zip(ranges, qs)):
            b2, e2 = _clamp(b, e, n)
            assert (got[qi], got[nq + qi]) == (bisect.bisect_left(keys, q, b2, e2) - b2, bisect.bisect_right(keys, q, b2, e2) - b2), (lay, qi)
        nb = 20
        less = torch.full((nb * 256,), -1, dtype=torch.int64, device="cuda")
        for digit in range(kb - 1, -1, -1):
            low = (1 << (8 * (digit + 1))) - 1
            prefixes = [keys[int(i)] & ~low for i in rng.integers(0, n, size=nb)]
            dp = _dev_u64(torch, _pairs(prefixes))
            ctx.splitter_count_device(x.data_ptr(), n, d, dr.data_ptr(), dp.data_ptr(), nb, digit, less.data_ptr())
            got = _host_u64(less)
            for b, ((beg, end), p) in enumerate(zip(ranges[:nb], prefixes)):
                b2, e2 = _clamp(beg, end, n)
                assert got[b * 256:(b + 1) * 256] == [bisect.bisect_left(keys, p | (j << (8 * digit)), b2, e2) - b2 for j in range(256)], (lay, digit, b)
        ctx.check()
    lib = ctx._L
    x = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    q = torch.zeros(64, dtype=torch.int64, device="cuda")
    for bad in ((8, 0, 6, U), (40, 0, 6, U), (16, 0, 12, S), (8, 0, 3, U)):
        lay = rs._lib.Layout(*bad)
        p = x.data_ptr()
        assert lib.rsx_bounds_device(ctx._h, p, 100, ctypes.byref(lay), q.data_ptr(), 4, q.data_ptr() + 128, None) == rs._lib.ERR_ARG
        assert lib.rsx_bounds_ranges_device(ctx._h, p, 100, ctypes.byref(lay), q.data_ptr(), q.data_ptr(), 4, q.data_ptr() + 128, None) == rs._lib.ERR_ARG
        assert lib.rsx_splitter_count_device(ctx._h, p, 100, ctypes.byref(lay), q.data_ptr(), q.data_ptr(), 1, 0, q.data_ptr(), None) == rs._lib.ERR_ARG
