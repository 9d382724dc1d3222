"""GPU: rsx_bucket16_direct_kernel -- the hybrid's buckets of key-only elements sorted by one unstable counting pass and a
rank among neighbours -- bit for bit against the CPU oracle, and what it hands over to the stable passes against numpy.

As in test_gpu_bucket_finish.py a few dozen values of the window (the key's top 16 bits, or the 16 bits below the top of a
narrow range) hold thousands of keys each, `grid` apart, so that every form runs and every workgroup has a chain of
buckets.  Groups of small buckets are switched off (they stay with the old kernel): the verdict is then the smallest plain
form that holds all but eight buckets.  Every input's bucket sizes, and the form they lead to, are checked with numpy."""
import numpy as np
import pytest

import bucket_direct_ref as ref
import util

pytestmark = pytest.mark.gpu

CAPE = {8: 1024 * 17, 16: 1024 * 7}  # the 1024-thread form (cape()); the 512-thread form: half, the 256-thread one: a quarter
PER_CU = {1024: 1, 512: 2, 256: 3}
NONE = (1 << 64) - 1  # INFO_LAST_DIRECT: no direct kernel was enqueued
KEY_ONLY = ["u64", "i64", "f64", "u128"]


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
def num_cu(torch):
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


# ---- inputs: mapped keys as (window, low, ext) -- low: the b_lo bits below the window (< 2^48), ext: 64 bits below those (u128)
def _raw(t, window, low, ext, range_bits):
    """Raw element bytes of the keys whose MAPPED form is window << b_lo | low (8 bytes), or that << 64 | ext (u128)."""
    es, _ko, _kb, kind = util.TYPES[t]
    m = (window.astype(np.uint64) << np.uint64(range_bits - 16)) | low
    if kind == util.SIGNED:
        m = m ^ np.uint64(1 << 63)
    elif kind == util.FLOAT:  # mapped: negative -> all bits flipped, else the sign bit set
        m = np.where(m >> np.uint64(63) != 0, m ^ np.uint64(1 << 63), ~m)
    if es == 8:
        return m.astype("<u8").view(np.uint8).reshape(-1, 8)
    return np.stack([ext.astype("<u8"), m.astype("<u8")], axis=1).view(np.uint8).reshape(-1, 16)


def _uniform(rng, m, b_lo=48):
    low = rng.integers(0, 1 << b_lo, size=m, dtype=np.uint64)
    ext = rng.integers(0, 1 << 63, size=m, dtype=np.uint64)
    if m >= 200:  # keys that agree on `low` and differ below it (u128: the low dwords decide), and a few equal keys
        low[1:m:50] = low[0:m - 1:50]
        low[2:m:100] = low[0:m - 2:100]
        ext[2:m:100] = ext[0:m - 2:100]
    return low, ext


def _runs(rng, B, lengths, b_lo=48):
    """Runs of equal keys of the given lengths, every run in a sub-bucket of its own."""
    k = len(lengths)
    dig = rng.permutation(1 << B)[:k].astype(np.uint64)
    val = (dig << np.uint64(b_lo - B)) | rng.integers(0, 1 << (b_lo - B), size=k, dtype=np.uint64)
    return np.repeat(val, lengths), np.repeat(rng.integers(0, 1 << 63, size=k, dtype=np.uint64), lengths)


def _one_digit(rng, B, m, b_lo=48):
    """m DISTINCT keys that share the digit bits."""
    low = (np.uint64(rng.integers(0, 1 << B)) << np.uint64(b_lo - B)) | rng.permutation(1 << 20)[:m].astype(np.uint64)
    return low, rng.integers(0, 1 << 63, size=m, dtype=np.uint64)


def _with_sub(rng, B, bucket, m, b_lo=48):
    """The bucket with ONE sub-bucket of exactly m distinct keys (what it held of that digit is taken out)."""
    low, ext = _one_digit(rng, B, m, b_lo)
    keep = ref.digits(bucket[0], b_lo, B) != ref.digits(low[:1], b_lo, B)[0]
    return np.concatenate([bucket[0][keep], low]), np.concatenate([bucket[1][keep], ext])


def _assemble(t, form, num_cu, chains, range_bits=64, seed=0):
    """chains: {base window value: [(low, ext), ...]} -- bucket k of a chain has window value base + k * grid.
    -> raw bytes (a seeded random order), the form the device will pick, and what the direct kernel hands over."""
    es = util.TYPES[t][0]
    grid = num_cu * PER_CU[form]
    B, b_lo = ref.BITS[form], range_bits - 16
    cape = CAPE[es] * form // 1024
    counts = np.zeros(65536, dtype=np.int64)
    largest = np.zeros(65536, dtype=np.int64)
    win, lows, exts = [], [], []
    for base, buckets in chains.items():
        for k, (low, ext) in enumerate(buckets):
            w = base + k * grid
            assert w < 65536 and counts[w] == 0
            assert len(low) == 0 or int(low.max()) < 1 << b_lo
            counts[w] = len(low)
            largest[w] = ref.largest_sub_bucket(low, b_lo, B)
            win.append(np.full(len(low), w, dtype=np.uint64))
            lows.append(low)
            exts.append(ext)
    win, lows, exts = np.concatenate(win), np.concatenate(lows), np.concatenate(exts)
    n = len(win)
    assert 65536 <= n < 1_100_000, n
    assert np.count_nonzero(counts[:32768]) and np.count_nonzero(counts[32768:])  # the window is the range's top 16 bits
    # the verdict: the smallest form that holds all but eight buckets; above that form's workgroup: the medium kernel's
    above = lambda f: int(np.count_nonzero(counts > CAPE[es] * f // 1024))
    picked = 256 if above(256) <= 8 else 512 if above(512) <= 8 else 1024
    assert picked == form, (t, form, picked, above(256), above(512), above(1024))
    perm = np.random.default_rng(seed).permutation(n)
    raw = _raw(t, win[perm], lows[perm], exts[perm], range_bits).reshape(-1)
    left = ref.handed_over(counts, largest, cape, grid, everything=b_lo == 0)
    return raw, left


def _filler(rng, form, es, how_many, b_lo=48):
    """Uniform buckets above the next smaller form's workgroup (they decide the form), below this one's."""
    cape = CAPE[es] * form // 1024
    return [_uniform(rng, int(rng.integers(cape // 2 + 50, cape - 50)), b_lo) for _ in range(how_many)]


def _input_sizes(t, form, num_cu):
    """Bucket counts of 1, 2, cape(), cape() - 1, odd and even ones in between (the buckets behind an odd count start at an
    odd element index: the tile's 16-byte words and the bucket's elements are then out of step), uniform keys."""
    es = util.TYPES[t][0]
    cape = CAPE[es] * form // 1024
    rng = np.random.default_rng(3000 + es + form + util.TYPES[t][3])
    per = max(4, -(-70000 // (cape * 3 // 4) // 4))
    chains = {8: [_uniform(rng, m) for m in (1, 2, cape, cape - 1)] + _filler(rng, form, es, per),
              9: _filler(rng, form, es, per + 2), 33000: [_uniform(rng, 3)] + _filler(rng, form, es, per + 2),
              40005: _filler(rng, form, es, per + 2) + [_uniform(rng, 77)]}
    raw, left = _assemble(t, form, num_cu, chains)
    assert left == 0
    return raw, left


def _input_duplicates(t, form, num_cu):
    es = util.TYPES[t][0]
    B = ref.BITS[form]
    rng = np.random.default_rng(4000 + es + form)
    fill = lambda k: _filler(rng, form, es, k)
    runs = lambda: _runs(rng, B, 1 + np.arange(600 * form // 1024 * 8 // es) % ref.LIMIT)
    at_limit = _with_sub(rng, B, fill(1)[0], ref.LIMIT)        # one sub-bucket AT the limit, distinct keys
    over_limit = _with_sub(rng, B, fill(1)[0], ref.LIMIT + 1)  # ... and one above it by one
    assert ref.largest_sub_bucket(at_limit[0], 48, B) == ref.LIMIT and ref.largest_sub_bucket(over_limit[0], 48, B) == ref.LIMIT + 1
    chains = {8: fill(1) + [over_limit] + fill(3),                          # the SECOND bucket: it and the three behind it are left
              9: [runs()] + fill(2) + [runs()],                             # runs of equal keys of 1 .. limit
              700: [_runs(rng, B, [5000 * form // 1024 * 8 // es])] + fill(2),  # one repeated key: left, and the chain with it
              33000: [at_limit, _one_digit(rng, B, ref.LIMIT)] + fill(3),       # all keys share the digit bits: T = limit - 1
              40005: fill(4) + [_one_digit(rng, B, ref.LIMIT + 1)],        # ... one more: left (the chain's last)
              50100: fill(6)}
    raw, left = _assemble(t, form, num_cu, chains)
    assert left == 4 + 3 + 1, left
    return raw, left


def _input_narrow(range_bits, num_cu):
    """u64 keys below 2^range_bits: b_lo = range_bits - 16 bits below the window (40: the digit lies across two dwords;
    8: fewer than B; 0: the window reaches bit 0 and the old kernel's map-back loop is all there is)."""
    rng = np.random.default_rng(5000 + range_bits)
    b_lo = range_bits - 16
    if b_lo == 0:
        w = rng.integers(0, 65536, size=70000)
        raw = _raw("u64", w.astype(np.uint64), np.zeros(70000, dtype=np.uint64), None, 16).reshape(-1)
        return raw, int(np.count_nonzero(np.bincount(w, minlength=65536)))
    form = 1024
    if b_lo == 8:  # 256 values below the window: small buckets go through, the big ones (which decide the form) are left
        small = lambda: _uniform(rng, int(rng.integers(500, 2000)), b_lo)
        chains = {8: [small(), small()] + _filler(rng, form, 8, 3, b_lo), 9: [small()] + _filler(rng, form, 8, 3, b_lo),
                  33000: _filler(rng, form, 8, 4, b_lo) + [small()]}
        raw, left = _assemble("u64", form, num_cu, chains, range_bits)
        assert left == 3 + 3 + 5, left
        return raw, left
    chains = {8: [_uniform(rng, m, b_lo) for m in (1, 2, 12345)] + _filler(rng, form, 8, 3, b_lo), 9: _filler(rng, form, 8, 4, b_lo),
              33000: _filler(rng, form, 8, 4, b_lo)}
    raw, left = _assemble("u64", form, num_cu, chains, range_bits)
    assert left == 0
    return raw, left


def _input_medium(t, num_cu):
    """VERDICT_MEDIUM: three buckets above cape() inside chains of the 1024-thread form."""
    es = util.TYPES[t][0]
    rng = np.random.default_rng(6000 + es)
    cape = CAPE[es]
    chains = {8: _filler(rng, 1024, es, 2) + [_uniform(rng, cape + 37)] + _filler(rng, 1024, es, 2),
              9: [_uniform(rng, cape + 1)] + _filler(rng, 1024, es, 3), 33000: _filler(rng, 1024, es, 4) + [_uniform(rng, 2 * cape)]}
    raw, left = _assemble(t, 1024, num_cu, chains)
    assert left == 3
    return raw, left


_CASES = {}  # name -> (type, input, expected, what the direct kernel leaves): made once, shared, never changed


def _case(orc, key, t, make):
    if key not in _CASES:
        raw, left = make()
        exp = orc.sort_parallel(raw, orc.Layout(*util.TYPES[t]), 8)
        raw.setflags(write=False)
        exp.setflags(write=False)
        _CASES[key] = (raw, exp, left)
    return _CASES[key]


def _sort(rs, torch, t, raw, direct):
    c = rs.Context(torch.cuda.current_device())
    c.set_option(rs.OPT_WIDE_SORT, 2)
    c.set_option(rs.OPT_BUCKET_GROUP, 0)
    c.set_option(rs.OPT_BUCKET_DIRECT, direct)
    x = torch.from_numpy(raw.copy()).cuda()
    rs.radix_sort(x, digits=rs.RadixDigits(*util.TYPES[t]), ctx=c)
    c.check()
    path = (c.get_info(rs.INFO_LAST_PASSES) >> 24) & 15
    info = c.get_info(rs.INFO_LAST_DIRECT)
    got = x.cpu().numpy()
    c.close()
    assert path == 5, (t, path)
    return got, info


def _run(rs, torch, orc, key, t, make):
    raw, exp, left = _case(orc, key, t, make)
    es = util.TYPES[t][0]
    got, info = _sort(rs, torch, t, raw, 1)
    print(key, "n", raw.size // es, "left", info, "expected", left)
    assert np.array_equal(got, exp), (key, int(np.flatnonzero(got != exp)[0]) // es)
    assert info == left, (key, info, left)
    got0, info0 = _sort(rs, torch, t, raw, 0)  # OPT_BUCKET_DIRECT = 0: the same bytes by the stable passes
    assert info0 == NONE and np.array_equal(got0, got), key


@pytest.mark.parametrize("form", [1024, 512, 256])
@pytest.mark.parametrize("t", KEY_ONLY)
def test_every_form_and_bucket_size(rs, torch, orc, num_cu, t, form):
    """u64, i64, f64, u128 in the 1024-, 512- and 256-thread form: buckets of 1, 2, cape(), cape() - 1 keys and random sizes
    in between, chains of them per workgroup; nothing is handed over."""
    _run(rs, torch, orc, ("sizes", t, form), t, lambda: _input_sizes(t, form, num_cu))


@pytest.mark.parametrize("t,form", [("u64", 1024), ("u64", 512), ("u64", 256), ("u128", 1024), ("f64", 512)])
def test_duplicates_and_hand_over(rs, torch, orc, num_cu, t, form):
    """A bucket of one repeated key, runs of equal keys up to the limit, buckets whose keys all share the digit bits (limit
    and limit + 1 of them), a sub-bucket above the limit in the SECOND bucket of a chain: that workgroup's later buckets go
    to the old kernel too, and INFO_LAST_DIRECT is the number handed over."""
    _run(rs, torch, orc, ("dup", t, form), t, lambda: _input_duplicates(t, form, num_cu))


@pytest.mark.parametrize("range_bits", [56, 40, 36, 24, 16])
def test_narrow_ranges(rs, torch, orc, num_cu, range_bits):
    """Keys below 2^56 (the digit lies across two dwords), 2^40 and 2^36 (b_lo 24 and 20), 2^24 (b_lo = 8 < B) and 2^16
    (the window reaches bit 0: everything is left to the old kernel)."""
    _run(rs, torch, orc, ("narrow", range_bits), "u64", lambda: _input_narrow(range_bits, num_cu))


@pytest.mark.parametrize("t", ["u64", "u128"])
def test_buckets_above_the_workgroup(rs, torch, orc, num_cu, t):
    """VERDICT_MEDIUM with a key-only type: the buckets above cape() are left (and counted), the medium kernel takes them."""
    _run(rs, torch, orc, ("medium", t), t, lambda: _input_medium(t, num_cu))


def test_payload_never_takes_the_direct_kernel(rs, torch, orc):
    """(u64,u64), many equal keys, payload = index: the stable result, and no direct kernel enqueued."""
    t = "(u64,u64)"
    rng = np.random.default_rng(7)
    n = 200003
    raw = util.make_input(t, n, "uniform", 7).reshape(n, 16).copy()
    raw[:, 0:6] = rng.integers(0, 3, size=(n, 6), dtype=np.uint8)  # 3^6 values below each window value
    raw = raw.reshape(-1)
    exp = orc.sort_parallel(raw, orc.Layout(*util.TYPES[t]), 8)
    got, info = _sort(rs, torch, t, raw, 1)
    assert info == NONE and np.array_equal(got, exp)


@pytest.mark.parametrize("name", ["1024", "512", "edges"])
@pytest.mark.parametrize("t", ["u64", "u128"])
def test_old_kernel_still_mends_key_only_types(rs, torch, orc, num_cu, t, name):
    """OPT_BUCKET_DIRECT = 0 on the planted pairs and runs of test_gpu_bucket_finish.py: the old kernel's mend stays covered
    for the types that no longer reach it by default."""
    import test_gpu_bucket_finish as fin
    raw, exp = fin._case(orc, t, name, num_cu)
    c = rs.Context(torch.cuda.current_device())
    c.set_option(rs.OPT_WIDE_SORT, 2)
    c.set_option(rs.OPT_BUCKET_DIRECT, 0)
    x = torch.from_numpy(raw.copy()).cuda()
    rs.radix_sort(x, digits=rs.RadixDigits(*util.TYPES[t]), ctx=c)
    c.check()
    info = c.get_info(rs.INFO_LAST_DIRECT)
    got = x.cpu().numpy()
    c.close()
    assert info == NONE and np.array_equal(got, exp), (t, name)


def test_option_default_range_and_info_before_any_sort(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    try:
        assert c.get_info(rs.INFO_LAST_DIRECT) == NONE  # nothing sorted yet
        for bad in (2, 3, 1 << 40):
            with pytest.raises(rs.RsxError):
                c.set_option(rs.OPT_BUCKET_DIRECT, bad)
        # the default is 1: a forced hybrid sort of u64 keys enqueues the direct kernel, which leaves nothing
        c.set_option(rs.OPT_WIDE_SORT, 2)
        c.set_option(rs.OPT_BUCKET_GROUP, 0)  # (where groups of small buckets are on offer the direct kernel is not enqueued)
        x = torch.from_numpy(util.make_input("u64", 100003, "uniform", 3)).cuda()
        rs.radix_sort(x, digits=rs.RadixDigits(*util.TYPES["u64"]), ctx=c)
        c.check()
        assert c.get_info(rs.INFO_LAST_DIRECT) == 0
        c.set_option(rs.OPT_BUCKET_GROUP, 1)
        x = torch.from_numpy(util.make_input("u64", 100003, "uniform", 4)).cuda()
        rs.radix_sort(x, digits=rs.RadixDigits(*util.TYPES["u64"]), ctx=c)
        c.check()
        assert c.get_info(rs.INFO_LAST_DIRECT) == NONE  # groups on offer: the old kernel alone
        # ... and a sort that is no hybrid reports none again
        y = torch.from_numpy(util.make_input("u32", 5000, "uniform", 3)).cuda()
        rs.radix_sort(y, digits=rs.RadixDigits(*util.TYPES["u32"]), ctx=c)
        c.check()
        assert c.get_info(rs.INFO_LAST_DIRECT) == NONE
    finally:
        c.close()
