"""Inputs of test_gpu_bucket_direct_packed.py, built without a GPU so that test_bucket_direct_packed_ref.py can put every
bucket of them through the numpy model first.  As in test_gpu_bucket_direct.py (whose helpers these are made from) a few
dozen window values hold buckets of the size that selects the form, `grid` apart; the special buckets sit at the head of
their chains.  A case: {"t", "form", "range_bits", "chains": {base window value: [(low, ext, kind), ...]}, "left"} --
kind: "direct" (the direct kernel sorts it), "over" (a B-bit sub-bucket above the limit: handed over), "behind" (behind
such a bucket in its workgroup's chain: left with it)."""
import numpy as np

import bucket_direct_packed_ref as ref
import test_gpu_bucket_direct as base
import util

LIMIT = ref.LIMIT
FORMS = [1024, 512, 256]


def model_low(es, low, ext, range_bits):
    """What the model is given of a key: the bits below the window that the digit can reach, and how many they are."""
    b = range_bits - 16
    if es == 16 and b < 16:  # u128 keys of a narrow range: the digit reaches into the low eight bytes
        return (low << np.uint64(16)) | (ext >> np.uint64(48)), b + 16
    return low, b


def _ext(rng, m):
    return rng.integers(0, 1 << 63, size=m, dtype=np.uint64)


def _plant(rng, B, bucket, subs, b_lo=48):
    """The bucket with its B-bit sub-buckets `subs` = {digit: (even, odd)} replaced by that many DISTINCT keys in the
    halves of the word: digits 2 * digit and 2 * digit + 1 of the counting pass."""
    low, ext = bucket
    keep = ~np.isin(ref.old.digits(low, b_lo, B), np.array(list(subs), dtype=np.uint64))
    lows, exts = [low[keep]], [ext[keep]]
    w = b_lo - B - 1
    assert w >= 5
    for dig, halves in subs.items():
        for half, m in enumerate(halves):
            lows.append((np.uint64(2 * dig + half) << np.uint64(w)) | rng.permutation(1 << min(w, 20))[:m].astype(np.uint64))
            exts.append(_ext(rng, m))
    return np.concatenate(lows), np.concatenate(exts)


def _digits_apart(rng, B, k):
    """k B-bit digits, none of them first, last or next to another."""
    return [int(v) for v in 2 + 4 * rng.permutation((1 << B) // 4 - 1)[:k]]


def _tag(buckets, kind="direct"):
    return [(low, ext, kind) for low, ext in buckets]


def _per(cape):
    return max(4, -(-70000 // (cape * 3 // 4) // 4))


def case_combined(t, form):
    """Every size and every way two halves share a word, full-range keys of type t in the given form."""
    es = util.TYPES[t][0]
    B, cape = ref.BITS[form], base.CAPE[es] * form // 1024
    rng = np.random.default_rng(8000 + es + form + util.TYPES[t][3])
    fill = lambda k: base._filler(rng, form, es, k)
    per = _per(cape)
    w = 48 - B - 1  # the bits below the extra digit bit
    d = _digits_apart(rng, B, 8)
    halves = _plant(rng, B, fill(1)[0], {d[0]: (12, 12), d[1]: (LIMIT, 0), d[2]: (0, LIMIT), d[3]: (LIMIT - 1, 1)})
    # digits 2k + 1 and 2k + 2 (neighbouring words) with the limit each; digit 0 and the last one crowded to the limit
    ends = _plant(rng, B, fill(1)[0], {d[4]: (0, LIMIT), d[4] + 1: (LIMIT, 0), 0: (LIMIT, 0), (1 << B) - 1: (0, LIMIT)})
    ends2 = _plant(rng, B, fill(1)[0], {0: (0, LIMIT), 1: (LIMIT, 0), (1 << B) - 2: (0, LIMIT), (1 << B) - 1: (LIMIT, 0)})
    one = base._one_digit(rng, B + 1, LIMIT)  # all keys share the B + 1 digit bits: T = limit - 1
    top = ((np.uint64((2 << B) - 1) << np.uint64(w)) | rng.permutation(1 << 20)[:LIMIT].astype(np.uint64), _ext(rng, LIMIT))  # ... the last digit
    zero = (rng.permutation(1 << 20)[:LIMIT].astype(np.uint64), _ext(rng, LIMIT))                                           # ... digit 0
    # keys that differ only in the extra digit bit; keys that differ only below it
    x = base._uniform(rng, cape * 5 // 16)[0] & ~np.uint64(1 << w)
    extra = (np.concatenate([x, x | np.uint64(1 << w)]), np.concatenate([_ext(rng, len(x))] * 2))
    y = base._uniform(rng, cape * 5 // 16)[0]
    below = (np.concatenate([y, y ^ (np.uint64(1) << rng.integers(0, w, size=len(y)).astype(np.uint64))]), np.concatenate([_ext(rng, len(y))] * 2))
    runs = base._runs(rng, B, 1 + np.arange(600 * form // 1024 * 8 // es) % LIMIT)  # equal keys: one half each
    # many empty sub-buckets: keys on every 4th digit of the counting pass only (a wave's positions span many digits)
    z = base._uniform(rng, cape // 3)
    fourth = (z[0] & ~np.uint64(3 << w), z[1])
    over_sum = _plant(rng, B, fill(1)[0], {d[5]: (13, 12)})
    over_half = _plant(rng, B, fill(1)[0], {d[6]: (0, LIMIT + 1)})
    chains = {8: _tag([base._uniform(rng, m) for m in (1, 2, cape, cape - 1, 77)] + fill(per)),
              9: _tag([halves, ends, ends2, one, top, zero] + fill(per)),
              33000: _tag([extra, below, runs, fourth] + fill(per)),
              40005: _tag(fill(2)) + [over_sum + ("over",)] + _tag(fill(2), "behind"),
              50100: _tag(fill(per)) + [over_half + ("over",)]}
    return {"t": t, "form": form, "range_bits": 64, "chains": chains, "left": 3 + 1}


def case_range(form, range_bits):
    """u64 keys below 2^range_bits: where the digit lies in the element, and how many bits there are for it."""
    B, cape = ref.BITS[form], base.CAPE[8] * form // 1024
    b_lo = range_bits - 16
    rng = np.random.default_rng(9000 + form + range_bits)
    fill = lambda k: base._filler(rng, form, 8, k, b_lo)
    per = _per(cape)
    chains = {8: _tag([base._uniform(rng, m, b_lo) for m in (1, 2, 12345 * form // 1024)] + fill(per)), 9: _tag(fill(per + 1)),
              33000: _tag(fill(per + 1)), 40005: _tag(fill(per + 1))}
    left = 0
    if b_lo == B:  # a half is a B-bit sub-bucket by itself: neighbouring values with 20 equal keys each stay, 25 go
        f = fill(2)
        twenty = (np.concatenate([f[0][0][f[0][0] >> np.uint64(1) != np.uint64(100)], np.repeat(np.array([200, 201], dtype=np.uint64), 20)]),)
        twenty += (_ext(rng, len(twenty[0])),)
        over = (np.concatenate([f[1][0][f[1][0] != np.uint64(77)], np.full(LIMIT + 1, 77, dtype=np.uint64)]),)
        over += (_ext(rng, len(over[0])),)
        chains[9] = _tag([twenty]) + chains[9]
        chains[40005] = chains[40005] + [over + ("over",)]
        left = 1
    return {"t": "u64", "form": form, "range_bits": range_bits, "chains": chains, "left": left}


def case_u128_across():
    """u128 keys below 2^88: b_lo = 72, the 13 digit bits are bits 59 .. 71 -- the element's second and third dwords."""
    rng = np.random.default_rng(9900)
    def bucket(m):
        low, _ = base._uniform(rng, m, 8)
        return low, rng.integers(0, 1 << 64, size=m, dtype=np.uint64)
    cape = base.CAPE[16]
    sizes = lambda k: [int(rng.integers(cape // 2 + 50, cape - 50)) for _ in range(k)]
    chains = {8: _tag([bucket(m) for m in [1, 2, cape, cape - 1] + sizes(4)]), 9: _tag([bucket(m) for m in sizes(5)]),
              33000: _tag([bucket(m) for m in [77] + sizes(5)]), 40005: _tag([bucket(m) for m in sizes(5)])}
    return {"t": "u128", "form": 1024, "range_bits": 24, "chains": chains, "left": 0}


# name -> how the case is made.  dshift = b_lo - 13 in the 1024-thread form: 0 (range_bits 29), 15 .. 18, 23 and 31 (52 and
# 60: the digit lies across two dwords), 32 (61), 35 (64: full-range keys).
CASES = {}
for _t in base.KEY_ONLY:
    for _f in FORMS:
        CASES[f"all-{_t}-{_f}"] = (lambda t=_t, f=_f: case_combined(t, f))
for _r in (28, 29, 30, 44, 45, 47, 52, 60, 61, 64):  # (28, 29, 30: b_lo = B, B + 1, B + 2)
    CASES[f"range-1024-{_r}"] = (lambda r=_r: case_range(1024, r))
for _f, _r in ((512, 27), (512, 28), (256, 26), (256, 27)):  # b_lo = B and B + 1 in the smaller forms
    CASES[f"range-{_f}-{_r}"] = (lambda f=_f, r=_r: case_range(f, r))
CASES["u128-across-dwords"] = case_u128_across

_MADE = {}


def make(name):
    """The case, made once and shared."""
    if name not in _MADE:
        _MADE[name] = CASES[name]()
    return _MADE[name]


def assemble(case, num_cu, seed=0):
    """-> raw bytes (a seeded random order) and what the direct kernel hands over; the form the device will pick is checked."""
    t, form, range_bits = case["t"], case["form"], case["range_bits"]
    es = util.TYPES[t][0]
    grid = num_cu * base.PER_CU[form]
    B = ref.BITS[form]
    cape = base.CAPE[es] * form // 1024
    counts = np.zeros(65536, dtype=np.int64)
    largest = np.zeros(65536, dtype=np.int64)
    win, lows, exts = [], [], []
    for b0, buckets in case["chains"].items():
        for k, (low, ext, _kind) in enumerate(buckets):
            w = b0 + k * grid
            assert w < 65536 and counts[w] == 0
            assert int(low.max()) < 1 << (range_bits - 16)
            counts[w] = len(low)
            largest[w] = ref.old.largest_sub_bucket(*model_low(es, low, ext, range_bits), B)
            win.append(np.full(len(low), w, dtype=np.uint64))
            lows.append(low)
            exts.append(ext)
    win, lows, exts = np.concatenate(win), np.concatenate(lows), np.concatenate(exts)
    n = len(win)
    assert 65536 <= n < 1_100_000, n
    assert np.count_nonzero(counts[:32768]) and np.count_nonzero(counts[32768:])  # the window is the range's top 16 bits
    above = lambda f: int(np.count_nonzero(counts > base.CAPE[es] * f // 1024))
    picked = 256 if above(256) <= 8 else 512 if above(512) <= 8 else 1024
    assert picked == form and above(form) == 0, (t, form, picked, above(256), above(512), above(1024))
    perm = np.random.default_rng(seed).permutation(n)
    raw = base._raw(t, win[perm], lows[perm], exts[perm], range_bits).reshape(-1)
    return raw, ref.handed_over(counts, largest, cape, grid)
