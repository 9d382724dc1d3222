"""Inputs of test_gpu_bucket_direct_prefetch.py, built without a GPU so that test_bucket_direct_prefetch_inputs.py can check
them with numpy alone.  rsx_bucket16_direct_kernel loads the next bucket of a workgroup's chain while it ranks the current
one; these are the chains on which such a load can go wrong and a load at the top of every trip cannot.  As in
test_gpu_bucket_direct.py (whose helpers these are made from) bucket k of a chain has window value base + k * grid, so ONE
workgroup sorts the chain in order.  A chain is a list of (low, ext); an empty bucket is a pair of empty arrays.

  long / tiny / long   cape(), 1, cape() - 1, 2, cape(), 3, cape() - 1 keys: a register left over from the longer bucket
                       must not be counted with the shorter one.  Three copies at neighbouring window values, a bucket of
                       one key between the first two: every one of those counts then starts once at an even and once at an
                       odd element of the array (16-byte words at 8-byte alignment), which `parities` lets a test check.
  skips                valid, EMPTY, valid, ABOVE cape(), valid, two empty ones, valid, two above cape(), valid; chains whose
                       FIRST bucket is empty / above cape(); a chain of one bucket; a chain whose last bucket is one of the
                       last `grid` of the 65536.
  hand-over            a sub-bucket above the limit in the SECOND bucket of a chain, valid buckets behind it: that bucket had
                       been fetched when the workgroup gives up, it and the ones behind it are left.
"""
import numpy as np

import bucket_direct_ref as ref
import test_gpu_bucket_direct as base
import util

EMPTY = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64))
HEAD = 8  # window value of the first chain: the head of the array


def _cape(t, form):
    return base.CAPE[util.TYPES[t][0]] * form // 1024


def _long_tiny(rng, cape, b_lo):
    return [base._uniform(rng, m, b_lo) for m in (cape, 1, cape - 1, 2, cape, 3, cape - 1)]


def _with_sub(rng, B, bucket, m, b_lo):
    """The bucket with ONE B-bit sub-bucket of exactly m distinct keys (base._with_sub, for any b_lo > B)."""
    w = b_lo - B
    low = (np.uint64(rng.integers(0, 1 << B)) << np.uint64(w)) | rng.permutation(1 << min(w, 20))[:m].astype(np.uint64)
    keep = ref.digits(bucket[0], b_lo, B) != ref.digits(low[:1], b_lo, B)[0]
    return np.concatenate([bucket[0][keep], low]), np.concatenate([bucket[1][keep], rng.integers(0, 1 << 63, size=m, dtype=np.uint64)])


def chains_full(t, form, num_cu, b_lo=48):
    """Every pattern, keys that fill the range (or, b_lo = 24, leave 2^24 values below the window)."""
    es = util.TYPES[t][0]
    cape, grid, B = _cape(t, form), num_cu * base.PER_CU[form], ref.BITS[form]
    rng = np.random.default_rng(12000 + es + form + util.TYPES[t][3] + b_lo)
    fill = lambda: base._filler(rng, form, es, 1, b_lo)[0]
    above = lambda: base._uniform(rng, cape + 37, b_lo)
    over = _with_sub(rng, B, fill(), ref.LIMIT + 1, b_lo)
    assert ref.largest_sub_bucket(over[0], b_lo, B) == ref.LIMIT + 1
    last = 65532 - 2 * grid  # its third bucket is window value 65532: nothing of this workgroup lies behind it
    chains = {HEAD: _long_tiny(rng, cape, b_lo), HEAD + 1: [base._uniform(rng, 1, b_lo) for _ in range(7)],
              HEAD + 2: _long_tiny(rng, cape, b_lo), HEAD + 3: _long_tiny(rng, cape, b_lo),
              HEAD + 4: [fill(), EMPTY, fill(), above(), fill(), EMPTY, EMPTY, fill(), above(), above(), fill()],
              HEAD + 5: [EMPTY, fill(), fill()], HEAD + 6: [above(), fill()], HEAD + 7: [fill()],
              HEAD + 8: [fill(), over, fill(), fill()], last: [fill(), fill(), fill()]}
    left = 3 + 1 + 3  # above cape(): three and one; the hand-over: the bucket and the two behind it
    return chains, left, last


def chains_few_values(num_cu):
    """u64 keys below 2^24 in the 1024-thread form: 256 values below the window, so only buckets of up to about 2000 keys
    stay under the limit.  The first two patterns with such buckets as the long ones; the fillers that decide the form end
    the chains, are handed over (and everything of their workgroup behind them)."""
    form, b_lo = 1024, 8
    cape, grid = _cape("u64", form), num_cu * base.PER_CU[form]
    rng = np.random.default_rng(12500)
    fill = lambda k: base._filler(rng, form, 8, k, b_lo)
    ok = lambda m: base._uniform(rng, m, b_lo)
    above = lambda: ok(cape + 37)
    chains = {HEAD: [ok(m) for m in (2000, 1, 1999, 2, 2000, 3, 1999)] + fill(2), HEAD + 1: [ok(1) for _ in range(7)],
              HEAD + 2: [ok(m) for m in (2000, 1, 1999, 2, 2000, 3, 1999)] + fill(2),
              HEAD + 3: [ok(m) for m in (2000, 1, 1999, 2, 2000, 3, 1999)] + fill(2),
              HEAD + 4: [ok(1500), EMPTY, ok(1800), above(), ok(900), EMPTY, EMPTY, ok(1200), above(), above(), ok(1700)] + fill(2),
              HEAD + 5: [EMPTY, ok(1000), ok(1100)] + fill(1), 40005: [above(), ok(1300)] + fill(1)}
    left = 3 * 2 + (3 + 2) + 1 + (1 + 1)  # per chain: its fillers, and the buckets above cape()
    return chains, left, None


def counts_of(chains, grid):
    counts = np.zeros(65536, dtype=np.int64)
    for b0, buckets in chains.items():
        for k, (low, _ext) in enumerate(buckets):
            counts[b0 + k * grid] = len(low)
    return counts


def parities(chains, grid, sizes):
    """{count: the set of (element offset & 1) at which a bucket of that many keys starts in the sorted array}."""
    counts = counts_of(chains, grid)
    starts = np.concatenate([[0], np.cumsum(counts)])[:-1]
    return {m: {int(s) & 1 for s, c in zip(starts, counts) if c == m} for m in sizes}


# name -> (type, form, range_bits, maker of (chains, left, base window value of the chain that ends the 65536 or None))
CASES = {
    "u64-1024": ("u64", 1024, 64, lambda cu: chains_full("u64", 1024, cu)),
    "u64-512": ("u64", 512, 64, lambda cu: chains_full("u64", 512, cu)),
    "u64-256": ("u64", 256, 64, lambda cu: chains_full("u64", 256, cu)),  # (no pipelined load: the loop around it is the same)
    "f64-1024": ("f64", 1024, 64, lambda cu: chains_full("f64", 1024, cu)),  # the mapped store
    "u128-1024": ("u128", 1024, 64, lambda cu: chains_full("u128", 1024, cu)),  # (no pipelined load either)
    "u64-1024-below-2^40": ("u64", 1024, 40, lambda cu: chains_full("u64", 1024, cu, 24)),
    "u64-1024-below-2^24": ("u64", 1024, 24, chains_few_values),
}

_MADE = {}


def make(name, num_cu):
    """-> (type, form, raw bytes, what the direct kernel hands over, chains, last): made once per name and shared."""
    if (name, num_cu) not in _MADE:
        t, form, range_bits, maker = CASES[name]
        chains, left, last = maker(num_cu)
        raw, handed = base._assemble(t, form, num_cu, chains, range_bits)  # (checks the form the device picks, and n)
        assert handed == left, (name, handed, left)
        raw.setflags(write=False)
        _MADE[(name, num_cu)] = (t, form, raw, left, chains, last)
    return _MADE[(name, num_cu)]
