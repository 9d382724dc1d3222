"""numpy model of ONE bucket in rsx_bucket16_direct_kernel (key-only elements), and of what that kernel hands over.

A bucket's keys agree on the window and on everything above it; the model takes the b_lo bits below the window as uint64
values.  The counting pass places every key in the sub-bucket of its top B of those bits, in ARBITRARY order inside it
(on the device: the order in which LDS atomics arrive -- here a seeded random one); the rank pass then gives the key at
position i the place  i - #{k < i: s[k] > s[i]} + #{k > i: s[k] < s[i]},  looking T positions to either side only, with T
taken per block of `block` positions from the sub-buckets those positions lie in (the device: per wave and round)."""
import numpy as np

LIMIT = 24  # DIRECT_LIMIT: a bucket with a larger sub-bucket is left to the stable passes
BITS = {1024: 12, 512: 11, 256: 10}  # B by workgroup size


def digits(low, b_lo, B):
    bd = min(b_lo, B)
    return (low >> np.uint64(b_lo - bd)) & np.uint64((1 << bd) - 1)


def largest_sub_bucket(low, b_lo, B):
    return int(np.bincount(digits(low, b_lo, B).astype(np.int64)).max()) if len(low) else 0


def counting_pass(low, b_lo, B, rng):
    """The tile after the counting pass (sub-buckets in digit order, a random order inside each) and the sub-buckets' starts."""
    d = digits(low, b_lo, B).astype(np.int64)
    order = np.lexsort((rng.random(len(low)), d))
    bd = min(b_lo, B)
    starts = np.concatenate([[0], np.cumsum(np.bincount(d, minlength=1 << bd))])
    return low[order], starts


def windowed_rank(s, starts, b_lo, B, block=128):
    """The place of every position of the tile `s`, from T neighbours on either side (T per block of positions)."""
    n = len(s)
    d = digits(s, b_lo, B).astype(np.int64)
    pos = np.arange(n)
    need = np.maximum(pos - starts[d], starts[d + 1] - 1 - pos)
    rank = pos.copy()
    for b0 in range(0, n, block):
        p = pos[b0:b0 + block]
        T = int(need[b0:b0 + block].max())
        for k in range(1, T + 1):
            lo, hi = p - k, p + k
            ok = lo >= 0
            rank[p[ok]] -= (s[lo[ok]] > s[p[ok]]).astype(np.int64)
            ok = hi < n
            rank[p[ok]] += (s[hi[ok]] < s[p[ok]]).astype(np.int64)
    return rank


def sort_bucket(low, b_lo, B, rng, limit=LIMIT, block=128):
    """The bucket as the direct kernel leaves it, or None where it hands the bucket over."""
    low = np.asarray(low, dtype=np.uint64)
    if len(low) == 0 or largest_sub_bucket(low, b_lo, B) > limit:
        return None
    s, starts = counting_pass(low, b_lo, B, rng)
    rank = windowed_rank(s, starts, b_lo, B, block)
    assert np.array_equal(np.sort(rank), np.arange(len(s))), "the ranks are a permutation"
    out = np.empty_like(s)
    out[rank] = s
    return out


def handed_over(counts, largest, cape, grid, everything=False):
    """How many buckets the direct kernel leaves to the kernels behind it: counts[b], largest[b] (its largest sub-bucket)
    for the 65536 buckets, workgroup w of `grid` taking b = w, w + grid, ...; a workgroup that meets a sub-bucket above
    LIMIT leaves that bucket and all its later ones; a bucket above cape() is left wherever it is; empty ones do not count.
    everything: the window reaches bit 0, nothing is the direct kernel's."""
    left = 0
    for w in range(min(grid, 65536)):
        leave = everything
        for b in range(w, 65536, grid):
            if counts[b] == 0:
                continue
            if not leave and counts[b] <= cape and largest[b] > LIMIT:
                leave = True
            if leave or counts[b] > cape:
                left += 1
    return left
