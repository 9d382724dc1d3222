"""numpy model of ONE bucket in rsx_bucket16_direct_kernel with its counters packed two to a word.

The counting pass takes B + 1 bits below the window (all b_lo of them if there are fewer); counter d is the 16-bit half
d & 1 of word d >> 1 of the 2^B words.  The scan turns counts into starts word by word, as the kernel does, in 32-bit
arithmetic: no half may carry into its neighbour.  A bucket is handed over if and only if a B-BIT sub-bucket exceeds
LIMIT: the two halves of a word together where the keys have more than B bits below the window, a half by itself where
they have not -- which is bucket_direct_ref's rule (`largest_sub_bucket` with B), so that model's `handed_over` holds.
The rank pass is bucket_direct_ref's with one more digit bit, every block's T applied to all its positions at once."""
import numpy as np

import bucket_direct_ref as old

LIMIT = old.LIMIT
BITS = old.BITS                                              # the counter WORDS: 2^B of them
COUNT_BITS = {wg: b + 1 for wg, b in old.BITS.items()}      # the digit of the counting pass
handed_over = old.handed_over


def packed_words(low, b_lo, B):
    """The 2^B counter words after the counting pass (uint32; the word behind the last is the sentinel's)."""
    d = old.digits(low, b_lo, B + 1).astype(np.int64)
    c = np.bincount(d, minlength=2 << B).astype(np.uint32)
    assert len(c) == 2 << B and int(c.max(initial=0)) < 1 << 16
    return c[0::2] | (c[1::2] << np.uint32(16))


def largest_b_bit(words, b_lo, B):
    """What the kernel compares with the limit, from the words alone."""
    lo, hi = words & np.uint32(0xFFFF), words >> np.uint32(16)
    return int((lo + hi).max()) if b_lo > B else int(np.maximum(lo, hi).max())


def packed_scan(words, n):
    """counts -> starts as the kernel does it: every thread four words, word = (w << 16) + base * 0x10001 in uint32
    (base: the keys before the word).  Returns the starts as the uint16 array the kernel reads, sentinel included."""
    pair = ((words & np.uint32(0xFFFF)) + (words >> np.uint32(16))).astype(np.uint64)
    base = np.concatenate([[0], np.cumsum(pair)[:-1]]).astype(np.uint64)
    out = ((words.astype(np.uint64) << np.uint64(16)) + base * np.uint64(0x10001)) & np.uint64(0xFFFFFFFF)
    out = np.concatenate([out.astype(np.uint32), np.array([n], dtype=np.uint32)])  # s_cnt[NB] = n
    return out.view(np.uint16)[:2 * len(words) + 1].astype(np.int64)


def windowed_rank(s, starts, b_lo, bits, block=128):
    """bucket_direct_ref.windowed_rank: the place of every position from T neighbours on either side, T per block."""
    n = len(s)
    d = old.digits(s, b_lo, bits).astype(np.int64)
    pos = np.arange(n)
    need = np.maximum(pos - starts[d], starts[d + 1] - 1 - pos)
    T = np.repeat(np.maximum.reduceat(need, np.arange(0, n, block)), block)[:n]
    rank = pos.copy()
    for k in range(1, int(T.max(initial=0)) + 1):
        p = pos[(T >= k) & (pos >= k)]
        rank[p] -= (s[p - k] > s[p]).astype(np.int64)
        p = pos[(T >= k) & (pos + k < n)]
        rank[p] += (s[p + k] < s[p]).astype(np.int64)
    return rank, int(T.max(initial=0))


def sort_bucket(low, b_lo, B, rng, limit=LIMIT, block=128):
    """The bucket as the direct kernel leaves it, or None where it hands the bucket over."""
    low = np.asarray(low, dtype=np.uint64)
    if len(low) == 0:
        return None
    words = packed_words(low, b_lo, B)
    if largest_b_bit(words, b_lo, B) > limit:
        return None
    s, starts = old.counting_pass(low, b_lo, B + 1, rng)
    bd = min(b_lo, B + 1)
    assert np.array_equal(packed_scan(words, len(low))[:(1 << bd) + 1], starts), "the packed scan gives the starts: no carry between halves"
    rank, T = windowed_rank(s, starts, b_lo, B + 1, block)
    assert T < limit, "a half never exceeds the limit"
    assert np.array_equal(np.sort(rank), np.arange(len(s))), "the ranks are a permutation"
    out = np.empty_like(s)
    out[rank] = s
    return out
