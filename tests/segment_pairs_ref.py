"""Reference for the segmented key / value calls (rsx_sort_segments_pairs_device, rsx_argsort_segments_device and their
row forms), numpy only; a helper, no tests.

Every good segment gets what pairs_ref.pairs_reference leaves on that segment alone; a bad segment (begin > end, or
end > n) and everything no segment covers stays as it was.  Index slots no good segment of length >= 1 covers are -1.

segments_reference is the reference; segments_reference_fast computes the same for good offsets without a Python loop
and is held equal to it by tests/test_segment_pairs_ref.py."""
from __future__ import annotations

import numpy as np

from pairs_ref import mapped_columns, pairs_reference

GUARD = 64  # bytes of 0xA5 on each side of every array the GPU tests hand to the library


def segments_reference(keys_raw, values_raw, key_bytes: int, kind: int, value_bytes: int, descending: bool, offsets):
    """-> (keys, values, local): the key bytes and value bytes after the call (values None when value_bytes == 0) and,
    per element, its source position INSIDE its segment (int64; -1 where no good segment covers the element)."""
    keys_raw = np.ascontiguousarray(keys_raw, dtype=np.uint8).reshape(-1)
    n = keys_raw.size // key_bytes
    keys = keys_raw.copy()
    values = None
    if value_bytes:
        values_raw = np.ascontiguousarray(values_raw, dtype=np.uint8).reshape(-1)
        values = values_raw.copy()
    local = np.full(n, -1, dtype=np.int64)
    offs = [int(o) for o in offsets]
    for b, e in zip(offs[:-1], offs[1:]):
        if b < 0 or b > e or e > n or e == b:
            continue
        v_in = values_raw[b * value_bytes:e * value_bytes] if value_bytes else None
        k, v, perm = pairs_reference(keys_raw[b * key_bytes:e * key_bytes], v_in, key_bytes, kind, value_bytes, descending)
        keys[b * key_bytes:e * key_bytes] = k
        if value_bytes:
            values[b * value_bytes:e * value_bytes] = v
        local[b:e] = perm
    return keys, values, local


def segments_reference_fast(keys_raw, values_raw, key_bytes: int, kind: int, value_bytes: int, descending: bool, offsets):
    """segments_reference without the Python loop, for calls of many thousand segments: one np.lexsort over (mapped key
    low word, mapped key high word, segment id) of the elements in [offsets[0], offsets[-1]).  lexsort is stable and the
    segment id is the primary key, so every segment keeps its own range and inside it the order is pairs_reference's.

    Only for good offsets: non-decreasing and within [0, n] (anything else raises).  tests/test_segment_pairs_ref.py holds
    the two forms equal on the CPU; a GPU test may use this form only with widths and kinds that test covers."""
    keys_raw = np.ascontiguousarray(keys_raw, dtype=np.uint8).reshape(-1)
    n = keys_raw.size // key_bytes
    offs = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if offs.size < 2 or offs[0] < 0 or offs[-1] > n or np.any(np.diff(offs) < 0):
        raise ValueError("segments_reference_fast takes non-decreasing offsets within [0, n]")
    keys = keys_raw.copy()
    values = None
    if value_bytes:
        values_raw = np.ascontiguousarray(values_raw, dtype=np.uint8).reshape(-1)
        values = values_raw.copy()
    local = np.full(n, -1, dtype=np.int64)
    b0, e0 = int(offs[0]), int(offs[-1])
    m = e0 - b0
    if m == 0:
        return keys, values, local
    cols = mapped_columns(keys_raw[b0 * key_bytes:e0 * key_bytes], key_bytes, kind, descending)
    pad = np.zeros((m, 16), dtype=np.uint8)
    pad[:, :key_bytes] = cols
    lo = np.ascontiguousarray(pad[:, :8]).view("<u8").reshape(m)
    hi = np.ascontiguousarray(pad[:, 8:]).view("<u8").reshape(m)
    # the segment of every covered element: the last i with offsets[i] <= position (empty segments never win)
    sid = np.searchsorted(offs, np.arange(b0, e0, dtype=np.int64), side="right") - 1
    perm = np.lexsort((lo, hi, sid)).astype(np.int64)  # the last key is the primary one
    keys[b0 * key_bytes:e0 * key_bytes] = keys_raw.reshape(n, key_bytes)[b0 + perm].reshape(-1)
    if value_bytes:
        values[b0 * value_bytes:e0 * value_bytes] = values_raw.reshape(n, value_bytes)[b0 + perm].reshape(-1)
    local[b0:e0] = b0 + perm - offs[sid]  # (sid is sorted, so sid[i] is also the segment of OUTPUT position i)
    return keys, values, local


def with_guards(raw: np.ndarray, shift: int = 0) -> np.ndarray:
    """What segment_pairs_gpu.guarded(raw, shift) allocates: GUARD + shift bytes of 0xA5, the array, GUARD bytes."""
    g = np.full(GUARD, 0xA5, dtype=np.uint8)
    return np.concatenate([g, np.full(shift, 0xA5, dtype=np.uint8), np.ascontiguousarray(raw).view(np.uint8).reshape(-1), g])


def expected_index(local: np.ndarray, index_bytes: int) -> np.ndarray:
    """The bytes of an index column that held 0xA5 everywhere before the call."""
    dt = "<i4" if index_bytes == 4 else "<i8"
    out = np.full(local.size * index_bytes, 0xA5, dtype=np.uint8).view(dt).copy()
    covered = local >= 0
    out[covered] = local[covered].astype(dt)
    return out.view(np.uint8)
