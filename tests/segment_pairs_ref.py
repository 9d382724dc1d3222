"""Reference for the segmented key / value calls (rsx_sort_segments_pairs_device, rsx_argsort_segments_device and their
row forms), numpy only; a helper, no tests.

Every good segment gets what pairs_ref.pairs_reference leaves on that segment alone; a bad segment (begin > end, or
end > n) and everything no segment covers stays as it was.  Index slots no good segment of length >= 1 covers are -1."""
from __future__ import annotations

import numpy as np

from pairs_ref import pairs_reference

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


def with_guards(raw: np.ndarray) -> np.ndarray:
    g = np.full(GUARD, 0xA5, dtype=np.uint8)
    return np.concatenate([g, np.ascontiguousarray(raw).view(np.uint8).reshape(-1), g])


def expected_index(local: np.ndarray, index_bytes: int) -> np.ndarray:
    """The bytes of an index column that held 0xA5 everywhere before the call."""
    dt = "<i4" if index_bytes == 4 else "<i8"
    out = np.full(local.size * index_bytes, 0xA5, dtype=np.uint8).view(dt).copy()
    covered = local >= 0
    out[covered] = local[covered].astype(dt)
    return out.view(np.uint8)
