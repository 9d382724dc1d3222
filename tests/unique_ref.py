"""Reference for rsx_unique_device / radix_group, numpy only; a helper, no tests.

The definition of include/rsx.h: p is the stable permutation by mapped key (pairs_ref.stable_perm of pairs_ref.mapped_columns,
complemented for descending order), s[i] = keys[p[i]], position i is a head when i == 0 or the mapped keys of s[i] and
s[i-1] differ in any byte, h[0] < ... < h[m-1] are the heads and h[m] = n."""
from __future__ import annotations

import numpy as np

from pairs_ref import mapped_columns, stable_perm


def unique_reference(keys_raw, key_bytes: int, kind: int, descending: bool):
    """-> (out_keys, offsets, perm, inverse, m): the m distinct keys as raw bytes (uint8, m * key_bytes), the m + 1 CSR
    offsets of the groups inside perm, the permutation and, per input position, the index of its group (all int64)."""
    keys_raw = np.ascontiguousarray(keys_raw, dtype=np.uint8).reshape(-1)
    n = keys_raw.size // key_bytes
    cols = mapped_columns(keys_raw, key_bytes, kind, descending)
    perm = stable_perm(cols)
    s = cols[perm]
    head = np.ones(n, dtype=bool)
    if n > 1:
        head[1:] = (s[1:] != s[:-1]).any(axis=1)
    heads = np.nonzero(head)[0].astype(np.int64)
    m = int(heads.size)
    offsets = np.concatenate([heads, np.array([n], dtype=np.int64)])
    out_keys = keys_raw.reshape(n, key_bytes)[perm[heads]].reshape(-1).copy()
    inverse = np.empty(n, dtype=np.int64)
    inverse[perm] = np.cumsum(head, dtype=np.int64) - 1
    return out_keys, offsets, perm, inverse, m
