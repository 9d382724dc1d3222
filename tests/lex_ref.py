"""Reference for the calls on several key columns (rsx_lexsort_device, rsx_sort_columns_device), numpy only; a helper, no
tests.

The permutation both calls promise: column 0 the MOST significant, every column compared by its mapped key
(radix_digits.rs), complemented where that column is descending, rows equal in every column in input order.  Here: the
mapped key bytes of every column as pairs_ref.mapped_columns builds them (it complements for descending), laid side by
side with the least significant column first, and one np.lexsort over the byte columns in that order -- np.lexsort is
stable and takes its LAST key as the primary one, so the last byte column, the top byte of column 0, decides first.  The
number of byte columns is not capped: this reference knows nothing of rounds or of 16-byte compound keys."""
from __future__ import annotations

import numpy as np

from pairs_ref import mapped_columns


def lex_columns(columns_raw, specs, descending) -> np.ndarray:
    """(n, K) uint8: the mapped key bytes of all columns, the least significant column first, each little-endian."""
    assert len(columns_raw) == len(specs) == len(descending) >= 1
    parts = []
    for raw, (kb, kind), desc in zip(columns_raw, specs, descending):
        parts.append(mapped_columns(np.ascontiguousarray(raw).view(np.uint8).reshape(-1), kb, kind, bool(desc)))
    n = parts[0].shape[0]
    assert all(p.shape[0] == n for p in parts), "columns of different lengths"
    return np.concatenate(parts[::-1], axis=1) if n else np.zeros((0, sum(kb for kb, _ in specs)), dtype=np.uint8)


def lex_reference(columns_raw, specs, descending) -> np.ndarray:
    """-> perm (int64): perm[t] = the input row that stands at place t.  columns_raw: per column the raw little-endian key
    bytes (any array; viewed as uint8); specs: per column (key_bytes, key_kind); descending: per column a bool."""
    cols = lex_columns(columns_raw, specs, descending)
    n, k = cols.shape
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    return np.lexsort(tuple(cols[:, b] for b in range(k))).astype(np.int64)


def columns_reference(columns_raw, specs, descending, values_raw=None, value_bytes=0):
    """-> (the bytes of every column after rsx_sort_columns_device, the value bytes or None, perm)."""
    perm = lex_reference(columns_raw, specs, descending)
    n = perm.size
    cols = [np.ascontiguousarray(raw).view(np.uint8).reshape(n, kb)[perm].reshape(-1).copy() for raw, (kb, _kind) in zip(columns_raw, specs)]
    vals = None
    if value_bytes:
        vals = np.ascontiguousarray(values_raw).view(np.uint8).reshape(n, value_bytes)[perm].reshape(-1).copy()
    return cols, vals, perm
