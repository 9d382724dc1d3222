"""Reference for the key / value calls (rsx_sort_pairs_device, rsx_argsort_device), numpy only; a helper, no tests.

The order both calls promise is the STABLE permutation by mapped key (radix_digits.rs), ascending, or descending =
larger mapped key first with equal keys still in input order.  Here: the mapped key columns as
oracle.numpy_mapped_key_columns builds them, complemented for descending order, then a stable argsort / lexsort."""
from __future__ import annotations

import numpy as np

from oracle import oracle as _orc  # numpy_mapped_key_columns is numpy alone; the C oracle is not loaded here


def mapped_columns(keys_raw: np.ndarray, key_bytes: int, kind: int, descending: bool) -> np.ndarray:
    """(n, key_bytes) uint8 little-endian: the mapped key, complemented when descending."""
    raw = np.ascontiguousarray(keys_raw, dtype=np.uint8).reshape(-1)
    k = _orc.numpy_mapped_key_columns(raw, _orc.Layout(key_bytes, 0, key_bytes, kind))
    if descending:
        k = k ^ np.uint8(0xFF)
    return k


def stable_perm(cols: np.ndarray) -> np.ndarray:
    """Stable ascending permutation of (n, w <= 16) little-endian unsigned byte columns (int64)."""
    n, w = cols.shape
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    pad = np.zeros((n, 16), dtype=np.uint8)
    pad[:, :w] = cols
    lo = np.ascontiguousarray(pad[:, :8]).view("<u8").reshape(n)
    if w <= 8:
        return np.argsort(lo, kind="stable").astype(np.int64)
    hi = np.ascontiguousarray(pad[:, 8:]).view("<u8").reshape(n)
    return np.lexsort((lo, hi)).astype(np.int64)  # stable; the last key is the primary one


def pairs_reference(keys_raw, values_raw, key_bytes: int, kind: int, value_bytes: int, descending: bool):
    """-> (keys, values, perm): the sorted key bytes, the value bytes carried along (None when value_bytes == 0) and
    the permutation, perm[i] = input position of output element i."""
    keys_raw = np.ascontiguousarray(keys_raw, dtype=np.uint8).reshape(-1)
    n = keys_raw.size // key_bytes
    perm = stable_perm(mapped_columns(keys_raw, key_bytes, kind, descending))
    keys = keys_raw.reshape(n, key_bytes)[perm].reshape(-1).copy()
    values = None
    if value_bytes:
        v = np.ascontiguousarray(values_raw, dtype=np.uint8).reshape(n, value_bytes)
        values = v[perm].reshape(-1).copy()
    return keys, values, perm
