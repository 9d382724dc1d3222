"""Reference for rsx_compact_device / radix_compact / radix_nonzero, numpy only; a helper, no tests.

The definition of include/rsx.h restated: with N = n or min(n, num) and M the mapped key of rsx_argsort_device
(pairs_ref.mapped_columns: sign flip, float total order, complemented when descending), row i < N passes when its flag byte
is non-zero (mask given), M(lo) <= M(keys[i]) (lo given) and M(keys[i]) < M(hi) (hi given); invert keeps the others.  The
result is the list of source rows in output order -- the kept rows in input order, then, with partition, the others in
input order -- and the number kept.  Everything else is plain boolean indexing."""
from __future__ import annotations

import numpy as np

import util
from pairs_ref import mapped_columns


def _wide(cols: np.ndarray):
    """(n, kb <= 16) little-endian byte columns -> (hi, lo) uint64 halves of the unsigned integer they spell"""
    n, w = cols.shape
    pad = np.zeros((n, 16), dtype=np.uint8)
    pad[:, :w] = cols
    return np.ascontiguousarray(pad[:, 8:]).view("<u8").reshape(n), np.ascontiguousarray(pad[:, :8]).view("<u8").reshape(n)


def _less(a, b):
    """a < b for (hi, lo) pairs, elementwise with broadcasting"""
    return (a[0] < b[0]) | ((a[0] == b[0]) & (a[1] < b[1]))


def compact_reference(n: int, tname=None, keys_raw=None, mask=None, lo=None, hi=None, descending: bool = False, invert: bool = False,
                      partition: bool = False, num=None):
    """-> (rows, m): rows = int64 source rows in output order (m kept ones; with partition the N - m others behind them),
    m = the number kept.  keys_raw: the raw key bytes (needed for lo / hi, which are the raw bytes of ONE key each);
    mask: n bytes, non-zero passes."""
    N = n if num is None else min(int(num), n)
    passes = np.ones(N, dtype=bool)
    if mask is not None:
        passes &= np.asarray(mask).view(np.uint8).reshape(-1)[:N] != 0
    if lo is not None or hi is not None:
        _es, _ko, kb, kind = util.TYPES[tname]
        raw = np.ascontiguousarray(keys_raw).view(np.uint8).reshape(-1)[:N * kb]
        M = _wide(mapped_columns(raw, kb, kind, descending))
        if lo is not None:
            passes &= ~_less(M, _wide(mapped_columns(np.ascontiguousarray(lo).view(np.uint8).reshape(-1), kb, kind, descending)))
        if hi is not None:
            passes &= _less(M, _wide(mapped_columns(np.ascontiguousarray(hi).view(np.uint8).reshape(-1), kb, kind, descending)))
    keep = ~passes if invert else passes
    rows = np.arange(N, dtype=np.int64)
    kept = rows[keep]
    if partition:
        return np.concatenate([kept, rows[~keep]]), int(kept.size)
    return kept, int(kept.size)


def expected_column(column_raw, width: int, n: int, rows: np.ndarray) -> np.ndarray:
    """The bytes of an n-row output column that held 0xA5 everywhere before the call: row t = input row rows[t]."""
    out = np.full((n, width), 0xA5, dtype=np.uint8)
    out[:rows.size] = np.ascontiguousarray(column_raw).view(np.uint8).reshape(-1, width)[rows]
    return out.reshape(-1)


def expected_index(n: int, index_bytes: int, rows: np.ndarray) -> np.ndarray:
    out = np.full(n * index_bytes, 0xA5, dtype=np.uint8).view("<i4" if index_bytes == 4 else "<i8").copy()
    out[:rows.size] = rows
    return out.view(np.uint8)
