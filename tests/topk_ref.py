"""Reference for the top-k calls (rsx_topk_rows_device, radix_topk), numpy only; a helper, no tests.

One definition: row r of the result is the first k columns of what pairs_ref.pairs_reference -- the stable sort by
mapped key, ascending or descending, equal keys in input order -- leaves on row r alone: the keys and their positions
inside the row.  Rows are the segments [r * row_len, (r + 1) * row_len) of segment_pairs_ref.segments_reference."""
from __future__ import annotations

import numpy as np

from pairs_ref import pairs_reference
from segment_pairs_ref import segments_reference


def rows_reference(keys_raw, key_bytes: int, kind: int, rows: int, row_len: int, descending: bool):
    """-> (keys, local): every row fully sorted, as (rows, row_len, key_bytes) bytes and (rows, row_len) positions inside
    the row (int64).  What the top-k of any k is cut from: compute once per input and order, share, leave unchanged."""
    keys_raw = np.ascontiguousarray(keys_raw, dtype=np.uint8).reshape(-1)
    assert keys_raw.size == rows * row_len * key_bytes
    if rows == 1:  # (a flat array: the one segment, without the segment loop's copies)
        skeys, _, local = pairs_reference(keys_raw, None, key_bytes, kind, 0, descending)
    else:
        offsets = np.arange(rows + 1, dtype=np.int64) * row_len
        skeys, _, local = segments_reference(keys_raw, None, key_bytes, kind, 0, descending, offsets)
    return skeys.reshape(rows, row_len, key_bytes), np.asarray(local, dtype=np.int64).reshape(rows, row_len)


def first_k(full, k: int):
    """-> (out_keys, out_index) of rows_reference's result: rows * k * key_bytes key bytes, rows * k positions (int64)."""
    skeys, local = full
    return skeys[:, :k, :].reshape(-1).copy(), local[:, :k].reshape(-1).copy()


def topk_reference(keys_raw, key_bytes: int, kind: int, rows: int, row_len: int, k: int, descending: bool):
    """-> (out_keys, out_index): rows * k * key_bytes key bytes and rows * k positions (int64)."""
    assert 0 <= k <= row_len
    if rows == 0 or k == 0:
        return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int64)
    return first_k(rows_reference(keys_raw, key_bytes, kind, rows, row_len, descending), k)


def index_bytes_of(out_index: np.ndarray, index_bytes: int) -> np.ndarray:
    return out_index.astype("<i4" if index_bytes == 4 else "<i8").view(np.uint8)
