"""Reference for the order-statistics calls (rsx_select_device, radix_select and what is composed from it), numpy only; a
helper, no tests.

The call promises column r of the full stable sort: with p the stable permutation by mapped key (pairs_ref: ascending, or
complemented for descending order, equal keys in input order), the key bytes keys[p[r]] and the position p[r]."""
from __future__ import annotations

import math

import numpy as np

from pairs_ref import mapped_columns, stable_perm


def select_reference(keys_raw, kb: int, kind: int, ranks, descending: bool):
    """-> (key bytes (len(ranks), kb) uint8, positions int64) of the ranks (each in 0 .. n - 1, any order, repeats allowed)."""
    keys_raw = np.ascontiguousarray(keys_raw, dtype=np.uint8).reshape(-1)
    n = keys_raw.size // kb
    perm = stable_perm(mapped_columns(keys_raw, kb, kind, descending))
    pos = perm[np.asarray(list(ranks), dtype=np.int64)] if len(ranks) else np.zeros(0, dtype=np.int64)
    return keys_raw.reshape(n, kb)[pos].copy(), pos.astype(np.int64)


def quantile_ranks(n: int, q, method: str):
    """The rank each quantile of q (floats in [0, 1]) selects among n keys: numpy's rules on the virtual index q * (n - 1),
    "lower" its floor, "higher" its ceiling, "nearest" rounded half to even."""
    out = []
    for x in q:
        v = float(x) * (n - 1)
        if method == "lower":
            r = math.floor(v)
        elif method == "higher":
            r = math.ceil(v)
        elif method == "nearest":
            r = int(np.around(v))
        else:
            raise ValueError(method)
        out.append(min(max(int(r), 0), n - 1))
    return out
