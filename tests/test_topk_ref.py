"""The top-k reference (tests/topk_ref.py) against torch on the CPU (no GPU)."""
import numpy as np
import pytest
import torch

import util
from topk_ref import topk_reference


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("tname,dt", [("i32", torch.int32), ("u8", torch.uint8), ("i64", torch.int64)])
def test_integer_keys_with_ties_against_stable_sort(tname, dt, descending):
    """Few distinct values: the threshold falls inside a run of ties, which go to the lowest positions."""
    kb, kind = util.TYPES[tname][2], util.TYPES[tname][3]
    rows, row_len = 7, 300
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(0 if tname == "u8" else -3, 4, size=(rows, row_len)).astype(np.int64)).to(dt)
    raw = x.numpy().view(np.uint8).reshape(-1)
    for k in (0, 1, 2, 150, 299, 300):
        keys, index = topk_reference(raw, kb, kind, rows, row_len, k, descending)
        want = torch.sort(x, dim=-1, stable=True, descending=descending)
        assert np.array_equal(index.reshape(rows, k), want.indices[:, :k].numpy())
        assert np.array_equal(keys, want.values[:, :k].contiguous().numpy().view(np.uint8).reshape(-1))


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_distinct_float_keys_against_torch_topk(dt, largest):
    rows, row_len, k = 5, 1000, 64
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rows, row_len, dtype=torch.float64, generator=g).to(dt)
    assert all(len(torch.unique(r)) == row_len for r in x)
    kb = x.element_size()
    keys, index = topk_reference(x.numpy().view(np.uint8).reshape(-1), kb, util.FLOAT, rows, row_len, k, largest)
    want = torch.topk(x, k, dim=-1, largest=largest, sorted=True)
    assert np.array_equal(keys, want.values.contiguous().numpy().view(np.uint8).reshape(-1))
    assert np.array_equal(index.reshape(rows, k), want.indices.numpy())  # (distinct keys: no tie order to differ in)


def test_flat_array_is_one_row():
    raw = util.make_input("u32", 5000, "two", seed=1)
    a = topk_reference(raw, 4, util.UNSIGNED, 1, 5000, 100, True)
    cols = raw.view("<u4")
    perm = np.argsort(~cols, kind="stable")[:100]
    assert np.array_equal(a[1], perm) and np.array_equal(a[0], cols[perm].view(np.uint8))
