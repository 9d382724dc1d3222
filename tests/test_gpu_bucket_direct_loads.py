"""GPU: the 16-byte global loads of the bucket in rsx_bucket16_direct_kernel (8-byte elements: a thread takes words of two
neighbouring elements, at the bucket's 8-byte alignment; 16-byte elements load as before).

A bucket starts wherever the buckets before it end.  One chain holds buckets of 1, 2, 3, an odd number, cape() - 1 and
cape() elements twice over with a single element in between, so that every one of those counts starts once at an even and
once at an odd element of the array (checked below on the counts); the chain sits at the head of the array, the fillers
that decide the form behind it.  1024- and 512-thread form, u64 and u128: parity with the oracle, nothing handed over."""
import numpy as np
import pytest

import bucket_direct_packed_inputs as inputs
import util
from test_gpu_bucket_direct import CAPE, PER_CU, _filler, _sort, _uniform, num_cu, rs, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _case(t, form, num_cu):
    es = util.TYPES[t][0]
    cape = CAPE[es] * form // 1024
    rng = np.random.default_rng(11000 + es + form)
    odd = 2 * int(rng.integers(50, cape // 2 - 50)) + 1
    special = [1, 2, 3, odd, cape - 1, cape]
    head = special + [1] + special
    fillers = max(12, -(-80000 // (cape // 2)))  # (more than eight decide the form; 65536 elements make the hybrid)
    chains = {8: inputs._tag([_uniform(rng, m) for m in head]), 40005: inputs._tag(_filler(rng, form, es, fillers))}
    # the chain at window value 8 is the head of the array: no other bucket lies between or ahead of its buckets
    grid = num_cu * PER_CU[form]
    assert 8 + len(head) * grid < 40005
    starts = np.concatenate([[0], np.cumsum(head)])[:-1]
    for m in special:
        assert {int(s) & 1 for s, c in zip(starts, head) if c == m} == {0, 1}, (m, starts)
    return {"t": t, "form": form, "range_bits": 64, "chains": chains, "left": 0}


@pytest.mark.parametrize("form", [1024, 512])
@pytest.mark.parametrize("t", ["u64", "u128"])
def test_buckets_at_odd_and_even_offsets(rs, torch, orc, num_cu, t, form):
    raw, left = inputs.assemble(_case(t, form, num_cu), num_cu)
    assert left == 0
    exp = orc.sort_parallel(raw, orc.Layout(*util.TYPES[t]), 8)
    got, info = _sort(rs, torch, t, raw, 1)
    es = util.TYPES[t][0]
    assert np.array_equal(got, exp), (t, form, int(np.flatnonzero(got != exp)[0]) // es)
    assert info == 0, (t, form, info)
