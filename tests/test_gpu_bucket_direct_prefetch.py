"""GPU: the pipelined load of rsx_bucket16_direct_kernel (8-byte elements, 1024 and 512 threads: the next bucket of a
workgroup's chain is fetched while the current one is ranked) on the chains of bucket_direct_prefetch_inputs.py: a long
bucket, a tiny one and a long one again; empty buckets and buckets above cape() between valid ones, two in a row, at the
head of a chain; a chain of one bucket; a chain that ends with the 65536; a hand-over in the second bucket of a chain; every
special count at an even and at an odd element offset; keys below 2^40 and below 2^24.  Bit for bit against the CPU oracle,
INFO_LAST_DIRECT against bucket_direct_ref.handed_over, and OPT_BUCKET_DIRECT 1 against 0.  The forms without the pipelined
load (256 threads, u128) run the same chains: the loop around the load is the same code."""
import numpy as np
import pytest

import bucket_direct_prefetch_inputs as inputs
import util
from test_gpu_bucket_direct import CAPE, NONE, PER_CU, _sort, num_cu, rs, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

_EXPECTED = {}  # name -> the oracle's bytes: made once, shared, never changed


def _expected(orc, name, t, raw):
    if name not in _EXPECTED:
        exp = orc.sort_parallel(raw, orc.Layout(*util.TYPES[t]), 8)
        exp.setflags(write=False)
        _EXPECTED[name] = exp
    return _EXPECTED[name]


@pytest.mark.parametrize("name", list(inputs.CASES))
def test_chains_where_a_pipelined_load_can_go_wrong(rs, torch, orc, num_cu, name):
    t, form, raw, left, chains, last = inputs.make(name, num_cu)
    es = util.TYPES[t][0]
    grid = num_cu * PER_CU[form]
    if last is not None:  # the chain that ends the 65536, for the grid of THIS device
        assert last + 2 * grid < 65536 <= last + 3 * grid and len(chains[last]) == 3 and len(chains[last][2][0]) > 0
        cape = CAPE[es] * form // 1024
        special = (1, 2, 3, cape - 1, cape)
        assert inputs.parities(chains, grid, special) == {m: {0, 1} for m in special}
    exp = _expected(orc, name, t, raw)
    got, info = _sort(rs, torch, t, raw, 1)
    print(name, "n", raw.size // es, "left", info, "expected", left)
    assert np.array_equal(got, exp), (name, int(np.flatnonzero(got != exp)[0]) // es)
    assert info == left, (name, info, left)
    got0, info0 = _sort(rs, torch, t, raw, 0)  # the same bytes by the stable passes
    assert info0 == NONE and np.array_equal(got0, got), name
