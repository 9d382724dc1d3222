"""GPU: rsx_bucket16_direct_kernel with its counters packed two to a word -- B + 1 digit bits counted in the 16-bit halves
of 2^B words, the starts read back as 16-bit halves, the hand-over still on B-bit sub-buckets -- bit for bit against the CPU oracle,
and RSX_INFO_LAST_DIRECT against the numpy model.  The inputs (bucket_direct_packed_inputs.py, checked against the model in
test_bucket_direct_packed_ref.py) are the smallest at which the packing can go wrong:
  all-<type>-<form>   bucket counts 1, 2, odd, cape() and cape() - 1 in one chain; B-bit sub-buckets of distinct keys split
                      by the extra bit as 12 + 12, 24 + 0, 0 + 24, 23 + 1; digits 2k + 1 and 2k + 2 (neighbouring words)
                      with 24 each; digit 0 and the last digit crowded to the limit; buckets whose keys all share the B + 1
                      digit bits (any digit, the last, the first); keys that differ only in the extra bit, and only below
                      it; runs of 1 .. 24 equal keys; keys on every 4th digit only; 13 + 12 and 25 in one half: handed over
  range-<form>-<bits> u64 keys below 2^bits: the digit at bit 0, across two dwords, at bit 31 and 32 of the element; b_lo = B
                      (a half is a B-bit sub-bucket by itself: 20 + 20 in one word stay, 25 equal keys go), B + 1, B + 2
  u128-across-dwords  a digit across the element's second and third dwords"""
import numpy as np
import pytest

import bucket_direct_packed_inputs as inputs
import util
from test_gpu_bucket_direct import _sort, num_cu, rs, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

_CASES = {}  # name -> (type, input, expected, what the direct kernel leaves): made once, shared, never changed


@pytest.mark.parametrize("name", list(inputs.CASES))
def test_packed_counters(rs, torch, orc, num_cu, name):
    if name not in _CASES:
        case = inputs.make(name)
        raw, left = inputs.assemble(case, num_cu)
        exp = orc.sort_parallel(raw, orc.Layout(*util.TYPES[case["t"]]), 8)
        raw.setflags(write=False)
        exp.setflags(write=False)
        _CASES[name] = (case["t"], raw, exp, left, case["left"])
    t, raw, exp, left, meant = _CASES[name]
    es = util.TYPES[t][0]
    assert left == meant, (name, left, meant)
    got, info = _sort(rs, torch, t, raw, 1)
    print(name, "n", raw.size // es, "left", info, "expected", left)
    assert np.array_equal(got, exp), (name, int(np.flatnonzero(got != exp)[0]) // es)
    assert info == left, (name, info, left)
