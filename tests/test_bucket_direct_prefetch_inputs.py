"""CPU: the inputs of test_gpu_bucket_direct_prefetch.py, made for 256 compute units and checked with numpy alone: the form
the device will pick is the intended one and n is in range (test_gpu_bucket_direct._assemble), what the direct kernel hands
over is what the maker says, the chains hold the patterns they are named for, and bucket_direct_ref's model sorts every
bucket that the kernel is meant to sort."""
import numpy as np
import pytest

import bucket_direct_prefetch_inputs as inputs
import bucket_direct_ref as ref
import test_gpu_bucket_direct as base
import util

NUM_CU = 256


@pytest.mark.parametrize("name", list(inputs.CASES))
def test_inputs_are_what_they_are_named_for(name):
    t, form, raw, left, chains, last = inputs.make(name, NUM_CU)
    es = util.TYPES[t][0]
    grid = NUM_CU * base.PER_CU[form]
    cape = base.CAPE[es] * form // 1024
    counts = inputs.counts_of(chains, grid)
    assert 65536 <= raw.size // es == counts.sum() < 1_100_000
    assert left > 0
    valid = lambda m: 0 < m <= cape
    seqs = [[len(low) for low, _ext in buckets] for buckets in chains.values()]
    has = lambda pred: any(pred(s, i) for s in seqs for i in range(len(s)))
    # valid, empty, valid; valid, above cape(), valid; two skipped in a row; a first bucket that is skipped
    assert has(lambda s, i: i + 2 < len(s) and valid(s[i]) and s[i + 1] == 0 and valid(s[i + 2]))
    assert has(lambda s, i: i + 2 < len(s) and valid(s[i]) and s[i + 1] > cape and valid(s[i + 2]))
    assert has(lambda s, i: i + 3 < len(s) and valid(s[i]) and s[i + 1] == 0 and s[i + 2] == 0 and valid(s[i + 3]))
    assert has(lambda s, i: i + 3 < len(s) and valid(s[i]) and s[i + 1] > cape and s[i + 2] > cape and valid(s[i + 3]))
    assert any(s[0] == 0 and valid(s[1]) for s in seqs) and any(s[0] > cape and valid(s[1]) for s in seqs)
    # a long bucket, one of 1, 2 or 3 keys, a long one again
    longest = cape if last is not None else 2000  # (256 values below the window: the longest that stays under the limit)
    for tiny in (1, 2, 3):
        assert has(lambda s, i: i + 2 < len(s) and s[i] >= longest - 1 and s[i + 1] == tiny and s[i + 2] >= longest - 1)
    if last is not None:
        assert any(len(s) == 1 and valid(s[0]) for s in seqs)  # a chain of one bucket
        assert last + 2 * grid < 65536 <= last + 3 * grid and counts[last + 2 * grid] > 0
        special = (1, 2, 3, cape - 1, cape)
        assert inputs.parities(chains, grid, special) == {m: {0, 1} for m in special}


@pytest.mark.parametrize("name", ["u64-1024", "u64-1024-below-2^40", "u64-1024-below-2^24"])
def test_model_sorts_what_the_kernel_is_meant_to_sort(name):
    t, form, _raw, left, chains, _last = inputs.make(name, NUM_CU)
    range_bits = inputs.CASES[name][2]
    b_lo, B = range_bits - 16, ref.BITS[form]
    cape = base.CAPE[8] * form // 1024
    rng = np.random.default_rng(3)
    handed = 0
    for buckets in chains.values():
        gave_up = False
        for low, _ext in buckets:
            if len(low) == 0:
                continue
            if len(low) > cape or gave_up:
                handed += 1
                continue
            got = ref.sort_bucket(low, b_lo, B, rng)
            if got is None:
                gave_up = True
                handed += 1
            else:
                assert np.array_equal(got, np.sort(low))
    assert handed == left
