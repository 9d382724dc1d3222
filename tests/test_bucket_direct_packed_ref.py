"""CPU: the numpy model of the direct bucket kernel with packed counters (bucket_direct_packed_ref.py) on every bucket of
every input of test_gpu_bucket_direct_packed.py (made for 256 compute units): it returns the sorted bucket, or None
exactly where bucket_direct_ref's model does; the buckets meant to be sorted directly are, those meant to be handed over
are not, and what an input hands over is what its maker says."""
import numpy as np
import pytest

import bucket_direct_packed_inputs as inputs
import bucket_direct_packed_ref as ref
import util


@pytest.mark.parametrize("name", list(inputs.CASES))
def test_model_sorts_every_bucket_of_every_gpu_input(name):
    case = inputs.make(name)
    es = util.TYPES[case["t"]][0]
    B = ref.BITS[case["form"]]
    rng = np.random.default_rng(1)
    worst = 0
    for buckets in case["chains"].values():
        for low, ext, kind in buckets:
            m, b_lo = inputs.model_low(es, low, ext, case["range_bits"])
            got = ref.sort_bucket(m, b_lo, B, rng)
            old_leaves = ref.old.largest_sub_bucket(m, b_lo, B) > ref.LIMIT  # (bucket_direct_ref.sort_bucket's test)
            assert (got is None) == old_leaves == (kind == "over"), (name, kind, len(low))
            if got is not None:
                assert np.array_equal(got, np.sort(m)), (name, kind, len(low))
                worst = max(worst, ref.old.largest_sub_bucket(m, b_lo, B + 1))
    assert worst <= ref.LIMIT
    _raw, left = inputs.assemble(case, 256)
    assert left == case["left"], (name, left)


def test_old_model_agrees_on_a_few_buckets():
    """bucket_direct_ref.sort_bucket itself (the slow one) on the special buckets of one input: None in the same places."""
    case = inputs.make("all-u64-256")
    rng = np.random.default_rng(2)
    for base, buckets in case["chains"].items():
        for low, _ext, kind in buckets[:6] + buckets[-1:]:
            got, was = ref.sort_bucket(low, 48, 10, rng), ref.old.sort_bucket(low, 48, 10, rng)
            assert (got is None) == (was is None)
            if got is not None:
                assert np.array_equal(got, was)


def test_halves_never_carry():
    """The packed scan at its worst: cape() keys, one digit holding 24 of them at either end, the rest spread evenly."""
    for form, B in ref.BITS.items():
        n = 17 * form
        d = np.arange(n - 48, dtype=np.uint64) % np.uint64(2 << B)
        d = np.concatenate([d, np.zeros(24, dtype=np.uint64), np.full(24, (2 << B) - 1, dtype=np.uint64)])
        low = d << np.uint64(48 - B - 1)
        words = ref.packed_words(low, 48, B)
        starts = ref.packed_scan(words, n)
        assert np.array_equal(starts, np.concatenate([[0], np.cumsum(np.bincount(d.astype(np.int64), minlength=2 << B))]))
        assert starts[-1] == n and starts.max() == n
