"""CPU: the two forms of the segmented key / value reference (tests/segment_pairs_ref.py) agree: segments_reference, which
calls pairs_ref.pairs_reference once per segment, and segments_reference_fast, one lexsort for the whole call.  The GPU
tests use the fast form where the per-segment loop would take too long (65000 short segments); they may do so only for
the key types and value widths held equal here."""
import numpy as np
import pytest

import util
from segment_pairs_ref import segments_reference, segments_reference_fast

KEY_TYPES = ["u8", "i16", "u32", "i32", "f32", "u64", "i64", "f64", "u128"]


def ragged(rng, nseg, head, tail):
    lens = rng.choice(np.asarray([0, 0, 1, 2, 3, 17, 64, 65, 300], dtype=np.int64), size=nseg)
    offs = np.concatenate([[head], head + np.cumsum(lens)]).astype(np.int64)
    return offs, int(offs[-1]) + tail


def values_for(rng, n, vb):
    if not vb:
        return None
    return rng.integers(0, 256, size=n * vb, dtype=np.uint8)


def equal(a, b):
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        else:
            assert x.dtype == y.dtype and np.array_equal(x, y)


@pytest.mark.parametrize("vb", [0, 4, 8, 16, 20])
@pytest.mark.parametrize("dist", ["uniform", "two"])
@pytest.mark.parametrize("tname", KEY_TYPES)
def test_fast_form_equals_the_loop(tname, dist, vb):
    """Ragged segments with empty ones (also the first and the last), a head of 5 and a tail of 7 elements no segment
    covers, and ties: `two` has two distinct keys, `uniform` one-byte keys collide and floats carry the specials."""
    _es, _ko, kb, kind = util.TYPES[tname]
    rng = np.random.default_rng(sum(map(ord, tname + dist)) + vb)
    offs, n = ragged(rng, 200, head=5, tail=7)
    offs = np.concatenate([[5], offs, [offs[-1]]])  # an empty first and an empty last segment
    assert np.count_nonzero(np.diff(offs) == 0) > 10
    keys_raw = util.make_input(tname, n, dist, seed=7)
    values_raw = values_for(rng, n, vb)
    for desc in (False, True):
        slow = segments_reference(keys_raw, values_raw, kb, kind, vb, desc, offs)
        fast = segments_reference_fast(keys_raw, values_raw, kb, kind, vb, desc, offs)
        equal(slow, fast)
        # something was sorted, something tied, and head and tail stayed: the inputs are not trivial
        local = slow[2]
        assert np.all(local[:5] == -1) and np.all(local[-7:] == -1) and np.all(local[5:-7] >= 0)
        assert not np.array_equal(slow[0], keys_raw)
    if dist == "two":
        k = keys_raw.reshape(n, kb)
        assert len(np.unique(k, axis=0)) == 2


@pytest.mark.parametrize("tname", ["u32", "u64", "u128"])
def test_fast_form_on_rows_and_on_nothing(tname):
    """Back-to-back rows (what the row forms sort) and the degenerate calls: one empty segment, all segments empty."""
    _es, _ko, kb, kind = util.TYPES[tname]
    rows, row_len = 37, 101
    n = rows * row_len
    keys_raw = util.make_input(tname, n, "step16", seed=3)
    values_raw = values_for(np.random.default_rng(1), n, 4)
    offs = np.arange(rows + 1, dtype=np.int64) * row_len
    for desc in (False, True):
        equal(segments_reference(keys_raw, values_raw, kb, kind, 4, desc, offs),
              segments_reference_fast(keys_raw, values_raw, kb, kind, 4, desc, offs))
    for offs in ([9, 9], [0, 0, 0], [n, n]):
        equal(segments_reference(keys_raw, values_raw, kb, kind, 4, True, offs),
              segments_reference_fast(keys_raw, values_raw, kb, kind, 4, True, offs))


def test_fast_form_refuses_offsets_it_cannot_judge():
    keys_raw = util.make_input("u32", 100, "uniform", seed=1)
    for offs in ([10, 5, 20], [0, 101], [-1, 5], [7]):
        with pytest.raises(ValueError):
            segments_reference_fast(keys_raw, None, 4, util.UNSIGNED, 0, False, offs)
