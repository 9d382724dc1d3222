"""CPU: the numpy restatement of rsx_verify_device's three words (util.verify_reference), which the GPU tests of
the verifier compare it with, checked on the oracle's output and against a plain python loop."""
import numpy as np
import pytest

import util

LAYOUTS = [(t, util.TYPES[t]) for t in util.TYPES] + [("any%d-%d-%d" % L[:3], L) for L in util.ANY_LAYOUTS]
DISTS = ["uniform", "two", "zipf", "reversed", "step16", "equal"]


def _input(name, lay, n, dist, seed):
    return util.make_input(name, n, dist, seed) if name in util.TYPES else util.make_input_layout(lay, n, dist, seed)


def _slow_reference(raw, lay):
    """The three words, element by element on python ints."""
    es, ko, kb, kind = lay
    n = len(raw) // es
    elems = [bytes(raw[i * es:(i + 1) * es]) for i in range(n)]

    def mapped(e):
        k = bytearray(e[ko:ko + kb])
        if kind == util.SIGNED:
            k[-1] ^= 0x80
        elif kind == util.FLOAT:
            if k[-1] & 0x80:
                k = bytearray(b ^ 0xFF for b in k)
            else:
                k[-1] ^= 0x80
        return int.from_bytes(k, "little")

    def payload(e):
        return int.from_bytes(bytes(e[b] for b in range(es) if not ko <= b < ko + kb)[:8], "little")

    down = sum(mapped(a) > mapped(b) for a, b in zip(elems, elems[1:]))
    unstable = sum(mapped(a) == mapped(b) and payload(a) > payload(b) for a, b in zip(elems, elems[1:]))
    return down, sum(util.element_hash_int(e) for e in elems) & ((1 << 64) - 1), unstable


@pytest.mark.parametrize("name,lay", LAYOUTS, ids=[x[0] for x in LAYOUTS])
def test_restatement_on_oracle_output(orc, name, lay):
    es, ko, kb, kind = lay
    pay_bytes = es - kb
    for i, dist in enumerate(DISTS):
        for n in (200, 4099):
            raw = _input(name, lay, n, dist, seed=60 + i)
            want = orc.sort_parallel(raw, orc.Layout(*lay), 3)
            down, csum, unstable = util.verify_reference(want, lay, orc)
            assert down == 0, (name, dist, n)
            if pay_bytes == 0 or n <= 256 ** min(pay_bytes, 8):  # the index in the payload has not wrapped
                assert unstable == 0, (name, dist, n)
            assert csum == util.verify_reference(raw, lay, orc)[1], (name, dist, n)
    # the inputs really are out of order, and the restatement says so
    n = 4099
    assert util.verify_reference(_input(name, lay, n, "uniform", 7), lay, orc)[0] > n // 4
    rev = util.verify_reference(_input(name, lay, n, "reversed", 7), lay, orc)[0]
    assert rev == n - 1 if kb >= 2 else rev > 0  # keys n-1 .. 0 (one-byte keys wrap)


@pytest.mark.parametrize("name,lay", LAYOUTS, ids=[x[0] for x in LAYOUTS])
def test_restatement_against_a_python_loop(orc, name, lay):
    for dist in ("uniform", "two", "reversed"):
        raw = _input(name, lay, 311, dist, seed=5)
        assert util.verify_reference(raw, lay, orc) == _slow_reference(raw, lay), (name, dist)
    assert util.verify_reference(np.zeros(0, np.uint8), lay, orc) == (0, 0, 0)
    one = _input(name, lay, 1, "uniform", seed=6)
    assert util.verify_reference(one, lay, orc) == (0, util.element_hash_int(one.tobytes()), 0)


def test_checksum_sees_every_byte_and_every_element(orc):
    """What a checksum is for: a lost, duplicated or altered element changes it, whichever byte differs."""
    lay = (100, 36, 16, util.UNSIGNED)
    raw = util.make_input_layout(lay, 50, "uniform", 3)
    base = util.verify_checksum(raw, 100)
    for byte in range(100):
        bad = raw.copy()
        bad[17 * 100 + byte] ^= 0x10
        assert util.verify_checksum(bad, 100) != base, byte
    dup = raw.copy()
    dup[300:400] = dup[400:500]
    assert util.verify_checksum(dup, 100) != base
    perm = raw.reshape(50, 100)[::-1].reshape(-1).copy()
    assert util.verify_checksum(perm, 100) == base  # order does not matter
