"""CPU: the host side of the key / value calls (rsx_sort_pairs_device, rsx_argsort_device, rsx_ctx_reserve_pairs) --
the numpy reference of tests/pairs_ref.py held against the C oracle, the argument checks that need no device, and the
join / split kernels' presence and register budget in the gfx950 code object."""
import ctypes

import numpy as np
import pytest

import util
from pairs_ref import mapped_columns, pairs_reference
from resources import kernel_resources

U, S, F = util.UNSIGNED, util.SIGNED, util.FLOAT


def _index_elements(key_cols: np.ndarray) -> np.ndarray:
    """(key, u64 index) elements: the key bytes given, the element's position behind them."""
    n, kb = key_cols.shape
    e = np.zeros((n, kb + 8), dtype=np.uint8)
    e[:, :kb] = key_cols
    e[:, kb:] = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)
    return e.reshape(-1)


def _index_payload(sorted_raw: np.ndarray, kb: int) -> np.ndarray:
    n = sorted_raw.size // (kb + 8)
    return np.ascontiguousarray(sorted_raw.reshape(n, kb + 8)[:, kb:]).view("<u8").reshape(n).astype(np.int64)


@pytest.mark.parametrize("tname", util.PRIMS)
def test_reference_against_the_c_oracle(orc, tname):
    """Ascending perm == the index payload of the oracle's sort of (key, u64 index) elements; descending perm == the
    ascending one of keys whose mapped form was complemented on the CPU (sorted as unsigned keys).  Float inputs
    hold NaN of both signs, +-0 and +-inf (util.make_input)."""
    es, _ko, kb, kind = util.TYPES[tname]
    for dist, n in (("uniform", 5003), ("two", 4099), ("equal", 700), ("lowbyte", 3001), ("uniform", 17)):
        keys_raw = util.make_input(tname, n, dist, seed=len(tname) * 131 + n)
        cols = keys_raw.reshape(n, kb)
        vals = np.arange(n, dtype="<u4").view(np.uint8)
        k_up, v_up, p_up = pairs_reference(keys_raw, vals, kb, kind, 4, False)
        want_up = _index_payload(orc.sort_parallel(_index_elements(cols), orc.Layout(kb + 8, 0, kb, kind), 4), kb)
        assert np.array_equal(p_up, want_up), (tname, dist, n)
        assert np.array_equal(v_up.view("<u4"), p_up), (tname, dist, n)
        assert np.array_equal(k_up.reshape(n, kb), cols[p_up])
        k_dn, v_dn, p_dn = pairs_reference(keys_raw, vals, kb, kind, 4, True)
        comp = orc.map_keys(keys_raw, orc.Layout(kb, 0, kb, kind)) ^ np.uint8(0xFF)  # the C oracle's mapping
        assert np.array_equal(comp, mapped_columns(keys_raw, kb, kind, True))
        want_dn = _index_payload(orc.sort_parallel(_index_elements(comp), orc.Layout(kb + 8, 0, kb, U), 4), kb)
        assert np.array_equal(p_dn, want_dn), (tname, dist, n)
        assert np.array_equal(v_dn.view("<u4"), p_dn)
        if dist == "equal":  # all keys equal: both orders keep the input order
            assert np.array_equal(p_up, np.arange(n)) and np.array_equal(p_dn, np.arange(n))


def test_reference_float_order_is_the_total_order():
    bits = np.array([0x7FC00000, 0x7F800000, 0x00000000, 0x80000000, 0xFF800000, 0xFFC00000, 0x3F800000, 0xBF800000], dtype="<u4")
    keys, _v, perm = pairs_reference(bits.view(np.uint8), None, 4, F, 0, False)
    # -NaN < -inf < -1 < -0 < +0 < 1 < +inf < +NaN
    assert list(keys.view("<u4")) == [0xFFC00000, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x3F800000, 0x7F800000, 0x7FC00000]
    _k, _v, down = pairs_reference(bits.view(np.uint8), None, 4, F, 0, True)
    assert list(down) == list(perm[::-1])  # (all keys distinct)


@pytest.fixture(scope="module")
def lib():
    from radix_sort_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_null_context_is_an_argument_error(lib):
    assert lib.rsx_sort_pairs_device(None, None, None, 10, 4, 0, 4, 0, None) == -1
    assert lib.rsx_argsort_device(None, None, None, 10, 4, 0, 8, 1, None) == -1
    assert lib.rsx_ctx_reserve_pairs(None, 10, 4, 4) == -1


@pytest.fixture()
def no_context(monkeypatch):
    """Any attempt to make a context fails the test: the argument checks come first."""
    from radix_sort_amd import api

    def boom(*_a, **_k):
        raise AssertionError("a context was made before the arguments were checked")

    monkeypatch.setattr(api, "Context", boom)
    monkeypatch.setattr(api, "default_context", boom)


def test_python_checks_raise_before_any_context(no_context):
    import torch
    import radix_sort_amd as rs
    k = torch.arange(8, dtype=torch.int32)
    v = torch.arange(8, dtype=torch.float32)
    with pytest.raises(ValueError, match="one row per key"):
        rs.radix_sort_pairs(k, torch.arange(9, dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_sort_pairs(torch.arange(16, dtype=torch.int32)[::2], v)
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_sort_pairs(k, torch.zeros(8, 4)[:, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_argsort(torch.arange(16, dtype=torch.int32)[::2])
    with pytest.raises(TypeError, match="no RadixDigits"):
        rs.radix_sort_pairs(torch.zeros(8, dtype=torch.bool), v)
    with pytest.raises(TypeError, match="no RadixDigits"):
        rs.radix_argsort(torch.zeros(8, dtype=torch.float16))
    with pytest.raises(ValueError, match="1-D"):
        rs.radix_argsort(torch.zeros(8, 2, dtype=torch.int32))
    with pytest.raises(TypeError):
        rs.radix_sort_pairs(np.arange(8, dtype=np.int32), v)
    with pytest.raises(TypeError):
        rs.radix_sort_pairs(k, np.arange(8))
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_sort_pairs(k, v)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_sort_pairs(k, None, descending=True)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_argsort(k)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_argsort(torch.zeros(8, 16, dtype=torch.uint8), key_kind=rs.KEY_SIGNED)
    with pytest.raises(ValueError, match="key_kind"):
        rs.radix_argsort(k, key_kind=rs.KEY_SIGNED)
    with pytest.raises(ValueError, match="128-bit"):
        rs.radix_argsort(torch.zeros(8, 16, dtype=torch.uint8), key_kind=rs.KEY_FLOAT)
    with pytest.raises(TypeError, match="int32 or int64"):
        rs.radix_argsort(k, out=torch.zeros(8, dtype=torch.float32))
    with pytest.raises(TypeError, match="int32 or int64"):
        rs.radix_argsort(k, out=torch.zeros(8, dtype=torch.int16))
    with pytest.raises(ValueError, match="8 elements"):
        rs.radix_argsort(k, out=torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ValueError, match="8 elements"):
        rs.radix_argsort(k, out=torch.zeros(16, dtype=torch.int64)[::2])
    with pytest.raises(ValueError, match="bytes"):
        rs.radix_sort_pairs(k, torch.zeros(8, 0))
    with pytest.raises(ValueError, match="bytes"):
        rs.radix_sort_pairs(k, torch.zeros(8, 32769, dtype=torch.uint8))


def test_code_object_holds_the_join_and_split_kernels():
    from radix_sort_amd import _build
    _build.build()
    blob = open(_build.LIB, "rb").read()
    for name in (b"rsx_pairs_join_kernel", b"rsx_pairs_split_kernel", b"rsx_pairs_join_any_kernel", b"rsx_pairs_split_any_kernel"):
        assert name in blob, name


def test_join_and_split_kernels_use_no_scratch():
    res = kernel_resources("rsx_pairs.hip")
    names = [n for n in res if "rsx_pairs_" in n]
    typed_join = [n for n in names if "rsx_pairs_join_kernel" in n]
    typed_split = [n for n in names if "rsx_pairs_split_kernel" in n]
    # keys of 1, 2, 4, 8, 16 bytes x values of 0, 1, 2, 4, 8, 16 bytes, and the generated positions of 4 and 8 bytes
    assert len(typed_join) >= 40 and len(typed_split) >= 50, (len(typed_join), len(typed_split))
    assert any("join_any" in n for n in names) and any("split_any" in n for n in names)
    for n in names:
        assert res[n].get("ScratchSize [bytes/lane]", -1) == 0, (n, res[n])
        assert res[n].get("VGPRs Spill", -1) == 0, (n, res[n])
