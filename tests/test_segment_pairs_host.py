"""CPU: the host side of the segmented key / value calls (rsx_sort_segments_pairs_device, rsx_argsort_segments_device,
rsx_sort_rows_pairs_device, rsx_argsort_rows_device, rsx_segment_pairs_caps): the exported prototypes, the size classes
of the joined element, and every argument check and early return that needs no device."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_BYTES = (1, 2, 4, 8, 16)
TYPED_VALUE_BYTES = (0, 1, 2, 4, 8, 16)
ERR_ARG = -1


# ---- include/rsx.h restated: where the value sits in the joined element and how large that element is ----
def voff(kb, vb):
    a = 1 if vb == 0 else 4 if vb % 4 == 0 else 2 if vb % 2 == 0 else 1
    return (kb + a - 1) // a * a


def joined_elem(kb, vb):
    need = voff(kb, vb) + vb
    return next((z for z in (1, 2, 4, 8, 12, 16, 24, 32) if z >= need and z % kb == 0), 0)


@pytest.fixture(scope="module")
def lib():
    from radix_sort_amd import _build, _lib
    _build.build()
    return _lib.load()


PROTOTYPES = {
    "rsx_sort_segments_pairs_device": "int rsx_sort_segments_pairs_device(rsx_ctx *ctx, void *d_keys, void *d_values, size_t n, uint32_t key_bytes, "
                                      "uint32_t key_kind, uint32_t value_bytes, int order, const uint64_t *d_offsets, size_t nseg, "
                                      "uint64_t max_seg_len, void *stream);",
    "rsx_argsort_segments_device": "int rsx_argsort_segments_device(rsx_ctx *ctx, const void *d_keys, void *d_index, size_t n, uint32_t key_bytes, "
                                   "uint32_t key_kind, uint32_t index_bytes, int order, const uint64_t *d_offsets, size_t nseg, "
                                   "uint64_t max_seg_len, void *stream);",
    "rsx_sort_rows_pairs_device": "int rsx_sort_rows_pairs_device(rsx_ctx *ctx, void *d_keys, void *d_values, size_t rows, size_t row_len, "
                                  "uint32_t key_bytes, uint32_t key_kind, uint32_t value_bytes, int order, void *stream);",
    "rsx_argsort_rows_device": "int rsx_argsort_rows_device(rsx_ctx *ctx, const void *d_keys, void *d_index, size_t rows, size_t row_len, "
                               "uint32_t key_bytes, uint32_t key_kind, uint32_t index_bytes, int order, void *stream);",
    "rsx_segment_pairs_caps": "int rsx_segment_pairs_caps(uint32_t key_bytes, uint32_t value_bytes, uint32_t *caps);",
}


def test_the_five_symbols_are_declared_and_exported(lib):
    from radix_sort_amd import _lib
    header = " ".join(open(os.path.join(ROOT, "include", "rsx.h")).read().split())
    assert "#define RSX_VERSION 200" in header
    for name, proto in PROTOTYPES.items():
        assert " ".join(proto.split()) in header, name
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
    # the binding passes what the prototypes take (counting the context)
    for name, proto in PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == proto.count(",") + 1, name


def test_caps_are_those_of_the_joined_element(lib):
    from radix_sort_amd import _lib
    import radix_sort_amd as rs
    for kb in KEY_BYTES:
        for vb in TYPED_VALUE_BYTES:
            es = joined_elem(kb, vb)
            assert es, (kb, vb)
            caps = (ctypes.c_uint32 * _lib.SEG_CLASSES)()
            assert lib.rsx_segment_pairs_caps(kb, vb, caps) == 0
            want = (ctypes.c_uint32 * _lib.SEG_CLASSES)()
            lay = _lib.Layout(es, 0, kb, _lib.KEY_UNSIGNED)
            assert lib.rsx_segment_caps(ctypes.byref(lay), want) == 0
            assert list(caps) == list(want), (kb, vb, es)
            assert rs.segment_pairs_caps(kb, vb) == list(want)
            assert list(caps) == sorted(caps) and caps[0] > 1
    # values without a fused kernel ride behind a four-byte position
    for kb, vb in ((4, 20), (8, 100), (1, 3), (16, 12)):
        assert rs.segment_pairs_caps(kb, vb) == rs.segment_pairs_caps(kb, 4)


def test_caps_argument_errors(lib):
    import radix_sort_amd as rs
    caps = (ctypes.c_uint32 * 2)()
    assert lib.rsx_segment_pairs_caps(3, 4, caps) == ERR_ARG
    assert lib.rsx_segment_pairs_caps(0, 4, caps) == ERR_ARG
    assert lib.rsx_segment_pairs_caps(4, 32769, caps) == ERR_ARG
    assert lib.rsx_segment_pairs_caps(4, 4, None) == ERR_ARG
    with pytest.raises(rs.RsxError) as e:
        rs.segment_pairs_caps(3, 4)
    assert e.value.status == ERR_ARG


def test_null_context_is_an_argument_error(lib):
    assert lib.rsx_sort_segments_pairs_device(None, None, None, 10, 4, 0, 4, 0, None, 1, 0, None) == ERR_ARG
    assert lib.rsx_argsort_segments_device(None, None, None, 10, 4, 0, 8, 1, None, 1, 0, None) == ERR_ARG
    assert lib.rsx_sort_rows_pairs_device(None, None, None, 2, 5, 4, 0, 4, 0, None) == ERR_ARG
    assert lib.rsx_argsort_rows_device(None, None, None, 2, 5, 4, 0, 4, 0, None) == ERR_ARG


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
    k2 = torch.arange(24, dtype=torch.int32).reshape(4, 6)
    k1 = torch.arange(24, dtype=torch.int32)
    offs = torch.tensor([0, 10, 24], dtype=torch.int64)
    # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_sort_rows_pairs(k2, torch.zeros(4, 6))
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_sort_rows_pairs(k2, None, descending=True)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_argsort_rows(k2)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_sort_segments_pairs(k1, torch.zeros(24), offs)
    with pytest.raises(ValueError, match="GPU"):
        rs.radix_argsort_segments(k1, offs)
    # not tensors at all
    with pytest.raises(TypeError):
        rs.radix_sort_rows_pairs(np.zeros((4, 6), dtype=np.int32), None)
    with pytest.raises(TypeError):
        rs.radix_argsort_rows(np.zeros((4, 6), dtype=np.int32))
    with pytest.raises(TypeError):
        rs.radix_sort_segments_pairs(np.zeros(24, dtype=np.int32), None, offs)
    with pytest.raises(TypeError):
        rs.radix_sort_rows_pairs(k2, np.zeros((4, 6)))
    # mismatched leading shapes
    with pytest.raises(ValueError, match="leading shape"):
        rs.radix_sort_rows_pairs(k2, torch.zeros(4, 5))
    with pytest.raises(ValueError, match="leading shape"):
        rs.radix_sort_rows_pairs(k2, torch.zeros(6, 4))
    with pytest.raises(ValueError, match="leading shape"):
        rs.radix_sort_rows_pairs(k2, torch.zeros(4))
    with pytest.raises(ValueError, match="leading shape"):
        rs.radix_sort_segments_pairs(k1, torch.zeros(23), offs)
    with pytest.raises(ValueError, match="bytes"):
        rs.radix_sort_rows_pairs(k2, torch.zeros(4, 6, 0))
    with pytest.raises(ValueError, match="bytes"):
        rs.radix_sort_segments_pairs(k1, torch.zeros(24, 32769, dtype=torch.uint8), offs)
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_sort_rows_pairs(k2, torch.zeros(4, 12)[:, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        rs.radix_argsort_rows(torch.arange(48, dtype=torch.int32).reshape(4, 12)[:, ::2])
    with pytest.raises(TypeError, match="no RadixDigits"):
        rs.radix_argsort_rows(torch.zeros(4, 6, dtype=torch.float16))
    # wrong `out` dtype or shape
    with pytest.raises(TypeError, match="int32 or int64"):
        rs.radix_argsort_rows(k2, out=torch.zeros(4, 6, dtype=torch.float32))
    with pytest.raises(TypeError, match="int32 or int64"):
        rs.radix_argsort_segments(k1, offs, out=torch.zeros(24, dtype=torch.int16))
    with pytest.raises(ValueError, match="shape"):
        rs.radix_argsort_rows(k2, out=torch.zeros(6, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        rs.radix_argsort_rows(k2, out=torch.zeros(24, dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        rs.radix_argsort_segments(k1, offs, out=torch.zeros(23, dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        rs.radix_argsort_rows(k2, out=torch.zeros(4, 12, dtype=torch.int64)[:, ::2])
    # offsets of the wrong dtype / kind / shape
    with pytest.raises(TypeError, match="int64 or uint64"):
        rs.radix_sort_segments_pairs(k1, None, offs.to(torch.int32))
    with pytest.raises(TypeError, match="int64 or uint64"):
        rs.radix_argsort_segments(k1, offs.to(torch.float64))
    with pytest.raises(TypeError):
        rs.radix_argsort_segments(k1, [0, 10, 24])
    with pytest.raises(ValueError, match="1-D"):
        rs.radix_sort_segments_pairs(k1, None, offs.reshape(1, 3))
    with pytest.raises(ValueError, match="negative"):
        rs.radix_argsort_segments(k1, offs, max_seg_len=-1)
    with pytest.raises(ValueError, match="1-D"):
        rs.radix_argsort_segments(k2, offs)


def test_python_returns_without_a_device_where_nothing_is_to_do(no_context):
    """rows == 0, row_len <= 1 and nseg == 0 on CPU tensors whose device check passes trivially: nothing to sort."""
    import torch
    import radix_sort_amd as rs

    class Cuda(torch.Tensor):
        """A CPU tensor that says it is on a GPU: the early returns below must come before any context is made."""
        is_cuda = True

    def fake(t):
        return t.as_subclass(Cuda)

    assert rs.radix_sort_rows_pairs(fake(torch.zeros(0, 5, dtype=torch.int32)), None) is None
    assert rs.radix_sort_rows_pairs(fake(torch.zeros(7, 1, dtype=torch.int32)), fake(torch.zeros(7, 1))) is None
    assert rs.radix_sort_rows_pairs(fake(torch.zeros(7, 0, dtype=torch.int32)), None, descending=True) is None
    k1 = fake(torch.zeros(10, dtype=torch.int32))
    assert rs.radix_sort_segments_pairs(k1, None, fake(torch.zeros(1, dtype=torch.int64))) is None  # nseg == 0
    assert rs.radix_sort_segments_pairs(fake(torch.zeros(0, dtype=torch.int32)), None, fake(torch.zeros(3, dtype=torch.int64))) is None
