"""CPU: tests/compact_ref.py, the numpy restatement of rsx_compact_device's definition, held against cases written out by
hand: float specials on both sides of a bound, empty ranges, descending order, invert, and a partition that keeps both
sides in input order."""
import numpy as np

from compact_ref import compact_reference, expected_column, expected_index

#                  0 -NaN       1 -inf      2 -1.0      3 -0.0      4 +0.0      5 1.0       6 +inf      7 +NaN      8 -denormal 9 +denormal
F32 = np.array([0xFFC00000, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x3F800000, 0x7F800000, 0x7FC00000, 0x80000001, 0x00000001],
               dtype="<u4")


def f32(bits):
    return np.array([bits], dtype="<u4").view(np.uint8)


def rows(got):
    return got[0].tolist(), got[1]


def test_float_specials_on_both_sides_of_a_bound():
    k = F32.view(np.uint8)
    # from +0.0 on: -0.0 and the negative denormal are below it, +NaN is above +inf
    assert rows(compact_reference(10, "f32", k, lo=f32(0x00000000))) == ([4, 5, 6, 7, 9], 5)
    # below -0.0: -NaN is below -inf; -0.0 itself is not below itself, the negative denormal is
    assert rows(compact_reference(10, "f32", k, hi=f32(0x80000000))) == ([0, 1, 2, 8], 4)
    # [-inf, +inf): everything but the two NaNs and +inf
    assert rows(compact_reference(10, "f32", k, lo=f32(0xFF800000), hi=f32(0x7F800000))) == ([1, 2, 3, 4, 5, 8, 9], 7)
    # [-NaN, +NaN): everything but +NaN
    assert rows(compact_reference(10, "f32", k, lo=f32(0xFFC00000), hi=f32(0x7FC00000))) == ([0, 1, 2, 3, 4, 5, 6, 8, 9], 9)
    # [-0.0, +0.0): -0.0 alone
    assert rows(compact_reference(10, "f32", k, lo=f32(0x80000000), hi=f32(0x00000000))) == ([3], 1)


def test_empty_ranges():
    k = np.array([5, 1, 9, 3, 5], dtype="<u4")
    five, three = np.array([5], dtype="<u4"), np.array([3], dtype="<u4")
    assert rows(compact_reference(5, "u32", k, lo=five, hi=five)) == ([], 0)    # lo == hi
    assert rows(compact_reference(5, "u32", k, lo=five, hi=three)) == ([], 0)   # lo above hi
    assert rows(compact_reference(5, "u32", k, lo=five, hi=three, invert=True)) == ([0, 1, 2, 3, 4], 5)
    assert rows(compact_reference(0, "u32", k[:0], lo=five)) == ([], 0)


def test_signed_and_wide_keys():
    k = np.array([-3, 7, 0, -128, 127], dtype="<i1")
    assert rows(compact_reference(5, "i8", k, lo=np.array([0], dtype="<i1"))) == ([1, 2, 4], 3)
    assert rows(compact_reference(5, "i8", k, hi=np.array([-3], dtype="<i1"))) == ([3], 1)
    w = np.zeros((4, 16), dtype=np.uint8)
    w[0, 15], w[1, 0], w[2, 8], w[3, 7] = 1, 255, 1, 255  # 2^120, 255, 2^64, 255 * 2^56
    bound = np.zeros(16, dtype=np.uint8)
    bound[8] = 1  # 2^64: the high half decides first
    assert rows(compact_reference(4, "u128", w, lo=bound)) == ([0, 2], 2)
    assert rows(compact_reference(4, "u128", w, hi=bound)) == ([1, 3], 2)


def test_descending_turns_both_comparisons_round():
    k = np.array([5, 1, 9, 3], dtype="<u4")
    five, three = np.array([5], dtype="<u4"), np.array([3], dtype="<u4")
    assert rows(compact_reference(4, "u32", k, lo=five, descending=True)) == ([0, 1, 3], 3)   # key <= 5
    assert rows(compact_reference(4, "u32", k, hi=three, descending=True)) == ([0, 2], 2)     # key > 3
    assert rows(compact_reference(4, "u32", k, lo=five, hi=three, descending=True)) == ([0], 1)  # 3 < key <= 5
    assert rows(compact_reference(4, "u32", k, lo=three, hi=five, descending=True)) == ([], 0)
    f = F32.view(np.uint8)
    assert rows(compact_reference(10, "f32", f, lo=f32(0x80000000), descending=True)) == ([0, 1, 2, 3, 8], 5)  # -0.0 and everything below


def test_mask_invert_and_num():
    mask = np.array([1, 0, 2, 0x80, 0, 1], dtype=np.uint8)  # any non-zero byte passes
    assert rows(compact_reference(6, mask=mask)) == ([0, 2, 3, 5], 4)
    assert rows(compact_reference(6, mask=mask, invert=True)) == ([1, 4], 2)
    assert rows(compact_reference(6, mask=mask, num=3)) == ([0, 2], 2)
    assert rows(compact_reference(6, mask=mask, num=0)) == ([], 0)
    assert rows(compact_reference(6, mask=mask, num=11)) == ([0, 2, 3, 5], 4)
    assert rows(compact_reference(6)) == ([0, 1, 2, 3, 4, 5], 6)  # no predicate: a copy
    assert rows(compact_reference(6, invert=True)) == ([], 0)
    k = np.array([5, 1, 9, 3, 5, 7], dtype="<u4")
    assert rows(compact_reference(6, "u32", k, mask=mask, lo=np.array([5], dtype="<u4"))) == ([0, 2, 5], 3)  # mask and range together


def test_partition_keeps_both_sides_in_input_order():
    mask = np.array([0, 1, 0, 1, 1, 0, 0], dtype=np.uint8)
    assert rows(compact_reference(7, mask=mask, partition=True)) == ([1, 3, 4, 0, 2, 5, 6], 3)
    assert rows(compact_reference(7, mask=mask, partition=True, invert=True)) == ([0, 2, 5, 6, 1, 3, 4], 4)
    assert rows(compact_reference(7, mask=mask, partition=True, num=4)) == ([1, 3, 0, 2], 2)  # rows behind N are in neither part


def test_expected_columns_leave_the_tail_alone():
    r = np.array([2, 0], dtype=np.int64)
    vals = np.arange(12, dtype=np.uint8)  # 4 rows of 3 bytes
    assert expected_column(vals, 3, 4, r).tolist() == [6, 7, 8, 0, 1, 2] + [0xA5] * 6
    assert expected_index(3, 4, r).view("<i4").tolist() == [2, 0, np.array([0xA5A5A5A5], dtype="<u4").view("<i4")[0]]
    assert expected_index(2, 8, r).view("<i8").tolist() == [2, 0]
