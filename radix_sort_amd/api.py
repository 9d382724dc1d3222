"""Python host mirror of the reference's operator interface over the C-ABI.

Reference interface (src/radix_sort/mod.rs:18-20, radix_digits.rs:1-5):

    pub trait RadixDigits { const NUMBER_OF_DIGITS: u8; fn get_digit(&self, index: u8) -> u8; }
    pub trait RadixSort<T: RadixDigits> { fn radix_sort(&mut self); }   // impl for [T]

Here `RadixDigits` is a descriptor (what the Rust shim forwards as `rsx_layout`)
and `radix_sort(x)` sorts `x` in place, ascending, stably, by the mapped key --
same name, same argument meaning, blocking for host arrays like mod.rs:62.
torch is used for device memory and streams only.
"""
from __future__ import annotations

import ctypes
import math
import operator
import threading
from collections import namedtuple
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import KEY_FLOAT, KEY_SIGNED, KEY_UNSIGNED, Layout, RsxError


@dataclass(frozen=True)
class RadixDigits:
    """Key model of one element type (radix_digits.rs).  NUMBER_OF_DIGITS == key_bytes."""
    elem_bytes: int
    key_offset: int
    key_bytes: int
    key_kind: int

    @property
    def NUMBER_OF_DIGITS(self) -> int:  # noqa: N802 (reference name)
        return self.key_bytes

    def layout(self) -> Layout:
        return Layout(self.elem_bytes, self.key_offset, self.key_bytes, self.key_kind)

    def get_digit(self, element: bytes, index: int) -> int:
        """radix_digits.rs get_digit on the little-endian bytes of one element (host-side helper)."""
        k = element[self.key_offset:self.key_offset + self.key_bytes]
        top = self.key_bytes - 1
        b = k[index]
        if self.key_kind == KEY_SIGNED:
            if index == top:
                b ^= 0x80
        elif self.key_kind == KEY_FLOAT:
            if k[top] & 0x80:
                b ^= 0xFF
            elif index == top:
                b ^= 0x80
        return b


def _prim(name: str) -> RadixDigits:
    kinds = {"u": KEY_UNSIGNED, "i": KEY_SIGNED, "f": KEY_FLOAT}
    bits = int(name[1:])
    return RadixDigits(bits // 8, 0, bits // 8, kinds[name[0]])


#: the reference's built-in impls (radix_digits.rs:7-124); usize/isize are 64-bit
PRIMITIVES = {n: _prim(n) for n in
              ("u8", "u16", "u32", "u64", "u128", "i8", "i16", "i32", "i64", "i128", "f32", "f64")}
PRIMITIVES["usize"] = PRIMITIVES["u64"]
PRIMITIVES["isize"] = PRIMITIVES["i64"]


def tuple_of(key: str, payload_bytes: int, key_offset: Optional[int] = None,
             elem_bytes: Optional[int] = None) -> RadixDigits:
    """`(K, U)` (radix_digits.rs:126-136): key `.0` of primitive `key`, opaque payload.
    Default layout = key first, payload after it, size rounded up to the key alignment
    (what rustc does for (K, U) with size_of::<U>() <= size_of::<K>(); pass explicit
    offsets for anything else -- Rust tuple layout is not ABI-stable)."""
    k = PRIMITIVES[key]
    off = 0 if key_offset is None else key_offset
    if elem_bytes is None:
        al = min(k.key_bytes, 16)
        elem_bytes = -(-(k.key_bytes + payload_bytes) // al) * al
    return RadixDigits(elem_bytes, off, k.key_bytes, k.key_kind)


_NP_KIND = {"u": KEY_UNSIGNED, "i": KEY_SIGNED, "f": KEY_FLOAT}


def digits_of(dtype) -> RadixDigits:
    """RadixDigits of a numpy dtype: primitives, or a structured dtype whose FIRST field is the key."""
    dt = np.dtype(dtype)
    if dt.fields:
        name0 = dt.names[0]
        kdt, koff = dt.fields[name0][0], dt.fields[name0][1]
        if kdt.kind not in _NP_KIND or kdt.itemsize not in (1, 2, 4, 8):
            if kdt.kind == "V" and not kdt.fields and 1 <= kdt.itemsize <= 16:  # V1..V16: unsigned key of that width
                return RadixDigits(dt.itemsize, koff, kdt.itemsize, KEY_UNSIGNED)  # (V16: u128 stored as 16 raw bytes)
            raise TypeError(f"unsupported key field dtype {kdt}")
        return RadixDigits(dt.itemsize, koff, kdt.itemsize, _NP_KIND[kdt.kind])
    if dt.kind in _NP_KIND and dt.itemsize in (1, 2, 4, 8):
        if dt.kind == "f" and dt.itemsize not in (4, 8):
            raise TypeError(f"unsupported float width {dt}")
        return RadixDigits(dt.itemsize, 0, dt.itemsize, _NP_KIND[dt.kind])
    raise TypeError(f"no RadixDigits for dtype {dt}; pass digits= explicitly")


class Context:
    """rsx_ctx: owns the device workspace (replaces the per-call temp alloc of mod.rs:71-82)."""

    def __init__(self, device: int = -1):
        self._L = _lib.load()
        h = ctypes.c_void_p()
        rc = self._L.rsx_ctx_create(device, ctypes.byref(h))
        _check_rc(self._L, rc)
        self._h = h

    def _check(self, rc: int):
        if rc != 0:
            raise RsxError(rc, f"{self._L.rsx_strerror(rc).decode()} ({self._L.rsx_last_error(self._h).decode()})")

    def close(self):
        if getattr(self, "_h", None):
            self._L.rsx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- raw C-ABI calls (pointers are ints) ------------------------------------
    def reserve(self, n: int, d: RadixDigits):
        lay = d.layout()
        self._check(self._L.rsx_ctx_reserve(self._h, n, ctypes.byref(lay)))

    def check(self, stream: int = 0):
        """rsx_ctx_check: synchronises `stream` and raises if a kernel of this context gave up a
        device-side wait (the stream-ordered entry points cannot report that by themselves)."""
        self._check(self._L.rsx_ctx_check(self._h, stream))

    def set_option(self, option: int, value: int):
        """rsx_ctx_set_option (OPT_* in _lib): forces one of the bit-exact alternative kernel paths."""
        self._check(self._L.rsx_ctx_set_option(self._h, option, value))

    def get_info(self, what: int) -> int:
        out = ctypes.c_uint64(0)
        self._check(self._L.rsx_ctx_get_info(self._h, what, ctypes.byref(out)))
        return int(out.value)

    def profile(self, enable: bool):
        """Per-launch HIP-event timing on/off (rsx_ctx_profile); enabling clears the counters."""
        self._check(self._L.rsx_ctx_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        """-> {kind: (total_ms, launches)} for kinds hist/scan/sweep/other."""
        ms = (ctypes.c_double * _lib.PROF_KINDS)()
        cnt = (ctypes.c_uint64 * _lib.PROF_KINDS)()
        self._check(self._L.rsx_ctx_profile_read(self._h, ms, cnt))
        names = ("hist", "scan", "sweep", "other")
        return {names[k]: (ms[k], int(cnt[k])) for k in range(_lib.PROF_KINDS)}

    def sort_device(self, d_data: int, d_tmp: int, n: int, d: RadixDigits, stream: int = 0):
        lay = d.layout()
        self._check(self._L.rsx_sort_device(self._h, d_data, d_tmp, n, ctypes.byref(lay), stream))

    def sort_host(self, ptr: int, n: int, d: RadixDigits):
        lay = d.layout()
        self._check(self._L.rsx_sort_host(self._h, ptr, n, ctypes.byref(lay)))

    def histogram_device(self, d_src: int, n: int, d: RadixDigits, digit: int, d_hist: int, stream: int = 0):
        lay = d.layout()
        self._check(self._L.rsx_histogram_device(self._h, d_src, n, ctypes.byref(lay), digit, d_hist, stream))

    def partition_device(self, d_src: int, d_dst: int, n: int, d: RadixDigits, digit: int, d_hist: int = 0,
                         stream: int = 0):
        lay = d.layout()
        self._check(self._L.rsx_partition_device(self._h, d_src, d_dst, n, ctypes.byref(lay), digit, d_hist, stream))

    def partition_count_device(self, d_src: int, n: int, d: RadixDigits, digit: int, nsub: int, d_hist: int, stream: int = 0):
        lay = d.layout()
        self._check(self._L.rsx_partition_count_device(self._h, d_src, n, ctypes.byref(lay), digit, nsub, d_hist, stream))

    def partition_scatter_device(self, d_src: int, d_dst: int, n: int, d: RadixDigits, digit: int, nsub: int, k: int,
                                 stream: int = 0):
        lay = d.layout()
        self._check(self._L.rsx_partition_scatter_device(self._h, d_src, d_dst, n, ctypes.byref(lay), digit, nsub, k, stream))

    def splitter_count_device(self, d_data: int, n: int, d: RadixDigits, d_ranges: int, d_prefix: int, nb: int, digit: int,
                              d_less: int, stream: int = 0):
        lay = d.layout()
        self._check(self._L.rsx_splitter_count_device(self._h, d_data, n, ctypes.byref(lay), d_ranges, d_prefix, nb, digit,
                                                      d_less, stream))

    def splitter_pick_device(self, d_total: int, d_rank: int, d_prefix: int, nb: int, digit: int, stream: int = 0):
        self._check(self._L.rsx_splitter_pick_device(self._h, d_total, d_rank, d_prefix, nb, digit, stream))

    def segmented_copy_device(self, d_src: int, d_dst: int, elem_bytes: int, d_src_off: int, d_dst_off: int,
                              d_len: int, nseg: int, stream: int = 0):
        self._check(self._L.rsx_segmented_copy_device(self._h, d_src, d_dst, elem_bytes, d_src_off, d_dst_off,
                                                      d_len, nseg, stream))

    def bounds_device(self, d_sorted: int, n: int, d: RadixDigits, d_queries: int, nq: int, d_out: int, stream: int = 0):
        lay = d.layout()
        self._check(self._L.rsx_bounds_device(self._h, d_sorted, n, ctypes.byref(lay), d_queries, nq, d_out, stream))

    def bounds_ranges_device(self, d_data: int, n: int, d: RadixDigits, d_queries: int, d_ranges: int, nq: int, d_out: int,
                             stream: int = 0):
        lay = d.layout()
        self._check(self._L.rsx_bounds_ranges_device(self._h, d_data, n, ctypes.byref(lay), d_queries, d_ranges, nq, d_out,
                                                     stream))

    def generate_device(self, d_data: int, n: int, d: RadixDigits, gen: int, seed: int, param: float = 0.0,
                        index_base: int = 0, stream: int = 0):
        lay = d.layout()
        self._check(self._L.rsx_generate_device(self._h, d_data, n, ctypes.byref(lay), gen, seed, param,
                                                index_base, stream))

    def verify_device(self, d_data: int, n: int, d: RadixDigits, d_out: int, stream: int = 0):
        lay = d.layout()
        self._check(self._L.rsx_verify_device(self._h, d_data, n, ctypes.byref(lay), d_out, stream))

    def sort_segments_device(self, d_data: int, d_tmp: int, n: int, d: RadixDigits, d_offsets: int, nseg: int,
                             max_seg_len: int = 0, stream: int = 0):
        """rsx_sort_segments_device: every segment [offsets[i], offsets[i+1]) of the n elements sorted on its own;
        d_offsets: nseg + 1 uint64 on the device."""
        lay = d.layout()
        self._check(self._L.rsx_sort_segments_device(self._h, d_data, d_tmp, n, ctypes.byref(lay), d_offsets, nseg,
                                                     max_seg_len, stream))

    def sort_rows_device(self, d_data: int, d_tmp: int, rows: int, row_len: int, d: RadixDigits, stream: int = 0):
        """rsx_sort_rows_device: `rows` back-to-back segments of `row_len` elements each."""
        lay = d.layout()
        self._check(self._L.rsx_sort_rows_device(self._h, d_data, d_tmp, rows, row_len, ctypes.byref(lay), stream))


    def reserve_pairs(self, n: int, key_bytes: int, value_bytes: int):
        """rsx_ctx_reserve_pairs: workspace for sort_pairs_device / argsort_device of up to n pairs (argsort:
        value_bytes = index_bytes), so that the call allocates nothing and can be captured into a graph.  The segmented
        and row forms (radix_sort_rows_pairs, radix_argsort_rows, radix_sort_segments_pairs, radix_argsort_segments)
        need it only where a segment can exceed segment_pairs_caps(...)[-1] or the values are wider than 16 bytes; n is
        then the length of the whole key column."""
        self._check(self._L.rsx_ctx_reserve_pairs(self._h, n, key_bytes, value_bytes))

    def sort_pairs_device(self, d_keys: int, d_values: int, n: int, key_bytes: int, key_kind: int, value_bytes: int,
                          descending: bool = False, stream: int = 0):
        """rsx_sort_pairs_device: n keys and n values in separate device arrays, both sorted in place by key
        (d_values 0 and value_bytes 0: keys only)."""
        self._check(self._L.rsx_sort_pairs_device(self._h, d_keys, d_values or None, n, key_bytes, key_kind, value_bytes,
                                                  1 if descending else 0, stream))

    def argsort_device(self, d_keys: int, d_index: int, n: int, key_bytes: int, key_kind: int, index_bytes: int,
                       descending: bool = False, stream: int = 0):
        """rsx_argsort_device: the stable sorting permutation of n keys as index_bytes-wide integers; keys untouched."""
        self._check(self._L.rsx_argsort_device(self._h, d_keys, d_index, n, key_bytes, key_kind, index_bytes,
                                               1 if descending else 0, stream))

    def sort_segments_pairs_device(self, d_keys: int, d_values: int, n: int, key_bytes: int, key_kind: int, value_bytes: int,
                                   d_offsets: int, nseg: int, descending: bool = False, max_seg_len: int = 0, stream: int = 0):
        """rsx_sort_segments_pairs_device: every segment of the key column sorted on its own, the value column with it
        (d_values 0 and value_bytes 0: keys only)."""
        self._check(self._L.rsx_sort_segments_pairs_device(self._h, d_keys, d_values or None, n, key_bytes, key_kind, value_bytes,
                                                           1 if descending else 0, d_offsets, nseg, max_seg_len, stream))

    def argsort_segments_device(self, d_keys: int, d_index: int, n: int, key_bytes: int, key_kind: int, index_bytes: int,
                                d_offsets: int, nseg: int, descending: bool = False, max_seg_len: int = 0, stream: int = 0):
        """rsx_argsort_segments_device: every segment's stable sorting permutation as positions inside the segment."""
        self._check(self._L.rsx_argsort_segments_device(self._h, d_keys, d_index, n, key_bytes, key_kind, index_bytes,
                                                        1 if descending else 0, d_offsets, nseg, max_seg_len, stream))

    def sort_rows_pairs_device(self, d_keys: int, d_values: int, rows: int, row_len: int, key_bytes: int, key_kind: int,
                               value_bytes: int, descending: bool = False, stream: int = 0):
        """rsx_sort_rows_pairs_device: `rows` back-to-back segments of `row_len` keys (and values) each."""
        self._check(self._L.rsx_sort_rows_pairs_device(self._h, d_keys, d_values or None, rows, row_len, key_bytes, key_kind,
                                                       value_bytes, 1 if descending else 0, stream))

    def argsort_rows_device(self, d_keys: int, d_index: int, rows: int, row_len: int, key_bytes: int, key_kind: int,
                            index_bytes: int, descending: bool = False, stream: int = 0):
        """rsx_argsort_rows_device: torch.sort(dim=-1).indices of a (rows, row_len) key array."""
        self._check(self._L.rsx_argsort_rows_device(self._h, d_keys, d_index, rows, row_len, key_bytes, key_kind, index_bytes,
                                                    1 if descending else 0, stream))


    def reserve_topk(self, rows: int, row_len: int, k: int, key_bytes: int):
        """rsx_ctx_reserve_topk: the context's first-call set-up and, for rows above topk_caps(key_bytes)[0][-1], the two
        candidate arrays of topk_rows_device for this shape, so that the call allocates nothing and can be captured."""
        self._check(self._L.rsx_ctx_reserve_topk(self._h, rows, row_len, k, key_bytes))

    def topk_rows_device(self, d_keys: int, d_out_keys: int, d_out_index: int, rows: int, row_len: int, k: int, key_bytes: int,
                         key_kind: int, index_bytes: int, descending: bool = False, stream: int = 0):
        """rsx_topk_rows_device: the first k columns of every row's stable sort -- the keys into d_out_keys and their
        positions in the row into d_out_index (either may be 0: not produced); d_keys is only read."""
        self._check(self._L.rsx_topk_rows_device(self._h, d_keys, d_out_keys or None, d_out_index or None, rows, row_len, k, key_bytes,
                                                 key_kind, index_bytes, 1 if descending else 0, stream))

    def reserve_select(self, n: int, key_bytes: int):
        """rsx_ctx_reserve_select: the context's first-call set-up and the workspace of select_device on up to n keys of this
        width, so that the call allocates nothing and can be captured."""
        self._check(self._L.rsx_ctx_reserve_select(self._h, n, key_bytes))

    def select_device(self, d_keys: int, n: int, key_bytes: int, key_kind: int, ranks, d_out_keys: int, d_out_index: int,
                      index_bytes: int, descending: bool = False, stream: int = 0):
        """rsx_select_device: for every rank of `ranks` (host integers, at most select_caps(key_bytes)[0] of them) the key
        at that position of the stable sort of the n keys into d_out_keys and its input position into d_out_index (either
        may be 0: not produced); d_keys is only read."""
        host = (ctypes.c_uint64 * max(1, len(ranks)))(*ranks)
        self._check(self._L.rsx_select_device(self._h, d_keys or None, n, key_bytes, key_kind, host, len(ranks), d_out_keys or None,
                                              d_out_index or None, index_bytes, 1 if descending else 0, stream))

    def bin_count_device(self, d_keys: int, n: int, key_bytes: int, key_kind: int, d_edges: int, m: int, mode: int, d_counts: int,
                         count_bytes: int, descending: bool = False, d_num: int = 0, flags: int = 0, stream: int = 0):
        """rsx_bin_count_device: the number of the first n (or min(n, *d_num)) keys in each of the m + 1 bins of `mode`
        (BIN_UPPER / BIN_LOWER: between the m sorted edges at d_edges; BIN_INDEX: the key's own value, d_edges 0) into the
        m + 1 counts of count_bytes at d_counts, overwritten unless flags has BIN_ACCUMULATE; no workspace."""
        self._check(self._L.rsx_bin_count_device(self._h, d_keys or None, n, d_num or None, key_bytes, key_kind, d_edges or None, m, mode,
                                                 1 if descending else 0, d_counts or None, count_bytes, flags, stream))

    def reserve_compact(self, n: int, key_bytes: int = 0, value_bytes: int = 0, index_bytes: int = 0):
        """rsx_ctx_reserve_compact: the context's first-call set-up and the workspace of compact_device on up to n rows with
        keys, values and indices of these widths (0: the calls have no such column), so that the call allocates nothing
        and can be captured."""
        self._check(self._L.rsx_ctx_reserve_compact(self._h, n, key_bytes, value_bytes, index_bytes))

    def compact_device(self, d_keys: int, n: int, key_bytes: int, key_kind: int, d_flags: int, d_lo: int, d_hi: int, d_values: int,
                       value_bytes: int, d_out_keys: int, d_out_values: int, d_out_index: int, index_bytes: int, d_out_num: int,
                       descending: bool = False, d_num: int = 0, flags: int = 0, stream: int = 0):
        """rsx_compact_device: of the first n (or min(n, *d_num)) rows those whose flag byte at d_flags is non-zero and whose
        key lies in [*d_lo, *d_hi) (each of the three may be 0: no such condition; flags COMPACT_INVERT: the others), in
        input order -- keys, values and positions into the outputs that are not 0, their number into d_out_num; flags
        COMPACT_PARTITION: the remaining rows behind them, in input order too.  Not in place."""
        self._check(self._L.rsx_compact_device(self._h, d_keys or None, n, d_num or None, key_bytes, key_kind, 1 if descending else 0,
                                               d_flags or None, d_lo or None, d_hi or None, d_values or None, value_bytes, flags,
                                               d_out_keys or None, d_out_values or None, d_out_index or None, index_bytes, d_out_num or None,
                                               stream))

    def reserve_multisplit(self, n: int, m: int, key_bytes: int, value_bytes: int = 0, index_bytes: int = 0):
        """rsx_ctx_reserve_multisplit: the context's first-call set-up and the workspace of multisplit_device on up to n rows
        and m edges (index mode: m values) with keys, values and indices of these widths (0: the calls have no such
        column), so that the call allocates nothing and can be captured."""
        self._check(self._L.rsx_ctx_reserve_multisplit(self._h, n, m, key_bytes, value_bytes, index_bytes))

    def multisplit_device(self, d_keys: int, n: int, key_bytes: int, key_kind: int, d_edges: int, m: int, mode: int, d_values: int,
                          value_bytes: int, d_out_keys: int, d_out_values: int, d_out_index: int, index_bytes: int, d_out_offsets: int,
                          descending: bool = False, d_num: int = 0, stream: int = 0):
        """rsx_multisplit_device: the first n (or min(n, *d_num)) rows regrouped by the bin of their key (`mode` and the m
        edges at d_edges as in bin_count_device), in input order inside each bin -- keys, values and positions into the
        outputs that are not 0, the m + 2 offsets of the bins (uint64) into d_out_offsets.  Not in place."""
        self._check(self._L.rsx_multisplit_device(self._h, d_keys or None, n, d_num or None, key_bytes, key_kind, d_edges or None, m, mode,
                                                  1 if descending else 0, d_values or None, value_bytes, d_out_keys or None,
                                                  d_out_values or None, d_out_index or None, index_bytes, d_out_offsets or None, stream))

    def reserve_bin_reduce(self, n: int, m: int, key_bytes: int, value_bytes: int):
        """rsx_ctx_reserve_bin_reduce: the context's first-call set-up and the workspace of bin_reduce_device on up to n rows
        and m edges (index mode: m values) with keys and values of these widths, so that the call allocates nothing and
        can be captured."""
        self._check(self._L.rsx_ctx_reserve_bin_reduce(self._h, n, m, key_bytes, value_bytes))

    def bin_reduce_device(self, d_keys: int, d_values: int, n: int, key_bytes: int, key_kind: int, d_edges: int, m: int, mode: int,
                          value_bytes: int, value_kind: int, op: int, d_out_values: int, d_out_counts: int = 0, count_bytes: int = 8,
                          descending: bool = False, d_num: int = 0, flags: int = 0, stream: int = 0):
        """rsx_bin_reduce_device: the values of the first n (or min(n, *d_num)) rows combined by `op` (REDUCE_SUM / MIN / MAX)
        per bin of their key (`mode` and the m edges at d_edges as in bin_count_device) into the m + 1 values at
        d_out_values, an empty bin holding the operator's identity; the bins' sizes into the m + 1 counts of count_bytes at
        d_out_counts unless it is 0.  flags BIN_ACCUMULATE: combined onto / added to what the outputs hold."""
        self._check(self._L.rsx_bin_reduce_device(self._h, d_keys or None, d_values or None, n, d_num or None, key_bytes, key_kind,
                                                  d_edges or None, m, mode, 1 if descending else 0, value_bytes, value_kind, op,
                                                  d_out_values or None, d_out_counts or None, count_bytes, flags, stream))

    def reserve_unique(self, n: int, key_bytes: int, with_positions: bool = True):
        """rsx_ctx_reserve_unique: the context's first-call set-up and the workspace of unique_device on up to n keys of this
        width, by the route with positions (perm or inverse asked for) or keys only, so that the call allocates nothing and
        can be captured."""
        self._check(self._L.rsx_ctx_reserve_unique(self._h, n, key_bytes, 1 if with_positions else 0))

    def unique_device(self, d_keys: int, n: int, key_bytes: int, key_kind: int, d_out_keys: int, d_out_offsets: int, d_out_perm: int,
                      d_out_inverse: int, index_bytes: int, d_out_num: int, descending: bool = False, stream: int = 0):
        """rsx_unique_device: the groups of equal keys of the stable sort of n keys -- the distinct keys, the CSR offsets of
        the groups, the sorting permutation, the group of every input position (each output may be 0: not produced) and
        their number m into d_out_num; d_keys is only read."""
        self._check(self._L.rsx_unique_device(self._h, d_keys or None, n, key_bytes, key_kind, 1 if descending else 0, d_out_keys or None,
                                              d_out_offsets or None, d_out_perm or None, d_out_inverse or None, index_bytes,
                                              d_out_num or None, stream))

    def reserve_search(self, m: int, key_bytes: int):
        """rsx_ctx_reserve_search: the context's first-call set-up and the workspace of search_sorted_device with
        SEARCH_PRESORT on up to m needles of this width, so that the call allocates nothing and can be captured."""
        self._check(self._L.rsx_ctx_reserve_search(self._h, m, key_bytes))

    def search_sorted_device(self, d_sorted: int, n: int, d_needles: int, m: int, key_bytes: int, key_kind: int, d_out_lower: int,
                             d_out_upper: int, index_bytes: int, descending: bool = False, d_sorted_num: int = 0, flags: int = 0,
                             stream: int = 0):
        """rsx_search_sorted_device: for each of m needles the number of the first n (or min(n, *d_sorted_num)) sorted keys
        that order before it (d_out_lower) and that do not order behind it (d_out_upper); either output may be 0."""
        self._check(self._L.rsx_search_sorted_device(self._h, d_sorted or None, n, d_sorted_num or None, d_needles or None, m, key_bytes,
                                                     key_kind, 1 if descending else 0, d_out_lower or None, d_out_upper or None,
                                                     index_bytes, flags, stream))

    def reserve_merge(self, n_total: int, key_bytes: int, value_bytes: int = 0):
        """rsx_ctx_reserve_merge: the context's first-call set-up and the workspace of merge_device into up to n_total
        outputs of these widths (values of 1, 2, 4, 8, 16 bytes need none), so that the call allocates nothing and can be
        captured."""
        self._check(self._L.rsx_ctx_reserve_merge(self._h, n_total, key_bytes, value_bytes))

    def merge_device(self, d_a_keys: int, d_a_values: int, na: int, d_b_keys: int, d_b_values: int, nb: int, key_bytes: int,
                     key_kind: int, value_bytes: int, d_out_keys: int, d_out_values: int, d_out_index: int, index_bytes: int = 8,
                     descending: bool = False, stream: int = 0):
        """rsx_merge_device: the stable merge of two sorted key arrays (equal keys of a first) -- the merged keys, the
        values moved with them and the position of every output in a ++ b (each output may be 0: not produced); the inputs
        are only read and no output may overlap them."""
        self._check(self._L.rsx_merge_device(self._h, d_a_keys or None, d_a_values or None, na, d_b_keys or None, d_b_values or None, nb,
                                             key_bytes, key_kind, value_bytes, 1 if descending else 0, d_out_keys or None,
                                             d_out_values or None, d_out_index or None, index_bytes, stream))

    def reserve_setop(self, n_total: int, key_bytes: int):
        """rsx_ctx_reserve_setop: the context's first-call set-up and the workspace of setop_device on up to n_total =
        na + nb keys of this width, so that the call allocates nothing and can be captured."""
        self._check(self._L.rsx_ctx_reserve_setop(self._h, n_total, key_bytes))

    def setop_device(self, op: int, d_a_keys: int, d_a_values: int, na: int, d_a_num: int, d_b_keys: int, d_b_values: int, nb: int,
                     d_b_num: int, key_bytes: int, key_kind: int, value_bytes: int, d_out_keys: int, d_out_values: int, d_out_index: int,
                     index_bytes: int, d_out_num: int, descending: bool = False, stream: int = 0):
        """rsx_setop_device: union (op 0), intersection (1), difference (2) or symmetric difference (3) of two sorted key
        arrays as multisets -- the kept keys in merge order, their values, their positions in a ++ b (each output may be
        0: not produced) and their number into d_out_num; d_a_num / d_b_num (0: none) are device words that bound the
        inputs.  The inputs are only read and no output may overlap them."""
        self._check(self._L.rsx_setop_device(self._h, op, d_a_keys or None, d_a_values or None, na, d_a_num or None, d_b_keys or None,
                                             d_b_values or None, nb, d_b_num or None, key_bytes, key_kind, value_bytes,
                                             1 if descending else 0, d_out_keys or None, d_out_values or None, d_out_index or None,
                                             index_bytes, d_out_num or None, stream))

    def reserve_join(self, na: int, key_bytes: int):
        """rsx_ctx_reserve_join: the context's first-call set-up and the workspace of join_device with up to na keys of this
        width on its left side, so that the call allocates nothing and can be captured."""
        self._check(self._L.rsx_ctx_reserve_join(self._h, na, key_bytes))

    def join_device(self, how: int, d_a_keys: int, na: int, d_a_num: int, d_a_index: int, d_b_keys: int, nb: int, d_b_num: int,
                    d_b_index: int, key_bytes: int, key_kind: int, d_out_a: int, d_out_b: int, index_bytes: int, capacity: int,
                    d_out_num: int, descending: bool = False, stream: int = 0):
        """rsx_join_device: the inner (how 0), left (1), semi (2) or anti (3) join of two sorted key arrays -- for every row
        its position in a (d_out_a) and in b (d_out_b; all ones: none), or the words of d_a_index / d_b_index at those
        positions, up to `capacity` rows, and the FULL number of rows into d_out_num.  Both outputs 0 with capacity 0: the
        count alone.  d_a_num / d_b_num (0: none) are device words that bound the inputs, which are only read."""
        self._check(self._L.rsx_join_device(self._h, how, d_a_keys or None, na, d_a_num or None, d_a_index or None, d_b_keys or None, nb,
                                            d_b_num or None, d_b_index or None, key_bytes, key_kind, 1 if descending else 0,
                                            d_out_a or None, d_out_b or None, index_bytes, capacity, d_out_num or None, stream))

    def reserve_reduce(self, n: int, key_bytes: int, value_bytes: int):
        """rsx_ctx_reserve_reduce: the context's first-call set-up and the workspace of reduce_by_key_device on up to n keys
        of these widths, so that the call allocates nothing and can be captured."""
        self._check(self._L.rsx_ctx_reserve_reduce(self._h, n, key_bytes, value_bytes))

    def reduce_by_key_device(self, d_keys: int, d_values: int, n: int, key_bytes: int, key_kind: int, value_bytes: int, value_kind: int,
                             op: int, d_out_keys: int, d_out_values: int, d_out_offsets: int, d_out_num: int, descending: bool = False,
                             stream: int = 0):
        """rsx_reduce_by_key_device: the sum (op 0), minimum (1) or maximum (2) of the values of every group of equal keys
        of the stable sort of n keys -- the distinct keys, one value per group, the CSR offsets of the groups (each output
        may be 0: not produced, but not both keys and values) and their number m into d_out_num; d_keys and d_values are
        only read, and may be the outputs."""
        self._check(self._L.rsx_reduce_by_key_device(self._h, d_keys or None, d_values or None, n, key_bytes, key_kind, value_bytes,
                                                     value_kind, op, 1 if descending else 0, d_out_keys or None, d_out_values or None,
                                                     d_out_offsets or None, d_out_num or None, stream))

    def reserve_scan_by_key(self, n: int, key_bytes: int, value_bytes: int, runs: bool = False):
        """rsx_ctx_reserve_scan_by_key: the context's first-call set-up and the workspace of scan_by_key_device on up to n
        keys of these widths under this group rule, so that the call allocates nothing and can be captured."""
        self._check(self._L.rsx_ctx_reserve_scan_by_key(self._h, n, key_bytes, value_bytes, _lib.SCAN_RUNS if runs else 0))

    def scan_by_key_device(self, d_keys: int, d_values: int, n: int, key_bytes: int, key_kind: int, value_bytes: int, value_kind: int,
                           op: int, flags: int, first: int, d_out: int, d_out_num: int = 0, stream: int = 0):
        """rsx_scan_by_key_device: for every position the running sum (op 0), minimum (1) or maximum (2) of the values of
        its group up to it, into d_out at that position -- the group being every position with the same key, or under
        SCAN_RUNS the run of consecutive equal keys; SCAN_EXCLUSIVE: the result of the predecessor in the group, the low
        value_bytes bytes of `first` at a group's first position.  d_values 0: every value is 1 (ranks).  d_out_num (0:
        none) receives the number of groups.  d_keys and d_values are only read; d_out may be d_values."""
        self._check(self._L.rsx_scan_by_key_device(self._h, d_keys or None, d_values or None, n, key_bytes, key_kind, value_bytes, value_kind,
                                                   op, flags, first & 0xFFFFFFFFFFFFFFFF, d_out or None, d_out_num or None, stream))


    @staticmethod
    def _key_columns(columns):
        """(ptr, key_bytes, key_kind, descending) tuples -> a ctypes array of rsx_key_column."""
        arr = (_lib.KeyColumn * max(1, len(columns)))()
        for j, (ptr, kb, kind, desc) in enumerate(columns):
            arr[j] = _lib.KeyColumn(ptr or None, kb, kind, 1 if desc else 0, 0)
        return arr

    def reserve_lex(self, n: int, columns, value_bytes: int = 0):
        """rsx_ctx_reserve_lex: the context's first-call set-up and the workspace of lexsort_device / sort_columns_device on
        up to n keys of these columns ((ptr, key_bytes, key_kind, descending) tuples; ptr is not looked at), so that the
        call allocates nothing and can be captured."""
        self._check(self._L.rsx_ctx_reserve_lex(self._h, n, self._key_columns(columns), len(columns), value_bytes))

    def lexsort_device(self, columns, d_index: int, n: int, index_bytes: int, stream: int = 0):
        """rsx_lexsort_device: the stable permutation that sorts n rows by several key columns, column 0 the most
        significant; columns: (ptr, key_bytes, key_kind, descending) tuples.  The columns are only read."""
        self._check(self._L.rsx_lexsort_device(self._h, self._key_columns(columns), len(columns), d_index or None, n, index_bytes, stream))

    def sort_columns_device(self, columns, d_values: int, value_bytes: int, n: int, stream: int = 0):
        """rsx_sort_columns_device: that permutation applied in place to every column and to the values (d_values 0 and
        value_bytes 0: the columns alone)."""
        self._check(self._L.rsx_sort_columns_device(self._h, self._key_columns(columns), len(columns), d_values or None, value_bytes, n, stream))


_DEFAULT = {}
_DEFAULT_LOCK = threading.Lock()


def default_context(device: int) -> Context:
    with _DEFAULT_LOCK:
        c = _DEFAULT.get(device)
        if c is None:
            c = _DEFAULT[device] = Context(device)
        return c


def _torch_digits(t, digits: Optional[RadixDigits]) -> RadixDigits:
    if digits is not None:
        return digits
    import torch
    m = {torch.uint8: "u8", torch.int8: "i8", torch.int16: "i16", torch.int32: "i32", torch.int64: "i64",
         torch.float32: "f32", torch.float64: "f64"}
    for name, key in (("uint16", "u16"), ("uint32", "u32"), ("uint64", "u64")):
        if hasattr(torch, name):
            m[getattr(torch, name)] = key
    if t.dtype not in m:
        raise TypeError(f"no RadixDigits for torch dtype {t.dtype}; pass digits=")
    return PRIMITIVES[m[t.dtype]]


_KERNEL_SIZES = (1, 2, 4, 8, 12, 16, 24, 32)


def _check_element_stated(shape, itemsize: int, d: RadixDigits):
    """Element sizes and key widths with sort kernels of their own may be read from any buffer of packed elements.
    Any other layout (include/rsx.h, "Any layout") is sorted from an array that states its element: a dtype of
    elem_bytes bytes (numpy structured or void dtype), or a last dimension of elem_bytes bytes ((n, elem_bytes)
    uint8).  A flat byte buffer with such a descriptor is refused, as before those layouts could be sorted."""
    if d.elem_bytes in _KERNEL_SIZES and d.key_bytes in (1, 2, 4, 8, 16):
        return
    if itemsize == d.elem_bytes or (len(shape) >= 2 and shape[-1] * itemsize == d.elem_bytes):
        return
    raise RsxError(_lib.ERR_UNSUPPORTED,
                   f"{d.elem_bytes}-byte elements with {d.key_bytes}-byte keys have no kernels of their own: pass an "
                   f"array whose dtype or last dimension is the {d.elem_bytes}-byte element")


class _on_device:
    """`with _on_device(t, ctx) as (c, stream):` -- a call on the GPU tensor `t`: its device selected, c = ctx or that
    device's default context, stream = the handle of the device's current stream.  (A class, not a generator under
    contextlib.contextmanager: that costs 1.5 us a call, which a sort of 2^16 keys shows.)"""
    __slots__ = ("_c", "_dev", "_guard", "_torch")

    def __init__(self, t, ctx: Optional[Context]):
        import torch
        self._dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
        self._c = ctx or default_context(self._dev)
        self._guard = torch.cuda.device(self._dev)
        self._torch = torch

    def __enter__(self):
        self._guard.__enter__()
        try:
            return self._c, self._torch.cuda.current_stream(self._dev).cuda_stream
        except BaseException:
            self._guard.__exit__(None, None, None)
            raise

    def __exit__(self, *exc):
        return self._guard.__exit__(*exc)


def _check_rc(L, rc: int):
    """Raises what a call that takes no context returned, unless it is 0."""
    if rc != 0:
        raise RsxError(rc, L.rsx_strerror(rc).decode())


def _index_dtype(index_dtype):
    """The index_dtype argument of a call that makes its index tensors: torch.int64 unless torch.int32 is asked for."""
    import torch
    if index_dtype is None:
        index_dtype = torch.int64
    if index_dtype not in (torch.int32, torch.int64):
        raise ValueError(f"index_dtype must be torch.int32 or torch.int64, not {index_dtype}")
    return index_dtype


def radix_sort(x, digits: Optional[RadixDigits] = None, tmp=None, ctx: Optional[Context] = None):
    """`<[T]>::radix_sort(&mut self)` (mod.rs:62): sorts `x` in place and returns None.

    x: a contiguous torch tensor on a GPU (device-resident path, enqueued on the
       current stream, not synchronised), or a contiguous numpy array / CPU torch
       tensor (host drop-in path: H2D -> sort -> D2H, blocking).
    digits: RadixDigits of the element type; inferred for primitive dtypes and
       numpy structured dtypes (first field = key).  When given for a byte tensor
       (uint8), x is read as packed elements of digits.elem_bytes.  Layouts without
       kernels of their own (any other element size, keys of 3, 5-7, 9-15 bytes) need
       an array that states the element: dtype itemsize or last dimension == elem_bytes
       (e.g. a structured array, or a uint8 tensor of shape (n, elem_bytes)).
    tmp: optional ping-pong buffer of the same shape/dtype/device (mod.rs:71-83 `temp`).
    """
    if isinstance(x, np.ndarray):
        if not x.flags["C_CONTIGUOUS"] or not x.flags["WRITEABLE"]:
            raise ValueError("radix_sort needs a contiguous, writable array")
        d = digits if digits is not None else digits_of(x.dtype)
        n = x.nbytes // d.elem_bytes
        if x.nbytes % d.elem_bytes:
            raise ValueError("array size is not a multiple of elem_bytes")
        _check_element_stated(x.shape, x.dtype.itemsize, d)
        c = ctx or default_context(-1)
        c.sort_host(x.ctypes.data, n, d)
        return None
    import torch
    if not isinstance(x, torch.Tensor):
        raise TypeError("radix_sort expects a numpy array or a torch tensor")
    if not x.is_contiguous():
        raise ValueError("radix_sort needs a contiguous tensor")
    d = _torch_digits(x, digits)
    nbytes = x.numel() * x.element_size()
    if nbytes % d.elem_bytes:
        raise ValueError("tensor size is not a multiple of elem_bytes")
    n = nbytes // d.elem_bytes
    _check_element_stated(tuple(x.shape), x.element_size(), d)
    if not x.is_cuda:
        c = ctx or default_context(-1)
        c.sort_host(x.data_ptr(), n, d)
        return None
    with _on_device(x, ctx) as (c, stream):
        if n <= 1:
            return None
        if tmp is None:
            tmp = torch.empty_like(x)
        elif tmp.device != x.device or tmp.numel() * tmp.element_size() < nbytes or not tmp.is_contiguous():
            raise ValueError("tmp must be a contiguous buffer on the same device, at least as large as x")
        c.sort_device(x.data_ptr(), tmp.data_ptr(), n, d, stream)
    return None


def segment_caps(digits: RadixDigits):
    """rsx_segment_caps: the longest segment each size class of a segmented sort holds in LDS (ascending); longer
    segments are sorted through memory.  Needs no device."""
    L = _lib.load()
    caps = (ctypes.c_uint32 * _lib.SEG_CLASSES)()
    lay = digits.layout()
    rc = L.rsx_segment_caps(ctypes.byref(lay), caps)
    _check_rc(L, rc)
    return [int(c) for c in caps]


def _segment_args(x, digits, tmp):
    """The checks radix_sort_segments and radix_sort_rows share; no context is made before they pass."""
    import torch
    if not isinstance(x, torch.Tensor):
        raise TypeError("a segmented sort takes a torch tensor on a GPU")
    if not x.is_contiguous():
        raise ValueError("a segmented sort needs a contiguous tensor")
    if not x.is_cuda:
        raise ValueError("a segmented sort takes a tensor on a GPU (host arrays: radix_sort per segment)")
    d = _torch_digits(x, digits)
    if d.elem_bytes not in _KERNEL_SIZES or d.key_bytes not in (1, 2, 4, 8, 16):
        raise RsxError(_lib.ERR_UNSUPPORTED, f"{d.elem_bytes}-byte elements with {d.key_bytes}-byte keys have no kernels of their own")
    nbytes = x.numel() * x.element_size()
    if nbytes % d.elem_bytes:
        raise ValueError("tensor size is not a multiple of elem_bytes")
    if tmp is not None:
        if not isinstance(tmp, torch.Tensor):
            raise TypeError("tmp must be a torch tensor")
        if tmp.device != x.device or tmp.numel() * tmp.element_size() < nbytes or not tmp.is_contiguous():
            raise ValueError("tmp must be a contiguous buffer on the same device, at least as large as x")
    return d, nbytes // d.elem_bytes


def _check_offsets(offsets):
    import torch
    if not isinstance(offsets, torch.Tensor):
        raise TypeError("offsets must be a torch tensor on the device of x")
    ok = [torch.int64] + ([torch.uint64] if hasattr(torch, "uint64") else [])
    if offsets.dtype not in ok:
        raise TypeError(f"offsets must be int64 or uint64, not {offsets.dtype}")
    if not offsets.is_contiguous() or offsets.dim() != 1:
        raise ValueError("offsets must be a contiguous 1-D tensor")


def radix_sort_segments(x, offsets, digits: Optional[RadixDigits] = None, tmp=None, ctx: Optional[Context] = None,
                        max_seg_len: int = 0):
    """Sorts every segment [offsets[i], offsets[i+1]) of `x` on its own, in place, ascending and stably -- what
    radix_sort would leave if called on each segment -- in one call (rsx_sort_segments_device).  Returns None;
    enqueued on the current stream, not synchronised.

    x: a contiguous GPU tensor (dtype inferred as in radix_sort; with digits= a uint8 tensor of packed elements).
    offsets: a contiguous GPU tensor of nseg + 1 int64 or uint64 on the same device, in elements, non-decreasing,
       the last at most len(x).  Elements outside [offsets[0], offsets[-1]) are not touched.  The offsets are
       checked on the device: a bad segment is left as it is and the context's next check() raises.
    max_seg_len: an upper bound on the segment lengths, if the caller has one (0: unknown): saves the launches
       of the size classes above it (segment_caps)."""
    import torch
    if not isinstance(x, torch.Tensor):
        raise TypeError("a segmented sort takes a torch tensor on a GPU")
    _check_offsets(offsets)
    d, n = _segment_args(x, digits, tmp)
    if offsets.device != x.device:
        raise ValueError("offsets must live on the device of x")
    if max_seg_len < 0:
        raise ValueError("max_seg_len must not be negative")
    nseg = offsets.numel() - 1
    if nseg <= 0 or n == 0:
        return None
    with _on_device(x, ctx) as (c, stream):
        if tmp is None:
            tmp = torch.empty_like(x)
        c.sort_segments_device(x.data_ptr(), tmp.data_ptr(), n, d, offsets.data_ptr(), nseg, max_seg_len, stream)
    return None


def radix_sort_rows(x, digits: Optional[RadixDigits] = None, tmp=None, ctx: Optional[Context] = None):
    """Sorts every row along the last dimension of `x` in place, ascending and stably
    (`torch.sort(x, dim=-1, stable=True).values` written into x; rsx_sort_rows_device).  Returns None; enqueued on the
    current stream, not synchronised.

    x: a contiguous GPU tensor of at least one dimension; dtype inferred as in radix_sort.  With digits= on a uint8
       tensor the last dimension is row_len * elem_bytes bytes."""
    import torch
    d, n = _segment_args(x, digits, tmp)
    if x.dim() < 1:
        raise ValueError("radix_sort_rows needs a tensor of at least one dimension")
    last_bytes = x.shape[-1] * x.element_size()
    if last_bytes % d.elem_bytes:
        raise ValueError("the last dimension is not a multiple of elem_bytes")
    row_len = last_bytes // d.elem_bytes
    if row_len <= 1 or n == 0:
        return None
    rows = n // row_len
    with _on_device(x, ctx) as (c, stream):
        if tmp is None:
            tmp = torch.empty_like(x)
        c.sort_rows_device(x.data_ptr(), tmp.data_ptr(), rows, row_len, d, stream)
    return None


def _pairs_keys(keys, key_kind):
    """(key_bytes, key_kind, n) of the key column of radix_sort_pairs / radix_argsort."""
    import torch
    if not isinstance(keys, torch.Tensor):
        raise TypeError("keys must be a torch tensor on a GPU")
    if not keys.is_contiguous():
        raise ValueError("keys must be contiguous")
    if keys.dim() == 2 and keys.dtype == torch.uint8 and keys.shape[1] == 16:  # 128-bit keys as raw bytes
        kind = KEY_UNSIGNED if key_kind is None else key_kind
        if kind not in (KEY_UNSIGNED, KEY_SIGNED):
            raise ValueError("128-bit keys are KEY_UNSIGNED or KEY_SIGNED")
        return 16, kind, keys.shape[0]
    if keys.dim() != 1:
        raise ValueError("keys must be 1-D (or an (n, 16) uint8 tensor of 128-bit keys)")
    if key_kind is not None:
        raise ValueError("key_kind= is for (n, 16) uint8 keys; other widths take it from the dtype")
    d = _torch_digits(keys, None)
    return d.key_bytes, d.key_kind, keys.shape[0]


def _pairs_device(keys, other, what: str):
    """Last of the argument checks (none of them needs a context): both tensors on one GPU."""
    if not keys.is_cuda:
        raise ValueError("keys must live on a GPU (host arrays: radix_sort on interleaved elements)")
    if other is not None and other.device != keys.device:
        raise ValueError(f"keys and {what} must live on the same device")


def radix_sort_pairs(keys, values, descending: bool = False, ctx: Optional[Context] = None, key_kind: Optional[int] = None):
    """Sorts `keys` and `values` in place by key and returns None (rsx_sort_pairs_device): what
    `k, i = torch.sort(keys, stable=True, descending=descending); values = values[i]` computes, without the
    interleaving a caller of radix_sort would have to do.  Stable in both orders: equal keys keep their input order.

    keys: a contiguous 1-D GPU tensor of a dtype radix_sort knows, or an (n, 16) uint8 tensor of 128-bit keys
       (key_kind= KEY_UNSIGNED, the default, or KEY_SIGNED).
    values: a contiguous GPU tensor on the same device with values.shape[0] == len(keys), any dtype; one row
       (values[i], trailing dimensions included) is one value of up to 32768 bytes, moved bitwise.  None: keys only.

    The order is the reference's total order on bit patterns (radix_digits.rs), not torch.sort's: -NaN sorts below
    -inf, +NaN above +inf, and -0.0 below +0.0.  Enqueued on the current stream, not synchronised."""
    import torch
    kb, kind, n = _pairs_keys(keys, key_kind)
    vb = 0
    if values is not None:
        if not isinstance(values, torch.Tensor):
            raise TypeError("values must be a torch tensor or None")
        if not values.is_contiguous():
            raise ValueError("values must be contiguous")
        if values.dim() < 1 or values.shape[0] != n:
            raise ValueError(f"values must have one row per key ({n}), not shape {tuple(values.shape)}")
        vb = values.element_size()
        for s in values.shape[1:]:
            vb *= s
        if vb == 0 or vb > 32768:
            raise ValueError(f"one value must have 1 .. 32768 bytes, not {vb}")
    _pairs_device(keys, values, "values")
    if n <= 1:
        return None
    with _on_device(keys, ctx) as (c, stream):
        c.sort_pairs_device(keys.data_ptr(), values.data_ptr() if values is not None else 0, n, kb, kind, vb, descending, stream)
    return None


def radix_argsort(keys, descending: bool = False, out=None, ctx: Optional[Context] = None, key_kind: Optional[int] = None):
    """The stable permutation that sorts `keys` (rsx_argsort_device), like `torch.argsort(keys, stable=True,
    descending=descending)`: returns a new int64 tensor, or fills and returns `out` (a contiguous 1-D int32 or int64
    tensor of len(keys) on the same device).  `keys` (as in radix_sort_pairs) is not modified.

    The order is the reference's total order on bit patterns (radix_digits.rs), not torch's: -NaN sorts below -inf,
    +NaN above +inf, -0.0 below +0.0.  Enqueued on the current stream, not synchronised."""
    import torch
    kb, kind, n = _pairs_keys(keys, key_kind)
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch tensor")
        if out.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"out must be int32 or int64, not {out.dtype}")
        if out.dim() != 1 or out.shape[0] != n or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous 1-D tensor of {n} elements")
    _pairs_device(keys, out, "out")
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=keys.device)
    if n == 0:
        return out
    with _on_device(keys, ctx) as (c, stream):
        c.argsort_device(keys.data_ptr(), out.data_ptr(), n, kb, kind, out.element_size(), descending, stream)
    return out


def lex_plan(specs):
    """rsx_lex_plan: how radix_lexsort / radix_sort_columns would sort columns of these (key_bytes, key_kind) specs, column
    0 the most significant: a list of rounds in the order they run, each (first_col, key_bytes, elem_bytes) -- the
    round takes the columns from first_col up to the previous round's first_col (round 0: to the end), key_bytes is the
    sum of their widths, elem_bytes the size of the joined (compound key, position) element it sorts.  Needs no device."""
    L = _lib.load()
    specs = [tuple(s) for s in specs]
    arr = (_lib.KeyColumn * max(1, len(specs)))()
    for j, (kb, kind) in enumerate(specs):
        arr[j] = _lib.KeyColumn(None, kb, kind, 0, 0)
    rounds = ctypes.c_uint32()
    first, kbs, ebs = ((ctypes.c_uint32 * _lib.LEX_MAX_COLUMNS)() for _ in range(3))
    rc = L.rsx_lex_plan(arr, len(specs), ctypes.byref(rounds), first, kbs, ebs)
    _check_rc(L, rc)
    return [(int(first[r]), int(kbs[r]), int(ebs[r])) for r in range(rounds.value)]


def _lex_columns(columns, descending):
    """The checks of radix_lexsort / radix_sort_columns on their columns (none needs a context) ->
    ([(tensor, key_bytes, key_kind, descending)], n)."""
    import torch
    if isinstance(columns, torch.Tensor) or not isinstance(columns, (list, tuple)):
        raise TypeError("columns must be a list or tuple of key columns")
    if not 1 <= len(columns) <= _lib.LEX_MAX_COLUMNS:
        raise ValueError(f"1 .. {_lib.LEX_MAX_COLUMNS} key columns, not {len(columns)}")
    if isinstance(descending, (bool, np.bool_)):
        desc = [bool(descending)] * len(columns)
    else:
        desc = list(descending)
        if len(desc) != len(columns) or not all(isinstance(d, (bool, np.bool_)) for d in desc):
            raise ValueError(f"descending must be a bool or one bool per column ({len(columns)})")
    out, n = [], None
    for j, col in enumerate(columns):
        kind = None
        if isinstance(col, tuple):
            if len(col) != 2:
                raise TypeError("a column is a tensor or a (tensor, key_kind) pair")
            col, kind = col
        kb, kind, m = _pairs_keys(col, kind)
        if n is None:
            n = m
        elif m != n:
            raise ValueError(f"every column must have the length of the first ({n}); column {j} has {m}")
        out.append((col, kb, kind, bool(desc[j])))
    return out, n


def _lex_device(cols, other, what: str):
    """Last of the argument checks (none of them needs a context): every tensor on one GPU."""
    first = cols[0][0]
    for j, (col, _kb, _kind, _d) in enumerate(cols):
        if not col.is_cuda:
            raise ValueError("the columns must live on a GPU")
        if col.device != first.device:
            raise ValueError(f"column {j} must live on the device of column 0")
    if other is not None and other.device != first.device:
        raise ValueError(f"the columns and {what} must live on the same device")


def radix_lexsort(columns, descending=False, out=None, ctx: Optional[Context] = None):
    """The stable permutation that sorts rows by several key columns (rsx_lexsort_device): returns a new int64 tensor, or
    fills and returns `out` (a contiguous 1-D int32 or int64 tensor of the columns' length on their device).

    columns[0] is the MOST significant column -- the opposite of numpy.lexsort, whose last key is the primary one:
    radix_lexsort([a, b, c]) is np.lexsort((c, b, a)).  Each column is a contiguous 1-D GPU tensor of a dtype radix_sort
    knows, or an (n, 16) uint8 tensor of 128-bit keys, alone (unsigned) or as a (tensor, key_kind) pair; all of one
    length on one device, at most 16 of them.  descending: a bool, or one bool per column.  Rows that are equal in every
    column keep their input order whatever the directions.  No column is modified.

    The order within a column is the reference's total order on bit patterns (radix_digits.rs), not torch's: -NaN sorts
    below -inf, +NaN above +inf, -0.0 below +0.0.  Enqueued on the current stream, not synchronised."""
    import torch
    cols, n = _lex_columns(columns, descending)
    _index_out(out, (n,), "the columns")
    _lex_device(cols, out, "out")
    keys = cols[0][0]
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=keys.device)
    if n == 0:
        return out
    with _on_device(keys, ctx) as (c, stream):
        c.lexsort_device([(t.data_ptr(), kb, kind, d) for t, kb, kind, d in cols], out.data_ptr(), n, out.element_size(), stream)
    return out


def radix_sort_columns(columns, values=None, descending=False, ctx: Optional[Context] = None):
    """Sorts rows that are kept as several key columns, in place, and returns None (rsx_sort_columns_device): every column
    and `values` are permuted by radix_lexsort(columns, descending) -- columns[0] the most significant, equal rows in
    input order.

    columns, descending: as in radix_lexsort; THE COLUMNS ARE WRITTEN.  values: as in radix_sort_pairs, a contiguous GPU
    tensor on the same device with one row of 1 .. 32768 bytes per key, moved bitwise; None: the columns alone.  Columns
    that share memory with each other or with values are undefined.  Enqueued on the current stream, not synchronised."""
    cols, n = _lex_columns(columns, descending)
    vb = _value_bytes(values, (n,), "the columns")
    _lex_device(cols, values, "values")
    keys = cols[0][0]
    if n <= 1:
        return None
    with _on_device(keys, ctx) as (c, stream):
        c.sort_columns_device([(t.data_ptr(), kb, kind, d) for t, kb, kind, d in cols], values.data_ptr() if values is not None else 0,
                              vb, n, stream)
    return None


def segment_pairs_caps(key_bytes: int, value_bytes: int):
    """rsx_segment_pairs_caps: the longest segment each LDS size class of the segmented key / value sorts holds for
    these widths (argsort: value_bytes = 4).  Needs no device."""
    L = _lib.load()
    caps = (ctypes.c_uint32 * _lib.SEG_CLASSES)()
    rc = L.rsx_segment_pairs_caps(key_bytes, value_bytes, caps)
    _check_rc(L, rc)
    return [int(c) for c in caps]


def _value_bytes(values, lead, what: str) -> int:
    """Bytes of one value of `values`, whose leading shape must be `lead`; None: keys only (0)."""
    import torch
    if values is None:
        return 0
    if not isinstance(values, torch.Tensor):
        raise TypeError("values must be a torch tensor or None")
    if not values.is_contiguous():
        raise ValueError("values must be contiguous")
    if values.dim() < len(lead) or tuple(values.shape[:len(lead)]) != tuple(lead):
        raise ValueError(f"values must have the leading shape of {what} {tuple(lead)}, not shape {tuple(values.shape)}")
    vb = values.element_size()
    for s in values.shape[len(lead):]:
        vb *= s
    if vb == 0 or vb > 32768:
        raise ValueError(f"one value must have 1 .. 32768 bytes, not {vb}")
    return vb


def _index_out(out, shape, what: str):
    import torch
    if out is None:
        return
    if not isinstance(out, torch.Tensor):
        raise TypeError("out must be a torch tensor")
    if out.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"out must be int32 or int64, not {out.dtype}")
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous tensor of shape {tuple(shape)} like {what}")


def _rows_keys(keys):
    """(key_bytes, key_kind, rows, row_len) of a key tensor sorted along its last dimension."""
    import torch
    if not isinstance(keys, torch.Tensor):
        raise TypeError("keys must be a torch tensor on a GPU")
    if not keys.is_contiguous():
        raise ValueError("keys must be contiguous")
    if keys.dim() < 1:
        raise ValueError("keys must have at least one dimension")
    d = _torch_digits(keys, None)
    row_len = keys.shape[-1]
    return d.key_bytes, d.key_kind, (keys.numel() // row_len if row_len else 0), row_len


def radix_sort_rows_pairs(keys, values, descending: bool = False, ctx: Optional[Context] = None):
    """Sorts every row along the last dimension of `keys` in place and moves `values` with it
    (rsx_sort_rows_pairs_device): `k, i = torch.sort(keys, dim=-1, stable=True, descending=descending)`,
    `values = values.gather(-1, i)`, fused into one kernel per row.  Returns None; enqueued on the current stream.

    keys: a contiguous GPU tensor of at least one dimension, of a dtype radix_sort knows.
    values: a contiguous GPU tensor on the same device whose leading shape is keys.shape; one value is values[..., j]
       (a scalar) or values[..., j, :] with its trailing dimensions, 1 .. 32768 bytes, moved bitwise.  None: keys only,
       which is how rows of plain keys are sorted in descending order.
    The order is radix_sort_pairs' (a total order on bit patterns, stable in both directions).  Values of 1, 2, 4, 8 or 16
    bytes stay in registers and LDS with their keys; wider ones are gathered through a copy in the context's workspace.
    Rows above segment_pairs_caps(key_bytes, value_bytes)[-1] are sorted through memory or row by row: slow."""
    kb, kind, rows, row_len = _rows_keys(keys)
    vb = _value_bytes(values, keys.shape, "keys")
    _pairs_device(keys, values, "values")
    if rows == 0 or row_len <= 1:
        return None
    with _on_device(keys, ctx) as (c, stream):
        c.sort_rows_pairs_device(keys.data_ptr(), values.data_ptr() if values is not None else 0, rows, row_len, kb, kind, vb,
                                 descending, stream)
    return None


def radix_argsort_rows(keys, descending: bool = False, out=None, ctx: Optional[Context] = None):
    """`torch.sort(keys, dim=-1, stable=True, descending=descending).indices` (rsx_argsort_rows_device): returns a new
    int64 tensor of keys.shape, or fills and returns `out` (contiguous, int32 or int64, keys.shape, same device).  `keys`
    is not modified.  The order is radix_argsort's.  Enqueued on the current stream, not synchronised."""
    import torch
    kb, kind, rows, row_len = _rows_keys(keys)
    _index_out(out, keys.shape, "keys")
    _pairs_device(keys, out, "out")
    if out is None:
        out = torch.empty(keys.shape, dtype=torch.int64, device=keys.device)
    if rows == 0 or row_len == 0:
        return out
    with _on_device(keys, ctx) as (c, stream):
        c.argsort_rows_device(keys.data_ptr(), out.data_ptr(), rows, row_len, kb, kind, out.element_size(), descending, stream)
    return out


def topk_caps(key_bytes: int):
    """rsx_topk_caps -> (caps, max_k): the longest row each LDS size class of the top-k selects in one launch for this
    key width, and the largest k taken for longer rows.  Needs no device."""
    L = _lib.load()
    caps = (ctypes.c_uint32 * _lib.SEG_CLASSES)()
    max_k = ctypes.c_uint32()
    rc = L.rsx_topk_caps(key_bytes, caps, ctypes.byref(max_k))
    _check_rc(L, rc)
    return [int(c) for c in caps], int(max_k.value)


# Shapes radix_topk hands to the full sort although rsx_topk_rows_device takes them: (no entry: none measured slower)
def _topk_by_sort(rows: int, row_len: int, k: int, key_bytes: int) -> bool:
    return False


def radix_topk(keys, k: int, largest: bool = True, index_dtype=None, ctx: Optional[Context] = None):
    """(values, indices) of the k largest (largest=False: smallest) keys along the last dimension, sorted, like
    `torch.topk(keys, k, largest=largest, sorted=True)` -- with the tie order specified: the result is the first k
    columns of the stable sort `radix_argsort_rows(keys, descending=largest)` and of the keys gathered through it, byte
    for byte, so equal keys appear in input order and ties at the threshold go to the lowest positions
    (rsx_topk_rows_device: a radix select in LDS and a sort of k elements, not a sort of the row).

    keys: a contiguous GPU tensor of at least one dimension, of a dtype radix_sort knows; it is not modified.
    Returns new tensors of shape keys.shape[:-1] + (k,): values of keys.dtype and indices of index_dtype (torch.int64,
    the default, or torch.int32).  The order is radix_argsort's total order on bit patterns (+NaN is the largest float).
    Enqueued on the current stream, not synchronised.

    Total: where the C call is unsupported (rows longer than topk_caps(key_bytes)[0][-1] with k above its max_k), the
    rows are sorted by radix_argsort_rows and the first k columns gathered -- the same bytes, at the cost of the sort."""
    import torch
    kb, kind, rows, row_len = _rows_keys(keys)
    k = operator.index(k)
    if k < 0 or k > row_len:
        raise ValueError(f"k must be in 0 .. {row_len} (the last dimension), not {k}")
    index_dtype = _index_dtype(index_dtype)
    _pairs_device(keys, None, "")
    shape = tuple(keys.shape[:-1]) + (k,)
    values = torch.empty(shape, dtype=keys.dtype, device=keys.device)
    indices = torch.empty(shape, dtype=index_dtype, device=keys.device)
    if rows == 0 or k == 0:
        return values, indices
    with _on_device(keys, ctx) as (c, stream):
        caps, max_k = topk_caps(kb)
        if (row_len > caps[-1] and k > max_k) or _topk_by_sort(rows, row_len, k, kb):
            full = radix_argsort_rows(keys, descending=largest, ctx=c)
            first = full[..., :k]
            indices.copy_(first)
            # (a gather of the raw bits: dtypes torch cannot index, uint32 / uint64, go as their signed twins)
            bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[kb]
            values.view(bits).copy_(torch.gather(keys.view(bits), -1, first))
            return values, indices
        c.topk_rows_device(keys.data_ptr(), values.data_ptr(), indices.data_ptr(), rows, row_len, k, kb, kind,
                           indices.element_size(), largest, stream)
    return values, indices


def select_caps(key_bytes: int):
    """rsx_select_caps -> (max_ranks, digit_bits, tile, cand_div, cand_floor): the ranks one rsx_select_device call takes,
    the bits of one level's digit, the keys per workgroup of its index launches, and the capacity of its candidate
    buffer, n // cand_div + cand_floor keys.  Needs no device."""
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(5)]
    rc = L.rsx_select_caps(key_bytes, *[ctypes.byref(o) for o in out])
    _check_rc(L, rc)
    return tuple(int(o.value) for o in out)


# Shapes radix_select hands to radix_argsort although rsx_select_device takes them: (no entry: no crossover measured)
def _select_by_sort(n: int, key_bytes: int) -> bool:
    return False


def _select_ranks(ranks, n: int):
    """(list of ranks in 0 .. n - 1, scalar?) of the ranks argument of radix_select: negative ranks count from the end."""
    scalar = False
    try:
        ranks = [operator.index(ranks)]
        scalar = True
    except TypeError:
        ranks = [operator.index(r) for r in ranks]
    out = []
    for r in ranks:
        if r < -n or r >= n:
            raise ValueError(f"rank {r} is out of range for {n} keys")
        out.append(r + n if r < 0 else r)
    return out, scalar


def _select_flat(keys, kb: int, kind: int, n: int, ranks, descending: bool, want_index: bool, index_dtype, ctx):
    """values (and indices, or None) of the ranks of one flat key array, in batches of select_caps(kb)[0] ranks."""
    import torch
    m = len(ranks)
    values = torch.empty((m,) + tuple(keys.shape[1:]), dtype=keys.dtype, device=keys.device)
    indices = torch.empty(m, dtype=index_dtype, device=keys.device) if want_index else None
    if m == 0:
        return values, indices
    with _on_device(keys, ctx) as (c, stream):
        if _select_by_sort(n, kb):
            perm = radix_argsort(keys, descending=descending, ctx=c, key_kind=kind if kb == 16 else None)
            at = perm[torch.tensor(ranks, dtype=torch.int64, device=keys.device)]
            bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64, 16: torch.uint8}[kb]
            values.view(bits).copy_(keys.view(bits)[at])
            if want_index:
                indices.copy_(at)
            return values, indices
        step = select_caps(kb)[0]
        ib = indices.element_size() if want_index else 0
        for b in range(0, m, step):
            c.select_device(keys.data_ptr(), n, kb, kind, ranks[b:b + step], values.data_ptr() + b * kb,
                            indices.data_ptr() + b * ib if want_index else 0, ib, descending, stream)
    return values, indices


def radix_select(keys, ranks, descending: bool = False, return_index: bool = False, index_dtype=None, ctx: Optional[Context] = None,
                 key_kind: Optional[int] = None):
    """The elements at sorted positions `ranks` of `keys`, without sorting them (rsx_select_device): with p =
    radix_argsort(keys, descending=descending), the values keys[p[ranks]] and, with return_index, the positions p[ranks]
    -- column `ranks` of the full stable sort, byte for byte, so equal keys count in input order and the call agrees
    with radix_topk wherever the two overlap.

    keys: a contiguous 1-D GPU tensor of a dtype radix_argsort takes, or an (n, 16) uint8 tensor of 128-bit keys
       (key_kind= as there); it is not modified.
    ranks: an int (the results are 0-d, or (16,) for 128-bit keys) or a sequence of ints (1-D results); negative ranks
       count from the end; ranks may repeat and come in any order.  More than select_caps(key_bytes)[0] go in batches.
    Returns values, or (values, indices) with indices of index_dtype (torch.int64, the default, or torch.int32).
    The order is radix_argsort's total order on bit patterns.  A counting select: about two reads of the keys on
    spread-out keys and a third for the index, against the passes of a sort.  Enqueued on the current stream, not
    synchronised."""
    kb, kind, n = _pairs_keys(keys, key_kind)
    ranks, scalar = _select_ranks(ranks, n)
    index_dtype = _index_dtype(index_dtype)
    _pairs_device(keys, None, "")
    values, indices = _select_flat(keys, kb, kind, n, ranks, descending, return_index, index_dtype, ctx)
    if scalar:
        values = values[0]
        indices = indices[0] if return_index else None
    return (values, indices) if return_index else values


def radix_kthvalue(keys, k: int, largest: bool = False, index_dtype=None, ctx: Optional[Context] = None):
    """(values, indices) of the k-th smallest (largest=True: largest) key along the last dimension, k counted from 1 as
    in `torch.kthvalue(keys, k)` -- with the tie index specified: column k - 1 of the stable sort
    `radix_argsort_rows(keys, descending=largest)`, so among equal keys the one at the lowest position comes first.

    keys: a contiguous GPU tensor of at least one dimension, of a dtype radix_sort knows; it is not modified.
    Returns tensors of shape keys.shape[:-1].  Rows of at most topk_caps(key_bytes)[0][-1] keys take radix_topk(k) and its
    last column, one launch for all rows; longer rows take radix_select once per row.  Enqueued on the current stream,
    not synchronised."""
    import torch
    kb, kind, rows, row_len = _rows_keys(keys)
    k = operator.index(k)
    if k < 1 or k > row_len:
        raise ValueError(f"k must be in 1 .. {row_len} (the last dimension), not {k}")
    index_dtype = _index_dtype(index_dtype)
    _pairs_device(keys, None, "")
    shape = tuple(keys.shape[:-1])
    if row_len <= topk_caps(kb)[0][-1]:
        v, i = radix_topk(keys, k, largest=largest, index_dtype=index_dtype, ctx=ctx)
        return v[..., k - 1].contiguous(), i[..., k - 1].contiguous()
    values = torch.empty(rows, dtype=keys.dtype, device=keys.device)
    indices = torch.empty(rows, dtype=index_dtype, device=keys.device)
    flat = keys.reshape(rows, row_len)
    for r in range(rows):
        v, i = _select_flat(flat[r], kb, kind, row_len, [k - 1], largest, True, index_dtype, ctx)
        values[r:r + 1].copy_(v)
        indices[r:r + 1].copy_(i)
    return values.reshape(shape), indices.reshape(shape)


def radix_median(keys, index_dtype=None, ctx: Optional[Context] = None):
    """(value, index) of the lower median of a 1-D key tensor, rank (n - 1) // 2 of its stable sort, as `torch.median`
    picks -- with the tie index specified (radix_select)."""
    kb, kind, n = _pairs_keys(keys, None)
    if n == 0:
        raise ValueError("the median of no keys")
    return radix_select(keys, (n - 1) // 2, return_index=True, index_dtype=index_dtype, ctx=ctx)


_QUANTILE_METHODS = ("lower", "higher", "nearest")


def _quantile_ranks(n: int, q, method: str):
    """numpy's rules on the virtual index q * (n - 1), on the host: lower floor, higher ceil, nearest round-half-even."""
    out = []
    for x in q:
        v = x * (n - 1)
        lo = math.floor(v)
        if method == "lower":
            r = lo
        elif method == "higher":
            r = math.ceil(v)
        else:
            d = v - lo
            r = lo + 1 if d > 0.5 or (d == 0.5 and lo % 2 == 1) else lo
        out.append(min(max(int(r), 0), n - 1))
    return out


def radix_quantile(keys, q, method: str = "lower", ctx: Optional[Context] = None):
    """The q-quantiles of a 1-D key tensor by one of numpy's non-interpolating methods ("lower", "higher", "nearest" on
    the virtual index q * (n - 1), computed on the host): always one of the keys (radix_select), so integer keys and floats
    by bit pattern work, with no limit on n.  q: a float (0-d result) or a sequence of floats in [0, 1] (1-D result)."""
    kb, kind, n = _pairs_keys(keys, None)
    scalar = isinstance(q, (int, float))
    qs = [float(q)] if scalar else [float(x) for x in q]
    for x in qs:
        if not 0.0 <= x <= 1.0:  # (NaN too)
            raise ValueError(f"q must lie in [0, 1], not {x}")
    if method not in _QUANTILE_METHODS:
        raise ValueError(f"method must be one of {_QUANTILE_METHODS}, not {method!r}")
    if n == 0:
        raise ValueError("a quantile of no keys")
    ranks = _quantile_ranks(n, qs, method)
    return radix_select(keys, ranks[0] if scalar else ranks, ctx=ctx)


def unique_caps(key_bytes: int, with_positions: bool = True):
    """rsx_unique_caps -> (tile, scan_span): the elements one workgroup of the run kernels of radix_group takes for this key
    width and route, and the tiles one sweep of their scan kernel sums.  Needs no device."""
    L = _lib.load()
    tile, span = ctypes.c_uint32(), ctypes.c_uint32()
    rc = L.rsx_unique_caps(key_bytes, 1 if with_positions else 0, ctypes.byref(tile), ctypes.byref(span))
    _check_rc(L, rc)
    return int(tile.value), int(span.value)


Group = namedtuple("Group", ["num", "keys", "offsets", "perm", "inverse"])


def radix_group(keys, descending: bool = False, perm: bool = True, inverse: bool = False, index_dtype=None,
                ctx: Optional[Context] = None, key_kind: Optional[int] = None):
    """Groups equal keys (rsx_unique_device) and returns Group(num, keys, offsets, perm, inverse) without synchronising:

    num      a 0-d int64 device tensor: m, the number of distinct keys.
    keys     the distinct keys in sorted order in its first m entries (a tensor like `keys`; the rest is not written).
    offsets  int64, len(keys) + 1: offsets[j], j <= m, is where group j starts in the stable sort of the keys (the rest is
             not written); the counts are the differences, and offsets[: m + 1] is the `offsets` of radix_sort_segments and
             its siblings, made on the device.
    perm     the stable sorting permutation (radix_argsort): perm[offsets[j] : offsets[j + 1]] are the input positions of
             group j in input order, the first of them its first occurrence.  None unless perm=True.
    inverse  for every input position the j of its group.  None unless inverse=True.

    `keys` follows the rules of radix_argsort (1-D of a supported dtype, or (n, 16) uint8 128-bit keys with key_kind=) and
    is not modified; perm and inverse are of index_dtype (torch.int64, the default, or torch.int32).  Equality is
    bit-pattern equality and the order radix_argsort's total order on bit patterns: -0.0 and +0.0 are two groups, NaNs
    of different payloads too.  With perm=False and inverse=False the keys are sorted alone, without positions."""
    import torch
    kb, kind, n = _pairs_keys(keys, key_kind)
    index_dtype = _index_dtype(index_dtype)
    _pairs_device(keys, None, "")
    if n >= 1 << 32:
        raise ValueError("radix_group takes fewer than 2^32 keys")
    num = torch.empty((), dtype=torch.int64, device=keys.device)
    out_keys = torch.empty_like(keys)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=keys.device)
    out_perm = torch.empty(n, dtype=index_dtype, device=keys.device) if perm else None
    out_inverse = torch.empty(n, dtype=index_dtype, device=keys.device) if inverse else None
    with _on_device(keys, ctx) as (c, stream):
        c.unique_device(keys.data_ptr(), n, kb, kind, out_keys.data_ptr(), offsets.data_ptr(),
                        out_perm.data_ptr() if perm else 0, out_inverse.data_ptr() if inverse else 0,
                        8 if index_dtype == torch.int64 else 4, num.data_ptr(), descending, stream)
    return Group(num, out_keys, offsets, out_perm, out_inverse)


def reduce_caps(key_bytes: int, value_bytes: int):
    """rsx_reduce_caps -> (tile, scan_span): the elements one workgroup of the run kernels of radix_reduce_by_key takes for
    these key and value widths, and the tiles one sweep of their scan kernel takes.  Needs no device."""
    L = _lib.load()
    tile, span = ctypes.c_uint32(), ctypes.c_uint32()
    rc = L.rsx_reduce_caps(key_bytes, value_bytes, ctypes.byref(tile), ctypes.byref(span))
    _check_rc(L, rc)
    return int(tile.value), int(span.value)


Reduced = namedtuple("Reduced", ["num", "keys", "values", "offsets"])
_REDUCE_OPS = {"sum": _lib.REDUCE_SUM, "min": _lib.REDUCE_MIN, "max": _lib.REDUCE_MAX}


def _reduce_value_types():
    import torch
    types = {torch.int32: (4, KEY_SIGNED), torch.int64: (8, KEY_SIGNED), torch.float32: (4, KEY_FLOAT), torch.float64: (8, KEY_FLOAT)}
    for name, vb in (("uint32", 4), ("uint64", 8)):  # where the torch build has them
        if hasattr(torch, name):
            types[getattr(torch, name)] = (vb, KEY_UNSIGNED)
    return types


def radix_reduce_by_key(keys, values, op: str = "sum", descending: bool = False, offsets: bool = False,
                        ctx: Optional[Context] = None, key_kind: Optional[int] = None):
    """Reduces `values` over every group of equal `keys` (rsx_reduce_by_key_device) and returns
    Reduced(num, keys, values, offsets) without synchronising:

    num      a 0-d int64 device tensor: m, the number of distinct keys.
    keys     the distinct keys in sorted order in its first m entries (a tensor like `keys`; the rest is not written).
    values   a tensor like `values`: entry j < m is the sum ("sum"), minimum ("min") or maximum ("max") of the values whose
             key is keys[j], taken in input order (the rest is not written).
    offsets  int64, len(keys) + 1, as in radix_group: where group j starts in the stable sort.  None unless offsets=True.

    `keys` follows the rules of radix_group and is not modified; `values` is a 1-D contiguous tensor on the same device
    with len(keys) entries, of dtype int32, int64, float32 or float64 (uint32 / uint64 where torch has them).  Integer
    sums wrap; float minima and maxima follow radix_argsort's total order on bit patterns (-0.0 below +0.0, +NaN the
    largest); a float sum is added in an order fixed by the input's size and the group's place alone, so the same input
    gives the same bits on every call (there are no atomics)."""
    import torch
    kb, kind, n = _pairs_keys(keys, key_kind)
    if not isinstance(values, torch.Tensor):
        raise TypeError("values must be a torch tensor on a GPU")
    if op not in _REDUCE_OPS:
        raise ValueError(f"op must be 'sum', 'min' or 'max', not {op!r}")
    vt = _reduce_value_types().get(values.dtype)
    if vt is None:
        raise ValueError(f"values must be int32, int64, float32, float64, uint32 or uint64, not {values.dtype}")
    if values.dim() != 1 or values.shape[0] != n:
        raise ValueError(f"values must be 1-D with one entry per key ({n}), not of shape {tuple(values.shape)}")
    if not values.is_contiguous():
        raise ValueError("values must be contiguous")
    if values.device != keys.device:
        raise ValueError(f"keys and values must be on the same device ({keys.device}, {values.device})")
    _pairs_device(keys, None, "")
    if n >= 1 << 32:
        raise ValueError("radix_reduce_by_key takes fewer than 2^32 keys")
    num = torch.empty((), dtype=torch.int64, device=keys.device)
    out_keys = torch.empty_like(keys)
    out_values = torch.empty_like(values)
    out_offsets = torch.empty(n + 1, dtype=torch.int64, device=keys.device) if offsets else None
    if n == 0:  # (empty tensors have no address to hand to the C call, which wants one of keys and values: its two memsets)
        num.zero_()
        if offsets:
            out_offsets.zero_()
        return Reduced(num, out_keys, out_values, out_offsets)
    with _on_device(keys, ctx) as (c, stream):
        c.reduce_by_key_device(keys.data_ptr(), values.data_ptr(), n, kb, kind, vt[0], vt[1], _REDUCE_OPS[op], out_keys.data_ptr(),
                               out_values.data_ptr(), out_offsets.data_ptr() if offsets else 0, num.data_ptr(), descending, stream)
    return Reduced(num, out_keys, out_values, out_offsets)


def scan_by_key_caps(key_bytes: int, value_bytes: int, runs: bool = False):
    """rsx_scan_by_key_caps -> (tile, scan_span): the elements one workgroup of the count and write kernels of
    radix_scan_by_key takes for these widths and this group rule, and the tiles one sweep of the scan kernel takes.
    Needs no device."""
    L = _lib.load()
    tile, span = ctypes.c_uint32(), ctypes.c_uint32()
    rc = L.rsx_scan_by_key_caps(key_bytes, value_bytes, _lib.SCAN_RUNS if runs else 0, ctypes.byref(tile), ctypes.byref(span))
    _check_rc(L, rc)
    return int(tile.value), int(span.value)


def _scan_first_bits(first, op: str, dtype) -> int:
    """The bit pattern, as an unsigned integer, of what an exclusive scan stores at a group's first position: `first`, or
    for None 0 ("sum"), the type's largest value ("min", +inf for floats) or its smallest ("max", -inf)."""
    import torch
    name = str(dtype).split(".")[-1]
    nd = np.dtype(name)
    if first is None:
        if op == "sum":
            first = 0
        elif nd.kind == "f":
            first = float("inf") if op == "min" else float("-inf")
        else:
            info = np.iinfo(nd)
            first = info.max if op == "min" else info.min
    elif isinstance(first, torch.Tensor):
        raise TypeError("first must be a Python number (it is an argument of the launch, not a device value)")
    if nd.kind != "f" and (isinstance(first, bool) or not isinstance(first, (int, np.integer))):
        raise TypeError(f"first must be an integer for {name} values, not {first!r}")
    if nd.kind != "f" and not (np.iinfo(nd).min <= int(first) <= np.iinfo(nd).max):
        raise ValueError(f"first={first} does not fit {name}")
    word = np.array([first], dtype=nd).view(np.uint32 if nd.itemsize == 4 else np.uint64)
    return int(word[0])


def radix_scan_by_key(keys, values, op: str = "sum", exclusive: bool = False, first=None, runs: bool = False, out=None,
                      return_num: bool = False, index_dtype=None, ctx: Optional[Context] = None, key_kind: Optional[int] = None):
    """The running `op` of `values` inside every group of `keys` (rsx_scan_by_key_device), one result per row at the
    row's own position, without synchronising: groupby().cumsum() / cummin() / cummax() and, with values=None,
    cumcount() / row_number().

    runs=False  the group of a row is every row with the same key, anywhere in `keys` (a stable sort of (key, position)
                elements in the workspace finds them; rows of a group are taken in input order).
    runs=True   the group of a row is the run of CONSECUTIVE rows with its key: nothing is sorted, the call streams the two
                columns, and a key that appears again later starts a new group.
    exclusive   a row receives the result of its predecessor in the group, and the first row of every group `first`,
                which is stored and never combined: None is 0 for "sum", the dtype's largest value for "min" (+inf for
                floats) and its smallest for "max" (-inf).
    values=None every value is 1: the result, int64 or with index_dtype=torch.int32 int32, is the 1-based rank of the row
                in its group, or exclusive the 0-based rank.  Only with op="sum".

    Returns a tensor like `values`, or `out` when given (same dtype, shape and device as `values`; it may be `values`
    itself); with return_num=True the pair (out, num), num a 0-d int64 device tensor: the number of groups (runs).
    `keys` follows the rules of radix_group (bit-pattern equality: -0.0 and +0.0 are two keys) and is not modified; `values`
    and the operators follow radix_reduce_by_key: integer sums wrap, float minima and maxima follow the total order on bit
    patterns, and a float sum is added in an order fixed by the input's size, the group's start and the row's rank alone,
    so the same input gives the same bits on every call (there are no atomics)."""
    import torch
    kb, kind, n = _pairs_keys(keys, key_kind)
    if op not in _REDUCE_OPS:
        raise ValueError(f"op must be 'sum', 'min' or 'max', not {op!r}")
    if values is None:
        if op != "sum":
            raise ValueError(f"values=None (the count form) takes op='sum', not {op!r}")
        dtype = _index_dtype(index_dtype)
        vt = _reduce_value_types()[dtype]
    else:
        if not isinstance(values, torch.Tensor):
            raise TypeError("values must be a torch tensor on a GPU or None")
        if index_dtype is not None:
            raise ValueError("index_dtype= is for values=None; the result has the dtype of values")
        vt = _reduce_value_types().get(values.dtype)
        if vt is None:
            raise ValueError(f"values must be int32, int64, float32, float64, uint32 or uint64, not {values.dtype}")
        if values.dim() != 1 or values.shape[0] != n:
            raise ValueError(f"values must be 1-D with one entry per key ({n}), not of shape {tuple(values.shape)}")
        if not values.is_contiguous():
            raise ValueError("values must be contiguous")
        if values.device != keys.device:
            raise ValueError(f"keys and values must be on the same device ({keys.device}, {values.device})")
        dtype = values.dtype
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch tensor on a GPU")
        if out.dtype != dtype or out.dim() != 1 or out.shape[0] != n:
            raise ValueError(f"out must be 1-D of dtype {dtype} with one entry per key ({n}), not {out.dtype} of shape {tuple(out.shape)}")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
        if out.device != keys.device:
            raise ValueError(f"keys and out must be on the same device ({keys.device}, {out.device})")
    bits = _scan_first_bits(first, op, dtype)
    _pairs_device(keys, None, "")
    if n >= 1 << 32:
        raise ValueError("radix_scan_by_key takes fewer than 2^32 keys")
    if out is None:
        out = torch.empty(n, dtype=dtype, device=keys.device)
    num = torch.empty((), dtype=torch.int64, device=keys.device) if return_num else None
    if n == 0:  # (empty tensors have no address to hand to the C call)
        if return_num:
            num.zero_()
        return (out, num) if return_num else out
    flags = (_lib.SCAN_EXCLUSIVE if exclusive else 0) | (_lib.SCAN_RUNS if runs else 0)
    with _on_device(keys, ctx) as (c, stream):
        c.scan_by_key_device(keys.data_ptr(), values.data_ptr() if values is not None else 0, n, kb, kind, vt[0], vt[1], _REDUCE_OPS[op],
                             flags, bits, out.data_ptr(), num.data_ptr() if return_num else 0, stream)
    return (out, num) if return_num else out


def radix_unique(keys, return_inverse: bool = False, return_counts: bool = False, descending: bool = False,
                 ctx: Optional[Context] = None, key_kind: Optional[int] = None):
    """`torch.unique(keys, sorted=True, return_inverse=..., return_counts=...)` through radix_group: the distinct keys in
    sorted order and, where asked for, the int64 index of every key's group and the int64 counts, as a tuple in that
    order (the keys alone when neither is asked for).  Reads the number of groups once, which synchronises, as torch does.

    Floats differ from torch: the order is radix_argsort's total order on bit patterns (-NaN first, -0.0 below +0.0, +NaN
    last) and equality is bit-pattern equality, so -0.0 and +0.0 are two keys and every NaN payload is a key of its own."""
    g = radix_group(keys, descending=descending, perm=False, inverse=return_inverse, ctx=ctx, key_kind=key_kind)
    m = int(g.num)
    out = (g.keys[:m],)
    if return_inverse:
        out += (g.inverse,)
    if return_counts:
        out += (g.offsets[1:m + 1] - g.offsets[:m],)
    return out if len(out) > 1 else out[0]


def search_caps(key_bytes: int, with_positions: bool = False):
    """rsx_search_caps -> (tile, window): the needles one workgroup of the search kernel takes and the most sorted keys it
    stages in LDS for this key width.  Needs no device."""
    L = _lib.load()
    tile, window = ctypes.c_uint32(), ctypes.c_uint32()
    rc = L.rsx_search_caps(key_bytes, 1 if with_positions else 0, ctypes.byref(tile), ctypes.byref(window))
    _check_rc(L, rc)
    return int(tile.value), int(window.value)


def _search_presort(n: int, m: int, key_bytes: int) -> bool:
    """presort=None of radix_searchsorted: sort the needles first?  The rule of DESIGN.md section 5 ("Search"), which cannot
    see whether the needles are ordered: from 2^19 needles on, in a haystack of 512 MiB or more -- where scattered needles
    measured 1.3 (2^19) to 6 times (m = n) faster sorted first, and ordered ones up to 3.6 times slower.  Callers who know
    their needles are ordered (both sides of a join out of this library) pass presort=False."""
    return m >= 1 << 19 and n * key_bytes >= 1 << 29


def radix_searchsorted(sorted_keys, needles, side: str = "left", descending: bool = False, out=None, index_dtype=None,
                       sorted_num=None, presort: Optional[bool] = None, ctx: Optional[Context] = None, key_kind: Optional[int] = None):
    """Where every needle falls in `sorted_keys` (rsx_search_sorted_device), like `torch.searchsorted(sorted_keys, needles,
    right=...)`: side="left" gives, per needle, the number of sorted keys that order before it, side="right" the number
    that do not order behind it, side="both" the tuple (left, right), so that sorted_keys[left:right] are the keys equal
    to the needle.  The result has the needles' shape and index_dtype (torch.int64, the default, or torch.int32), or is
    `out` (for "both": a pair), contiguous int32 or int64 tensors of that shape on the same device.

    sorted_keys: a contiguous 1-D GPU tensor of a dtype radix_sort knows, or (n, 16) uint8 128-bit keys (key_kind=), in the
       order radix_sort / radix_sort_pairs(descending=descending) / radix_group leave: the total order on bit patterns
       (-NaN below -inf, -0.0 below +0.0, +NaN above +inf), not torch's.  Only its first min(n, sorted_num) keys count
       when sorted_num is given: a one-element int64 device tensor such as radix_group(...).num, read on the device.
    needles: a contiguous tensor of any shape, the same dtype and device (128-bit keys: shape (..., 16)).
    presort: sort the needles first (True), take them as given (False), or decide from the sizes (None: sorted first
       from 2^19 needles on in a haystack of 512 MiB or more).  The result is the same; needles that are ordered or
       clustered run at streaming speed as given, so pass presort=False for those.

    Enqueued on the current stream, not synchronised."""
    import torch
    kb, kind, n = _pairs_keys(sorted_keys, key_kind)
    if not isinstance(needles, torch.Tensor):
        raise TypeError("needles must be a torch tensor on a GPU")
    if needles.dtype != sorted_keys.dtype:
        raise TypeError(f"needles must have the dtype of sorted_keys ({sorted_keys.dtype}), not {needles.dtype}")
    if needles.device != sorted_keys.device:
        raise ValueError("sorted_keys and needles must live on the same device")
    if not needles.is_contiguous():
        raise ValueError("needles must be contiguous")
    if kb == 16:
        if needles.dim() < 1 or needles.shape[-1] != 16:
            raise ValueError("needles of 128-bit keys must have shape (..., 16)")
        shape = tuple(needles.shape[:-1])
    else:
        shape = tuple(needles.shape)
    if side not in ("left", "right", "both"):
        raise ValueError(f'side must be "left", "right" or "both", not {side!r}')
    outs = out if side == "both" and out is not None else (out,)
    if side == "both" and out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
        raise TypeError('out must be a pair of tensors for side="both"')
    for o in outs:
        _index_out(o, shape, "the needles")
        if o is not None and o.device != sorted_keys.device:
            raise ValueError("sorted_keys and out must live on the same device")
    if out is not None:
        if len({o.dtype for o in outs}) != 1:
            raise TypeError("both tensors of out must have one dtype")
        index_dtype = outs[0].dtype
    index_dtype = _index_dtype(index_dtype)
    if sorted_num is not None:
        if not isinstance(sorted_num, torch.Tensor) or sorted_num.dtype != torch.int64 or sorted_num.numel() != 1:
            raise TypeError("sorted_num must be a one-element int64 tensor")
        if sorted_num.device != sorted_keys.device:
            raise ValueError("sorted_keys and sorted_num must live on the same device")
    _pairs_device(sorted_keys, None, "")
    if index_dtype == torch.int32 and n >= 1 << 32:
        raise ValueError("2^32 or more sorted keys need int64 indices")
    m = 1
    for d in shape:
        m *= d
    want_lower, want_upper = side in ("left", "both"), side in ("right", "both")
    if out is None:
        lower = torch.empty(shape, dtype=index_dtype, device=needles.device) if want_lower else None
        upper = torch.empty(shape, dtype=index_dtype, device=needles.device) if want_upper else None
    else:
        lower = outs[0] if want_lower else None
        upper = outs[-1] if want_upper else None
    if m > 0:
        if presort is None:
            presort = _search_presort(n, m, kb)
        with _on_device(sorted_keys, ctx) as (c, stream):
            c.search_sorted_device(sorted_keys.data_ptr() if n else 0, n, needles.data_ptr(), m, kb, kind,
                                   lower.data_ptr() if want_lower else 0, upper.data_ptr() if want_upper else 0,
                                   8 if index_dtype == torch.int64 else 4, descending,
                                   sorted_num.data_ptr() if sorted_num is not None else 0,
                                   _lib.SEARCH_PRESORT if presort and m < 1 << 32 else 0, stream)
    if side == "both":
        return lower, upper
    return lower if want_lower else upper


def bin_caps(key_bytes: int):
    """rsx_bin_caps -> (max_edges, max_index_bins_lds, share): the most edges rsx_bin_count_device takes for this key
    width, the values its index mode counts in LDS in one pass over the keys, and the fewest keys worth a workgroup.  Needs no device."""
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(3)]
    rc = L.rsx_bin_caps(key_bytes, *[ctypes.byref(o) for o in out])
    _check_rc(L, rc)
    return tuple(int(o.value) for o in out)


def _bin_args(keys, bins: int, num, out, accumulate: bool, count_dtype):
    """The checks radix_histogram and radix_bincount share (none needs a context) -> the count dtype."""
    import torch
    if accumulate and out is None:
        raise ValueError("accumulate=True adds to out=, which must be given")
    if count_dtype is not None and count_dtype not in (torch.int32, torch.int64):
        raise ValueError(f"count_dtype must be torch.int32 or torch.int64, not {count_dtype}")
    if out is not None:
        _index_out(out, (bins,), "the bins")
        if count_dtype is not None and count_dtype != out.dtype:
            raise TypeError(f"count_dtype ({count_dtype}) is not the dtype of out ({out.dtype})")
        if out.device != keys.device:
            raise ValueError("keys and out must live on the same device")
        count_dtype = out.dtype
    if num is not None:
        if not isinstance(num, torch.Tensor) or num.dtype != torch.int64 or num.numel() != 1:
            raise TypeError("num must be a one-element int64 tensor")
        if num.device != keys.device:
            raise ValueError("keys and num must live on the same device")
    count_dtype = torch.int64 if count_dtype is None else count_dtype
    if count_dtype == torch.int32 and keys.numel() >= 1 << 32:
        raise ValueError("2^32 or more keys need int64 counts")
    return count_dtype


def radix_histogram(keys, edges, side: str = "right", descending: bool = False, num=None, out=None, accumulate: bool = False,
                    count_dtype=None, ctx: Optional[Context] = None, key_kind: Optional[int] = None, weights=None):
    """How many keys fall between the cut points `edges` (rsx_bin_count_device): the m + 1 counts
    `torch.bincount(radix_searchsorted(edges, keys, side=side, descending=descending).flatten(), minlength=m + 1)` for
    m = len(edges), in one read of the keys and with no index array.  side="right" (the default, `torch.bucketize(keys,
    edges, right=True)`) counts in bin b the keys with edges[b - 1] <= key < edges[b]; side="left" those with
    edges[b - 1] < key <= edges[b].  counts[0] and counts[m] are the two open ends: the keys before the first and from
    the last edge on (side="left": up to the first and behind the last).

    Against `numpy.histogram(x, edges)[0]` with side="right": it equals counts[1:m], except that numpy closes its last
    bin on the right, so keys equal to the last edge are in counts[m] here and in the last bin there.

    keys: a contiguous GPU tensor of any shape and of a dtype radix_sort knows (128-bit keys: (..., 16) uint8 with (m, 16)
       uint8 edges, key_kind= as in radix_argsort); it is not modified.
    edges: a contiguous 1-D tensor of the same dtype on the same device, sorted in the order radix_sort(descending=
       descending) leaves -- the total order on bit patterns (-NaN below -inf, -0.0 below +0.0, +NaN above +inf), not
       torch's; equal edges give empty bins; m = 0 gives one bin.  Unsorted edges give unspecified counts.
    num: a one-element int64 device tensor such as radix_group(...).num: only the first min(n, num) keys count; it is
       read on the device.
    out: a contiguous int32 or int64 tensor of m + 1 counts to write (accumulate=True: to add to); otherwise a new
       tensor of count_dtype (torch.int64, the default, or torch.int32).
    weights: a tensor with one entry per key: the m + 1 SUMS of the weights per bin instead of the counts, in
       weights.dtype -- `numpy.histogram(keys, edges, weights=weights)`; the call is radix_bin_reduce(keys, weights,
       edges=edges, op="sum", ...), whose rules for out=, accumulate= and the dtypes hold (count_dtype is not taken).
    More edges than bin_caps(key_bytes)[0] go through radix_searchsorted into an index array and the index form.
    Enqueued on the current stream, not synchronised; the host reads nothing."""
    import torch
    if weights is not None:
        if count_dtype is not None:
            raise ValueError("count_dtype= has no meaning with weights=: the sums have the dtype of the weights")
        return radix_bin_reduce(keys, weights, edges=edges, op="sum", side=side, descending=descending, num=num, out=out, accumulate=accumulate,
                                ctx=ctx, key_kind=key_kind)
    if not isinstance(keys, torch.Tensor) or not isinstance(edges, torch.Tensor):
        raise TypeError("keys and edges must be torch tensors on a GPU")
    if edges.dtype != keys.dtype:
        raise TypeError(f"edges must have the dtype of keys ({keys.dtype}), not {edges.dtype}")
    if not keys.is_contiguous():
        raise ValueError("keys must be contiguous")
    kb, kind, m = _pairs_keys(edges, key_kind)
    if kb == 16:
        if keys.dim() < 1 or keys.shape[-1] != 16:
            raise ValueError("128-bit keys must have shape (..., 16)")
        n = keys.numel() // 16
    else:
        n = keys.numel()
    if side not in ("left", "right"):
        raise ValueError(f'side must be "left" or "right", not {side!r}')
    if edges.device != keys.device:
        raise ValueError("keys and edges must live on the same device")
    count_dtype = _bin_args(keys, m + 1, num, out, accumulate, count_dtype)
    _pairs_device(keys, None, "")
    if out is None:
        out = torch.empty(m + 1, dtype=count_dtype, device=keys.device)
    flags = _lib.BIN_ACCUMULATE if accumulate else 0
    d_num = num.data_ptr() if num is not None else 0
    if m > bin_caps(kb)[0]:  # too many edges for LDS: the bin of every key as an index, then the index form
        flat = keys.reshape(-1, 16) if kb == 16 else keys.reshape(-1)
        idx = radix_searchsorted(edges, flat, side=side, descending=descending, index_dtype=torch.int32 if m < (1 << 31) - 1 else torch.int64,
                                 ctx=ctx, key_kind=key_kind)
        with _on_device(keys, ctx) as (c, stream):
            c.bin_count_device(idx.data_ptr() if n else 0, n, idx.element_size(), KEY_SIGNED, 0, m, _lib.BIN_INDEX, out.data_ptr(),
                               out.element_size(), False, d_num, flags, stream)
        return out
    with _on_device(keys, ctx) as (c, stream):
        c.bin_count_device(keys.data_ptr() if n else 0, n, kb, kind, edges.data_ptr() if m else 0, m,
                           _lib.BIN_UPPER if side == "right" else _lib.BIN_LOWER, out.data_ptr(), out.element_size(), descending, d_num,
                           flags, stream)
    return out


def radix_bincount(keys, num_bins: int, num=None, out=None, accumulate: bool = False, count_dtype=None, ctx: Optional[Context] = None,
                   weights=None):
    """How often every value 0 .. num_bins - 1 occurs among integer `keys` (rsx_bin_count_device, index mode):
    num_bins + 1 counts, of which [:num_bins] equals `torch.bincount(in-range keys, minlength=num_bins)` and the last
    entry counts the keys outside -- negative ones and those of num_bins or more, which torch refuses or grows for.

    keys: a contiguous GPU tensor of any shape and an integer dtype (uint8, int8, int16, int32, int64 and, where torch has
       them, uint16, uint32, uint64); it is not modified.
    num, out, accumulate, count_dtype: as in radix_histogram; out holds num_bins + 1 counts.
    Up to bin_caps(key_bytes)[1] values are counted in LDS in one pass over the keys, up to 16 times as many in as many
    passes, more by atomics straight into the counts.
    weights: a tensor with one entry per key: the num_bins + 1 SUMS of the weights per value instead of the counts, in
       weights.dtype -- `torch.bincount(keys, weights=weights)`; the call is radix_bin_reduce(keys, weights,
       num_bins=num_bins, op="sum", ...), whose rules for out=, accumulate= and the dtypes hold (count_dtype is not taken).
    Enqueued on the
    current stream, not synchronised; the host reads nothing."""
    import torch
    if weights is not None:
        if count_dtype is not None:
            raise ValueError("count_dtype= has no meaning with weights=: the sums have the dtype of the weights")
        return radix_bin_reduce(keys, weights, num_bins=num_bins, op="sum", num=num, out=out, accumulate=accumulate, ctx=ctx)
    if not isinstance(keys, torch.Tensor):
        raise TypeError("keys must be a torch tensor on a GPU")
    if not keys.is_contiguous():
        raise ValueError("keys must be contiguous")
    d = _torch_digits(keys, None)
    if d.key_kind == KEY_FLOAT or d.key_bytes != d.elem_bytes:
        raise TypeError(f"radix_bincount takes integer keys, not {keys.dtype}")
    num_bins = operator.index(num_bins)
    if num_bins < 0 or num_bins >= (1 << 32) - 1:
        raise ValueError(f"num_bins must be in 0 .. 2^32 - 2, not {num_bins}")
    count_dtype = _bin_args(keys, num_bins + 1, num, out, accumulate, count_dtype)
    _pairs_device(keys, None, "")
    if out is None:
        out = torch.empty(num_bins + 1, dtype=count_dtype, device=keys.device)
    n = keys.numel()
    with _on_device(keys, ctx) as (c, stream):
        c.bin_count_device(keys.data_ptr() if n else 0, n, d.key_bytes, d.key_kind, 0, num_bins, _lib.BIN_INDEX, out.data_ptr(),
                           out.element_size(), False, num.data_ptr() if num is not None else 0,
                           _lib.BIN_ACCUMULATE if accumulate else 0, stream)
    return out


def bin_reduce_caps(key_bytes: int, value_bytes: int):
    """rsx_bin_reduce_caps -> (max_edges, max_index_bins, tile, share): the most edges and the largest num_bins
    rsx_bin_reduce_device takes for these key and value widths, the rows of one tile of its first launch and the fewest
    rows worth a workgroup.  Needs no device."""
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(4)]
    _check_rc(L, L.rsx_bin_reduce_caps(key_bytes, value_bytes, *[ctypes.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def _bin_reduce_bits(values):
    """`values` as signed integers of its width: the bit patterns the operators are defined on."""
    import torch
    return values.view(torch.int32 if values.element_size() == 4 else torch.int64)


def _bin_reduce_identity(vb: int, vkind: int, op: str) -> int:
    """The bit pattern an empty bin holds, as a signed integer of vb bytes."""
    top = 1 << (8 * vb - 1)
    if op == "sum":
        return 0
    if op == "max":
        return -1 if vkind == KEY_FLOAT else -top if vkind == KEY_SIGNED else 0  # the float of all ones; the signed minimum; 0
    return -1 if vkind == KEY_UNSIGNED else top - 1  # the unsigned maximum; all ones below the sign: the signed maximum, a +NaN


def _bin_reduce_join(a, b, vkind: int, op: str, float_dtype):
    """a (+) b on bit patterns held as signed integers: a wrapping or IEEE sum, or min / max by the value's order."""
    import torch
    if op == "sum":
        return (a.view(float_dtype) + b.view(float_dtype)).view(a.dtype) if vkind == KEY_FLOAT else a + b
    top = -(1 << (8 * a.element_size() - 1))
    if vkind == KEY_FLOAT:  # negative floats: the bits below the sign flipped, then signed order is the total order
        ka, kb = a ^ ((a >> (8 * a.element_size() - 1)) & ~top), b ^ ((b >> (8 * b.element_size() - 1)) & ~top)
    elif vkind == KEY_SIGNED:
        ka, kb = a, b
    else:
        ka, kb = a ^ top, b ^ top
    return torch.where((ka < kb) == (op == "min"), a, b)


def _bin_reduce_by_sort(flat, n, edges, m, side, descending, values, vt, op, out, accumulate, counts, key_kind, ctx):
    """radix_bin_reduce past bin_reduce_caps: the bin of every row (radix_searchsorted, or the id itself with the outside
    ones set to m), radix_reduce_by_key on the bins, the first `num` group results copied into an identity-filled array
    through a spare slot, the counts by radix_histogram / radix_bincount.  No host read."""
    import torch
    vb, vkind = vt
    small = m < (1 << 31) - 2
    if edges is not None:
        bins = radix_searchsorted(edges, flat, side=side, descending=descending, index_dtype=torch.int32 if small else torch.int64, ctx=ctx,
                                  key_kind=key_kind)
        if counts is not None:
            radix_histogram(flat, edges, side=side, descending=descending, out=counts, accumulate=accumulate, ctx=ctx, key_kind=key_kind)
    else:
        wide = flat.to(torch.int64) if flat.dtype != torch.uint64 else flat.view(torch.int64)  # (uint64 ids of 2^63 or more: negative, outside)
        bins = torch.where((wide < 0) | (wide >= m), m, wide).to(torch.int32 if small else torch.int64)
        if counts is not None:
            radix_bincount(flat, m, out=counts, accumulate=accumulate, ctx=ctx)
    int_dtype = torch.int32 if vb == 4 else torch.int64
    full = torch.full((m + 2,), _bin_reduce_identity(vb, vkind, op), dtype=int_dtype, device=flat.device)
    if n:
        red = radix_reduce_by_key(bins, values.reshape(-1), op=op, ctx=ctx)
        slot = torch.where(torch.arange(n, device=flat.device) < red.num, red.keys.to(torch.int64), m + 1)  # (the groups behind num: the spare slot)
        full.scatter_(0, slot, _bin_reduce_bits(red.values))
    res = full[:m + 1]
    if op == "sum" and vkind == KEY_FLOAT:
        res = (res.view(values.dtype) + 0.0).view(int_dtype)  # a sum starts from +0.0
    bits = _bin_reduce_bits(out)
    bits.copy_(_bin_reduce_join(bits, res, vkind, op, values.dtype) if accumulate else res)


def radix_bin_reduce(keys, values, edges=None, num_bins=None, op: str = "sum", side: str = "right", descending: bool = False, num=None,
                     out=None, accumulate: bool = False, return_counts: bool = False, count_dtype=None, ctx: Optional[Context] = None,
                     key_kind: Optional[int] = None):
    """A value column combined per bin, nothing sorted (rsx_bin_reduce_device): `numpy.histogram(keys, weights=values)`,
    `torch.bincount(ids, weights=values)`, `zeros.index_add_(0, ids, values)`, `scatter_reduce` over a few hundred labels
    -- the sum ("sum"), minimum ("min") or maximum ("max") of values[i] over the rows whose key falls into bin b, for
    b = 0 .. m, in one read of the keys and the values.  Returns a tensor of m + 1 values of values.dtype, or
    (values, counts) with return_counts=True, counts being what radix_histogram / radix_bincount give.

    Exactly one of `edges` and `num_bins` is given, under the rules of radix_partition: edges= m cut points as in
    radix_histogram (side=, descending=), num_bins= m for integer keys that are bin ids themselves, the last bin m holding
    the rows outside 0 .. m - 1.
    keys: a contiguous GPU tensor of any shape of a dtype radix_sort knows ((..., 16) uint8 128-bit keys with key_kind=, edge
       modes only); it is not modified.
    values: a contiguous tensor with one entry per key, of dtype int32, int64, float32 or float64 (uint32 / uint64 where
       torch has them); anything else raises TypeError.  Integer sums wrap; float minima and maxima follow the total order
       on bit patterns (-0.0 below +0.0, +NaN the largest) and return one of the bin's values bit for bit; a float sum is
       IEEE addition in values.dtype, associated in an order fixed by the input's contents and size and the device's grid
       alone -- there are no atomics, so the same input gives the same bits on every call.
    An empty bin holds the operator's identity: 0 or +0.0 for "sum"; the largest value of the order for "min" (the integer
       maximum; for floats the +NaN of all ones below the sign); the smallest for "max" (the integer minimum; the float of
       all ones).  Divide by the counts for a mean.
    num: a one-element int64 device tensor: only the first min(n, num) rows count.
    out: a contiguous tensor of m + 1 values of values.dtype to write; accumulate=True combines onto it instead (and adds
       to the counts of a (values, counts) pair given as out=).
    More edges than bin_reduce_caps(key_bytes, value_bytes)[0], or a num_bins above [1], take the sorted route through
    this library's own calls (radix_searchsorted, radix_reduce_by_key): the same result for integers, minima and maxima,
    another association for float sums; with num= they raise ValueError instead.  The host reads nothing.
    Enqueued on the current stream, not synchronised."""
    import torch
    if (edges is None) == (num_bins is None):
        raise ValueError("exactly one of edges= and num_bins= must be given")
    if not isinstance(keys, torch.Tensor) or not isinstance(values, torch.Tensor):
        raise TypeError("keys and values must be torch tensors on a GPU")
    if op not in _REDUCE_OPS:
        raise ValueError(f"op must be 'sum', 'min' or 'max', not {op!r}")
    vt = _reduce_value_types().get(values.dtype)
    if vt is None:
        raise TypeError(f"values must be int32, int64, float32, float64, uint32 or uint64, not {values.dtype}")
    if not keys.is_contiguous():
        raise ValueError("keys must be contiguous")
    if edges is not None:
        if not isinstance(edges, torch.Tensor):
            raise TypeError("edges must be a torch tensor")
        if edges.dtype != keys.dtype:
            raise TypeError(f"edges must have the dtype of keys ({keys.dtype}), not {edges.dtype}")
        kb, kind, m = _pairs_keys(edges, key_kind)
        if side not in ("left", "right"):
            raise ValueError(f'side must be "left" or "right", not {side!r}')
        if edges.device != keys.device:
            raise ValueError("keys and edges must live on the same device")
        mode = _lib.BIN_UPPER if side == "right" else _lib.BIN_LOWER
    else:
        d = _torch_digits(keys, None)
        if d.key_kind == KEY_FLOAT or d.key_bytes != d.elem_bytes or key_kind is not None:
            raise TypeError(f"num_bins= takes integer keys, not {keys.dtype}")
        if descending:
            raise ValueError("num_bins= takes no order: descending must be False")
        kb, kind = d.key_bytes, d.key_kind
        m = operator.index(num_bins)
        if m < 0 or m >= (1 << 32) - 2:
            raise ValueError(f"num_bins must be in 0 .. 2^32 - 3, not {m}")
        mode = _lib.BIN_INDEX
    if kb == 16:
        if keys.dim() < 1 or keys.shape[-1] != 16:
            raise ValueError("128-bit keys must have shape (..., 16)")
        n = keys.numel() // 16
    else:
        n = keys.numel()
    if values.numel() != n:
        raise ValueError(f"values must have one entry per key ({n}), not {values.numel()}")
    if not values.is_contiguous():
        raise ValueError("values must be contiguous")
    if values.device != keys.device:
        raise ValueError("keys and values must live on the same device")
    if n >= 1 << 32:
        raise ValueError("radix_bin_reduce takes fewer than 2^32 rows")
    out_counts = None
    if out is not None and isinstance(out, (tuple, list)):
        if len(out) != 2:
            raise TypeError("out must be a tensor of values or a (values, counts) pair")
        out, out_counts = out
    if out_counts is not None and not return_counts:
        raise ValueError("out=(values, counts) needs return_counts=True")
    if accumulate and (out is None or (return_counts and out_counts is None)):
        raise ValueError("accumulate=True combines onto out=, which must be given (with return_counts=True: a (values, counts) pair)")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != values.dtype:
            raise TypeError(f"out must be a tensor of the dtype of values ({values.dtype})")
        if tuple(out.shape) != (m + 1,) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous tensor of shape ({m + 1},)")
        if out.device != keys.device:
            raise ValueError("keys and out must live on the same device")
    count_dtype = _bin_args(keys, m + 1, num, out_counts, accumulate and out_counts is not None, count_dtype)
    max_edges, max_index_bins, _tile, _share = bin_reduce_caps(kb, vt[0])
    sorted_route = m > (max_edges if edges is not None else max_index_bins)
    if sorted_route and num is not None:
        raise ValueError(f"num= needs at most {max_edges} edges or {max_index_bins} bins for these widths (bin_reduce_caps), not {m}")
    _pairs_device(keys, None, "")
    if out is None:
        out = torch.empty(m + 1, dtype=values.dtype, device=keys.device)
    if return_counts and out_counts is None:
        out_counts = torch.empty(m + 1, dtype=count_dtype, device=keys.device)
    if sorted_route:
        flat = keys.reshape(-1, 16) if kb == 16 else keys.reshape(-1)
        _bin_reduce_by_sort(flat, n, edges, m, side, descending, values, vt, op, out, accumulate, out_counts, key_kind, ctx)
    else:
        with _on_device(keys, ctx) as (c, stream):
            c.bin_reduce_device(keys.data_ptr() if n else 0, values.data_ptr() if n else 0, n, kb, kind,
                                edges.data_ptr() if edges is not None and m else 0, m, mode, vt[0], vt[1], _REDUCE_OPS[op], out.data_ptr(),
                                out_counts.data_ptr() if out_counts is not None else 0,
                                out_counts.element_size() if out_counts is not None else 8, descending,
                                num.data_ptr() if num is not None else 0, _lib.BIN_ACCUMULATE if accumulate else 0, stream)
    return (out, out_counts) if return_counts else out


def partition_caps(key_bytes: int):
    """rsx_multisplit_caps -> (max_edges, max_index_bins, tile, share): the most edges and the largest num_bins
    rsx_multisplit_device takes for this key width, the rows of one tile of its write launch and the fewest rows worth a
    workgroup.  Needs no device."""
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(4)]
    _check_rc(L, L.rsx_multisplit_caps(key_bytes, *[ctypes.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


Partitioned = namedtuple("Partitioned", ["keys", "values", "index", "offsets"])


def _partition_by_sort(keys, kb, n, edges, m, side, descending, values, num, key_kind, outs, ctx):
    """radix_partition past partition_caps: the bin of every row (radix_searchsorted, or the id itself), a stable
    radix_argsort of the bins, a gather per column, and the offsets from the bin counts.  With num= the rows from
    min(n, num) on sort behind every bin and keep what the outputs held."""
    import torch
    out_keys, out_values, out_index, out_offsets = outs
    small = m < (1 << 31) - 2
    if edges is not None:
        bins = radix_searchsorted(edges, keys, side=side, descending=descending, index_dtype=torch.int32 if small else torch.int64, ctx=ctx,
                                  key_kind=key_kind)
        counts = radix_histogram(keys, edges, side=side, descending=descending, num=num, ctx=ctx, key_kind=key_kind)
    else:
        wide = keys.to(torch.int64) if keys.dtype != torch.uint64 else keys.view(torch.int64)  # (uint64 ids of 2^63 or more: negative, outside)
        bins = torch.where((wide < 0) | (wide >= m), m, wide).to(torch.int32 if small else torch.int64)
        counts = radix_bincount(keys, m, num=num, ctx=ctx)
    live = None
    if num is not None:
        live = torch.arange(n, device=keys.device) < num.reshape(())
        bins = torch.where(live, bins, m + 1)
    perm = radix_argsort(bins, ctx=ctx)
    out_offsets[0] = 0
    torch.cumsum(counts, 0, out=out_offsets[1:])
    for src, dst in ((keys, out_keys), (values, out_values)):
        if dst is not None:
            got = src.index_select(0, perm)
            dst.copy_(got if live is None else torch.where(live.reshape((n,) + (1,) * (src.dim() - 1)), got, dst))
    if out_index is not None:
        got = perm.to(out_index.dtype)
        out_index.copy_(got if live is None else torch.where(live, got, out_index))


def radix_partition(keys, edges=None, num_bins=None, values=None, side: str = "right", descending: bool = False,
                    return_index: bool = False, index_dtype=None, num=None, out=None, ctx: Optional[Context] = None,
                    key_kind: Optional[int] = None):
    """A stable multi-way partition (rsx_multisplit_device): every row moved into the bin of its key, in input order
    inside each bin, with the CSR offsets of the bins -- what `radix_searchsorted`, a stable `radix_argsort` of the bin
    ids, a gather per column and a cumsum of `radix_histogram` give, in two reads of the keys and one write of each
    column.  Token -> expert dispatch (num_bins=), range partitioning by the cuts radix_quantile leaves on the device
    (edges=), bucketing for radix_sort_segments.

    Exactly one of `edges` and `num_bins` is given.
    edges: m cut points under the rules of radix_histogram (same dtype and device, sorted in the order
       radix_sort(descending=descending) leaves, the total order on bit patterns; equal edges give empty bins; m = 0: one
       bin); side="right" puts edges[b - 1] <= key < edges[b] into bin b, side="left" edges[b - 1] < key <= edges[b].
       Unsorted edges give an unspecified grouping, still a permutation of the rows.
    num_bins: m, for integer keys that are bin ids themselves: bin k holds the rows with key k for k < m, the last bin m
       the rows outside (negative ids and those of m or more).

    Returns Partitioned(keys, values, index, offsets): keys and values (None without values=) regrouped, index (only with
    return_index=True; index_dtype torch.int64 or torch.int32) the input position of every output row -- `out.keys ==
    keys[out.index]`, and scattering by it un-permutes a result --, and offsets, an int64 tensor of m + 2 values: bin b is
    rows offsets[b] .. offsets[b + 1], offsets[m + 1] the number of rows.  It is the layout radix_group(...).offsets has
    and radix_sort_segments takes.

    keys: a contiguous 1-D GPU tensor of a dtype radix_sort knows, or (n, 16) uint8 128-bit keys (key_kind=, edge modes
       only); it is not modified.
    values: a contiguous tensor with one row per key; a row is one value of up to 32768 bytes, moved bitwise.  Widths of
       1, 2, 4, 8, 16 bytes move in the write kernel, others behind positions.
    num: a one-element int64 device tensor: only the first min(n, num) rows count; nothing is written behind them.
    out: a Partitioned of preallocated tensors (keys, values, index of n rows -- None for an output that is not wanted --
       and offsets of m + 2 int64): nothing is allocated, and after Context.reserve_multisplit the call can be captured.
       No output may overlap an input.
    More edges than partition_caps(key_bytes)[0], or a num_bins above partition_caps(key_bytes)[1], take the chain named
    above, through this library's own calls: the same result, more passes over the data.  The host still reads nothing.
    Enqueued on the current stream, not synchronised."""
    import torch
    if (edges is None) == (num_bins is None):
        raise ValueError("exactly one of edges= and num_bins= must be given")
    kb, kind, n = _pairs_keys(keys, key_kind)
    if edges is not None:
        if not isinstance(edges, torch.Tensor):
            raise TypeError("edges must be a torch tensor")
        if edges.dtype != keys.dtype:
            raise TypeError(f"edges must have the dtype of keys ({keys.dtype}), not {edges.dtype}")
        ekb, _ekind, m = _pairs_keys(edges, key_kind)
        if ekb != kb:
            raise ValueError("edges must be shaped like the keys: 1-D, or (m, 16) uint8 for 128-bit keys")
        if side not in ("left", "right"):
            raise ValueError(f'side must be "left" or "right", not {side!r}')
        if edges.device != keys.device:
            raise ValueError("keys and edges must live on the same device")
        mode = _lib.BIN_UPPER if side == "right" else _lib.BIN_LOWER
    else:
        if kind == KEY_FLOAT or kb == 16:
            raise TypeError(f"num_bins= takes integer keys, not {keys.dtype}")
        if descending:
            raise ValueError("num_bins= takes no order: descending must be False")
        m = operator.index(num_bins)
        if m < 0 or m >= (1 << 32) - 2:
            raise ValueError(f"num_bins must be in 0 .. 2^32 - 3, not {m}")
        mode = _lib.BIN_INDEX
    vb = _value_bytes(values, (n,), "keys")
    if values is not None and values.device != keys.device:
        raise ValueError("keys and values must live on the same device")
    _set_num(num, keys, "num")
    if n >= 1 << 32:
        raise ValueError("radix_partition takes fewer than 2^32 rows")
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise TypeError("out must be a Partitioned(keys, values, index, offsets)")
        out_keys, out_values, out_index, out_offsets = out
        if out_keys is not None:
            _merge_out(out_keys, keys, n, "keys")
        if out_values is not None:
            if values is None:
                raise ValueError("out.values needs values")
            _merge_out(out_values, values, n, "values")
        if out_index is not None:
            _index_out(out_index, (n,), "the rows")
            if out_index.device != keys.device:
                raise ValueError("the keys and out (index) must live on the same device")
            if index_dtype is not None and index_dtype != out_index.dtype:
                raise TypeError(f"index_dtype ({index_dtype}) is not the dtype of out.index ({out_index.dtype})")
        elif return_index:
            raise ValueError("return_index=True with out= needs out.index")
        if not isinstance(out_offsets, torch.Tensor) or out_offsets.dtype != torch.int64:
            raise TypeError("out.offsets must be an int64 tensor")
        if tuple(out_offsets.shape) != (m + 2,) or not out_offsets.is_contiguous():
            raise ValueError(f"out.offsets must be a contiguous tensor of shape ({m + 2},)")
        if out_offsets.device != keys.device:
            raise ValueError("the keys and out (offsets) must live on the same device")
    else:
        index_dtype = _index_dtype(index_dtype)
    _pairs_device(keys, None, "")
    if out is None:
        out_keys = torch.empty_like(keys)
        out_values = torch.empty_like(values) if values is not None else None
        out_index = torch.empty(n, dtype=index_dtype, device=keys.device) if return_index else None
        out_offsets = torch.empty(m + 2, dtype=torch.int64, device=keys.device)
    result = Partitioned(out_keys, out_values, out_index, out_offsets)
    max_edges, max_index_bins, _tile, _share = partition_caps(kb)
    if m > (max_edges if edges is not None else max_index_bins):
        _partition_by_sort(keys, kb, n, edges, m, side, descending, values, num, key_kind, result, ctx)
        return result
    with _on_device(keys, ctx) as (c, stream):
        c.multisplit_device(keys.data_ptr() if n else 0, n, kb, kind, edges.data_ptr() if edges is not None and m else 0, m, mode,
                            values.data_ptr() if out_values is not None and n else 0, vb if out_values is not None and n else 0,
                            out_keys.data_ptr() if out_keys is not None and n else 0,
                            out_values.data_ptr() if out_values is not None and n else 0,
                            out_index.data_ptr() if out_index is not None and n else 0,
                            out_index.element_size() if out_index is not None else 8, out_offsets.data_ptr(), descending,
                            num.data_ptr() if num is not None else 0, stream)
    return result


def compact_caps(key_bytes: int = 0, value_bytes: int = 0, index_bytes: int = 0):
    """rsx_compact_caps -> (tile, scan_span): the rows one workgroup of rsx_compact_device's count and write launches takes
    for these key, value and index widths (0: no such column), and the tiles one sweep of its scan takes.  Needs no
    device."""
    L = _lib.load()
    out = [ctypes.c_uint32() for _ in range(2)]
    _check_rc(L, L.rsx_compact_caps(key_bytes, value_bytes, index_bytes, *[ctypes.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


Compacted = namedtuple("Compacted", ["keys", "values", "index", "num"])


def _compact_bound(bound, keys, kb: int, what: str):
    """lo= / hi= of radix_compact -> None or a one-key tensor of the keys' dtype; a Python scalar is placed beside the
    keys with torch.tensor (a copy to the device, no read from it)."""
    import torch
    if bound is None:
        return None
    if keys is None:
        raise ValueError(f"{what} needs keys to compare with")
    if not isinstance(bound, torch.Tensor):
        if kb == 16 or isinstance(bound, (bool, str, bytes)) or not isinstance(bound, (int, float)):
            raise TypeError(f"{what} must be a one-element tensor of the keys' dtype or a Python number")
        return torch.tensor([bound], dtype=keys.dtype, device=keys.device)
    if bound.dtype != keys.dtype:
        raise TypeError(f"{what} must have the dtype of keys ({keys.dtype}), not {bound.dtype}")
    if bound.numel() != (16 if kb == 16 else 1) or not bound.is_contiguous():
        raise ValueError(f"{what} must hold one key: a one-element tensor" + (" ((16,) or (1, 16) uint8 for 128-bit keys)" if kb == 16 else ""))
    if bound.device != keys.device:
        raise ValueError(f"keys and {what} must live on the same device")
    return bound


def radix_compact(keys, mask=None, lo=None, hi=None, values=None, descending: bool = False, invert: bool = False,
                  partition: bool = False, return_index: bool = False, index_dtype=None, num=None, out=None,
                  ctx: Optional[Context] = None, key_kind: Optional[int] = None):
    """The rows that pass a mask and / or a key range, in input order, with their number left on the device
    (rsx_compact_device): `keys[mask]`, `torch.masked_select`, `values[(keys >= lo) & (keys < hi)]` without a host read,
    so that the call can be captured and chained.  Row i passes when mask[i] is non-zero (mask given), lo <= keys[i] (lo
    given) and keys[i] < hi (hi given), compared in the order radix_sort(descending=descending) leaves -- the total order
    on bit patterns (-NaN below -inf, -0.0 below +0.0, +NaN above +inf), not torch's; descending=True turns both
    comparisons round (lo is then the largest key that passes).  invert=True keeps the rows that do not pass.

    Returns Compacted(keys, values, index, num): tensors of n rows like the inputs (None for an input that was not given,
    index only with return_index=True: the input position of every output row, index_dtype torch.int64 or torch.int32)
    and num, a 0-d int64 device tensor.  Only the first num rows are defined; partition=True writes the other rows
    behind them, in input order too (a stable two-way partition), so that all min(n, num_in) rows are.

    keys: a contiguous 1-D GPU tensor of a dtype radix_sort knows, or (n, 16) uint8 128-bit keys (key_kind=); or None
       with a mask (then values and / or the index are the outputs).
    mask: a contiguous bool or uint8 tensor of n elements; any non-zero byte passes.
    lo, hi: one-element tensors of the keys' dtype on the device, such as radix_quantile(keys, [q]) or a slice
       Group.keys[i:i + 1], read on the device; or Python numbers.
    values: a contiguous tensor with one row per key; a row (trailing dimensions included) is one value of up to 32768
       bytes, moved bitwise.  Widths of 1, 2, 4, 8, 16 bytes move in the write kernel, others behind positions.
    num: a one-element int64 device tensor such as radix_group(...).num: only the first min(n, num) rows count.
    out: a Compacted of preallocated tensors (keys, values, index of n rows, num of one int64 element; None for an output
       that is not wanted): nothing is allocated, and after Context.reserve_compact the call can be captured.  No output
       may overlap an input.
    Enqueued on the current stream, not synchronised; the host reads nothing."""
    import torch
    if keys is None:
        if mask is None:
            raise ValueError("keys=None needs a mask")
        if key_kind is not None:
            raise ValueError("key_kind= is for (n, 16) uint8 keys")
        kb, kind = 0, KEY_UNSIGNED
    else:
        kb, kind, n = _pairs_keys(keys, key_kind)
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError("mask must be a torch tensor of dtype bool or uint8")
        if mask.dim() != 1 or not mask.is_contiguous():
            raise ValueError("mask must be a contiguous 1-D tensor with one element per row")
        if keys is None:
            n = mask.shape[0]
        elif mask.shape[0] != n:
            raise ValueError(f"mask must have one element per key ({n}), not {mask.shape[0]}")
    like = keys if keys is not None else mask
    lo = _compact_bound(lo, keys, kb, "lo")
    hi = _compact_bound(hi, keys, kb, "hi")
    vb = _value_bytes(values, (n,), "keys")
    for t, what in ((mask, "mask"), (values, "values")):
        if t is not None and t.device != like.device:
            raise ValueError(f"keys and {what} must live on the same device")
    _set_num(num, like, "num")
    if n >= 1 << 32:
        raise ValueError("radix_compact takes fewer than 2^32 rows")
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise TypeError("out must be a Compacted(keys, values, index, num)")
        out_keys, out_values, out_index, out_num = out
        if out_keys is not None:
            if keys is None:
                raise ValueError("out.keys needs keys")
            _merge_out(out_keys, keys, n, "keys")
        if out_values is not None:
            if values is None:
                raise ValueError("out.values needs values")
            _merge_out(out_values, values, n, "values")
        if out_index is not None:
            _index_out(out_index, (n,), "the rows")
            if out_index.device != like.device:
                raise ValueError("the keys and out (index) must live on the same device")
            if index_dtype is not None and index_dtype != out_index.dtype:
                raise TypeError(f"index_dtype ({index_dtype}) is not the dtype of out.index ({out_index.dtype})")
        elif return_index:
            raise ValueError("return_index=True with out= needs out.index")
        if not isinstance(out_num, torch.Tensor) or out_num.dtype != torch.int64 or out_num.numel() != 1:
            raise TypeError("out.num must be a one-element int64 tensor")
        if out_num.device != like.device:
            raise ValueError("the keys and out (num) must live on the same device")
    else:
        index_dtype = _index_dtype(index_dtype)
    if not like.is_cuda:
        raise ValueError("keys and mask must live on a GPU")
    if out is None:
        dev = like.device
        out_keys = torch.empty_like(keys) if keys is not None else None
        out_values = torch.empty_like(values) if values is not None else None
        out_index = torch.empty(n, dtype=index_dtype, device=dev) if return_index else None
        out_num = torch.empty((), dtype=torch.int64, device=dev)
    result = Compacted(out_keys, out_values, out_index, out_num)
    if n == 0:  # (empty tensors have no address to hand to the C call)
        out_num.zero_()
        return result
    flags = (_lib.COMPACT_INVERT if invert else 0) | (_lib.COMPACT_PARTITION if partition else 0)
    with _on_device(like, ctx) as (c, stream):
        c.compact_device(keys.data_ptr() if keys is not None else 0, n, kb, kind, mask.data_ptr() if mask is not None else 0,
                         lo.data_ptr() if lo is not None else 0, hi.data_ptr() if hi is not None else 0,
                         values.data_ptr() if out_values is not None else 0, vb if out_values is not None else 0,
                         out_keys.data_ptr() if out_keys is not None else 0, out_values.data_ptr() if out_values is not None else 0,
                         out_index.data_ptr() if out_index is not None else 0, out_index.element_size() if out_index is not None else 8,
                         out_num.data_ptr(), descending, num.data_ptr() if num is not None else 0, flags, stream)
    return result


def radix_nonzero(mask, num=None, index_dtype=None, out=None, ctx: Optional[Context] = None):
    """The positions where a 1-D mask is set, in ascending order, and their number on the device (rsx_compact_device with
    the index as its only output): returns (index, num); index[:num] equals `torch.nonzero(mask).flatten()`, the rest of
    its n entries is not written; num is a 0-d int64 device tensor.  No host read, so it can be captured.

    mask: a contiguous 1-D bool or uint8 GPU tensor; any non-zero byte counts.
    num: a one-element int64 device tensor: only the first min(n, num) elements are looked at.
    index_dtype: torch.int64 (default) or torch.int32.  out: a pair (index, num) of preallocated tensors."""
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise TypeError("out must be a pair (index, num)")
        if out[0] is None:
            raise TypeError("out must be a pair (index, num) of tensors")
        out = Compacted(None, None, out[0], out[1])
    if mask is None:
        raise TypeError("mask must be a torch tensor of dtype bool or uint8")
    r = radix_compact(None, mask=mask, return_index=True, index_dtype=index_dtype, num=num, out=out, ctx=ctx)
    return r.index, r.num


def merge_caps(key_bytes: int, value_bytes: int = 0):
    """rsx_merge_caps -> tile: the output positions one workgroup of the merge kernel takes for these widths.  Needs no
    device."""
    L = _lib.load()
    tile = ctypes.c_uint32()
    _check_rc(L, L.rsx_merge_caps(key_bytes, value_bytes, ctypes.byref(tile)))
    return int(tile.value)


def _merge_keys(a, b, key_kind):
    """(key_bytes, key_kind, na, nb) of the two key columns of radix_merge / radix_merge_pairs."""
    import torch
    kb, kind, na = _pairs_keys(a, key_kind)
    if not isinstance(b, torch.Tensor):
        raise TypeError("keys must be a torch tensor on a GPU")
    if b.dtype != a.dtype:
        raise TypeError(f"both key tensors must have one dtype, not {a.dtype} and {b.dtype}")
    if b.device != a.device:
        raise ValueError("both key tensors must live on the same device")
    kb2, _kind, nb = _pairs_keys(b, key_kind)
    if kb2 != kb:
        raise ValueError("both key tensors must be 1-D, or both (n, 16) uint8 tensors of 128-bit keys")
    return kb, kind, na, nb


def _merge_out(out, like, n: int, what: str):
    """An output tensor of radix_merge / radix_merge_pairs: n rows shaped and typed like `like` (the first input)."""
    import torch
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"out ({what}) must be a torch tensor")
    if out.dtype != like.dtype:
        raise TypeError(f"out ({what}) must have dtype {like.dtype}, not {out.dtype}")
    shape = (n,) + tuple(like.shape[1:])
    if tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"out ({what}) must be a contiguous tensor of shape {shape}")
    if out.device != like.device:
        raise ValueError(f"the keys and out ({what}) must live on the same device")


def _merge_out_index(out, return_index: bool, index_dtype, like, rows: int, n: int, what: str):
    """out= and index_dtype= of radix_merge / radix_set_op -> (keys, index) of `rows` rows: the tensors of `out` checked,
    a missing one made; index is None without return_index.  n: the keys of both inputs, which an index has to count."""
    import torch
    out_keys, out_index = out, None
    if return_index and out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise TypeError("out must be a pair (keys, index) with return_index=True")
        out_keys, out_index = out
    if out_keys is not None:
        _merge_out(out_keys, like, rows, "keys")
    if out_index is not None:
        _index_out(out_index, (rows,), what)
        if out_index.device != like.device:
            raise ValueError("the keys and out (index) must live on the same device")
        index_dtype = out_index.dtype
    index_dtype = _index_dtype(index_dtype)
    if return_index and index_dtype == torch.int32 and n > 1 << 32:
        raise ValueError("more than 2^32 keys need int64 indices")
    if out_keys is None:
        out_keys = torch.empty((rows,) + tuple(like.shape[1:]), dtype=like.dtype, device=like.device)
    if return_index and out_index is None:
        out_index = torch.empty(rows, dtype=index_dtype, device=like.device)
    return out_keys, out_index


def _merge_out_values(out, keys, values, rows: int):
    """out= of radix_merge_pairs / radix_set_op_pairs -> (keys, values) of `rows` rows: the pair checked, or made."""
    import torch
    if out is None:
        return (torch.empty((rows,) + tuple(keys.shape[1:]), dtype=keys.dtype, device=keys.device),
                torch.empty((rows,) + tuple(values.shape[1:]), dtype=values.dtype, device=keys.device))
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise TypeError("out must be a pair (keys, values)")
    _merge_out(out[0], keys, rows, "keys")
    _merge_out(out[1], values, rows, "values")
    return tuple(out)


def _merge_values(keys, a_values, na: int, b_values, nb: int) -> int:
    """Bytes of one value of radix_merge_pairs / radix_set_op_pairs: the two value tensors checked against their keys and
    against each other.  b_values None (where the caller lets it be absent): a_values alone."""
    va = _value_bytes(a_values, (na,), "a_keys")
    if b_values is not None:
        vb = _value_bytes(b_values, (nb,), "b_keys")
        if a_values.dtype != b_values.dtype:
            raise TypeError(f"both value tensors must have one dtype, not {a_values.dtype} and {b_values.dtype}")
        if tuple(a_values.shape[1:]) != tuple(b_values.shape[1:]) or va != vb:
            raise ValueError(f"both value tensors must have the same trailing shape, not {tuple(a_values.shape)} and {tuple(b_values.shape)}")
    for v, what in ((a_values, "a_values"), (b_values, "b_values")):
        if v is not None and v.device != keys.device:
            raise ValueError(f"keys and {what} must live on the same device")
    return va


def radix_merge(a, b, descending: bool = False, return_index: bool = False, index_dtype=None, out=None,
                ctx: Optional[Context] = None, key_kind: Optional[int] = None):
    """The stable merge of two sorted key tensors (rsx_merge_device): what `torch.sort(torch.cat((a, b)), stable=True,
    descending=descending)` gives for inputs that are each sorted already, in one read and one write of every key.  Equal
    keys of `a` come before equal keys of `b`.  Returns the merged 1-D keys, or with return_index=True the pair (keys,
    index): index[t] is the position of output t in the concatenation, below len(a) a position in `a`, otherwise
    index[t] - len(a) a position in `b` -- radix_argsort(torch.cat((a, b))).

    a, b: contiguous 1-D GPU tensors of one dtype radix_sort knows, or (n, 16) uint8 128-bit keys (key_kind=), each in the
       order radix_sort / radix_sort_pairs(descending=descending) / radix_group leave: the total order on bit patterns
       (-NaN below -inf, -0.0 below +0.0, +NaN above +inf), not torch's.  Neither is modified.
    out: the keys tensor to fill (with return_index: a pair (keys, index), index int32 or int64), contiguous, on the same
       device, len(a) + len(b) long; it must not overlap an input.  index_dtype: torch.int64 (default) or torch.int32.

    If an input is not sorted the result is unspecified but nothing outside the outputs is written.  Enqueued on the
    current stream, not synchronised."""
    kb, kind, na, nb = _merge_keys(a, b, key_kind)
    n = na + nb
    out_keys, out_index = _merge_out_index(out, return_index, index_dtype, a, n, n, "the merged keys")
    _pairs_device(a, None, "")
    if n > 0:
        with _on_device(a, ctx) as (c, stream):
            c.merge_device(a.data_ptr() if na else 0, 0, na, b.data_ptr() if nb else 0, 0, nb, kb, kind, 0, out_keys.data_ptr(), 0,
                           out_index.data_ptr() if return_index else 0, out_index.element_size() if return_index else 8, descending, stream)
    return (out_keys, out_index) if return_index else out_keys


def radix_merge_pairs(a_keys, a_values, b_keys, b_values, descending: bool = False, out=None, ctx: Optional[Context] = None,
                      key_kind: Optional[int] = None):
    """The stable merge of two sorted key tensors with their values (rsx_merge_device): returns (keys, values), what
    radix_sort_pairs leaves of torch.cat((a_keys, b_keys)) and torch.cat((a_values, b_values)) when each input is sorted
    already.  Equal keys of `a` come before equal keys of `b`.

    a_keys, b_keys: as in radix_merge.  a_values, b_values: contiguous GPU tensors of one dtype on the same device with one
       row per key and the same trailing dimensions; a row (trailing dimensions included) is one value of up to 32768
       bytes, moved bitwise.  Values of 1, 2, 4, 8 and 16 bytes move in the merge kernel; any other width goes through
       8-byte source positions in the context's workspace and a row gather.
    out: a pair (keys, values) to fill, shaped like the concatenations; it must not overlap an input.

    Enqueued on the current stream, not synchronised."""
    kb, kind, na, nb = _merge_keys(a_keys, b_keys, key_kind)
    n = na + nb
    if a_values is None or b_values is None:
        raise TypeError("a_values and b_values must be torch tensors (keys alone: radix_merge)")
    va = _merge_values(a_keys, a_values, na, b_values, nb)
    out_keys, out_values = _merge_out_values(out, a_keys, a_values, n)
    _pairs_device(a_keys, None, "")
    if n > 0:
        with _on_device(a_keys, ctx) as (c, stream):
            c.merge_device(a_keys.data_ptr() if na else 0, a_values.data_ptr() if na else 0, na, b_keys.data_ptr() if nb else 0,
                           b_values.data_ptr() if nb else 0, nb, kb, kind, va, out_keys.data_ptr(), out_values.data_ptr(), 0, 8, descending, stream)
    return out_keys, out_values


def setop_caps(key_bytes: int):
    """rsx_setop_caps -> tile: the positions of the merge one workgroup of the set-operation kernel takes for this key
    width.  Needs no device."""
    L = _lib.load()
    tile = ctypes.c_uint32()
    _check_rc(L, L.rsx_setop_caps(key_bytes, ctypes.byref(tile)))
    return int(tile.value)


SetResult = namedtuple("SetResult", ["keys", "index", "num"])
SetPairsResult = namedtuple("SetPairsResult", ["keys", "values", "num"])
_SET_OPS = {"union": _lib.SETOP_UNION, "intersection": _lib.SETOP_INTERSECTION, "difference": _lib.SETOP_DIFFERENCE,
            "symmetric_difference": _lib.SETOP_SYMMETRIC_DIFFERENCE}
_SET_FUSED = (1, 2, 4, 8, 16)


def _set_op(op):
    if op not in _SET_OPS:
        raise ValueError(f'op must be "union", "intersection", "difference" or "symmetric_difference", not {op!r}')
    return _SET_OPS[op]


def _set_cap(op: int, na: int, nb: int) -> int:
    """Rows of every output of a set operation."""
    return min(na, nb) if op == _lib.SETOP_INTERSECTION else na if op == _lib.SETOP_DIFFERENCE else na + nb


def _set_num(num, keys, what: str):
    """a_num= / b_num= of radix_set_op: None, or a one-element int64 tensor on the keys' device."""
    import torch
    if num is None:
        return
    if not isinstance(num, torch.Tensor) or num.dtype != torch.int64 or num.numel() != 1:
        raise TypeError(f"{what} must be a one-element int64 tensor")
    if num.device != keys.device:
        raise ValueError(f"the keys and {what} must live on the same device")


def radix_set_op(a, b, op: str, descending: bool = False, return_index: bool = False, index_dtype=None, out=None,
                 a_num=None, b_num=None, ctx: Optional[Context] = None, key_kind: Optional[int] = None):
    """A set operation on two sorted key tensors as multisets (rsx_setop_device), the rules of std::set_union and its
    siblings: a key that occurs m times in `a` and n times in `b` occurs max(m, n) times in the "union", min(m, n) times
    in the "intersection", max(m - n, 0) times in the "difference" and |m - n| times in the "symmetric_difference".  The
    kept keys come in sorted order, equal keys of `a` in front of equal keys of `b`.  Returns SetResult(keys, index, num)
    without synchronising:

    keys   a tensor like `a` of the capacity len(a) + len(b) (union, symmetric difference), len(a) (difference) or
           min(len(a), len(b)) (intersection); its first num entries are the result, the rest is not written.
    index  None, or with return_index=True the position of every kept key in the concatenation: below len(a) a position in
           `a`, otherwise index - len(a) a position in `b`; index_dtype torch.int64 (default) or torch.int32.
    num    a 0-d int64 device tensor: the number of kept keys.

    a, b: as in radix_merge.  a_num, b_num: one-element int64 device tensors such as radix_group(...).num; only the first
    min(len(a), a_num) keys of `a` count (`b` likewise), read on the device: two radix_group results combine without a
    host read.  out: the keys tensor to fill (with return_index: a pair (keys, index)), of the capacity above; it must not
    overlap an input.  If an input is not sorted the result is unspecified but nothing outside the outputs is written.
    Enqueued on the current stream."""
    import torch
    kb, kind, na, nb = _merge_keys(a, b, key_kind)
    code = _set_op(op)
    cap = _set_cap(code, na, nb)
    out_keys, out_index = _merge_out_index(out, return_index, index_dtype, a, cap, na + nb, "the kept keys")
    _set_num(a_num, a, "a_num")
    _set_num(b_num, a, "b_num")
    _pairs_device(a, None, "")
    num = torch.empty((), dtype=torch.int64, device=a.device)
    if na + nb == 0 or cap == 0:  # (empty outputs have no address to hand to the C call: nothing can be kept)
        num.zero_()
        return SetResult(out_keys, out_index, num)
    with _on_device(a, ctx) as (c, stream):
        c.setop_device(code, a.data_ptr() if na else 0, 0, na, a_num.data_ptr() if a_num is not None else 0, b.data_ptr() if nb else 0, 0, nb,
                       b_num.data_ptr() if b_num is not None else 0, kb, kind, 0, out_keys.data_ptr(), 0,
                       out_index.data_ptr() if return_index else 0, out_index.element_size() if return_index else 8, num.data_ptr(),
                       descending, stream)
    return SetResult(out_keys, out_index, num)


def radix_set_op_pairs(a_keys, a_values, b_keys, b_values, op: str, descending: bool = False, out=None, a_num=None, b_num=None,
                       ctx: Optional[Context] = None, key_kind: Optional[int] = None):
    """radix_set_op with values (rsx_setop_device): returns SetPairsResult(keys, values, num); values[t] is the value of the
    very element keys[t] came from (for a key in both inputs: `a`'s, except the surplus occurrences of `b` in a union).

    a_values, b_values: contiguous GPU tensors of one dtype with one row per key and the same trailing dimensions; a row
    is one value of 1, 2, 4, 8 or 16 bytes, moved bitwise.  b_values may be None for "intersection" and "difference",
    which never emit from `b`.  Other widths raise ValueError: use radix_set_op(..., return_index=True) and gather.
    out: a pair (keys, values) of the capacity of radix_set_op.  Enqueued on the current stream, not synchronised."""
    import torch
    kb, kind, na, nb = _merge_keys(a_keys, b_keys, key_kind)
    code = _set_op(op)
    cap = _set_cap(code, na, nb)
    emits_b = code in (_lib.SETOP_UNION, _lib.SETOP_SYMMETRIC_DIFFERENCE)
    if a_values is None:
        raise TypeError("a_values must be a torch tensor (keys alone: radix_set_op)")
    if b_values is None and emits_b:
        raise TypeError(f'b_values must be a torch tensor for "{op}", which can emit from b')
    va = _merge_values(a_keys, a_values, na, b_values, nb)
    if va not in _SET_FUSED:
        raise ValueError(f"one value must have 1, 2, 4, 8 or 16 bytes, not {va}: use radix_set_op(..., return_index=True) and gather")
    out_keys, out_values = _merge_out_values(out, a_keys, a_values, cap)
    _set_num(a_num, a_keys, "a_num")
    _set_num(b_num, a_keys, "b_num")
    _pairs_device(a_keys, None, "")
    num = torch.empty((), dtype=torch.int64, device=a_keys.device)
    if na + nb == 0 or cap == 0:
        num.zero_()
        return SetPairsResult(out_keys, out_values, num)
    with _on_device(a_keys, ctx) as (c, stream):
        c.setop_device(code, a_keys.data_ptr() if na else 0, a_values.data_ptr() if na else 0, na, a_num.data_ptr() if a_num is not None else 0,
                       b_keys.data_ptr() if nb else 0, b_values.data_ptr() if nb and b_values is not None and emits_b else 0, nb,
                       b_num.data_ptr() if b_num is not None else 0, kb, kind, va, out_keys.data_ptr(), out_values.data_ptr(), 0, 8,
                       num.data_ptr(), descending, stream)
    return SetPairsResult(out_keys, out_values, num)


def join_caps(key_bytes: int):
    """rsx_join_caps -> (tile, window, rows): the keys of `a` one count workgroup of the join takes, the keys of `b` it
    stages in LDS at most, and the output rows one write workgroup stores.  Needs no device."""
    L = _lib.load()
    tile, window, rows = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _check_rc(L, L.rsx_join_caps(key_bytes, ctypes.byref(tile), ctypes.byref(window), ctypes.byref(rows)))
    return int(tile.value), int(window.value), int(rows.value)


JoinResult = namedtuple("JoinResult", ["left", "right", "num"])
_JOINS = {"inner": _lib.JOIN_INNER, "left": _lib.JOIN_LEFT, "semi": _lib.JOIN_SEMI, "anti": _lib.JOIN_ANTI}


def _join_bound(how: int, na: int, nb: int) -> int:
    """The most rows a join can have."""
    return na * nb if how == _lib.JOIN_INNER else na * max(nb, 1) if how == _lib.JOIN_LEFT else na


def _join_index(index, keys, n: int, index_dtype, what: str):
    """a_index= / b_index= of radix_join: None, or one word of the index dtype per key, on the keys' device."""
    import torch
    if index is None:
        return
    if not isinstance(index, torch.Tensor) or index.dtype != index_dtype:
        raise TypeError(f"{what} must be a torch tensor of the index dtype {index_dtype}")
    if tuple(index.shape) != (n,) or not index.is_contiguous():
        raise ValueError(f"{what} must be a contiguous 1-D tensor with one entry per key ({n})")
    if index.device != keys.device:
        raise ValueError(f"the keys and {what} must live on the same device")


def radix_join(a, b, how: str = "inner", assume_sorted: bool = False, capacity: Optional[int] = None, descending: bool = False,
               index_dtype=None, a_num=None, b_num=None, a_index=None, b_index=None, out=None, ctx: Optional[Context] = None,
               key_kind: Optional[int] = None):
    """The join of two key tensors (rsx_join_device): which rows of `a` match which rows of `b`.  Returns
    JoinResult(left, right, num): for t < num, (left[t], right[t]) is one pair of positions with a[left[t]] equal to
    b[right[t]] in every bit.  A key that occurs m times in `a` and n times in `b` gives m * n pairs.

    how    "inner": the matching pairs.  "left": those, and one row (i, -1) for every a[i] without a match.  "semi": the
           positions of the a[i] with a match, once each.  "anti": those without.  For "semi" and "anti" `right` is None.
    num    a 0-d int64 device tensor: the FULL number of rows, whatever the capacity is.
    index_dtype  torch.int64 (default) or torch.int32, the dtype of left and right (taken from `out` when that is given).

    a, b: contiguous 1-D GPU tensors of one dtype radix_sort knows, or (n, 16) uint8 128-bit keys (key_kind=), fewer than
    2^32 keys each.  Neither is modified.  Keys match by bit pattern: -0.0 and +0.0 do not, a NaN matches the same NaN.

    assume_sorted=False (the default): both sides are sorted with their positions by radix_sort_pairs on copies, and the
    positions go into the join, so that left and right index the tensors as given: the result is exactly (pa[L], pb[R]) with
    pa = radix_argsort(a), pb = radix_argsort(b) and (L, R) the join of a[pa] and b[pb].  Rows are ordered by key, then by
    position in a, then by position in b.  a_num, b_num, a_index and b_index raise ValueError here.
    assume_sorted=True: a and b are each in the order radix_sort / radix_sort_pairs(descending=descending) / radix_group
    leave, and are used as they are.  a_num, b_num: one-element int64 device tensors such as radix_group(...).num; only
    the first min(len(a), a_num) keys of `a` count (`b` likewise), read on the device.  a_index, b_index: 1-D tensors of the
    index dtype, one entry per key, whose entries are returned in place of the positions.  If an input is not sorted the
    result is unspecified but nothing outside the outputs is written.

    capacity=int, or out=(left, right) (for "semi" / "anti" out=left or (left, None)) of one length and dtype: ONE call,
    never synchronised; rows beyond the capacity are dropped, and num tells.
    capacity=None without out: the count-only call, ONE host read of num (this synchronises the stream), tensors of exactly
    num rows, then the full call -- the keys are searched twice on this route.

    Enqueued on the current stream."""
    import torch
    if how not in _JOINS:
        raise ValueError(f'how must be "inner", "left", "semi" or "anti", not {how!r}')
    code = _JOINS[how]
    pairs = code in (_lib.JOIN_INNER, _lib.JOIN_LEFT)
    kb, kind, na, nb = _merge_keys(a, b, key_kind)
    if not assume_sorted and any(x is not None for x in (a_num, b_num, a_index, b_index)):
        raise ValueError("a_num, b_num, a_index and b_index go with assume_sorted=True")
    out_left = out_right = None
    if out is not None:
        if isinstance(out, torch.Tensor):
            out = (out, None)
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise TypeError("out must be a pair (left, right)")
        out_left, out_right = out
        if not pairs and out_right is not None:
            raise ValueError(f'a "{how}" join has no right-hand output: out must be left or (left, None)')
        if pairs and out_right is None:
            raise TypeError(f'out must be a pair (left, right) of tensors for a "{how}" join')
        rows = out_left.shape[0] if isinstance(out_left, torch.Tensor) and out_left.dim() == 1 else 0
        for o in (out_left, out_right) if pairs else (out_left,):
            _index_out(o, (rows,), "each other")
            if o.device != a.device:
                raise ValueError("the keys and out must live on the same device")
        if pairs and out_left.dtype != out_right.dtype:
            raise TypeError("both tensors of out must have one dtype")
        if capacity is not None and capacity != rows:
            raise ValueError(f"capacity ({capacity}) and the length of out ({rows}) disagree")
        capacity = rows
        index_dtype = out_left.dtype
    index_dtype = _index_dtype(index_dtype)
    if capacity is not None and (not isinstance(capacity, int) or capacity < 0):
        raise ValueError("capacity must be None or a non-negative int")
    if na >= 1 << 32 or nb >= 1 << 32:
        raise ValueError("radix_join takes fewer than 2^32 keys on each side (a position in b, int32 or int64, is kept in 32 bits)")
    _join_index(a_index, a, na, index_dtype, "a_index")
    _join_index(b_index, a, nb, index_dtype, "b_index")
    if not pairs and b_index is not None:
        raise ValueError(f'a "{how}" join has no right-hand output: b_index must be None')
    _set_num(a_num, a, "a_num")
    _set_num(b_num, a, "b_num")
    _pairs_device(a, None, "")
    dev = a.device
    num = torch.empty((), dtype=torch.int64, device=dev)

    def result(rows):
        left = out_left if out_left is not None else torch.empty(rows, dtype=index_dtype, device=dev)
        right = (out_right if out_right is not None else torch.empty(rows, dtype=index_dtype, device=dev)) if pairs else None
        return left, right

    if na == 0:  # no row (and no address to hand to the C call)
        num.zero_()
        return JoinResult(*result(capacity or 0), num)
    if not assume_sorted:  # the keys of both sides sorted on copies, their positions with them
        def sorted_with_positions(keys, n):
            k = keys.clone()
            p = torch.arange(n, dtype=index_dtype, device=dev) if n <= 1 << 31 else torch.arange(n, dtype=torch.int64, device=dev).to(index_dtype)
            radix_sort_pairs(k, p, descending=descending, ctx=ctx, key_kind=key_kind)
            return k, p

        a, a_index = sorted_with_positions(a, na)
        b, b_index = sorted_with_positions(b, nb)
        if not pairs:
            b_index = None
    ib = 8 if index_dtype == torch.int64 else 4
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0  # noqa: E731

    def call(c, stream, left, right, rows):
        c.join_device(code, a.data_ptr(), na, ptr(a_num), ptr(a_index), ptr(b), nb, ptr(b_num), ptr(b_index), kb, kind, ptr(left), ptr(right),
                      ib, rows, num.data_ptr(), descending, stream)

    with _on_device(a, ctx) as (c, stream):
        counted = capacity is None
        if counted:  # the count alone, the one host read, then the exact allocation
            call(c, stream, None, None, 0)
            capacity = min(int(num), _join_bound(code, na, nb))
        left, right = result(capacity)
        if capacity > 0:
            call(c, stream, left, right, capacity)
        elif not counted:  # (empty outputs have no address: the count alone)
            call(c, stream, None, None, 0)
    return JoinResult(left, right, num)


def _segments_common(keys, offsets, max_seg_len):
    import torch
    if not isinstance(keys, torch.Tensor):
        raise TypeError("keys must be a torch tensor on a GPU")
    _check_offsets(offsets)
    kb, kind, n = _pairs_keys(keys, None)
    if max_seg_len < 0:
        raise ValueError("max_seg_len must not be negative")
    return kb, kind, n


def radix_sort_segments_pairs(keys, values, offsets, descending: bool = False, max_seg_len: int = 0,
                              ctx: Optional[Context] = None):
    """Sorts every segment [offsets[i], offsets[i+1]) of `keys` on its own, in place, and moves `values` with it
    (rsx_sort_segments_pairs_device): what radix_sort_pairs would leave if called on each segment.  Returns None.

    keys: as in radix_sort_pairs (1-D, or (n, 16) uint8 for unsigned 128-bit keys).  values: one row per key, or None.
    offsets, max_seg_len: as in radix_sort_segments; keys and values outside [offsets[0], offsets[-1]) are not touched,
    a bad segment is left as it is and the context's next check() raises."""
    kb, kind, n = _segments_common(keys, offsets, max_seg_len)
    vb = _value_bytes(values, (n,), "one row per key,")
    _pairs_device(keys, values, "values")
    if offsets.device != keys.device:
        raise ValueError("offsets must live on the device of keys")
    nseg = offsets.numel() - 1
    if nseg <= 0 or n == 0:
        return None
    with _on_device(keys, ctx) as (c, stream):
        c.sort_segments_pairs_device(keys.data_ptr(), values.data_ptr() if values is not None else 0, n, kb, kind, vb,
                                     offsets.data_ptr(), nseg, descending, max_seg_len, stream)
    return None


def radix_argsort_segments(keys, offsets, descending: bool = False, out=None, max_seg_len: int = 0,
                           ctx: Optional[Context] = None):
    """The stable sorting permutation of every segment of `keys`, as positions INSIDE the segment (0 .. len-1;
    rsx_argsort_segments_device).  Returns a new int64 tensor of len(keys), zero-filled so that the slots no segment
    covers are defined, or fills and returns `out` (contiguous 1-D int32 or int64, len(keys)), whose slots outside every
    segment, and those of bad segments, stay as they were.  `keys` is not modified."""
    import torch
    kb, kind, n = _segments_common(keys, offsets, max_seg_len)
    _index_out(out, (n,), "one index per key,")
    _pairs_device(keys, out, "out")
    if offsets.device != keys.device:
        raise ValueError("offsets must live on the device of keys")
    if out is None:
        out = torch.zeros(n, dtype=torch.int64, device=keys.device)
    nseg = offsets.numel() - 1
    if nseg <= 0 or n == 0:
        return out
    with _on_device(keys, ctx) as (c, stream):
        c.argsort_segments_device(keys.data_ptr(), out.data_ptr(), n, kb, kind, out.element_size(), offsets.data_ptr(), nseg,
                                  descending, max_seg_len, stream)
    return out


def radix_sort_sharded(slices: Sequence, digits: RadixDigits, ctxs: Optional[Sequence[Context]] = None, tmps=None,
                       schedule: int = _lib.SHARD_EXCHANGE_FIRST):
    """rsx_sort_sharded: sorts the concatenation of `slices` (contiguous GPU tensors, one per
    context, possibly on different devices) as ONE array, stably and in place -- every slice
    keeps its length.  The single-process multi-GPU form of `<[T]>::radix_sort` with "chunk per
    thread" (mod.rs:66-70) read as "slice per GPU".  Blocking.  `schedule`: SHARD_EXCHANGE_FIRST (one
    partition pass by the top digit, exchange, one local sort) or SHARD_SORT_FIRST (sort, exchange, sort)."""
    import torch
    G = len(slices)
    if G == 0:
        return None
    if ctxs is None:
        ctxs = [Context(t.device.index if t.device.index is not None else torch.cuda.current_device()) for t in slices]
    if len(ctxs) != G:
        raise ValueError("one context per slice")
    if tmps is None:
        tmps = [torch.empty_like(t) for t in slices]
    ns = []
    for t, u in zip(slices, tmps):
        if not (t.is_cuda and t.is_contiguous() and u.is_cuda and u.is_contiguous() and u.device == t.device):
            raise ValueError("slices and tmps must be contiguous GPU tensors, pairwise on the same device")
        nbytes = t.numel() * t.element_size()
        if nbytes % digits.elem_bytes or u.numel() * u.element_size() < nbytes:
            raise ValueError("slice size is not a multiple of elem_bytes, or tmp too small")
        ns.append(nbytes // digits.elem_bytes)
    for t in slices:  # the library works on private streams: what torch enqueued must be done
        torch.cuda.synchronize(t.device)
    L = ctxs[0]._L
    hs = (ctypes.c_void_p * G)(*[c._h for c in ctxs])
    ps = (ctypes.c_void_p * G)(*[t.data_ptr() for t in slices])
    ts = (ctypes.c_void_p * G)(*[t.data_ptr() for t in tmps])
    nn = (ctypes.c_size_t * G)(*ns)
    lay = digits.layout()
    ctxs[0]._check(L.rsx_sort_sharded_ex(hs, G, ps, ts, nn, ctypes.byref(lay), schedule))
    return None
