"""MI355X-native LSD radix sort: drop-in for the hot path of jgrodzki/radix_sort.

`radix_sort(x)` mirrors `<[T]>::radix_sort(&mut self)` (reference
src/radix_sort/mod.rs:18-20,61-176); `RadixDigits` mirrors the key trait
(src/radix_sort/radix_digits.rs:1-5).  All compute runs in the HIP library
librsx.so behind the C-ABI of include/rsx.h; there is no CPU fallback.
"""
from .api import (PRIMITIVES, Context, RadixDigits, default_context, digits_of, radix_argsort, radix_argsort_rows,
                  radix_argsort_segments, radix_sort, radix_sort_pairs, radix_sort_rows, radix_sort_rows_pairs, radix_sort_segments,
                  radix_sort_segments_pairs, radix_sort_sharded, radix_topk, segment_caps, segment_pairs_caps, topk_caps, tuple_of,
                  Group, radix_group, radix_unique, unique_caps, Reduced, radix_reduce_by_key, reduce_caps,
                  radix_scan_by_key, scan_by_key_caps,
                  radix_lexsort, radix_sort_columns, lex_plan, radix_searchsorted, search_caps, radix_merge, radix_merge_pairs, merge_caps,
                  SetResult, SetPairsResult, radix_set_op, radix_set_op_pairs, setop_caps, JoinResult, radix_join, join_caps,
                  radix_select, radix_kthvalue, radix_median, radix_quantile, select_caps,
                  radix_histogram, radix_bincount, bin_caps,
                  Compacted, radix_compact, radix_nonzero, compact_caps,
                  Partitioned, radix_partition, partition_caps,
                  radix_bin_reduce, bin_reduce_caps)
from ._lib import (COMPACT_INVERT, COMPACT_PARTITION, BIN_UPPER, BIN_LOWER, BIN_INDEX, BIN_ACCUMULATE, SEARCH_PRESORT,SCAN_EXCLUSIVE, SCAN_RUNS,JOIN_INNER, JOIN_LEFT, JOIN_SEMI, JOIN_ANTI, GEN_CONSTANT, GEN_GEOMETRIC, GEN_PAYLOAD_ZERO, GEN_REVERSED, GEN_SORTED, GEN_STEP, GEN_UNIFORM,
                   GEN_ZIPF, INFO_L2_LOCAL, INFO_LAST_DIRECT, INFO_LAST_LEX, INFO_LAST_PAIRS, INFO_LAST_PASSES, INFO_RANK_ATOMIC, KEY_FLOAT, KEY_SIGNED, KEY_UNSIGNED, OPT_BYTE_COUNTING,
                   OPT_HOT_LANES, OPT_MAX_REGIONS, OPT_MID_SORT, OPT_WIDE_SORT, OPT_BUCKET_SKIP, OPT_BUCKET_GROUP, OPT_BUCKET_DIRECT, OPT_HOST_CHUNK, OPT_RANK_CHECK, OPT_RANKING, OPT_SMALL_SORT, OPT_STATUS_SCOPE, OPT_TILE_SCHEDULE, OPT_VERBOSE,
                   OPT_XCD_MAJOR, SHARD_EXCHANGE_FIRST, SHARD_SORT_FIRST, Layout, RsxError)

__all__ = ["radix_sort", "radix_sort_pairs", "radix_argsort", "radix_sort_segments", "radix_sort_rows", "segment_caps", "radix_sort_rows_pairs", "radix_argsort_rows",
           "radix_sort_segments_pairs", "radix_argsort_segments", "segment_pairs_caps", "radix_topk", "topk_caps", "radix_group", "radix_unique", "unique_caps", "Group", "radix_reduce_by_key", "reduce_caps", "Reduced", "radix_scan_by_key", "scan_by_key_caps", "SCAN_EXCLUSIVE", "SCAN_RUNS", "radix_lexsort", "radix_sort_columns", "lex_plan", "radix_searchsorted", "search_caps", "SEARCH_PRESORT", "radix_merge", "radix_merge_pairs", "merge_caps", "radix_set_op", "radix_set_op_pairs", "setop_caps", "SetResult", "SetPairsResult", "radix_join", "join_caps", "JoinResult", "JOIN_INNER", "JOIN_LEFT", "JOIN_SEMI", "JOIN_ANTI", "radix_select", "radix_kthvalue", "radix_median", "radix_quantile", "select_caps", "radix_histogram", "radix_bincount", "bin_caps", "BIN_UPPER", "BIN_LOWER", "BIN_INDEX", "BIN_ACCUMULATE", "radix_compact", "radix_nonzero", "compact_caps", "Compacted", "COMPACT_INVERT", "COMPACT_PARTITION", "radix_partition", "partition_caps", "Partitioned", "radix_bin_reduce", "bin_reduce_caps", "radix_sort_sharded", "RadixDigits", "PRIMITIVES", "tuple_of", "digits_of", "Context", "default_context",
           "Layout", "RsxError", "KEY_UNSIGNED", "KEY_SIGNED", "KEY_FLOAT", "GEN_UNIFORM", "GEN_ZIPF", "GEN_STEP",
           "GEN_SORTED", "GEN_REVERSED", "GEN_CONSTANT", "GEN_GEOMETRIC", "GEN_PAYLOAD_ZERO", "OPT_TILE_SCHEDULE",
           "OPT_RANKING", "OPT_STATUS_SCOPE", "OPT_XCD_MAJOR", "OPT_BYTE_COUNTING", "OPT_MAX_REGIONS", "OPT_HOT_LANES",
           "OPT_VERBOSE", "OPT_RANK_CHECK", "OPT_SMALL_SORT", "OPT_MID_SORT", "OPT_WIDE_SORT", "OPT_BUCKET_SKIP", "OPT_BUCKET_GROUP", "OPT_BUCKET_DIRECT", "OPT_HOST_CHUNK", "INFO_RANK_ATOMIC", "INFO_L2_LOCAL", "INFO_LAST_PASSES", "INFO_LAST_PAIRS", "INFO_LAST_DIRECT", "INFO_LAST_LEX", "SHARD_EXCHANGE_FIRST", "SHARD_SORT_FIRST"]
