"""GPU: the wide-key hybrid in its default mode (RSX_OPT_WIDE_SORT 1 and 3) on CLUSTERED keys -- byte for byte against the
CPU oracle's stable sort.

In these modes the first sweep's count matrix is the marginal of rsx_count16top_kernel's per-workgroup 16-bit counters.
0x8000 elements of one bucket inside one count chunk (zero or sentinel padding, a pre-sorted block appended to random
keys) park a counter in a table that is per bin, and the marginal is then short by a multiple of 0x8000 although the bin
totals, the starts and the verdict are right.  The count kernel therefore reports a parked counter (WidePlan::parked) and
the verdict gives such a sort to the LSD passes: RSX_INFO_LAST_PASSES reports path 0 for every input that parks, and path 5
(the hybrid) for every input that does not -- a bucket of 0x7FFF in one chunk, sorted keys, uniform keys.

The inputs and what each relies on are in tests/hybrid_clustered_inputs.py (exact (chunk, bin) counts over a mirror of the
host's geometry, taken with the device's CU count and asserted on the CPU before the GPU is touched);
tests/test_hybrid_clustered_inputs.py shows without a GPU that the marginal is short in exactly the cases marked `parks`.
Groups: the threshold of one counter (0x7FFF ... 0x10001 in one chunk); where the run lies (element 0, the end, across a
chunk, across a region, halves in two regions), in modes 1 and 3; element types; three and nine hot buckets; locally
ordered inputs; tile schedule and ranking; key / value calls; a captured graph replayed on changing inputs; the sort after
a refusal.  Payload = index wherever the type has one, so a lost tie shows."""
import numpy as np
import pytest

import hybrid_clustered_inputs as hci
import util
from pairs_ref import pairs_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def rs():
    import radix_sort_amd as rs
    return rs


@pytest.fixture(scope="module")
def num_cu(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    try:
        return int(c.get_info(rs._lib.INFO_NUM_CU))
    finally:
        c.close()


_INPUTS = {}  # case name -> (input, expected): made once, conditions asserted, shared, never changed


def _input(orc, name, num_cu):
    if name not in _INPUTS:
        case = hci.CASES[name]
        raw, geom, runs = hci.build(case, num_cu)
        hci.conditions(case, raw, geom, runs)
        exp = orc.sort_parallel(raw, orc.Layout(*util.TYPES[case.t]), 8)
        raw.setflags(write=False)
        exp.setflags(write=False)
        _INPUTS[name] = (raw, exp)
    return _INPUTS[name]


def _path(rs, c):
    return (c.get_info(rs.INFO_LAST_PASSES) >> 24) & 15


def _run(rs, torch, orc, num_cu, name, mode=3, schedule=0, ranking=0):
    case = hci.CASES[name]
    raw, exp = _input(orc, name, num_cu)
    es = util.TYPES[case.t][0]
    c = rs.Context(torch.cuda.current_device())
    try:
        c.set_option(rs.OPT_WIDE_SORT, mode)
        c.set_option(rs.OPT_MAX_REGIONS, case.cap)
        c.set_option(rs.OPT_TILE_SCHEDULE, schedule)
        c.set_option(rs.OPT_RANKING, ranking)
        x = torch.from_numpy(raw.copy()).cuda()
        c.profile(True)
        rs.radix_sort(x, digits=rs.RadixDigits(*util.TYPES[case.t]), ctx=c)
        c.check()
        tried = c.profile_read()["scan"][1]
        c.profile(False)
        lp = c.get_info(rs.INFO_LAST_PASSES)
        got = x.cpu().numpy()
    finally:
        c.close()
    # path 0 is also what a sort reports that never tried the hybrid.  Above the middle sizes only a try launches kernels
    # of the profile's "scan" kind (the plan kernel, the totals and the verdict): tried and refused, not passed over
    assert tried >= 1, (name, mode, tried)
    assert (lp >> 24) & 15 == case.path, (name, mode, hex(lp))
    assert np.array_equal(got, exp), (name, mode, schedule, ranking, int(np.flatnonzero(got != exp)[0]) // es)


@pytest.mark.parametrize("count", [0x7FFF, 0x8000, 0xFFFF, 0x10000, 0x10001])
def test_threshold_of_one_counter(rs, torch, orc, num_cu, count):
    """One hot bucket, all of it inside one count chunk: 0x7FFF parks nothing and keeps the hybrid (path 5); from 0x8000 on
    the counter parks once or twice and the LSD passes run (path 0)."""
    _run(rs, torch, orc, num_cu, "threshold-%#x" % count)


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("place", list(hci.PLACEMENTS))
def test_placement_of_the_run(rs, torch, orc, num_cu, place, mode):
    _run(rs, torch, orc, num_cu, "u64-" + place, mode=mode)


@pytest.mark.parametrize("name", ["u64-2^24-across-regions", "i64-across-regions", "f64-across-chunks", "(u32,u32)-ends-at-n",
                                  "(u64,u64)-across-regions", "u128-at-0"])
def test_types_and_sizes(rs, torch, orc, num_cu, name):
    _run(rs, torch, orc, num_cu, name)


@pytest.mark.parametrize("name", ["three-hot", "nine-hot"])
def test_several_hot_buckets(rs, torch, orc, num_cu, name):
    """Three hot buckets that all park; nine that park nothing, which the verdict refuses for their number."""
    _run(rs, torch, orc, num_cu, name)


@pytest.mark.parametrize("name", ["u64-sorted", "u64-reversed", "u64-blocks", "(u64,u64)-sorted"])
def test_locally_ordered_globally_uniform(rs, torch, orc, num_cu, name):
    """Every bucket is contiguous in the input but small: nothing parks, the hybrid runs."""
    _run(rs, torch, orc, num_cu, name)


@pytest.mark.parametrize("schedule,ranking", [(1, 0), (0, 1), (0, 2)])
def test_schedules_and_rankings(rs, torch, orc, num_cu, schedule, ranking):
    _run(rs, torch, orc, num_cu, "u64-across-chunks", schedule=schedule, ranking=ranking)


def _joined(orc, name, num_cu, es):
    """The keys of a u64 case for a key / value call that sorts joined elements of `es` bytes: what the case relies on is
    asserted again for THAT size -- its regions, its count chunks, its workgroup's capacity and medium_max."""
    case = hci.CASES[name]
    raw, geom, runs = hci.build(case, num_cu)
    assert np.array_equal(raw, _input(orc, name, num_cu)[0])
    hci.conditions(case, raw, hci.geometry(case.n, es, case.cap, num_cu), runs, es=es)
    return _input(orc, name, num_cu)[0]


def _joined_path(rs, c, es):
    """the inner sort of the joined elements: their size, and the path it took"""
    assert (c.get_info(rs.INFO_LAST_PAIRS) >> 8) & 0xFF == es, hex(c.get_info(rs.INFO_LAST_PAIRS))
    return _path(rs, c)


def test_pairs_on_clustered_keys(rs, torch, orc, num_cu):
    """radix_sort_pairs, u64 keys with u64 values: the joined 16-byte elements meet the same run, a counter parks in
    their geometry too, and the inner sort is given to the LSD passes."""
    keys_raw = _joined(orc, "u64-across-regions", num_cu, 16)
    n = keys_raw.size // 8
    want_keys, _v, perm = pairs_reference(keys_raw, None, 8, util.UNSIGNED, 0, False)
    c = rs.Context(torch.cuda.current_device())
    try:
        c.set_option(rs.OPT_WIDE_SORT, 3)
        keys = torch.from_numpy(keys_raw.copy()).cuda().view(torch.uint64)
        vals = torch.arange(n, dtype=torch.int64, device="cuda") * 3 + 1
        rs.radix_sort_pairs(keys, vals, ctx=c)
        c.check()
        assert _joined_path(rs, c, 16) == 0
        assert np.array_equal(keys.view(torch.uint8).cpu().numpy(), want_keys)
        assert np.array_equal(vals.cpu().numpy(), perm * 3 + 1)
    finally:
        c.close()


def test_argsort_on_clustered_keys(rs, torch, orc, num_cu):
    """radix_argsort into int64 positions: joined (key, position) elements of 16 bytes."""
    keys_raw = _joined(orc, "u64-at-0", num_cu, 16)
    perm = pairs_reference(keys_raw, None, 8, util.UNSIGNED, 0, False)[2]
    c = rs.Context(torch.cuda.current_device())
    try:
        c.set_option(rs.OPT_WIDE_SORT, 3)
        keys = torch.from_numpy(keys_raw.copy()).cuda().view(torch.uint64)
        got = rs.radix_argsort(keys, ctx=c)
        c.check()
        assert _joined_path(rs, c, 16) == 0
        assert np.array_equal(keys.view(torch.uint8).cpu().numpy(), keys_raw)  # the keys are not modified
        assert np.array_equal(got.cpu().numpy(), perm)
    finally:
        c.close()


def test_graph_replay_uniform_clustered_uniform_clustered(rs, torch, orc, num_cu):
    """Both sequences of the hybrid are captured once; every replay decides on the device.  A replay on a clustered input
    parks and takes the LSD passes, the next one on a uniform input takes the hybrid again: the parked word is reset on
    the device by the replayed kernels themselves."""
    names = ["u64-uniform", "u64-across-chunks", "u64-uniform", "u64-across-regions"]
    d = rs.RadixDigits(*util.TYPES["u64"])
    n = hci.N23
    c = rs.Context(torch.cuda.current_device())
    try:
        c.set_option(rs.OPT_WIDE_SORT, 3)
        c.reserve(n, d)
        src = torch.from_numpy(_input(orc, names[0], num_cu)[0].copy()).cuda()
        work, tmp = torch.empty_like(src), torch.empty_like(src)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            work.copy_(src)
            c.sort_device(work.data_ptr(), tmp.data_ptr(), n, d, s.cuda_stream)  # warm-up outside capture
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            work.copy_(src)
            c.sort_device(work.data_ptr(), tmp.data_ptr(), n, d, torch.cuda.current_stream().cuda_stream)
        for i, name in enumerate(names):
            raw, exp = _input(orc, name, num_cu)
            src.copy_(torch.from_numpy(raw.copy()))
            graph.replay()
            torch.cuda.synchronize()
            c.check()
            assert _path(rs, c) == hci.CASES[name].path, (i, name, hex(c.get_info(rs.INFO_LAST_PASSES)))
            assert np.array_equal(work.cpu().numpy(), exp), (i, name)
    finally:
        c.close()


def test_uniform_sort_after_a_clustered_one(rs, torch, orc, num_cu):
    """The context after a refusal: the refusal is remembered on the host (15 sorts without a try) until the option is set
    again; then a uniform input takes the hybrid, and nothing of the parked sort is left on the device."""
    d = rs.RadixDigits(*util.TYPES["u64"])
    c = rs.Context(torch.cuda.current_device())
    try:
        c.set_option(rs.OPT_WIDE_SORT, 3)
        for name in ("u64-ends-at-n", "u64-uniform"):
            raw, exp = _input(orc, name, num_cu)
            x = torch.from_numpy(raw.copy()).cuda()
            rs.radix_sort(x, digits=d, ctx=c)
            c.check()
            assert _path(rs, c) == hci.CASES[name].path, (name, hex(c.get_info(rs.INFO_LAST_PASSES)))
            assert np.array_equal(x.cpu().numpy(), exp), name
            c.set_option(rs.OPT_WIDE_SORT, 3)  # (forget the refusal)
    finally:
        c.close()
