"""Time of reduce by key (rsx_reduce_by_key_device: radix_reduce_by_key) beside the other ways to get the same sums.

    python tools/reduce_bench.py [--workloads "u32-values16;i64-quarter;i64-distinct"] [--log2n 0] [--reps 10] [--warmup 2]
                                 [--json profiles/reduce_bench.jsonl]

Workloads (keys generated on the device, float32 values uniform in [0, 1)):
  u32-values16   2^28 u32 keys uniform over 2^16 values
  i64-quarter    2^26 i64 keys uniform over n / 4 values (m about n / 4: the shape of coalescing a sparse COO tensor)
  i64-distinct   2^26 i64 keys, all distinct (a permutation spread over the 64 bits)
--log2n K runs every workload at 2^K keys instead.

One JSON line per workload with the median device time (HIP events around the call alone, warm-up first; the ways
alternate within a repetition, the protocol of tools/pairs_bench.py; a fresh context and an emptied allocator cache per
workload) of

  reduce_ms        radix_reduce_by_key(keys, values, "sum") -- keys, values and num, no offsets
  chain_group_ms   (i) what a caller writes without it: radix_group(perm=True), values[perm], torch.segment_reduce over
                   the offsets (the host reads m to slice them: one synchronisation, inside the events).  torch refuses
                   the launch of segment_reduce for 2^26 segments (invalid configuration), so above 2^25 groups the last
                   step is the difference of a float64 cumsum at the offsets instead; chain_group_last says which ran
  chain_torch_ms   (ii) torch.unique(sorted=True, return_inverse=True) and index_add_ (atomics: sums that differ from run
                   to run); torch has no unique of u32: its signed view is taken instead (another order, the same work)
  sort_pairs_ms    (iii) radix_sort_pairs on copies of the two columns (the copies are made outside the events): the floor
                   the sort alone sets
and the ratios reduce_vs_sort_pairs = reduce_ms / sort_pairs_ms, chain_group_vs_reduce = chain_group_ms / reduce_ms and
chain_torch_vs_reduce = chain_torch_ms / reduce_ms.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import radix_sort_amd as rs  # noqa: E402
from segment_bench import median, timed  # noqa: E402

# workload -> (key dtype, the view torch.unique takes, key bytes, default log2 n)
WORKLOADS = {
    "u32-values16": (torch.uint32, torch.int32, 4, 28),
    "i64-quarter": (torch.int64, torch.int64, 8, 26),
    "i64-distinct": (torch.int64, torch.int64, 8, 26),
}
SEGMENT_REDUCE_MAX = 1 << 25  # groups above which torch.segment_reduce cannot be launched


def make_keys(name, n):
    kdt, view, _kb, _k = WORKLOADS[name]
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED0009)
    if name == "u32-values16":
        x = torch.randint(0, 1 << 16, (n,), dtype=view, device="cuda", generator=g)
    elif name == "i64-quarter":
        x = torch.randint(0, max(1, n // 4), (n,), dtype=view, device="cuda", generator=g)
    else:
        x = torch.randperm(n, dtype=torch.int64, device="cuda", generator=g) * -7046029254386353131  # (odd: a bijection of 64 bits)
    return x.view(kdt)


def run_workload(name, k, reps, warmup):
    kdt, view, kb, _k = WORKLOADS[name]
    n = 1 << k
    ctx = rs.Context(torch.cuda.current_device())
    st = torch.cuda.current_stream()
    keys = make_keys(name, n)
    tkeys = keys.view(view)
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED000A)
    values = torch.rand(n, dtype=torch.float32, device="cuda", generator=g)
    kcopy, vcopy = torch.empty_like(keys), torch.empty_like(values)
    box = {}

    def reduce():
        box["r"] = rs.radix_reduce_by_key(keys, values, ctx=ctx)

    def chain_group():
        grp = rs.radix_group(keys, perm=True, ctx=ctx)
        gathered = values[grp.perm]
        m = int(grp.num)
        if m <= SEGMENT_REDUCE_MAX:
            box["chain"] = torch.segment_reduce(gathered, "sum", offsets=grp.offsets[:m + 1])
        else:
            total = torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), torch.cumsum(gathered, 0, dtype=torch.float64)])
            at = total[grp.offsets[:m + 1]]
            box["chain"] = (at[1:] - at[:-1]).float()

    def chain_torch():
        uniq, inverse = torch.unique(tkeys, sorted=True, return_inverse=True)
        torch.zeros(uniq.numel(), dtype=torch.float32, device="cuda").index_add_(0, inverse, values)

    def sort_pairs():
        rs.radix_sort_pairs(kcopy, vcopy, ctx=ctx)

    ways = {"reduce_ms": reduce, "chain_group_ms": chain_group, "chain_torch_ms": chain_torch, "sort_pairs_ms": sort_pairs}
    times = {w: [] for w in ways}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            if w == "sort_pairs_ms":
                kcopy.copy_(keys)
                vcopy.copy_(values)
            t = timed(fn, st)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    m = int(box["r"].num)
    assert box["chain"].numel() == m
    assert torch.allclose(box["r"].values[:m], box["chain"], rtol=1e-4, atol=1e-6)  # (two associations of the same sums)
    rec = {"workload": name, "log2n": k, "key_bytes": kb, "value": "f32", "groups": m, "reps": reps}
    for w, v in times.items():
        rec[w] = round(median(v), 4)
    rec["chain_group_last"] = "segment_reduce" if m <= SEGMENT_REDUCE_MAX else "cumsum"
    rec["reduce_vs_sort_pairs"] = round(rec["reduce_ms"] / rec["sort_pairs_ms"], 3)
    rec["chain_group_vs_reduce"] = round(rec["chain_group_ms"] / rec["reduce_ms"], 2)
    rec["chain_torch_vs_reduce"] = round(rec["chain_torch_ms"] / rec["reduce_ms"], 2)
    rec["library"] = os.path.basename(rs._lib.lib_path())
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=";".join(WORKLOADS))
    ap.add_argument("--log2n", type=int, default=0, help="every workload at 2^K keys (0: each at its own size)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()
    sink = open(a.json, "a") if a.json else None
    for name in [x for x in a.workloads.split(";") if x]:
        rec = run_workload(name, a.log2n or WORKLOADS[name][3], a.reps, a.warmup)
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
