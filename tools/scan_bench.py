"""Time of scan by key (rsx_scan_by_key_device: radix_scan_by_key) beside the other ways to get the same running sums.

    python tools/scan_bench.py [--workloads "runs-u32-f32;runs-i64-f64;grouped-u32-values16;grouped-i64-quarter"] [--log2n 0]
                               [--reps 10] [--warmup 2] [--json profiles/scan_bench.jsonl]

Workloads (keys generated on the device, values uniform in [0, 1)):
  runs-u32-f32          2^28 u32 keys lying in runs of about 2^12 (geometric lengths), f32 values -- RSX_SCAN_RUNS
  runs-i64-f64          2^26 i64 keys likewise, f64 values                                    -- RSX_SCAN_RUNS
  grouped-u32-values16  2^28 u32 keys uniform over 2^16 values, f32 values                    -- the grouped form
  grouped-i64-quarter   2^26 i64 keys uniform over n / 4 values, f32 values                   -- the grouped form
--log2n K runs every workload at 2^K keys instead.

One JSON line per workload with the median device time (HIP events around the call alone, warm-up first; the ways alternate
within a repetition, the protocol of tools/reduce_bench.py; a fresh context and an emptied allocator cache per workload).

The runs form:
  scan_ms          radix_scan_by_key(keys, values, runs=True)
  cumsum_ms        (i) torch.cumsum of the values alone: the floor of a plain scan
  chain_ms         (ii) what a caller writes today: head flags of neighbouring keys, the start of every row's run by a
                   cummax of the head positions, cumsum, the base gathered back and subtracted
  reduce_runs_ms   (iii) the three run kernels of radix_reduce_by_key on the same keys and values: its RSX_PROF_SCAN time
                   (rsx_ctx_profile) less that of radix_sort_pairs on the same columns, whose sort is the one in front of
                   the run kernels and has scan launches of its own -- the same scan without the n stores
  and scan_bytes = n * (key_bytes + 2 * value_bytes), what the call must move at the least were it one pass,
  scan_tbps = scan_bytes / scan_ms and scan_of_8tbps, its fraction of 8 TB/s.
The grouped form:
  scan_ms          radix_scan_by_key(keys, values)
  count_ms         radix_scan_by_key(keys, None, exclusive=True): the count form (cumcount)
  argsort_ms       radix_argsort(keys) alone: the floor the sort sets
  chain_ms         radix_group(perm=True), values[perm], cumsum, the base of every group gathered back and subtracted, and
                   the scatter through perm
  gather_ms, scatter_ms   values[perm] and out[perm] = x alone, perm being the sorting permutation
and the ratios scan_vs_argsort = scan_ms / argsort_ms and chain_vs_scan = chain_ms / scan_ms.
Both forms: chain_max_abs_diff, the largest difference between the call's results and the chain's (whose every result is
the difference of two prefix sums of the whole array).
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

# workload -> (runs, key dtype, the signed view torch indexes and compares, key bytes, value dtype, default log2 n)
WORKLOADS = {
    "runs-u32-f32": (True, torch.uint32, torch.int32, 4, torch.float32, 28),
    "runs-i64-f64": (True, torch.int64, torch.int64, 8, torch.float64, 26),
    "grouped-u32-values16": (False, torch.uint32, torch.int32, 4, torch.float32, 28),
    "grouped-i64-quarter": (False, torch.int64, torch.int64, 8, torch.float32, 26),
}
RUN_LENGTH = 1 << 12
PEAK_TBPS = 8.0


def make_keys(name, n):
    runs, kdt, view, _kb, _vdt, _k = WORKLOADS[name]
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED000B)
    if runs:  # a head with probability 2^-12 per row: run lengths are geometric around 2^12; the key is the run's number
        head = torch.rand(n, device="cuda", generator=g) < 1.0 / RUN_LENGTH
        x = torch.cumsum(head, 0).to(view)
    elif name == "grouped-u32-values16":
        x = torch.randint(0, 1 << 16, (n,), dtype=view, device="cuda", generator=g)
    else:
        x = torch.randint(0, max(1, n // 4), (n,), dtype=view, device="cuda", generator=g)
    return x.view(kdt)


def starts_of(skeys):
    """For every position of a key array in which equal keys are neighbours, the position its run starts at."""
    n = skeys.numel()
    idx = torch.arange(n, device=skeys.device)
    head = torch.ones(n, dtype=torch.bool, device=skeys.device)
    head[1:] = skeys[1:] != skeys[:-1]
    return torch.cummax(torch.where(head, idx, torch.zeros_like(idx)), 0).values


def scan_in_runs(skeys, svalues):
    """The running sum inside every run as a caller writes it: the difference of two long prefix sums (not the run's own)."""
    c = torch.cumsum(svalues, 0)
    start = starts_of(skeys)
    base = torch.where(start > 0, c[torch.clamp(start - 1, min=0)], torch.zeros_like(c))
    return c - base


def run_workload(name, k, reps, warmup):
    runs, kdt, view, kb, vdt, _k = WORKLOADS[name]
    n = 1 << k
    vb = 4 if vdt == torch.float32 else 8
    ctx = rs.Context(torch.cuda.current_device())
    st = torch.cuda.current_stream()
    keys = make_keys(name, n)
    tkeys = keys.view(view)
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED000C)
    values = torch.rand(n, dtype=vdt, device="cuda", generator=g)
    out = torch.empty_like(values)
    box = {}

    def scan():
        box["scan"], box["num"] = rs.radix_scan_by_key(keys, values, runs=runs, out=out, return_num=True, ctx=ctx)

    ways = {"scan_ms": scan}
    if runs:
        def cumsum():
            torch.cumsum(values, 0)

        def chain():
            box["chain"] = scan_in_runs(tkeys, values)

        ways.update({"cumsum_ms": cumsum, "chain_ms": chain})
    else:
        perm = rs.radix_argsort(keys, ctx=ctx)
        ranks = torch.empty(n, dtype=torch.int64, device="cuda")
        index = torch.empty(n, dtype=torch.int64, device="cuda")
        scattered = torch.empty_like(values)

        def count():
            rs.radix_scan_by_key(keys, None, exclusive=True, out=ranks, ctx=ctx)

        def argsort():
            rs.radix_argsort(keys, out=index, ctx=ctx)

        def chain():
            grp = rs.radix_group(keys, perm=True, ctx=ctx)
            res = scan_in_runs(tkeys[grp.perm], values[grp.perm])
            o = torch.empty_like(values)
            o[grp.perm] = res
            box["chain"] = o

        def gather():
            box["gathered"] = values[perm]

        def scatter():
            scattered[perm] = values

        ways.update({"count_ms": count, "argsort_ms": argsort, "chain_ms": chain, "gather_ms": gather, "scatter_ms": scatter})
    times = {w: [] for w in ways}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            t = timed(fn, st)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    # a sanity check only: the chain subtracts two prefix sums of up to n / 2, each off by several units of ITS last place
    assert torch.allclose(box["scan"], box["chain"], rtol=1e-2, atol=1e-2 + n * (1e-6 if vb == 4 else 1e-12))
    rec = {"workload": name, "log2n": k, "key_bytes": kb, "value": "f32" if vb == 4 else "f64", "groups": int(box["num"]), "reps": reps}
    for w, v in times.items():
        rec[w] = round(median(v), 4)
    rec["chain_max_abs_diff"] = float((box["scan"] - box["chain"]).abs().max())  # how far the chain's differences are off
    if runs:
        # (iii) the run kernels of reduce by key on the same columns, from the context's own launch timers.  The sort in
        # front of them has scan launches of its own under the same timer kind: radix_sort_pairs of the same columns runs
        # that sort and nothing else, so its total is taken off.
        kcopy, vcopy = torch.empty_like(keys), torch.empty_like(values)

        def scan_kind_ms(fn):
            ctx.profile(True)
            for _ in range(reps):
                fn()
            ctx.check()
            ms, _launches = ctx.profile_read()["scan"]
            ctx.profile(False)
            return ms / reps

        def sort_pairs():
            kcopy.copy_(keys)
            vcopy.copy_(values)
            rs.radix_sort_pairs(kcopy, vcopy, ctx=ctx)

        with_runs = scan_kind_ms(lambda: rs.radix_reduce_by_key(keys, values, ctx=ctx))
        rec["reduce_runs_ms"] = round(with_runs - scan_kind_ms(sort_pairs), 4)
        rec["scan_bytes"] = n * (kb + 2 * vb)
        rec["scan_tbps"] = round(rec["scan_bytes"] / (rec["scan_ms"] * 1e-3) / 1e12, 3)
        rec["scan_of_8tbps"] = round(rec["scan_tbps"] / PEAK_TBPS, 3)
        rec["chain_vs_scan"] = round(rec["chain_ms"] / rec["scan_ms"], 2)
        rec["scan_vs_cumsum"] = round(rec["scan_ms"] / rec["cumsum_ms"], 2)
    else:
        rec["scan_vs_argsort"] = round(rec["scan_ms"] / rec["argsort_ms"], 3)
        rec["chain_vs_scan"] = round(rec["chain_ms"] / rec["scan_ms"], 2)
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
        rec = run_workload(name, a.log2n or WORKLOADS[name][5], a.reps, a.warmup)
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
