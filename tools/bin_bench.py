"""Time of the bin-count call (rsx_bin_count_device: radix_histogram, radix_bincount) beside the chains a caller had before it.

    python tools/bin_bench.py [--shapes "hist:u32:28:uniform:64;...;ids:u32:28:12"] [--reps 9] [--warmup 3]
                              [--json profiles/bin_bench.jsonl] [--once]

A histogram shape is hist:type:log2(n):input:edges; the types: u32, f32, i64; the inputs: `uniform` (random keys, edges evenly
spaced over their range), `randn` (f32 only, torch.linspace(-4, 4) edges), `equal` (all keys equal), `sorted` (uniform keys,
sorted); edges: a number or `max` (bin_caps' max_edges).  A bincount shape is ids:type:log2(n):log2(values): ids uniform over
that many values, as many bins (12: one
LDS window; 16 and 18: 4 and 16 windows; 20: atomics into the counts).  One JSON line per shape with, for each way, the median, the smallest and the largest device
time of --reps runs (HIP events around the call alone, warm-up first; the ways alternate within a repetition, the protocol of
tools/select_bench.py):

  call      radix_histogram / radix_bincount
  chain     hist: torch.bincount(radix_searchsorted(edges, keys, side="right"), minlength=m + 1), the route before the call
  histc     hist, f32 only: torch.histc over the same range -- orientation only, its edge rule differs
  bincount  ids: torch.bincount(keys, minlength=bins)
  unique    ids: radix_unique(keys, return_counts=True) (it reads the number of groups: one synchronisation)

The yardstick is the fastest way that existed before the call (`chain`; for ids the faster of `bincount` and `unique`),
timed in the same run.  bytes = n * key_bytes is what the call HAS to read; frac_of_8TBps = bytes / 8 TB/s / call_ms.
faster_beyond_spread: the slowest run of the call was faster than the fastest run of the yardstick.  agrees: the call's counts
equal the yardstick's.  --once: every shape once through the call, nothing timed (for a kernel trace).
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

# type -> (key dtype the library sees, the view torch computes with, key bytes)
TYPES = {"u32": (torch.uint32, torch.int32, 4), "f32": (torch.float32, torch.float32, 4), "i64": (torch.int64, torch.int64, 8)}
DEFAULT_SHAPES = ("hist:u32:28:uniform:64;hist:u32:28:uniform:1024;hist:u32:28:uniform:max;hist:f32:28:randn:64;hist:u32:28:equal:1024;"
                  "hist:u32:28:sorted:1024;hist:i64:26:uniform:1024;hist:u32:16:uniform:1024;ids:u32:28:12;ids:u32:28:16;ids:u32:28:18;ids:u32:28:20")


def make_keys(tname, n, kind):
    _kdt, view, kb = TYPES[tname]
    g = torch.Generator(device="cuda")
    g.manual_seed(n % 1000 + kb)
    if kind == "equal":
        return torch.full((n,), 1 << 30, dtype=view, device="cuda")
    if kind == "randn":
        return torch.randn(n, dtype=torch.float32, device="cuda", generator=g)
    if kb == 4:  # below 2^31: the signed view orders alike
        x = torch.randint(0, 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    else:
        x = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g)
    return torch.sort(x).values if kind == "sorted" else x


def make_edges(tname, m, kind):
    _kdt, view, kb = TYPES[tname]
    if kind == "randn":
        return torch.linspace(-4, 4, m, device="cuda")
    lo, hi = (0, 1 << 31) if kb == 4 else (-(1 << 62), 1 << 62)
    step = (hi - lo) // (m + 1)
    return (torch.arange(1, m + 1, dtype=torch.int64, device="cuda") * step + lo).to(view)


def record(rec, times, yardsticks, n, kb, agree):
    for w, v in times.items():
        rec[w + "_ms"] = round(median(v), 4)
        rec[w + "_min_ms"] = round(min(v), 4)
        rec[w + "_max_ms"] = round(max(v), 4)
    best = min(yardsticks, key=lambda w: rec[w + "_min_ms"])
    rec["yardstick"] = best
    rec["bytes"] = n * kb
    rec["frac_of_8TBps"] = round(rec["bytes"] / 8e12 * 1e3 / rec["call_ms"], 3)
    rec["call_vs_yardstick"] = round(rec[best + "_ms"] / rec["call_ms"], 2)
    rec["faster_beyond_spread"] = bool(rec["call_max_ms"] < rec[best + "_min_ms"])
    rec["agrees"] = agree
    rec["caps"] = rs.bin_caps(kb)
    rec["library"] = os.path.basename(rs._lib.lib_path())
    return rec


def time_ways(ways, ctx, reps, warmup):
    st = torch.cuda.current_stream()
    times = {w: [] for w in ways}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            t = timed(fn, st)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    return times


def run_hist(tname, logn, kind, edges_arg, ctx, reps, warmup, once):
    kdt, view, kb = TYPES[tname]
    n = 1 << logn
    m = rs.bin_caps(kb)[0] if edges_arg == "max" else int(edges_arg)
    x = make_keys(tname, n, kind)
    e = make_edges(tname, m, kind)
    keys, edges = x.view(kdt), e.view(kdt)
    out = torch.empty(m + 1, dtype=torch.int64, device="cuda")
    kept = {}

    def call():
        kept["call"] = rs.radix_histogram(keys, edges, out=out, ctx=ctx)

    def chain():
        kept["chain"] = torch.bincount(rs.radix_searchsorted(edges, keys, side="right", ctx=ctx), minlength=m + 1)

    def histc():
        kept["histc"] = torch.histc(x, bins=m - 1, min=float(e[0]), max=float(e[-1]))

    rec = {"call": "radix_histogram", "type": tname, "log2n": logn, "input": kind, "edges": m, "key_bytes": kb, "reps": reps}
    if once:
        call()
        ctx.check()
        rec["once"] = True
        return rec
    ways = {"call": call, "chain": chain}
    if tname == "f32":
        ways["histc"] = histc
    times = time_ways(ways, ctx, reps, warmup)
    agree = bool(torch.equal(kept["call"], kept["chain"]))
    kept.clear()
    return record(rec, times, ["chain"], n, kb, agree)


def run_ids(tname, logn, logv, ctx, reps, warmup, once):
    kdt, view, kb = TYPES[tname]
    n, bins = 1 << logn, 1 << logv
    g = torch.Generator(device="cuda")
    g.manual_seed(logv)
    x = torch.randint(0, bins, (n,), dtype=torch.int64, device="cuda", generator=g).to(view)
    keys = x.view(kdt)
    out = torch.empty(bins + 1, dtype=torch.int64, device="cuda")
    kept = {}

    def call():
        kept["call"] = rs.radix_bincount(keys, bins, out=out, ctx=ctx)

    def bincount():
        kept["bincount"] = torch.bincount(x, minlength=bins)

    def unique():
        kept["unique"] = rs.radix_unique(keys, return_counts=True, ctx=ctx)

    rec = {"call": "radix_bincount", "type": tname, "log2n": logn, "input": "ids", "bins": bins, "key_bytes": kb, "reps": reps}
    if once:
        call()
        ctx.check()
        rec["once"] = True
        return rec
    times = time_ways({"call": call, "bincount": bincount, "unique": unique}, ctx, reps, warmup)
    agree = bool(torch.equal(kept["call"][:bins], kept["bincount"])) and int(kept["call"][bins]) == 0
    uk, uc = kept["unique"]
    agree = agree and bool(torch.equal(kept["call"][uk.view(view).to(torch.int64)], uc))
    kept.clear()
    return record(rec, times, ["bincount", "unique"], n, kb, agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="hist:type:log2n:input:edges or ids:type:log2n:log2values, separated by ;")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    ap.add_argument("--once", action="store_true", help="every shape once through the call, nothing timed")
    a = ap.parse_args()
    ctx = rs.Context(torch.cuda.current_device())
    sink = open(a.json, "a") if a.json else None
    for shape in [x for x in a.shapes.split(";") if x]:
        f = shape.split(":")
        if f[0] == "hist":
            rec = run_hist(f[1], int(f[2]), f[3], f[4], ctx, a.reps, a.warmup, a.once)
        else:
            rec = run_ids(f[1], int(f[2]), int(f[3]), ctx, a.reps, a.warmup, a.once)
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
