"""Time of the per-bin reduction (rsx_bin_reduce_device: radix_bin_reduce) beside the ways a caller had before it.

    python tools/bin_reduce_bench.py [--shapes "keys:u32:28:64;...;ids:u32:28:8"] [--reps 9] [--warmup 3]
                                     [--json profiles/bin_reduce_bench.jsonl] [--once]

A shape is form:type:log2(n):bins[:dist]; the types: u32 (f32 values), i64 (f64 values); dist: uniform (the default),
onebin (every key in one bin), sorted (the keys ascending); the forms:

  keys   a weighted histogram: the sums of the values between `bins` sorted edges
  ids    the keys are integer ids over `bins` values (num_bins=): torch.bincount(weights=), the per-expert sums

One JSON line per shape with, for each way, the median, the smallest and the largest device time of --reps runs (HIP events
around the way alone, warm-up first; the ways alternate within a repetition, the protocol of tools/bin_bench.py):

  call       radix_bin_reduce(op="sum") into a preallocated output (out=): nothing is read by the host
  chain      what a caller wrote before through this library: radix_searchsorted for the bin ids (ids: the keys
             themselves), radix_reduce_by_key on them -- which sorts --, and a scatter of the groups into a dense array
  bincount   torch.bincount(torch.bucketize(keys, edges, right=True), weights=values, minlength=bins + 1) (ids: no
             bucketize): floating-point atomics, sums that differ from run to run
  index_add  zeros(bins + 1).index_add_(0, the same bin ids, values)
  histogram  radix_histogram / radix_bincount of the same keys, the counts alone: the floor of the search and the read of
             the keys, so that call - histogram is what the value column and the ordered combine cost
  copy       a plain device copy (Tensor.copy_) of the bytes the call must read: the floor of the memory traffic

The yardstick is `chain`.  bytes is what the call reads: the keys and the values once.  frac_of_8TBps = bytes / 8 TB/s /
call_ms.  slower_than_chain / slower_than_torch: the call's median is above the chain's / above the faster of the two
torch ways.  agrees: the call's sums are within twice the order-free bound g(c - 1) * sum|v| of the chain's (both add the
same values in another order), and two calls give equal bytes.  --once: every shape once through the call, nothing timed (for a kernel
trace).  bins_beyond_the_bound: the bins with so many values (2^24 of f32) that the bound is vacuous; they are not compared.
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
from compact_bench import time_ways  # noqa: E402
from segment_bench import median  # noqa: E402

# type -> (key dtype the library sees, the view torch computes with, key bytes, value dtype)
TYPES = {"u32": (torch.uint32, torch.int32, 4, torch.float32), "i64": (torch.int64, torch.int64, 8, torch.float64)}
E = rs.bin_reduce_caps(4, 4)[0]
DEFAULT_SHAPES = (f"keys:u32:28:64;keys:u32:28:1024;keys:u32:28:{E};ids:u32:28:8;ids:u32:28:64;ids:u32:28:1024;keys:i64:26:64;ids:i64:26:64;"
                  "keys:u32:28:64:onebin;keys:u32:28:64:sorted;ids:u32:28:64:sorted;keys:u32:16:64;ids:u32:16:64")


def make_inputs(form, tname, n, bins, dist):
    """keys as torch computes with them (non-negative, so that torch's order is the library's), the edges, the values"""
    _kdt, view, kb, vdt = TYPES[tname]
    g = torch.Generator(device="cuda")
    g.manual_seed(n % 1000 + kb + bins)
    top = (1 << 31) - 1 if kb == 4 else (1 << 62)
    if form == "ids":
        x = torch.randint(0, bins, (n,), dtype=torch.int64, device="cuda", generator=g).to(view)
        edges = None
    else:
        x = torch.randint(0, top, (n,), dtype=torch.int64, device="cuda", generator=g).to(view)
        edges = torch.sort(torch.randint(0, top, (bins,), dtype=torch.int64, device="cuda", generator=g).to(view)).values
    if dist == "onebin":
        x.fill_(3)
    elif dist == "sorted":
        x = torch.sort(x).values
    vals = torch.randn(n, device="cuda", generator=g, dtype=torch.float32).to(vdt)
    return x, edges, vals


def run_shape(form, tname, logn, bins, dist, ctx, reps, warmup, once):
    kdt, _view, kb, vdt = TYPES[tname]
    n = 1 << logn
    x, edges, vals = make_inputs(form, tname, n, bins, dist)
    keys = x.view(kdt)
    kedges = edges.view(kdt) if edges is not None else None
    vb = vals.element_size()
    m = bins
    out = torch.empty(m + 1, dtype=vdt, device="cuda")
    kept = {}

    def call():
        if form == "ids":
            kept["call"] = rs.radix_bin_reduce(keys, vals, num_bins=m, out=out, ctx=ctx)
        else:
            kept["call"] = rs.radix_bin_reduce(keys, vals, edges=kedges, out=out, ctx=ctx)

    def chain():
        ids = keys if form == "ids" else rs.radix_searchsorted(kedges, keys, side="right", index_dtype=torch.int32, ctx=ctx)
        red = rs.radix_reduce_by_key(ids, vals, op="sum", ctx=ctx)
        dense = torch.zeros(m + 2, dtype=vdt, device="cuda")
        slot = torch.where(torch.arange(n, device="cuda") < red.num, red.keys.view(x.dtype if form == "ids" else torch.int32).to(torch.int64), m + 1)
        dense.scatter_(0, slot, red.values)
        kept["chain"] = dense[:m + 1]

    def bin_ids():
        return (x if form == "ids" else torch.bucketize(x, edges, right=True)).to(torch.int64)

    def bincount():
        kept["bincount"] = torch.bincount(bin_ids(), weights=vals, minlength=m + 1)

    def index_add():
        kept["index_add"] = torch.zeros(m + 1, dtype=vdt, device="cuda").index_add_(0, bin_ids(), vals)

    def histogram():
        kept["histogram"] = rs.radix_bincount(keys, m, ctx=ctx) if form == "ids" else rs.radix_histogram(keys, kedges, ctx=ctx)

    nbytes = n * (kb + vb)
    floor_src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")  # a copy reads and writes: half the bytes each way
    floor_dst = torch.empty_like(floor_src)
    ways = {"call": call, "chain": chain, "bincount": bincount, "index_add": index_add, "histogram": histogram,
            "copy": lambda: floor_dst.copy_(floor_src)}
    rec = {"call": "radix_bin_reduce", "form": form, "type": tname, "log2n": logn, "bins": bins, "dist": dist, "key_bytes": kb, "value_bytes": vb,
           "reps": reps}
    if once:
        call()
        ctx.check()
        rec["once"] = True
        return rec
    times = time_ways(ways, ctx, reps, warmup)
    # the same values added in another order: within g(c - 1) * sum|v| of each other, twice over
    counts = kept["histogram"][:m + 1].to(torch.float64)
    u = 2.0 ** -24 if vb == 4 else 2.0 ** -53
    k = (counts - 1).clamp(min=0) * u
    abs_sums = torch.zeros(m + 1, dtype=torch.float64, device="cuda").index_add_(0, bin_ids(), vals.abs().to(torch.float64))
    vacuous = k >= 1  # (f32 bins of 2^24 values and more: the bound says nothing about them)
    bound = torch.where(vacuous, float("inf"), 2 * k / (1 - k).clamp(min=u) * abs_sums)
    agree = bool(((out.to(torch.float64) - kept["chain"].to(torch.float64)).abs() <= bound).all())
    rec["bins_beyond_the_bound"] = int(vacuous.sum())
    first = out.clone()
    call()
    agree = agree and bool(torch.equal(first.view(torch.int32 if vb == 4 else torch.int64), out.view(torch.int32 if vb == 4 else torch.int64)))
    kept.clear()
    for w, v in times.items():
        rec[w + "_ms"] = round(median(v), 4)
        rec[w + "_min_ms"] = round(min(v), 4)
        rec[w + "_max_ms"] = round(max(v), 4)
    rec["yardstick"] = "chain"
    rec["bytes"] = nbytes
    rec["frac_of_8TBps"] = round(nbytes / 8e12 * 1e3 / rec["call_ms"], 3)
    rec["call_vs_chain"] = round(rec["chain_ms"] / rec["call_ms"], 2)
    rec["call_vs_bincount"] = round(rec["bincount_ms"] / rec["call_ms"], 2)
    rec["call_vs_index_add"] = round(rec["index_add_ms"] / rec["call_ms"], 2)
    rec["call_vs_histogram"] = round(rec["call_ms"] / rec["histogram_ms"], 2)
    rec["call_vs_copy"] = round(rec["call_ms"] / rec["copy_ms"], 2)
    rec["slower_than_chain"] = bool(rec["call_ms"] > rec["chain_ms"])
    rec["slower_than_torch"] = bool(rec["call_ms"] > min(rec["bincount_ms"], rec["index_add_ms"]))
    rec["agrees"] = agree
    rec["caps"] = rs.bin_reduce_caps(kb, vb)
    rec["library"] = os.path.basename(rs._lib.lib_path())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="form:type:log2n:bins[:dist], separated by ;")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    ap.add_argument("--once", action="store_true", help="every shape once through the call, nothing timed")
    a = ap.parse_args()
    ctx = rs.Context(torch.cuda.current_device())
    sink = open(a.json, "a") if a.json else None
    for shape in [x for x in a.shapes.split(";") if x]:
        f = shape.split(":")
        rec = run_shape(f[0], f[1], int(f[2]), int(f[3]), f[4] if len(f) > 4 else "uniform", ctx, a.reps, a.warmup, a.once)
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
