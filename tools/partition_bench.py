"""Time of the multi-way partition (rsx_multisplit_device: radix_partition) beside the chains a caller had before it.

    python tools/partition_bench.py [--shapes "keys:u32:28:64;...;ids:u32:24:8"] [--reps 9] [--warmup 3]
                                    [--json profiles/partition_bench.jsonl] [--once]

A shape is form:type:log2(n):bins[:dist]; the types: u32, i64; dist: uniform (the default), onebin (every key in one
bin), sorted (the keys ascending); the forms:

  keys   range partition by `bins` sorted edges, the keys alone
  pairs  the same with a value column (u32 values for 4-byte keys, f64 for i64) and int64 positions
  ids    the keys are integer ids over `bins` values (num_bins=), with the value column and positions: the dispatch shape

One JSON line per shape with, for each way, the median, the smallest and the largest device time of --reps runs (HIP events
around the way alone, warm-up first; the ways alternate within a repetition, the protocol of tools/bin_bench.py):

  call    radix_partition into preallocated outputs (out=): nothing is read by the host
  chain   what a caller wrote before through this library: radix_searchsorted for the bin ids (ids: the keys themselves),
          radix_argsort of them, one torch gather per column, radix_histogram / radix_bincount and a cumsum for the offsets
  torch   torch.bucketize, torch.sort(stable=True) of the bin ids, the gathers, torch.bincount and a cumsum
  copy    a plain device copy (Tensor.copy_) of the bytes the call must move: the floor

The yardstick is `chain`.  bytes is what the call moves: two reads of the keys, one read and one write of every column
that has an output.  frac_of_8TBps = bytes / 8 TB/s / call_ms.  slower_than_chain: the call's median is above the
chain's.  agrees: every output of the call equals the chain's.  --once: every shape once through the call, nothing timed
(for a kernel trace).
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
TYPES = {"u32": (torch.uint32, torch.int32, 4, torch.int32), "i64": (torch.int64, torch.int64, 8, torch.float64)}
E = rs.partition_caps(4)[0]
DEFAULT_SHAPES = (f"keys:u32:28:64;keys:u32:28:1024;keys:u32:28:{E};pairs:u32:28:64;pairs:u32:28:1024;pairs:u32:28:{E};"
                  "ids:u32:24:8;ids:u32:24:64;ids:u32:24:256;ids:u32:28:8;ids:u32:28:64;ids:u32:28:256;pairs:i64:26:64;"
                  "pairs:u32:28:64:onebin;pairs:u32:28:64:sorted;pairs:u32:16:64")


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
    vals = torch.arange(n, device="cuda").to(vdt)
    return x, edges, vals


def run_shape(form, tname, logn, bins, dist, ctx, reps, warmup, once):
    kdt, _view, kb, _vdt = TYPES[tname]
    n = 1 << logn
    x, edges, vals = make_inputs(form, tname, n, bins, dist)
    keys = x.view(kdt)
    kedges = edges.view(kdt) if edges is not None else None
    with_rows = form != "keys"
    vb = vals.element_size() if with_rows else 0
    m = bins
    out = rs.Partitioned(torch.empty(n, dtype=kdt, device="cuda"), torch.empty_like(vals) if with_rows else None,
                         torch.empty(n, dtype=torch.int64, device="cuda") if with_rows else None,
                         torch.empty(m + 2, dtype=torch.int64, device="cuda"))
    kept = {}

    def call():
        if form == "ids":
            kept["call"] = rs.radix_partition(keys, num_bins=m, values=vals, out=out, ctx=ctx)
        else:
            kept["call"] = rs.radix_partition(keys, edges=kedges, values=vals if with_rows else None, out=out, ctx=ctx)

    def gathers(perm, counts):
        off = torch.zeros(m + 2, dtype=torch.int64, device="cuda")
        torch.cumsum(counts, 0, out=off[1:])
        return x[perm], (vals[perm] if with_rows else None), (perm if with_rows else None), off

    def chain():
        if form == "ids":
            ids, counts = keys, rs.radix_bincount(keys, m, ctx=ctx)
        else:
            ids = rs.radix_searchsorted(kedges, keys, side="right", index_dtype=torch.int32, ctx=ctx)
            counts = rs.radix_histogram(keys, kedges, ctx=ctx)
        kept["chain"] = gathers(rs.radix_argsort(ids, ctx=ctx), counts)

    def torch_way():
        ids = x if form == "ids" else torch.bucketize(x, edges, right=True)
        perm = torch.sort(ids, stable=True).indices
        kept["torch"] = gathers(perm, torch.bincount(ids, minlength=m + 1))

    nbytes = n * (2 * kb + kb + 2 * vb + (8 if with_rows else 0))
    floor_src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")  # a copy reads and writes: half the bytes each way
    floor_dst = torch.empty_like(floor_src)
    ways = {"call": call, "chain": chain, "torch": torch_way, "copy": lambda: floor_dst.copy_(floor_src)}
    rec = {"call": "radix_partition", "form": form, "type": tname, "log2n": logn, "bins": bins, "dist": dist, "key_bytes": kb, "reps": reps}
    if once:
        call()
        ctx.check()
        rec["once"] = True
        return rec
    times = time_ways(ways, ctx, reps, warmup)
    agree = True
    for other in ("chain", "torch"):
        k, v, i, off = kept[other]
        agree = agree and bool(torch.equal(out.keys.view(x.dtype), k) and torch.equal(out.offsets, off))
        if with_rows:
            agree = agree and bool(torch.equal(out.values, v) and torch.equal(out.index, i))
    kept.clear()
    for w, v in times.items():
        rec[w + "_ms"] = round(median(v), 4)
        rec[w + "_min_ms"] = round(min(v), 4)
        rec[w + "_max_ms"] = round(max(v), 4)
    rec["yardstick"] = "chain"
    rec["bytes"] = nbytes
    rec["frac_of_8TBps"] = round(nbytes / 8e12 * 1e3 / rec["call_ms"], 3)
    rec["call_vs_chain"] = round(rec["chain_ms"] / rec["call_ms"], 2)
    rec["call_vs_torch"] = round(rec["torch_ms"] / rec["call_ms"], 2)
    rec["call_vs_copy"] = round(rec["call_ms"] / rec["copy_ms"], 2)
    rec["slower_than_chain"] = bool(rec["call_ms"] > rec["chain_ms"])
    rec["agrees"] = agree
    rec["caps"] = rs.partition_caps(kb)
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
