"""Time of the compaction call (rsx_compact_device: radix_compact, radix_nonzero) beside the torch forms a caller had before it.

    python tools/compact_bench.py [--shapes "mask:u32:28:2;...;range:f32:28"] [--reps 9] [--warmup 3]
                                  [--json profiles/compact_bench.jsonl] [--once]

A shape is form:type:log2(n)[:d], the mask density being 1/d (d = 1: every row passes); the types: u32, f32, i64; the forms:

  mask       keys[mask]: the keys alone under a bool mask
  pairs      the same with a value column (u32 values for 4-byte keys, f64 for i64) and int64 positions
  partition  `mask` with partition=True: the other rows behind the kept ones
  range      no mask: lo = a key near the median, as a device word
  nonzero    radix_nonzero(mask): positions only

One JSON line per shape with, for each way, the median, the smallest and the largest device time of --reps runs (HIP events
around the call alone, warm-up first; the ways alternate within a repetition, the protocol of tools/bin_bench.py):

  call      radix_compact / radix_nonzero into preallocated outputs (out=): nothing is read by the host
  index     keys[mask] (range: keys[keys >= lo], the comparison included): torch's boolean index, which reads the count
            back to size its result -- that host read is inside its time
  select    torch.masked_select(keys, mask)
  nonzero   torch.nonzero(mask)
  copy      a plain device copy (Tensor.copy_) of the bytes the call must move: the floor

The yardstick is `index` (for the nonzero form `nonzero`).  pairs and partition time torch's form on every column the call
moves: keys[mask], values[mask] and torch.nonzero(mask) for pairs; torch.cat((keys[mask], keys[~mask])) for partition.
bytes is what the call moves: n * (the predicate column) for the count launch, n * (every input column) + kept * (every
output column) for the write launch; frac_of_8TBps = bytes / 8 TB/s / call_ms.  slower_than_torch: the call's median is
above the yardstick's.  agrees: the call's first `num` rows equal the yardstick's result.  --once: every shape once
through the call, nothing timed (for a kernel trace).
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

# type -> (key dtype the library sees, the view torch computes with, key bytes, value dtype of the pairs form)
TYPES = {"u32": (torch.uint32, torch.int32, 4, torch.int32), "f32": (torch.float32, torch.float32, 4, torch.int32),
         "i64": (torch.int64, torch.int64, 8, torch.float64)}
DEFAULT_SHAPES = ("mask:u32:28:2;mask:u32:28:64;mask:u32:28:1;pairs:u32:28:2;pairs:u32:28:64;pairs:u32:28:1;range:f32:28;"
                  "pairs:i64:26:2;partition:u32:28:2;mask:u32:16:2;nonzero:u32:28:2;nonzero:u32:16:2")


def make_inputs(tname, n, density):
    _kdt, view, kb, vdt = TYPES[tname]
    g = torch.Generator(device="cuda")
    g.manual_seed(n % 1000 + kb + density)
    if tname == "f32":
        x = torch.randn(n, dtype=torch.float32, device="cuda", generator=g)
    elif kb == 4:
        x = torch.randint(0, 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    else:
        x = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g)
    mask = torch.ones(n, dtype=torch.bool, device="cuda") if density == 1 else \
        torch.randint(0, density, (n,), dtype=torch.int32, device="cuda", generator=g) == 0
    vals = torch.arange(n, device="cuda").to(vdt)
    return x, mask, vals


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


def run_shape(form, tname, logn, density, ctx, reps, warmup, once):
    kdt, _view, kb, _vdt = TYPES[tname]
    n = 1 << logn
    x, mask, vals = make_inputs(tname, n, density)
    keys = x.view(kdt)
    vb = vals.element_size()
    num = torch.empty((), dtype=torch.int64, device="cuda")
    lo = None
    if form == "range":
        lo = x[:1 << 16].median().reshape(1).view(kdt)  # about half the rows pass
        sel = x >= x[:1 << 16].median()
    else:
        sel = mask
    kept_rows = int(sel.sum())
    kept = {}
    if form == "nonzero":
        out = (torch.empty(n, dtype=torch.int64, device="cuda"), num)
        cols_in, cols_out, pred = 1, 8, 1

        def call():
            kept["call"] = rs.radix_nonzero(mask, out=out, ctx=ctx)

        def yard():
            kept["nonzero"] = torch.nonzero(mask)

        ways, yardstick = {"call": call, "nonzero": yard}, "nonzero"
    else:
        pairs, part = form == "pairs", form == "partition"
        out = rs.Compacted(torch.empty(n, dtype=kdt, device="cuda"), torch.empty_like(vals) if pairs else None,
                           torch.empty(n, dtype=torch.int64, device="cuda") if pairs else None, num)
        pred = kb if form == "range" else 1
        cols_in = kb + (0 if form == "range" else 1) + (vb if pairs else 0)
        cols_out = kb + (vb + 8 if pairs else 0)

        def call():
            kept["call"] = rs.radix_compact(keys, mask=None if form == "range" else mask, lo=lo, values=vals if pairs else None,
                                            partition=part, out=out, ctx=ctx)

        def index():
            m = x >= lo.view(x.dtype) if form == "range" else mask
            if part:
                kept["index"] = torch.cat((x[m], x[~m]))
            elif pairs:
                kept["index"] = (x[m], vals[m], torch.nonzero(m))
            else:
                kept["index"] = x[m]

        def select():
            kept["select"] = torch.masked_select(x, mask)

        def nonzero():
            kept["nonzero"] = torch.nonzero(mask)

        ways, yardstick = {"call": call, "index": index}, "index"
        if form == "mask":
            ways.update(select=select, nonzero=nonzero)
    written = n if form == "partition" else kept_rows
    nbytes = n * pred + n * cols_in + written * cols_out
    floor_src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")  # a copy reads and writes: half the bytes each way
    floor_dst = torch.empty_like(floor_src)
    ways["copy"] = lambda: floor_dst.copy_(floor_src)
    rec = {"call": "radix_nonzero" if form == "nonzero" else "radix_compact", "form": form, "type": tname, "log2n": logn, "density": f"1/{density}",
           "kept": kept_rows, "key_bytes": kb, "reps": reps}
    if once:
        call()
        ctx.check()
        rec["once"] = True
        return rec
    times = time_ways(ways, ctx, reps, warmup)
    m = int(num)
    agree = m == kept_rows
    if form == "nonzero":
        agree = agree and bool(torch.equal(kept["call"][0][:m], kept["nonzero"].flatten()))
    elif form == "partition":
        agree = agree and bool(torch.equal(out.keys.view(x.dtype), kept["index"]))
    elif form == "pairs":
        agree = agree and bool(torch.equal(out.keys.view(x.dtype)[:m], kept["index"][0]) and torch.equal(out.values[:m], kept["index"][1])
                               and torch.equal(out.index[:m], kept["index"][2].flatten()))
    else:
        agree = agree and bool(torch.equal(out.keys.view(x.dtype)[:m], kept["index"]))
    kept.clear()
    for w, v in times.items():
        rec[w + "_ms"] = round(median(v), 4)
        rec[w + "_min_ms"] = round(min(v), 4)
        rec[w + "_max_ms"] = round(max(v), 4)
    rec["yardstick"] = yardstick
    rec["bytes"] = nbytes
    rec["frac_of_8TBps"] = round(nbytes / 8e12 * 1e3 / rec["call_ms"], 3)
    rec["call_vs_yardstick"] = round(rec[yardstick + "_ms"] / rec["call_ms"], 2)
    rec["slower_than_torch"] = bool(rec["call_ms"] > rec[yardstick + "_ms"])
    rec["agrees"] = agree
    rec["caps"] = rs.compact_caps(kb if form != "nonzero" else 0, vb if form == "pairs" else 0, 8 if form in ("pairs", "nonzero") else 0)
    rec["library"] = os.path.basename(rs._lib.lib_path())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="form:type:log2n[:d], mask density 1/d, separated by ;")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    ap.add_argument("--once", action="store_true", help="every shape once through the call, nothing timed")
    a = ap.parse_args()
    ctx = rs.Context(torch.cuda.current_device())
    sink = open(a.json, "a") if a.json else None
    for shape in [x for x in a.shapes.split(";") if x]:
        f = shape.split(":")
        rec = run_shape(f[0], f[1], int(f[2]), int(f[3]) if len(f) > 3 else 2, ctx, a.reps, a.warmup, a.once)
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
