"""Time of the merge call (rsx_merge_device: radix_merge / radix_merge_pairs) beside the two routes a caller had before it.

    python tools/merge_bench.py [--shapes "u32:27:27;u32v:27:27;..."] [--keys "interleaved;a_below_b"] [--reps 9] [--warmup 3]
                                [--json profiles/merge_bench.jsonl]

A shape is row:log2(na):log2(nb); the rows: u32 (keys alone), u32v (u32 keys with u32 values), i64v (i64 keys with f32
values).  The keys: `interleaved`, a and b alternate one by one in the output (b's keys spread evenly over a's range when b
is the shorter), or `a_below_b`, every key of a below every key of b (whole tiles from one side).  One JSON line per shape
with, for each way, the median, the smallest and the largest device time of --reps runs (HIP events around the call alone,
warm-up first; the ways alternate within a repetition, the protocol of tools/unique_bench.py):

  merge        radix_merge / radix_merge_pairs into preallocated outputs
  cat_sort     torch.cat of keys (and values), then radix_sort / radix_sort_pairs in place: the only route before the merge
  torch_sort   torch.sort(torch.cat(keys), stable=True), then values = torch.cat(values)[index]

and bytes = 2 * n * (key_bytes + value_bytes), what a merge has to move, with roofline_ms = bytes / 8 TB/s and
frac_of_8TBps = roofline_ms / merge_ms.  faster_beyond_spread: the slowest merge run was faster than the fastest cat_sort
run.  The u32 keys are drawn below 2^31 so that the signed view torch sorts orders them the same way.
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

# row -> (key dtype the library sees, the signed view torch sorts, key bytes, value dtype or None)
ROWS = {
    "u32": (torch.uint32, torch.int32, 4, None),
    "u32v": (torch.uint32, torch.int32, 4, torch.int32),
    "i64v": (torch.int64, torch.int64, 8, torch.float32),
}
DEFAULT_SHAPES = "u32:27:27;u32v:27:27;u32:28:20;u32v:28:20;i64v:26:26;u32:16:16;u32v:16:16"


def make_keys(view, na, nb, kind):
    """(a, b): each ascending, as the signed view."""
    ia = torch.arange(na, dtype=torch.int64, device="cuda")
    ib = torch.arange(nb, dtype=torch.int64, device="cuda")
    if kind == "a_below_b":
        return ia.to(view), (ib + na).to(view)
    if na >= nb:
        return (2 * ia).to(view), (2 * (ib * (na // nb)) + 1).to(view)
    return (2 * (ia * (nb // na))).to(view), (2 * ib + 1).to(view)


def run_shape(row, ka, kb_, kind, ctx, reps, warmup):
    kdt, view, kbytes, vdt = ROWS[row]
    na, nb = 1 << ka, 1 << kb_
    n = na + nb
    st = torch.cuda.current_stream()
    a, b = make_keys(view, na, nb, kind)
    ak, bk = a.view(kdt), b.view(kdt)
    out_k = torch.empty(n, dtype=kdt, device="cuda")
    vbytes = 0
    if vdt is not None:
        av = torch.arange(na, device="cuda").to(vdt)
        bv = -torch.arange(nb, device="cuda").to(vdt) - 1
        out_v = torch.empty(n, dtype=vdt, device="cuda")
        vbytes = av.element_size()
    kept = {}

    def merge():
        if vdt is None:
            rs.radix_merge(ak, bk, out=out_k, ctx=ctx)
        else:
            rs.radix_merge_pairs(ak, av, bk, bv, out=(out_k, out_v), ctx=ctx)

    def cat_sort():
        k = torch.cat((a, b)).view(kdt)  # (the copy is part of the route)
        if vdt is None:
            rs.radix_sort(k, ctx=ctx)
            kept["cat_sort"] = (k, None)
        else:
            v = torch.cat((av, bv))
            rs.radix_sort_pairs(k, v, ctx=ctx)
            kept["cat_sort"] = (k, v)

    def torch_sort():
        k, i = torch.sort(torch.cat((a, b)), stable=True)
        kept["torch_sort"] = (k, torch.cat((av, bv))[i] if vdt is not None else None)

    ways = {"merge": merge, "cat_sort": cat_sort, "torch_sort": torch_sort}
    times = {w: [] for w in ways}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            t = timed(fn, st)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    agree = True
    for w in ("cat_sort", "torch_sort"):
        k, v = kept[w]
        agree = agree and bool(torch.equal(out_k.view(view), k.view(view))) and (v is None or bool(torch.equal(out_v, v)))
    kept.clear()
    rec = {"row": row, "log2na": ka, "log2nb": kb_, "keys": kind, "key_bytes": kbytes, "value_bytes": vbytes, "reps": reps}
    for w, v in times.items():
        rec[w + "_ms"] = round(median(v), 4)
        rec[w + "_min_ms"] = round(min(v), 4)
        rec[w + "_max_ms"] = round(max(v), 4)
    rec["bytes"] = 2 * n * (kbytes + vbytes)
    rec["roofline_ms"] = round(rec["bytes"] / 8e12 * 1e3, 4)
    rec["frac_of_8TBps"] = round(rec["roofline_ms"] / rec["merge_ms"], 3)
    rec["merge_vs_cat_sort"] = round(rec["cat_sort_ms"] / rec["merge_ms"], 2)
    rec["merge_vs_torch_sort"] = round(rec["torch_sort_ms"] / rec["merge_ms"], 2)
    rec["faster_beyond_spread"] = bool(rec["merge_max_ms"] < rec["cat_sort_min_ms"])
    rec["agrees"] = agree
    rec["tile"] = rs.merge_caps(kbytes, vbytes)
    rec["library"] = os.path.basename(rs._lib.lib_path())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="row:log2na:log2nb, separated by ;")
    ap.add_argument("--keys", default="interleaved;a_below_b")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()
    ctx = rs.Context(torch.cuda.current_device())
    sink = open(a.json, "a") if a.json else None
    for shape in [x for x in a.shapes.split(";") if x]:
        row, ka, kb_ = shape.split(":")
        for kind in [x for x in a.keys.split(";") if x]:
            rec = run_shape(row, int(ka), int(kb_), kind, ctx, a.reps, a.warmup)
            line = json.dumps(rec)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
