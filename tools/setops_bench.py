"""Time of the set-operation call (rsx_setop_device: radix_set_op / radix_set_op_pairs) beside the chain a caller wrote
before it and beside the merge of the same inputs.

    python tools/setops_bench.py [--shapes "u32:27:27:intersection:half;..."] [--reps 9] [--warmup 3]
                                 [--json profiles/setops_bench.jsonl]

A shape is row:log2(na):log2(nb):op:keys; the rows: u32 (keys alone), u32v (u32 keys with u32 values), i64 (keys alone).
The keys: `half`, both arrays hold distinct keys, a's spread evenly and every second key of b equal to one of a's (b's keys
spread over a's range when b is the shorter), or `a_below_b`, every key of a below every key of b (nothing shared, whole
tiles from one side).  One JSON line per shape with, for each way, the median, the smallest and the largest device time of
--reps runs (HIP events around the call alone, warm-up first; the ways alternate within a repetition, the protocol of
tools/merge_bench.py):

  setop   radix_set_op / radix_set_op_pairs into preallocated outputs; the count stays on the device
  chain   intersection and difference: radix_searchsorted(b, a, side="both"), radix_searchsorted(a, a) for the rank inside a
          run of equal keys, the mask rank < upper - lower, and torch's boolean index; union: radix_merge, the mask of the
          keys that differ from their predecessor, and the boolean index.  The boolean index is timed too, and it
          SYNCHRONISES the host (chain_synchronises), which the events do not show
  merge   radix_merge of the same inputs: the floor, since a set operation does the merge's tile work twice and writes less

and bytes = (na + nb + num) * (key_bytes + value_bytes), what the call has to move at least, with roofline_ms = bytes /
8 TB/s and frac_of_8TBps = roofline_ms / setop_ms.  x_vs_y = y_ms / x_ms.  faster_beyond_spread: the slowest setop run was
faster than the fastest chain run.  The u32 keys stay below 2^31 so that the signed view torch compares orders them alike.
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

# row -> (key dtype the library sees, the signed view torch compares, key bytes, value dtype or None)
ROWS = {
    "u32": (torch.uint32, torch.int32, 4, None),
    "u32v": (torch.uint32, torch.int32, 4, torch.int32),
    "i64": (torch.int64, torch.int64, 8, None),
}
DEFAULT_SHAPES = ("u32:27:27:intersection:half;u32:27:27:intersection:a_below_b;u32:27:27:union:half;u32:27:27:union:a_below_b;"
                  "u32v:27:27:intersection:half;i64:26:26:difference:half;u32:28:20:intersection:half;u32:16:16:intersection:half")


def make_keys(view, na, nb, kind):
    """(a, b): each strictly ascending, as the signed view."""
    ia = torch.arange(na, dtype=torch.int64, device="cuda")
    ib = torch.arange(nb, dtype=torch.int64, device="cuda")
    if kind == "a_below_b":
        return ia.to(view), (ib + na).to(view)
    # a: the even numbers; b: every second key even (one of a's), the others odd
    sa, sb = max(1, nb // na), max(1, na // nb)
    return (2 * ia * sa).to(view), (2 * ib * sb + (ib & 1)).to(view)


def run_shape(row, ka, kb_, op, kind, ctx, reps, warmup):
    kdt, view, kbytes, vdt = ROWS[row]
    na, nb = 1 << ka, 1 << kb_
    st = torch.cuda.current_stream()
    a, b = make_keys(view, na, nb, kind)
    ak, bk = a.view(kdt), b.view(kdt)
    cap = min(na, nb) if op == "intersection" else na if op == "difference" else na + nb
    out_k = torch.empty(cap, dtype=kdt, device="cuda")
    merged = torch.empty(na + nb, dtype=kdt, device="cuda")
    vbytes = 0
    if vdt is not None:
        assert op in ("intersection", "difference"), "the chain moves values of a only"
        av = torch.arange(na, device="cuda").to(vdt)
        out_v = torch.empty(cap, dtype=vdt, device="cuda")
        vbytes = av.element_size()
    kept = {}

    def setop():
        if vdt is None:
            kept["setop"] = rs.radix_set_op(ak, bk, op, out=out_k, ctx=ctx)
        else:
            kept["setop"] = rs.radix_set_op_pairs(ak, av, bk, None, op, out=(out_k, out_v), ctx=ctx)

    def chain():
        if op == "union":
            m = rs.radix_merge(ak, bk, ctx=ctx).view(view)
            mask = torch.ones(na + nb, dtype=torch.bool, device="cuda")
            mask[1:] = m[1:] != m[:-1]
            kept["chain"] = (m[mask], None)  # (synchronises)
            return
        lower, upper = rs.radix_searchsorted(bk, ak, side="both", presort=False, ctx=ctx)
        first = rs.radix_searchsorted(ak, ak, presort=False, ctx=ctx)
        rank = torch.arange(na, dtype=torch.int64, device="cuda") - first
        mask = rank < upper - lower
        if op == "difference":
            mask = ~mask
        kept["chain"] = (a[mask], av[mask] if vdt is not None else None)  # (synchronises)

    def merge():
        rs.radix_merge(ak, bk, out=merged, ctx=ctx)

    ways = {"setop": setop, "chain": chain, "merge": merge}
    times = {w: [] for w in ways}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            t = timed(fn, st)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    num = int(kept["setop"].num)
    ck, cv = kept["chain"]
    agree = ck.numel() == num and bool(torch.equal(out_k.view(view)[:num], ck)) and (cv is None or bool(torch.equal(out_v[:num], cv)))
    kept.clear()
    rec = {"row": row, "log2na": ka, "log2nb": kb_, "op": op, "keys": kind, "key_bytes": kbytes, "value_bytes": vbytes, "num": num, "reps": reps}
    for w, v in times.items():
        rec[w + "_ms"] = round(median(v), 4)
        rec[w + "_min_ms"] = round(min(v), 4)
        rec[w + "_max_ms"] = round(max(v), 4)
    rec["bytes"] = (na + nb + num) * (kbytes + vbytes)
    rec["roofline_ms"] = round(rec["bytes"] / 8e12 * 1e3, 4)
    rec["frac_of_8TBps"] = round(rec["roofline_ms"] / rec["setop_ms"], 3)
    rec["setop_vs_chain"] = round(rec["chain_ms"] / rec["setop_ms"], 2)
    rec["setop_vs_merge"] = round(rec["merge_ms"] / rec["setop_ms"], 2)
    rec["faster_beyond_spread"] = bool(rec["setop_max_ms"] < rec["chain_min_ms"])
    rec["chain_synchronises"] = True
    rec["agrees"] = agree
    rec["tile"] = rs.setop_caps(kbytes)
    rec["library"] = os.path.basename(rs._lib.lib_path())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="row:log2na:log2nb:op:keys, separated by ;")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()
    ctx = rs.Context(torch.cuda.current_device())
    sink = open(a.json, "a") if a.json else None
    for shape in [x for x in a.shapes.split(";") if x]:
        row, ka, kb_, op, kind = shape.split(":")
        rec = run_shape(row, int(ka), int(kb_), op, kind, ctx, a.reps, a.warmup)
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
