"""Time of the order-statistics call (rsx_select_device: radix_select) beside the routes a caller had before it.

    python tools/select_bench.py [--shapes "u32:28:uniform:1;u32:28:uniform:max;..."] [--reps 9] [--warmup 3]
                                 [--json profiles/select_bench.jsonl] [--once]

A shape is type:log2(n):input:ranks; the types: u32, f32, i64; the inputs: `uniform` (all bits random), `vals16` (2^16 distinct
values), `equal` (all keys equal: the candidates are never compacted); ranks: 1 (the median) or `max` (select_caps' max_ranks
ranks spread over the array).  One JSON line per shape with, for each way, the median, the smallest and the largest device
time of --reps runs (HIP events around the call alone, warm-up first; the ways alternate within a repetition, the protocol
of tools/unique_bench.py):

  select        radix_select, values only
  select_index  radix_select(return_index=True)
  argsort       radix_argsort, then the elements at the ranks gathered through the permutation
  clone_sort    keys.clone(), radix_sort in place, the ranks indexed
  kthvalue      torch.kthvalue (one rank, dtypes torch takes; no tie rule)

bytes_value = n * key_bytes and bytes_index = 2 * n * key_bytes are what the call HAS to move for the value and with the
index; frac_value_of_8TBps = bytes_value / 8 TB/s / select_ms and frac_index_of_8TBps likewise: the share of the nominal
memory rate the call reaches on those bytes (it reads more: one pass per level until the candidates are compacted).
faster_beyond_spread: the slowest select run was faster than the fastest clone_sort run.  compacted: bits 8-11 of
RSX_INFO_LAST_PASSES after the call (0: never, else 1 + the level).  --once: every shape once through radix_select with the
index, nothing timed (for a kernel trace).
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

# type -> (key dtype the library sees, the view torch indexes and sorts, key bytes)
TYPES = {"u32": (torch.uint32, torch.int32, 4), "f32": (torch.float32, torch.float32, 4), "i64": (torch.int64, torch.int64, 8)}
DEFAULT_SHAPES = "u32:28:uniform:1;u32:28:uniform:max;f32:28:uniform:1;i64:26:uniform:1;u32:28:vals16:1;u32:28:equal:1;u32:16:uniform:1"


def make_keys(tname, n, kind):
    kdt, view, kb = TYPES[tname]
    g = torch.Generator(device="cuda")
    g.manual_seed(n % 1000 + kb)
    if kind == "equal":
        return torch.full((n,), 12345, dtype=view, device="cuda")
    if kind == "vals16":
        return (torch.randint(0, 1 << 16, (n,), dtype=torch.int64, device="cuda", generator=g) * 32749).to(view)  # (below 2^31)
    if tname == "f32":
        return torch.randn(n, dtype=torch.float32, device="cuda", generator=g)
    if kb == 4:
        return torch.randint(0, 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)  # below 2^31: the signed view orders alike
    return torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g)


def run_shape(tname, logn, kind, nranks, ctx, reps, warmup, once):
    kdt, view, kb = TYPES[tname]
    n = 1 << logn
    st = torch.cuda.current_stream()
    x = make_keys(tname, n, kind)
    keys = x.view(kdt)
    m = rs.select_caps(kb)[0] if nranks == "max" else 1
    ranks = [(n - 1) // 2] if m == 1 else [(2 * i + 1) * n // (2 * m) for i in range(m)]
    at = torch.tensor(ranks, dtype=torch.int64, device="cuda")
    kept = {}

    def select():
        kept["select"] = rs.radix_select(keys, ranks, ctx=ctx)

    def select_index():
        kept["select_index"] = rs.radix_select(keys, ranks, return_index=True, ctx=ctx)

    def argsort():
        p = rs.radix_argsort(keys, ctx=ctx)[at]
        kept["argsort"] = (x[p], p)

    def clone_sort():
        c = x.clone()
        rs.radix_sort(c.view(kdt), ctx=ctx)
        kept["clone_sort"] = c[at]

    def kthvalue():
        kept["kthvalue"] = torch.kthvalue(x, ranks[0] + 1).values

    if once:
        select_index()
        ctx.check()
        return {"type": tname, "log2n": logn, "input": kind, "ranks": m, "once": True}
    ways = {"select": select, "select_index": select_index, "argsort": argsort, "clone_sort": clone_sort}
    if m == 1:
        try:
            kthvalue()
            ways["kthvalue"] = kthvalue
        except RuntimeError:  # an input torch.kthvalue does not take
            pass
    times = {w: [] for w in ways}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            t = timed(fn, st)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    select_index()
    ctx.check()
    compacted = (ctx.get_info(rs.INFO_LAST_PASSES) >> 8) & 0xF
    sv, si = kept["select_index"]
    av, ai = kept["argsort"]
    agree = bool(torch.equal(sv.view(view), av)) and bool(torch.equal(si, ai)) and bool(torch.equal(kept["select"].view(view), kept["clone_sort"]))
    if "kthvalue" in kept and tname != "f32":
        agree = agree and bool(torch.equal(kept["kthvalue"].reshape(1), av))
    kept.clear()
    rec = {"type": tname, "log2n": logn, "input": kind, "ranks": m, "key_bytes": kb, "reps": reps, "compacted": compacted}
    for w, v in times.items():
        rec[w + "_ms"] = round(median(v), 4)
        rec[w + "_min_ms"] = round(min(v), 4)
        rec[w + "_max_ms"] = round(max(v), 4)
    rec["bytes_value"] = n * kb
    rec["bytes_index"] = 2 * n * kb
    rec["frac_value_of_8TBps"] = round(rec["bytes_value"] / 8e12 * 1e3 / rec["select_ms"], 3)
    rec["frac_index_of_8TBps"] = round(rec["bytes_index"] / 8e12 * 1e3 / rec["select_index_ms"], 3)
    rec["select_vs_clone_sort"] = round(rec["clone_sort_ms"] / rec["select_ms"], 2)
    rec["select_index_vs_argsort"] = round(rec["argsort_ms"] / rec["select_index_ms"], 2)
    rec["faster_beyond_spread"] = bool(rec["select_max_ms"] < rec["clone_sort_min_ms"])
    rec["agrees"] = agree
    rec["caps"] = rs.select_caps(kb)
    rec["library"] = os.path.basename(rs._lib.lib_path())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="type:log2n:input:ranks, separated by ;")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    ap.add_argument("--once", action="store_true", help="every shape once, with the index, nothing timed")
    a = ap.parse_args()
    ctx = rs.Context(torch.cuda.current_device())
    sink = open(a.json, "a") if a.json else None
    for shape in [x for x in a.shapes.split(";") if x]:
        tname, logn, kind, nranks = shape.split(":")
        rec = run_shape(tname, int(logn), kind, nranks, ctx, a.reps, a.warmup, a.once)
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
