"""Time of the join call (rsx_join_device: radix_join on sorted inputs) beside the chain a caller wrote before it.

    python tools/join_bench.py [--shapes "u32:26:26:pairs;..."] [--reps 9] [--warmup 3] [--json profiles/join_bench.jsonl]

A shape is row:log2(na):log2(nb):keys; the rows: u32, i64 (keys alone, int64 positions out).  The keys, both arrays
ascending: `pairs`, distinct keys, every second key of a present once in b (c in {0, 1}); `dup2`, every key twice in a and
twice in b (four rows a key); `skew`, a's keys distinct and half of b one run of a single key of a (one key of a fans out
into nb / 2 rows) while the other half matches as in `pairs`.  One JSON line per shape with, for each way, the median, the
smallest and the largest device time of --reps runs (HIP events around the call alone, warm-up first; the ways alternate
within a repetition, the protocol of tools/merge_bench.py):

  join    radix_join(a, b, "inner", assume_sorted=True, out=(left, right)) into preallocated outputs; the count stays on
          the device
  chain   what a caller wrote before: radix_searchsorted(b, a, side="both"), the counts and torch.cumsum,
          torch.repeat_interleave with output_size given (so that it does not synchronise: the number of rows is handed in,
          which a real caller would have had to read back first), and the arithmetic for the right-hand positions

and bytes = (na + nb) * key_bytes + 2 * 8 * T, what the call has to move at least, with roofline_ms = bytes / 8 TB/s and
frac_of_8TBps = roofline_ms / join_ms.  join_vs_chain = chain_ms / join_ms.  faster_beyond_spread: the slowest join run was
faster than the fastest chain run.  The u32 keys stay below 2^31 so that the signed view torch builds them in orders alike.
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

# row -> (key dtype the library sees, the signed view torch builds, key bytes)
ROWS = {"u32": (torch.uint32, torch.int32, 4), "i64": (torch.int64, torch.int64, 8)}
DEFAULT_SHAPES = "u32:26:26:pairs;u32:25:25:dup2;u32:26:24:skew;i64:25:25:pairs;u32:26:20:pairs;u32:16:16:pairs"


def make_keys(view, na, nb, kind):
    """(a, b): each ascending, as the signed view."""
    ia = torch.arange(na, dtype=torch.int64, device="cuda")
    ib = torch.arange(nb, dtype=torch.int64, device="cuda")
    if kind == "pairs":
        return ia.to(view), (2 * ib).to(view)
    if kind == "dup2":
        return (ia // 2).to(view), (ib // 2).to(view)
    if kind == "skew":
        run = torch.full((nb // 2,), na // 2, dtype=torch.int64, device="cuda")
        return ia.to(view), torch.sort(torch.cat([run, 2 * ib[:nb - nb // 2]])).values.to(view)
    raise ValueError(kind)


def run_shape(row, ka, kb_, kind, ctx, reps, warmup):
    kdt, view, kbytes = ROWS[row]
    na, nb = 1 << ka, 1 << kb_
    st = torch.cuda.current_stream()
    a, b = make_keys(view, na, nb, kind)
    ak, bk = a.view(kdt), b.view(kdt)
    T = int(rs.radix_join(ak, bk, "inner", assume_sorted=True, capacity=0, ctx=ctx).num)  # the count-only call, read once
    left = torch.empty(T, dtype=torch.int64, device="cuda")
    right = torch.empty(T, dtype=torch.int64, device="cuda")
    rows_a = torch.arange(na, dtype=torch.int64, device="cuda")
    rows_t = torch.arange(T, dtype=torch.int64, device="cuda")
    kept = {}

    def join():
        kept["join"] = rs.radix_join(ak, bk, "inner", assume_sorted=True, out=(left, right), ctx=ctx)

    def chain():
        lo, hi = rs.radix_searchsorted(bk, ak, side="both", presort=False, ctx=ctx)
        cnt = hi - lo
        start = torch.cumsum(cnt, 0) - cnt
        li = torch.repeat_interleave(rows_a, cnt, output_size=T)
        kept["chain"] = (li, lo[li] + (rows_t - start[li]))

    ways = {"join": join, "chain": chain}
    times = {w: [] for w in ways}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            t = timed(fn, st)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    cl, cr = kept["chain"]
    agree = int(kept["join"].num) == T and bool(torch.equal(left, cl)) and bool(torch.equal(right, cr))
    kept.clear()
    rec = {"row": row, "log2na": ka, "log2nb": kb_, "keys": kind, "key_bytes": kbytes, "index_bytes": 8, "rows": T, "reps": reps}
    for w, v in times.items():
        rec[w + "_ms"] = round(median(v), 4)
        rec[w + "_min_ms"] = round(min(v), 4)
        rec[w + "_max_ms"] = round(max(v), 4)
    rec["bytes"] = (na + nb) * kbytes + 16 * T
    rec["roofline_ms"] = round(rec["bytes"] / 8e12 * 1e3, 4)
    rec["frac_of_8TBps"] = round(rec["roofline_ms"] / rec["join_ms"], 3)
    rec["join_vs_chain"] = round(rec["chain_ms"] / rec["join_ms"], 2)
    rec["faster_beyond_spread"] = bool(rec["join_max_ms"] < rec["chain_min_ms"])
    rec["chain_is_told_the_count"] = True
    rec["agrees"] = agree
    rec["caps"] = list(rs.join_caps(kbytes))
    rec["library"] = os.path.basename(rs._lib.lib_path())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="row:log2na:log2nb:keys, separated by ;")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()
    ctx = rs.Context(torch.cuda.current_device())
    sink = open(a.json, "a") if a.json else None
    for shape in [x for x in a.shapes.split(";") if x]:
        row, ka, kb_, kind = shape.split(":")
        rec = run_shape(row, int(ka), int(kb_), kind, ctx, a.reps, a.warmup)
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
