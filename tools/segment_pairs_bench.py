"""Time of the fused per-row key / value sorts (radix_sort_rows_pairs, radix_argsort_rows) beside the other ways to get
the same result.

    python tools/segment_pairs_bench.py [--shapes "pairs_4096;argsort_1024;pairs_32"] [--reps 10] [--warmup 2]
                                        [--shrink K] [--json profiles/segment_pairs_bench.jsonl]

Shapes (the project's own segment shapes):
  pairs_4096    32768 x 4096 u32 keys + u32 values, both columns sorted along the rows
  argsort_1024  131072 x 1024 f32 keys, the int64 positions inside each row
  pairs_32      2^27 u32 keys + u32 values in rows of 32 (the known weak spot: one workgroup per row)
--shrink K divides the number of rows by 2^K (a rehearsal; not a measurement).

One JSON line per shape with, per way, the median, the least and the greatest device time over --reps repetitions (HIP
events around the call alone; every repetition on a fresh copy of the same seeded input; the ways alternate inside every
repetition, --warmup repetitions first):
  fused      the new call
  composed   what a caller had to write before it, through the public calls that existed: torch interleave into
             (key, value) elements, radix_sort_rows(digits=tuple_of(...)), torch de-interleave into the columns
  torch      torch.sort(keys, dim=-1), which returns values and indices (pairs: plus the gather that moves the values,
             reported separately as torch_gather)
and the bytes the fused LDS classes must move (every column read once and written once) over the fused time.
The fused and the composed results are compared bit for bit, and the keys with torch's, before anything is timed.
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

SHAPES = {"pairs_4096": ("pairs", 32768, 4096), "argsort_1024": ("argsort", 131072, 1024), "pairs_32": ("pairs", (1 << 27) // 32, 32)}


def timed(fn, st):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def run_shape(name, kind, rows, L, ctx, reps, warmup):
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED0004)
    n = rows * L
    st = torch.cuda.current_stream()
    if kind == "pairs":
        # keys below 2^31: torch sorts their int32 view in the same order
        k_src = torch.randint(0, 2 ** 31 - 1, (rows, L), dtype=torch.int32, device="cuda", generator=g)
        v_src = torch.randint(0, 2 ** 31 - 1, (rows, L), dtype=torch.int32, device="cuda", generator=g)
        k, v = torch.empty_like(k_src), torch.empty_like(v_src)
        elems = torch.empty((rows, L, 2), dtype=torch.int32, device="cuda")
        tmp = torch.empty_like(elems)
        d = rs.tuple_of("u32", 4)
        state = {}

        def fresh():
            k.copy_(k_src)
            v.copy_(v_src)

        def fused():
            rs.radix_sort_rows_pairs(k.view(torch.uint32), v, ctx=ctx)

        def composed():
            torch.stack((k, v), dim=-1, out=elems)
            rs.radix_sort_rows(elems.view(torch.uint8).view(rows, L * 8), digits=d, tmp=tmp.view(torch.uint8).view(rows, L * 8), ctx=ctx)
            k.copy_(elems[..., 0])
            v.copy_(elems[..., 1])

        def torch_sort():
            state["sorted"] = torch.sort(k, dim=-1)

        def torch_gather():
            s = torch.sort(k, dim=-1)
            state["moved"] = v.gather(-1, s.indices)

        ways = {"fused": fused, "composed": composed, "torch": torch_sort, "torch_gather": torch_gather}
        results = lambda: (k.clone(), v.clone())  # noqa: E731
        column_bytes = n * (4 + 4)
    else:
        k_src = torch.randn((rows, L), dtype=torch.float32, device="cuda", generator=g)
        k = torch.empty_like(k_src)
        out = torch.empty((rows, L), dtype=torch.int64, device="cuda")
        pos = torch.arange(L, dtype=torch.int32, device="cuda").expand(rows, L)
        elems = torch.empty((rows, L, 2), dtype=torch.int32, device="cuda")
        tmp = torch.empty_like(elems)
        d = rs.tuple_of("f32", 4)
        state = {}

        def fresh():
            k.copy_(k_src)

        def fused():
            rs.radix_argsort_rows(k, out=out, ctx=ctx)

        def composed():
            torch.stack((k.view(torch.int32), pos), dim=-1, out=elems)
            rs.radix_sort_rows(elems.view(torch.uint8).view(rows, L * 8), digits=d, tmp=tmp.view(torch.uint8).view(rows, L * 8), ctx=ctx)
            out.copy_(elems[..., 1])

        def torch_sort():
            state["sorted"] = torch.sort(k, dim=-1)

        ways = {"fused": fused, "composed": composed, "torch": torch_sort}
        results = lambda: (out.clone(),)  # noqa: E731
        column_bytes = n * (4 + 8)

    # the same result from the fused call and from the composition, bit for bit; torch agrees on the keys
    fresh()
    fused()
    ctx.check()
    got = results()
    fresh()
    composed()
    ctx.check()
    want = results()
    same = all(torch.equal(a, b) for a, b in zip(got, want))
    ts = torch.sort(k_src, dim=-1, stable=True)
    if kind == "pairs":
        same = same and torch.equal(got[0], ts.values)
    else:  # (randn has no NaN and a negligible chance of -0.0: the total order is torch's here)
        same = same and torch.equal(k_src.gather(-1, got[0]), ts.values)
    del got, want, ts
    times = {w: [] for w in ways}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            fresh()
            t = timed(fn, st)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    rec = {"shape": name, "kind": kind, "rows": rows, "row_len": L, "n": n, "reps": reps, "warmup": warmup, "results_equal": bool(same),
           "caps": rs.segment_pairs_caps(4, 4), "last_pairs": None}
    fresh()
    fused()
    ctx.check()
    rec["last_pairs"] = ctx.get_info(rs.INFO_LAST_PAIRS)
    for w, v_ in times.items():
        rec[w + "_ms"] = stats(v_)
    rec["fused_vs_composed"] = round(rec["fused_ms"]["median"] / rec["composed_ms"]["median"], 3)
    rec["fused_vs_torch"] = round(rec["fused_ms"]["median"] / rec["torch_ms"]["median"], 3)
    rec["fused_column_GB_per_s"] = round(2 * column_bytes / rec["fused_ms"]["median"] / 1e6, 1)  # every column read and written once
    rec["library"] = os.path.basename(rs._lib.lib_path())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=";".join(SHAPES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shrink", type=int, default=0, help="divide the number of rows by 2^K (rehearsal)")
    ap.add_argument("--run", default="", help="a label kept in every line (repetitions of the whole command)")
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    ctx = rs.Context(torch.cuda.current_device())
    sink = open(a.json, "a") if a.json else None
    for name in [x for x in a.shapes.split(";") if x]:
        kind, rows, L = SHAPES[name]
        rec = run_shape(name, kind, max(1, rows >> a.shrink), L, ctx, a.reps, a.warmup)
        rec["shrink"] = a.shrink
        if a.run:
            rec["run"] = a.run
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
