"""Time of radix_topk beside the two other ways to get the k best of every row.

    python tools/topk_bench.py [--shapes "rows_1024;rows_4096;flat_24;flat_28"] [--reps 10] [--warmup 2]
                               [--shrink K] [--json profiles/topk_bench.jsonl]

Shapes:
  rows_1024  131072 x 1024 f32, k = 64
  rows_4096  32768 x 4096 u32, k = 128
  flat_24    1 x 2^24 f32, k = 64
  flat_28    1 x 2^28 f32, k = 1024
--shrink K divides the number of rows (flat shapes: the length) by 2^K (a rehearsal; not a measurement).

One JSON line per shape with, per way, the median, the least and the greatest device time over --reps repetitions (HIP
events around the call alone, on the same seeded input, which no way modifies; the ways alternate inside every
repetition, --warmup repetitions first):
  topk        rs.radix_topk(keys, k): the select kernel (rsx_topk_rows_device), forced even where radix_topk would route
              the shape to the sort
  sort_slice  what a caller wrote before it, from the same build: radix_argsort_rows(keys, descending=True)[..., :k]
              (flat: radix_argsort) made contiguous, and the gather of the values through it
  torch       torch.topk(keys, k, sorted=True)
`spread` is (max - min) / median of a way's repetitions.  The condition the select has to meet on a shape: its median is
no longer than sort_slice's (`topk_vs_sort_slice` <= 1); where it is not, radix_topk sends that shape class to the sort
(radix_sort_amd/api.py, _topk_by_sort).  `routed` says what radix_topk does with the shape as built.
The topk and sort_slice results are compared bit for bit, and the values with torch's, before anything is timed.
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
from radix_sort_amd import api  # noqa: E402

SHAPES = {"rows_1024": (131072, 1024, "f32", 64), "rows_4096": (32768, 4096, "u32", 128), "flat_24": (1, 1 << 24, "f32", 64),
          "flat_28": (1, 1 << 28, "f32", 1024)}


def timed(fn, st):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4), "spread": round((v[-1] - v[0]) / med, 3)}


def run_shape(name, rows, L, dtype, k, ctx, reps, warmup):
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED0007)
    flat = rows == 1
    shape = (L,) if flat else (rows, L)
    if dtype == "f32":
        keys = torch.randn(shape, dtype=torch.float32, device="cuda", generator=g)
        tkeys = keys
    else:  # keys below 2^31: torch orders their int32 view the same way
        tkeys = torch.randint(0, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda", generator=g)
        keys = tkeys.view(torch.uint32)
    st = torch.cuda.current_stream()
    state = {}
    routed = api._topk_by_sort(rows, L, k, 4)
    by_sort = api._topk_by_sort

    def topk():
        api._topk_by_sort = lambda *a: False  # the select itself, whatever the routing says
        try:
            state["topk"] = rs.radix_topk(keys, k, ctx=ctx)
        finally:
            api._topk_by_sort = by_sort

    def sort_slice():
        full = rs.radix_argsort(keys, descending=True, ctx=ctx) if flat else rs.radix_argsort_rows(keys, descending=True, ctx=ctx)
        idx = full[..., :k].contiguous()
        state["sort_slice"] = (torch.gather(tkeys, -1, idx), idx)

    def torch_topk():
        state["torch"] = torch.topk(tkeys, k, dim=-1, largest=True, sorted=True)

    ways = {"topk": topk, "sort_slice": sort_slice, "torch": torch_topk}
    for fn in ways.values():
        fn()
    ctx.check()
    tv, ti = state["topk"]
    sv, si = state["sort_slice"]
    same = torch.equal(tv.view(torch.int32), sv.view(torch.int32)) and torch.equal(ti, si)
    same_torch = torch.equal(tv.view(torch.int32), state["torch"].values.view(torch.int32))  # (randn: no NaN; ties keep equal values)
    info = None
    topk()
    ctx.check()
    info = ctx.get_info(rs.INFO_LAST_PASSES)
    state.clear()
    times = {w: [] for w in ways}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            t = timed(fn, st)
            state.clear()
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    caps, max_k = rs.topk_caps(4)
    rec = {"shape": name, "rows": rows, "row_len": L, "dtype": dtype, "k": k, "reps": reps, "warmup": warmup, "results_equal": bool(same),
           "values_equal_torch": bool(same_torch), "caps": caps, "max_k": max_k, "path": (info >> 24) & 0xF, "launches": info & 0xFF,
           "routed": "sort" if routed else "select"}
    for w, v_ in times.items():
        rec[w + "_ms"] = stats(v_)
    rec["topk_vs_sort_slice"] = round(rec["topk_ms"]["median"] / rec["sort_slice_ms"]["median"], 3)
    rec["topk_vs_torch"] = round(rec["topk_ms"]["median"] / rec["torch_ms"]["median"], 3)
    rec["topk_key_GB_per_s"] = round(rows * L * 4 / rec["topk_ms"]["median"] / 1e6, 1)  # the key column, read once
    rec["library"] = os.path.basename(rs._lib.lib_path())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=";".join(SHAPES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shrink", type=int, default=0, help="divide the rows (flat: the length) by 2^K (rehearsal)")
    ap.add_argument("--run", default="", help="a label kept in every line (repetitions of the whole command)")
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    ctx = rs.Context(torch.cuda.current_device())
    sink = open(a.json, "a") if a.json else None
    for name in [x for x in a.shapes.split(";") if x]:
        rows, L, dtype, k = SHAPES[name]
        if rows == 1:
            L = max(k, L >> a.shrink)
        else:
            rows = max(1, rows >> a.shrink)
        rec = run_shape(name, rows, L, dtype, k, ctx, a.reps, a.warmup)
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
