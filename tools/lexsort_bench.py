"""Time of the sort by several key columns (rsx_lexsort_device: radix_lexsort) beside the other ways to get the same
permutation.

    python tools/lexsort_bench.py [--workloads "u32-u32;i64-i32;i64-i64-i32"] [--log2n 0] [--reps 10] [--warmup 2]
                                  [--ways "lexsort_ms;pack_ms"] [--json profiles/lexsort_bench.jsonl]

Workloads (columns generated on the device; column 0 is the most significant, all ascending):
  u32-u32       2^28 rows of (u32 uniform over 2^16 values, u32 of any bits): one round, an 8-byte compound key
  i64-i32       2^26 rows of (i64 uniform over n / 4 values, i32 of any bits): one round, 12 key bytes in a 16-byte key
  i64-i64-i32   2^26 rows of (i64 over 2^10 values, i64 over n / 4 values, i32 of any bits): two rounds
--log2n K runs every workload at 2^K rows instead; --ways keeps the named ways only (a kernel trace of two of them).

One JSON line per workload with the median device time (HIP events around the call alone, warm-up first; the ways
alternate within a repetition, the protocol of tools/reduce_bench.py; a fresh context and an emptied allocator cache per
workload) of

  lexsort_ms   radix_lexsort(columns) into an int64 index made outside the events
  pack_ms      u32-u32 only, where the columns fit one integer: a << 32 | b with torch operations into a fresh int64
               column, then radix_argsort of it
  chain_ms     what a caller writes today with this library: radix_argsort of the last column, then for every earlier
               column a gather through the permutation and radix_sort_pairs(gathered, permutation)
  torch_ms     the same chain with torch.sort(stable=True); torch sorts no u32, so those columns go as their int32 views
               (another order, the same work)
  argsort_ms   radix_argsort of ONE column as wide as the compound key of the widest round (u64 or 128-bit keys of any
               bits): the floor the sort alone sets for one round
with the smallest and largest repetition of lexsort_ms and pack_ms (their own spread), and the ratios lexsort_vs_pack =
lexsort_ms / pack_ms, chain_vs_lexsort = chain_ms / lexsort_ms and torch_vs_lexsort = torch_ms / lexsort_ms.  The
permutations of lexsort, chain and pack are compared for equality before anything is reported.
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

# workload -> (column kinds, default log2 n, bytes of the widest round's compound key)
WORKLOADS = {
    "u32-u32": (("u32:2^16", "u32:any"), 28, 8),
    "i64-i32": (("i64:n/4", "i32:any"), 26, 16),
    "i64-i64-i32": (("i64:2^10", "i64:n/4", "i32:any"), 26, 16),
}


def make_column(kind, n, g):
    if kind == "u32:2^16":
        return torch.randint(0, 1 << 16, (n,), dtype=torch.int32, device="cuda", generator=g).view(torch.uint32)
    if kind in ("u32:any", "i32:any"):
        x = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device="cuda", generator=g)
        return x.view(torch.uint32) if kind[0] == "u" else x
    if kind == "i64:2^10":
        return torch.randint(-512, 512, (n,), dtype=torch.int64, device="cuda", generator=g)
    assert kind == "i64:n/4"
    return torch.randint(0, max(1, n // 4), (n,), dtype=torch.int64, device="cuda", generator=g) - n // 8


def signed_view(t):
    return t.view(torch.int32) if t.dtype == torch.uint32 else t


def run_workload(name, k, reps, warmup, only=None):
    kinds, _k, width = WORKLOADS[name]
    n = 1 << k
    ctx = rs.Context(torch.cuda.current_device())
    st = torch.cuda.current_stream()
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED000B)
    cols = [make_column(kind, n, g) for kind in kinds]
    views = [signed_view(c) for c in cols]
    if width == 8:
        wide = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=g).view(torch.uint64)
    else:
        wide = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    out_wide = torch.empty(n, dtype=torch.int64, device="cuda")
    box = {}

    def lexsort():
        rs.radix_lexsort(cols, out=out, ctx=ctx)

    def pack():
        packed = (views[0].to(torch.int64) << 32) | (views[1].to(torch.int64) & 0xFFFFFFFF)
        box["pack"] = rs.radix_argsort(packed, ctx=ctx)

    def chain():
        perm = rs.radix_argsort(cols[-1], ctx=ctx)
        for c in cols[-2::-1]:
            gathered = c[perm] if c.dtype != torch.uint32 else c.view(torch.int32)[perm].view(torch.uint32)
            rs.radix_sort_pairs(gathered, perm, ctx=ctx)
        box["chain"] = perm

    def chain_torch():
        perm = torch.sort(views[-1], stable=True).indices
        for c in views[-2::-1]:
            perm = perm[torch.sort(c[perm], stable=True).indices]
        box["torch"] = perm

    def argsort():
        rs.radix_argsort(wide, out=out_wide, ctx=ctx)

    ways = {"lexsort_ms": lexsort, "chain_ms": chain, "torch_ms": chain_torch, "argsort_ms": argsort}
    if name == "u32-u32":
        ways["pack_ms"] = pack
    if only:
        ways = {w: fn for w, fn in ways.items() if w in only}
    times = {w: [] for w in ways}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            t = timed(fn, st)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    if "lexsort_ms" in ways and "chain" in box:
        assert torch.equal(out, box["chain"]), "radix_lexsort and the chain of stable sorts disagree"
    if "lexsort_ms" in ways and "pack" in box:
        assert torch.equal(out, box["pack"]), "radix_lexsort and the argsort of the packed column disagree"
    plan = rs.lex_plan([(c.element_size(), rs.KEY_UNSIGNED if c.dtype == torch.uint32 else rs.KEY_SIGNED) for c in cols])
    rec = {"workload": name, "log2n": k, "columns": list(kinds), "rounds": len(plan), "round_elem_bytes": [p[2] for p in plan],
           "argsort_key_bytes": width, "reps": reps}
    for w, v in times.items():
        rec[w] = round(median(v), 4)
    for w in ("lexsort_ms", "pack_ms"):
        if w in times:
            rec[w[:-3] + "_min_ms"] = round(min(times[w]), 4)
            rec[w[:-3] + "_max_ms"] = round(max(times[w]), 4)
    if "pack_ms" in rec and "lexsort_ms" in rec:
        rec["lexsort_vs_pack"] = round(rec["lexsort_ms"] / rec["pack_ms"], 3)
    for w, key, digits in (("chain_ms", "chain_vs_lexsort", 2), ("torch_ms", "torch_vs_lexsort", 2)):
        if w in rec and "lexsort_ms" in rec:
            rec[key] = round(rec[w] / rec["lexsort_ms"], digits)
    if "argsort_ms" in rec and "lexsort_ms" in rec:
        rec["lexsort_vs_argsort"] = round(rec["lexsort_ms"] / rec["argsort_ms"], 3)
    rec["library"] = os.path.basename(rs._lib.lib_path())
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=";".join(WORKLOADS))
    ap.add_argument("--log2n", type=int, default=0, help="every workload at 2^K rows (0: each at its own size)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ways", default="", help="only these ways, separated by ';' (default: all)")
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()
    sink = open(a.json, "a") if a.json else None
    for name in [x for x in a.workloads.split(";") if x]:
        rec = run_workload(name, a.log2n or WORKLOADS[name][1], a.reps, a.warmup, [w for w in a.ways.split(";") if w])
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
