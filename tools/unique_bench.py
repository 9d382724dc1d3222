"""Time of the group calls (rsx_unique_device: radix_group) beside the other ways to get the same result.

    python tools/unique_bench.py [--rows "u32;i64"] [--log2n 24,28] [--dists "values16;full"] [--reps 10] [--warmup 2]
                                 [--json profiles/unique_bench.jsonl]

Keys uniform over 2^16 values (values16) or over the full range of the type (full), generated on the device.  One JSON
line per key type, size and distribution with the median device time (HIP events around the call alone, warm-up first;
the ways alternate within a repetition, the protocol of tools/pairs_bench.py) of

  group_all_ms   radix_group with every output (keys, offsets, perm, inverse; int64 indices)
  group_perm_ms  radix_group as it is called by default (keys, offsets, perm; no inverse, so no scatter)
  group_keys_ms  radix_group keys only (keys, offsets; the route without positions)
  argsort_ms     radix_argsort of the same input (int64 indices): group_all_ms - argsort_ms is the price of the three run
                 kernels with the split kernel saved
  torch_unique_ms  torch.unique(sorted=True, return_inverse=True, return_counts=True); torch has no unique of u32: its
                 signed view is taken instead (another order, the same work).  It synchronises inside; the events are
                 around the whole call
  torch_chain_ms what a caller writes today after radix_argsort: gather, compare with the shifted copy, cumsum, scatter
                 (and nonzero for the offsets, which synchronises)
  run_ms         the context's per-launch timing (rsx_ctx_profile, kind "scan") of radix_group with every output minus that
                 of radix_argsort: the sort's own scan launches are the same in both, what is left are the three run
                 kernels; run_bytes is what they read and write by the algorithm -- two reads of the sorted elements, m
                 keys and m + 1 offsets, n positions and n inverse entries -- and run_frac_of_8TBps = run_bytes / run_ms /
                 8e12.  run_perm_ms and its bytes: the same without the inverse; run_keys_ms and its bytes: the same for the
                 keys-only route against a keys-only descending sort
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

# row -> (torch key dtype, the view torch.unique takes, key bytes)
ROWS = {
    "u32": (torch.uint32, torch.int32, 4),
    "i64": (torch.int64, torch.int64, 8),
}
JOINED = {4: 8, 8: 16}  # (key, u32 position)


def make_keys(row, n, dist):
    kdt, view, kb = ROWS[row]
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED0008)
    if dist == "values16":
        x = torch.randint(0, 1 << 16, (n,), dtype=view, device="cuda", generator=g)
    else:
        info = torch.iinfo(view)
        x = torch.randint(info.min, info.max, (n,), dtype=view, device="cuda", generator=g)
    return x.view(kdt)


def run_row(row, k, dist, ctx, reps, warmup):
    kdt, view, kb = ROWS[row]
    n = 1 << k
    st = torch.cuda.current_stream()
    keys = make_keys(row, n, dist)
    tkeys = keys.view(view)
    sorted_tmp = torch.empty_like(keys)
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    m_box = {}

    def group_all():
        g = rs.radix_group(keys, perm=True, inverse=True, ctx=ctx)
        m_box["g"] = g

    def group_perm():
        rs.radix_group(keys, ctx=ctx)

    def group_keys():
        rs.radix_group(keys, perm=False, ctx=ctx)

    def argsort():
        rs.radix_argsort(keys, out=out, ctx=ctx)

    def keys_desc():  # the keys-only join and sort with a split behind it: the floor of group_keys' scan-kind time
        sorted_tmp.copy_(keys)
        rs.radix_sort_pairs(sorted_tmp, None, descending=True, ctx=ctx)

    def torch_unique():
        torch.unique(tkeys, sorted=True, return_inverse=True, return_counts=True)

    def torch_chain():
        p = rs.radix_argsort(keys, ctx=ctx)
        s = tkeys[p]
        head = torch.ones(n, dtype=torch.bool, device="cuda")
        head[1:] = s[1:] != s[:-1]
        rank = torch.cumsum(head, 0) - 1
        inverse = torch.empty(n, dtype=torch.int64, device="cuda")
        inverse[p] = rank
        offsets = torch.nonzero(head).view(-1)
        return s[offsets], offsets, p, inverse

    ways = {"group_all_ms": group_all, "group_perm_ms": group_perm, "group_keys_ms": group_keys, "argsort_ms": argsort, "keys_desc_ms": keys_desc,
            "torch_unique_ms": torch_unique, "torch_chain_ms": torch_chain}
    profiled = ("group_all_ms", "group_perm_ms", "group_keys_ms", "argsort_ms", "keys_desc_ms")
    times = {w: [] for w in ways}
    scan = {w: [] for w in profiled}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            if w in profiled:
                ctx.profile(True)
            t = timed(fn, st)
            if w in profiled:
                o = ctx.profile_read()["scan"][0]
                ctx.profile(False)
                if r >= warmup:
                    scan[w].append(o)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    m = int(m_box["g"].num)
    rec = {"row": row, "log2n": k, "dist": dist, "key_bytes": kb, "groups": m, "reps": reps}
    for w, v in times.items():
        if w != "keys_desc_ms":  # (it holds a copy of the keys too: only its profile is used)
            rec[w] = round(median(v), 4)
    es = JOINED[kb]
    run = median(scan["group_all_ms"]) - median(scan["argsort_ms"])
    run_bytes = 2 * n * es + m * kb + (m + 1) * 8 + 2 * n * 8
    rec["run_ms"] = round(run, 4)
    rec["run_bytes"] = run_bytes
    rec["run_frac_of_8TBps"] = round(run_bytes / (run * 1e-3) / 8e12, 3) if run > 0 else None
    runp = median(scan["group_perm_ms"]) - median(scan["argsort_ms"])
    runp_bytes = run_bytes - n * 8
    rec["run_perm_ms"] = round(runp, 4)
    rec["run_perm_bytes"] = runp_bytes
    rec["run_perm_frac_of_8TBps"] = round(runp_bytes / (runp * 1e-3) / 8e12, 3) if runp > 0 else None
    runk = median(scan["group_keys_ms"]) - median(scan["keys_desc_ms"])
    runk_bytes = 2 * n * kb + m * kb + (m + 1) * 8
    rec["run_keys_ms"] = round(runk, 4)
    rec["run_keys_bytes"] = runk_bytes
    rec["run_keys_frac_of_8TBps"] = round(runk_bytes / (runk * 1e-3) / 8e12, 3) if runk > 0 else None
    rec["group_all_vs_torch_unique"] = round(rec["torch_unique_ms"] / rec["group_all_ms"], 2)
    rec["group_all_vs_torch_chain"] = round(rec["torch_chain_ms"] / rec["group_all_ms"], 2)
    rec["library"] = os.path.basename(rs._lib.lib_path())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=";".join(ROWS))
    ap.add_argument("--log2n", default="24,28")
    ap.add_argument("--dists", default="values16;full")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()
    ctx = rs.Context(torch.cuda.current_device())
    sink = open(a.json, "a") if a.json else None
    for row in [x for x in a.rows.split(";") if x]:
        for k in (int(x) for x in a.log2n.split(",")):
            for dist in [x for x in a.dists.split(";") if x]:
                rec = run_row(row, k, dist, ctx, a.reps, a.warmup)
                line = json.dumps(rec)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
