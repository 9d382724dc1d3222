"""Time of the search call (rsx_search_sorted_device: radix_searchsorted) by both routes beside torch.searchsorted.

    python tools/searchsorted_bench.py [--rows "u32;i64"] [--m "16,22,n"] [--needles "ordered;shuffled;uniform"] [--reps 7]
                                       [--warmup 2] [--json profiles/searchsorted_bench.jsonl]

The haystack: 2^28 u32 or 2^26 i64 keys, uniform and sorted on the device (the u32 keys are drawn below 2^31, so that the
signed view torch takes is sorted too and both libraries do the same work on the same bytes).  The needles, m = 2^16, 2^22
or n of them: `ordered` members of the haystack in its order (at m = n the haystack itself), `shuffled` the same members
in random order, `uniform` keys drawn like the haystack's, mostly absent from it.  One JSON line per shape with the median
device time (HIP events around the call alone, warm-up first; the ways alternate within a repetition, the protocol of
tools/unique_bench.py) of

  as_given_ms   radix_searchsorted(presort=False): the needles as given, int64 lower bounds into a preallocated tensor
  presort_ms    radix_searchsorted(presort=True): the needles joined with their positions and sorted first
  argsort_ms    radix_argsort of the needles (int64 indices): the floor of the presort route
  torch_ms      torch.searchsorted on the signed view, out= preallocated

and, for ordered needles at m = n, stream_bytes = haystack + needles + outputs, the bytes the algorithm has to move, and
stream_frac_of_8TBps = stream_bytes / as_given_ms / 8e12.  rule_presort is what presort=None picks for the shape.
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

# row -> (torch key dtype, the view torch.searchsorted takes, key bytes, log2 of the haystack)
ROWS = {
    "u32": (torch.uint32, torch.int32, 4, 28),
    "i64": (torch.int64, torch.int64, 8, 26),
}


def draw(row, count, gen):
    _kdt, view, _kb, _k = ROWS[row]
    if row == "u32":
        return torch.randint(0, 2 ** 31 - 1, (count,), dtype=view, device="cuda", generator=gen)
    info = torch.iinfo(view)
    return torch.randint(info.min, info.max, (count,), dtype=view, device="cuda", generator=gen)


def make_needles(row, hay, m, kind, gen):
    n = hay.numel()
    if kind == "uniform":
        return draw(row, m, gen)
    if m == n:
        members = hay.clone()
    else:
        members = hay[torch.sort(torch.randint(0, n, (m,), device="cuda", generator=gen)).values]
    if kind == "ordered":
        return members
    return members[torch.randperm(m, device="cuda", generator=gen)]


def run_shape(row, hay, m, kind, ctx, reps, warmup):
    kdt, view, kb, k = ROWS[row]
    n = hay.numel()
    st = torch.cuda.current_stream()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x5EED000A)
    needles = make_needles(row, hay, m, kind, gen)  # (signed views: what torch takes; the library gets the key dtype)
    hk, nk = hay.view(kdt), needles.view(kdt)
    out = torch.empty(m, dtype=torch.int64, device="cuda")
    out_t = torch.empty(m, dtype=torch.int64, device="cuda")

    def as_given():
        rs.radix_searchsorted(hk, nk, out=out, presort=False, ctx=ctx)

    def presort():
        rs.radix_searchsorted(hk, nk, out=out, presort=True, ctx=ctx)

    def argsort():
        rs.radix_argsort(nk, out=out, ctx=ctx)

    def torch_way():
        torch.searchsorted(hay, needles, out=out_t)

    ways = {"as_given_ms": as_given, "presort_ms": presort, "argsort_ms": argsort, "torch_ms": torch_way}
    times = {w: [] for w in ways}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            t = timed(fn, st)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    as_given()
    agree = bool(torch.equal(out, out_t))
    rec = {"row": row, "log2n": k, "m": m, "needles": kind, "key_bytes": kb, "reps": reps}
    for w, v in times.items():
        rec[w] = round(median(v), 4)
    if kind == "ordered" and m == n:
        rec["stream_bytes"] = n * kb + m * kb + m * 8
        rec["stream_frac_of_8TBps"] = round(rec["stream_bytes"] / (rec["as_given_ms"] * 1e-3) / 8e12, 3)
    rec["as_given_vs_torch"] = round(rec["torch_ms"] / rec["as_given_ms"], 2)
    rec["presort_vs_torch"] = round(rec["torch_ms"] / rec["presort_ms"], 2)
    rec["rule_presort"] = bool(rs.api._search_presort(n, m, kb))
    rec["agrees_with_torch"] = agree
    rec["library"] = os.path.basename(rs._lib.lib_path())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=";".join(ROWS))
    ap.add_argument("--m", default="16,22,n", help="log2 of the needle counts; n: as many as the haystack")
    ap.add_argument("--needles", default="ordered;shuffled;uniform")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()
    ctx = rs.Context(torch.cuda.current_device())
    sink = open(a.json, "a") if a.json else None
    for row in [x for x in a.rows.split(";") if x]:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0x5EED0009)
        n = 1 << ROWS[row][3]
        hay = torch.sort(draw(row, n, gen)).values
        for ms in a.m.split(","):
            m = n if ms == "n" else 1 << int(ms)
            for kind in [x for x in a.needles.split(";") if x]:
                rec = run_shape(row, hay, m, kind, ctx, a.reps, a.warmup)
                line = json.dumps(rec)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
                torch.cuda.empty_cache()
        del hay
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
