#!/usr/bin/env python3
"""Device time of single u64 sorts at the sizes where the wide-key hybrid starts (2^23, 2^24), default options:
    python tools/hybrid_parked_bench.py [--label NAME] [--sizes 23,24] [--reps 40] [--clustered] [--out FILE]
One JSON line per size: uniform keys, a fresh array per repetition, device events around the sort alone; the median, the
fastest and the slowest repetition in microseconds and the path the last sort took (RSX_INFO_LAST_PASSES bits 24-27).
--clustered: the same array with one value of the top 16 bits written over a run of n / 80 elements (a padded or
pre-sorted block): a 16-bit counter of the count kernel parks and the device gives the sort to the LSD passes (path 0);
the context is told to try again before every repetition, so each one is a refused try: the count, then the LSD passes.
RSX_LIBRARY picks the build, so two builds are compared by alternating calls (profiles/hybrid_parked_bench.jsonl)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import radix_sort_amd as rs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--sizes", default="23,24")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--clustered", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = rs.default_context(0)
    d = rs.PRIMITIVES["u64"]
    for lg in (int(s) for s in a.sizes.split(",")):
        n = 1 << lg
        x = torch.empty(n, dtype=torch.int64, device="cuda")
        tmp = torch.empty_like(x)
        ctx.reserve(n, d)
        ctx.set_option(rs.OPT_WIDE_SORT, 1)  # (the default; setting it makes the context forget earlier refusals)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream().cuda_stream
        us = []
        for it in range(a.reps + 3):
            ctx.generate_device(x.data_ptr(), n, d, rs.GEN_UNIFORM, 77 + it)
            if a.clustered:
                x[n // 3:n // 3 + n // 80] = (x[n // 3:n // 3 + n // 80] & ((1 << 48) - 1)) | (0x5A3C << 48)
                ctx.set_option(rs.OPT_WIDE_SORT, 1)  # every repetition is a refused try (else 15 sorts go without one)
            e0.record()
            ctx.sort_device(x.data_ptr(), tmp.data_ptr(), n, d, stream)
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                us.append(e0.elapsed_time(e1) * 1e3)
        ctx.check()
        path = (ctx.get_info(rs.INFO_LAST_PASSES) >> 24) & 15
        out = torch.zeros(3, dtype=torch.int64, device="cuda")
        ctx.verify_device(x.data_ptr(), n, d, out.data_ptr(), stream)
        v = out.cpu().tolist()
        assert v[0] == 0 and v[2] == 0, f"output not sorted: {v}"
        us.sort()
        line = json.dumps({"tool": "hybrid_parked_bench", "label": a.label, "type": "u64", "n": n, "input": "clustered" if a.clustered else "uniform",
                           "reps": a.reps, "us_median": round(us[len(us) // 2], 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1), "path": path})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
