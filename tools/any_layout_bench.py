"""Sort time of layouts without kernels of their own (include/rsx.h "Any layout") beside direct layouts of similar size.

    python tools/any_layout_bench.py [--log2n 24,26] [--reps 30] [--warmup 3] [--only "NAME;NAME"]

One JSON line per workload: median / min / max of the device time of rsx_sort_device (HIP events around the call
alone; every repetition sorts a fresh copy of the same generated input), the route (RSX_INFO_LAST_PASSES bits 28-29),
and the time the context's own launch timers give the launches that are neither count, scan nor sweep ("other": the
re-layout / restore / proxy / gather kernels, plus the direct paths' own few).  RSX_LIBRARY=lib/v/NAME.so times another
build, e.g. one made with -DRSX_TUNING -DRSX_ANY_ROUTE=2, which sends every such layout through the proxy route.
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

U = rs.KEY_UNSIGNED
WORKLOADS = {  # name -> (elem_bytes, key_offset, key_bytes, key_kind)
    "(6,0,2)": (6, 0, 2, U), "(7,0,6)": (7, 0, 6, U), "(20,0,4)": (20, 0, 4, U), "(24,0,3)": (24, 0, 3, U),
    "(28,0,4)": (28, 0, 4, U), "(40,0,8)": (40, 0, 8, U), "(64,0,8)": (64, 0, 8, U), "(256,0,4)": (256, 0, 4, U),
    # direct layouts for comparison
    "(u32,u32)": (8, 0, 4, U), "(u64,u64)": (16, 0, 8, U), "u128": (16, 0, 16, U),
}


def run(name, lay, n, reps, warmup, ctx):
    d = rs.RadixDigits(*lay)
    nbytes = n * lay[0]
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    work, tmp = torch.empty_like(src), torch.empty_like(src)
    ctx.generate_device(src.data_ptr(), n, d, rs.GEN_UNIFORM, 0x5EED0001)
    ctx.reserve(n, d)
    st = torch.cuda.current_stream()
    times, other = [], []
    for r in range(warmup + reps):
        work.copy_(src)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.profile(r >= warmup)
        a.record(st)
        ctx.sort_device(work.data_ptr(), tmp.data_ptr(), n, d, st.cuda_stream)
        b.record(st)
        b.synchronize()
        if r >= warmup:
            times.append(a.elapsed_time(b))
            other.append(ctx.profile_read()["other"][0])
    ctx.profile(False)
    ctx.check()
    out = torch.zeros(3, dtype=torch.int64, device="cuda")
    ctx.verify_device(work.data_ptr(), n, d, out.data_ptr())
    v = out.cpu().tolist()
    route = (ctx.get_info(rs.INFO_LAST_PASSES) >> 28) & 3
    times.sort()
    med = times[len(times) // 2]
    return {"workload": name, "layout": list(lay), "n": n, "route": route, "median_ms": round(med, 4),
            "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4), "reps": reps,
            "other_ms": round(sorted(other)[len(other) // 2], 4), "GB_per_s": round(nbytes / med / 1e6, 1),
            "sorted": v[0] == 0, "stable": v[2] == 0, "library": os.path.basename(rs._lib.lib_path())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", default="24,26")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="workload names separated by ;")
    a = ap.parse_args()
    names = [x for x in a.only.split(";") if x] or list(WORKLOADS)
    ctx = rs.Context(torch.cuda.current_device())
    for k in (int(x) for x in a.log2n.split(",")):
        for name in names:
            print(json.dumps(run(name, WORKLOADS[name], 1 << k, max(20, a.reps), a.warmup, ctx)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
