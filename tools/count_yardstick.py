#!/usr/bin/env python3
"""The hybrid's count kernel against the histogram kernel on the same arrays, in one process.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o y -- python tools/count_yardstick.py
  python tools/count_yardstick.py --trace DIR/.../y_kernel_trace.csv

The first form sorts ITERS (default 6) arrays of 2^LG (default 30) uniform u64 keys with the wide-key hybrid
(RSX_OPT_WIDE_SORT = 1: rsx_count16top_kernel reads the array once) and ITERS more with the LSD passes (= 0:
rsx_hist_kernel reads its array once), alternately and back to back as bench.py does, so that both kernels start
behind a sort whose output still sits in the caches.  The second form reads the kernel trace of such a run and
prints both kernels' time per launch and their ratio (launches that their gate sent home at once are left out)."""
import csv, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def trace(path):
    t = {"rsx_count16top_kernel": [], "rsx_hist_kernel": []}
    for r in csv.DictReader(open(path)):
        for key in t:
            if key in r["Kernel_Name"]:
                ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
                if ms > 0.05:  # (a gated launch returns after a few microseconds)
                    t[key].append(ms)
    for key, v in t.items():
        if v:
            print(f"{key:24s} launches {len(v):3d}  avg {sum(v) / len(v):.4f} ms  min {min(v):.4f}  max {max(v):.4f}")
    c, h = t["rsx_count16top_kernel"], t["rsx_hist_kernel"]
    if c and h:
        print(f"count / histogram = {sum(c) / len(c) / (sum(h) / len(h)):.3f} (avg)  {min(c) / min(h):.3f} (min)")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        return trace(sys.argv[2])
    import torch, radix_sort_amd as rs
    lg, iters = int(os.environ.get("LG", "30")), int(os.environ.get("ITERS", "6"))
    d = rs.PRIMITIVES["u64"]
    n = 1 << lg
    bufs = [torch.empty(n * 8, dtype=torch.uint8, device="cuda") for _ in range(2 * iters)]
    tmp = torch.empty_like(bufs[0])
    ctxs = {}
    for mode in (1, 0):
        ctxs[mode] = rs.Context(0)
        ctxs[mode].set_option(rs.OPT_WIDE_SORT, mode)
    for i, b in enumerate(bufs):
        ctxs[1].generate_device(b.data_ptr(), n, d, rs.GEN_UNIFORM, 77 + i, 0.0)
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        ctxs[1 - i % 2].sort_device(b.data_ptr(), tmp.data_ptr(), n, d)
    torch.cuda.synchronize()
    for c in ctxs.values():
        c.check()
        c.close()
    print(f"sorted {iters} arrays of 2^{lg} u64 in each mode")


if __name__ == "__main__":
    main()
