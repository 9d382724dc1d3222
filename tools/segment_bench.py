"""Time of the segmented sort (rsx_sort_rows_device / rsx_sort_segments_device) beside the other ways to get the same bytes.

    python tools/segment_bench.py [--types "u32;u64;f32;(u64,u64)"] [--log2n 24,27] [--reps 10] [--warmup 2]
                                  [--baseline-library PATH] [--json profiles/segments_bench.jsonl]

Per element type and total size, rows of 32, 128, 1024 and 4096 elements, of every LDS class cap and of the largest
cap + 1, and a ragged CSR-like input (geometric lengths, mean 64).  One JSON line per shape with the median device time
(HIP events around the call alone, every repetition on a fresh copy of the same seeded input, warm-up first) of

  rows_ms        rsx_sort_rows_device (rows of one length only)
  seg_exact_ms   rsx_sort_segments_device with max_seg_len = the longest segment
  seg_any_ms     rsx_sort_segments_device with max_seg_len = 0 (every class launched)
  hostloop_ms    a host loop of rsx_sort_device over the segments -- the only way before this call existed.  Above 1024
                 segments the first 1024 are timed and the time scaled by nseg / 1024 (hostloop_timed says how many ran)
  whole_ms       rsx_sort_device on the whole array as ONE array (other bytes; the same memory), alternating with the above
  torch_ms       torch.sort(x.view(rows, L), dim=-1) where torch has the dtype (signed views of the unsigned types)

hostloop_ms and whole_ms come from --baseline-library (default: the library in use), loaded beside it: pass a build of
the parent commit to compare against it.  Nothing outside the repository is read.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import radix_sort_amd as rs  # noqa: E402

TYPES = {"u32": rs.PRIMITIVES["u32"], "u64": rs.PRIMITIVES["u64"], "f32": rs.PRIMITIVES["f32"], "(u64,u64)": rs.tuple_of("u64", 8)}
TORCH_VIEW = {"u32": torch.int32, "u64": torch.int64, "f32": torch.float32}


class Baseline:
    """rsx_sort_device of another build of the library (its own context), through plain ctypes."""

    def __init__(self, path, device):
        self.L = ctypes.CDLL(path)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        self.L.rsx_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        self.L.rsx_sort_device.argtypes = [vp, vp, vp, sz, ctypes.POINTER(rs.Layout), vp]
        self.L.rsx_ctx_reserve.argtypes = [vp, sz, ctypes.POINTER(rs.Layout)]
        self.L.rsx_ctx_check.argtypes = [vp, vp]
        self.h = vp()
        assert self.L.rsx_ctx_create(device, ctypes.byref(self.h)) == 0
        self.path = path

    def sort(self, data, tmp, n, lay, stream):
        rc = self.L.rsx_sort_device(self.h, data, tmp, n, ctypes.byref(lay), stream)
        assert rc == 0, rc

    def check(self):
        assert self.L.rsx_ctx_check(self.h, None) == 0


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(fn, st):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def run_shape(tname, d, total, lens_kind, L, ctx, base, reps, warmup):
    es = d.elem_bytes
    lay = d.layout()
    if lens_kind == "rows":
        rows = max(1, total // L)
        lens = None
        n = rows * L
        offs_np = np.arange(rows + 1, dtype=np.int64) * L
        longest = L
    else:  # ragged: geometric lengths of mean 64 (support 0, 1, 2, ...), seeded
        rng = np.random.default_rng(0x5E6)
        lens = rng.geometric(1.0 / 65.0, size=total // 64) - 1
        offs_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        n = int(offs_np[-1])
        rows = len(lens)
        longest = int(lens.max())
    nseg = len(offs_np) - 1
    src = torch.empty(n * es, dtype=torch.uint8, device="cuda")
    work, tmp = torch.empty_like(src), torch.empty_like(src)
    ctx.generate_device(src.data_ptr(), n, d, rs.GEN_UNIFORM, 0x5EED0003)
    offs = torch.from_numpy(offs_np).cuda()
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    caps = rs.segment_caps(d)
    loop_n = min(nseg, 1024)
    loop = [(int(offs_np[i]), int(offs_np[i + 1] - offs_np[i])) for i in range(loop_n)]

    def hostloop():
        for b, ln in loop:
            if ln > 1:
                base.sort(work.data_ptr() + b * es, tmp.data_ptr() + b * es, ln, lay, s)

    ways = {
        "seg_exact_ms": lambda: ctx.sort_segments_device(work.data_ptr(), tmp.data_ptr(), n, d, offs.data_ptr(), nseg, longest, s),
        "seg_any_ms": lambda: ctx.sort_segments_device(work.data_ptr(), tmp.data_ptr(), n, d, offs.data_ptr(), nseg, 0, s),
        "hostloop_ms": hostloop,
        "whole_ms": lambda: base.sort(work.data_ptr(), tmp.data_ptr(), n, lay, s),
    }
    if lens_kind == "rows":
        ways["rows_ms"] = lambda: ctx.sort_rows_device(work.data_ptr(), tmp.data_ptr(), rows, L, d, s)
        if tname in TORCH_VIEW:
            tv = work.view(TORCH_VIEW[tname]).view(rows, L)
            ways["torch_ms"] = lambda: torch.sort(tv, dim=-1)
    times = {k: [] for k in ways}
    for r in range(warmup + reps):
        for k, fn in ways.items():  # alternating: every way once per repetition
            work.copy_(src)
            t = timed(fn, st)
            if r >= warmup:
                times[k].append(t)
    ctx.check()
    base.check()
    # the last segmented result: first and last segment in order (the tests compare every byte)
    work.copy_(src)
    ways["rows_ms" if lens_kind == "rows" else "seg_exact_ms"]()
    ctx.check()
    out = torch.zeros(3, dtype=torch.int64, device="cuda")
    ok = True
    for i in (0, nseg - 1):
        b, ln = int(offs_np[i]), int(offs_np[i + 1] - offs_np[i])
        if ln > 1:
            ctx.verify_device(work.data_ptr() + b * es, ln, d, out.data_ptr())
            ok = ok and out.cpu().tolist()[0] == 0
    rec = {"type": tname, "elem_bytes": es, "n": n, "shape": lens_kind, "row_len": L if lens_kind == "rows" else None, "nseg": nseg,
           "longest": longest, "caps": caps, "reps": reps, "sorted": ok}
    for k, v in times.items():
        m = median(v)
        if k == "hostloop_ms":
            rec["hostloop_timed"] = loop_n
            m *= nseg / loop_n
        rec[k] = round(m, 4)
        rec[k.replace("_ms", "_min_ms")] = round(min(v) * (nseg / loop_n if k == "hostloop_ms" else 1.0), 4)
    best = rec.get("rows_ms", rec["seg_exact_ms"])
    rec["vs_hostloop"] = round(rec["hostloop_ms"] / best, 2)
    rec["vs_whole"] = round(best / rec["whole_ms"], 3)
    rec["GB_per_s"] = round(n * es / best / 1e6, 1)
    rec["library"] = os.path.basename(rs._lib.lib_path())
    rec["baseline_library"] = os.path.basename(base.path)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", default="u32;u64;f32;(u64,u64)")
    ap.add_argument("--log2n", default="24,27")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-library", default=os.environ.get("RSX_BASELINE_LIBRARY") or rs._lib.lib_path())
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    ap.add_argument("--shapes", default="", help="only these row lengths / 'ragged', separated by ;")
    a = ap.parse_args()
    dev = torch.cuda.current_device()
    ctx = rs.Context(dev)
    base = Baseline(a.baseline_library, dev)
    sink = open(a.json, "a") if a.json else None
    for tname in [x for x in a.types.split(";") if x]:
        d = TYPES[tname]
        caps = rs.segment_caps(d)
        shapes = [("rows", L) for L in (32, 128, 1024, 4096, *caps, caps[-1] + 1)] + [("ragged", 0)]
        if a.shapes:
            want = set(a.shapes.split(";"))
            shapes = [sh for sh in shapes if (sh[0] == "ragged" and "ragged" in want) or str(sh[1]) in want]
        for k in (int(x) for x in a.log2n.split(",")):
            for kind, L in shapes:
                rec = run_shape(tname, d, 1 << k, kind, L, ctx, base, a.reps, a.warmup)
                line = json.dumps(rec)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
