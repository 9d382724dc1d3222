"""Time of the key / value calls (rsx_sort_pairs_device, rsx_argsort_device) beside the other ways to get the same result.

    python tools/pairs_bench.py [--rows "u32+u32;u64+u64;f32+i64;u64+v40;argsort-u32;argsort-f32"] [--log2n 24,28]
                                [--reps 10] [--warmup 2] [--baseline-library PATH] [--json profiles/pairs_bench.jsonl]

Uniform keys (rsx_generate_device), the values the element's position.  One JSON line per row, size and order with the
median device time (HIP events around the call alone, every repetition on a fresh copy of the same generated input,
warm-up first; the ways alternate within a repetition) of

  new_ms     the new call: radix_sort_pairs / radix_argsort (int64 indices, as torch.argsort gives)
  parent_ms  what a caller had to do before these calls existed: interleave the columns with torch ops into a
             structured uint8 buffer, rsx_sort_device of --baseline-library on that buffer (radix_sort(digits=
             tuple_of(...))), pull the columns apart again; argsort: the key beside a u32 position, the position
             column widened to int64.  Descending order could not be asked for: the caller complements unsigned keys
             (flips the sign bit of float keys) before and after, two more passes over the key column.  The scratch
             buffers are allocated outside the timed region
  floor_ms   rsx_sort_device on already-joined elements of the same size (route 2: on the proxies): new_ms - floor_ms
             is the price of join and split (of join, copy, split and gather)
  torch_ms   torch.sort(stable=True) + a gather of the values / torch.argsort(stable=True); torch has no sort of u32 and
             u64: their signed views are sorted instead (another order, the same work).  An outside yardstick only
  join_split_ms  the context's per-launch timing (rsx_ctx_profile, kind "other") of the new call minus that of the
             floor sort: the join and split kernels (route 2: and the gather, not the copy of the values) alone; moved_bytes is what they read and
             write, frac_of_8TBps = moved_bytes / join_split_ms / 8e12, and copy_ms / copy_frac the same for ONE
             device-to-device copy that moves as many bytes (reads half, writes half), timed in the same repetitions

parent_ms comes from --baseline-library (default: the library in use), loaded beside it: pass a build of the parent
commit to compare against it.  Nothing outside the repository is read.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import radix_sort_amd as rs  # noqa: E402
from segment_bench import Baseline, median, timed  # noqa: E402

# row -> (key name, torch key dtype, torch view that torch.sort takes, value bytes (0: argsort))
ROWS = {
    "u32+u32": ("u32", torch.uint32, torch.int32, 4),
    "u64+u64": ("u64", torch.uint64, torch.int64, 8),
    "f32+i64": ("f32", torch.float32, torch.float32, 8),
    "u64+v40": ("u64", torch.uint64, torch.int64, 40),
    "argsort-u32": ("u32", torch.uint32, torch.int32, 0),
    "argsort-f32": ("f32", torch.float32, torch.float32, 0),
}


def voff(kb, vb):
    a = 1 if vb == 0 else 4 if vb % 4 == 0 else 2 if vb % 2 == 0 else 1
    return (kb + a - 1) // a * a


def joined_elem(kb, vb):
    need = voff(kb, vb) + vb
    return next((z for z in (1, 2, 4, 8, 12, 16, 24, 32) if z >= need and z % kb == 0), 0)


def run_row(row, k, desc, ctx, base, reps, warmup):
    kname, kdt, tview, vb = ROWS[row]
    d = rs.PRIMITIVES[kname]
    kb = d.key_bytes
    n = 1 << k
    argsort = vb == 0
    evb = 4 if argsort else vb  # bytes of the value inside the joined element
    es = joined_elem(kb, evb)
    route = 1 if es else 2
    if not es:
        es = joined_elem(kb, 4)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    keys_src = torch.empty(n, dtype=kdt, device="cuda")
    ctx.generate_device(keys_src.data_ptr(), n, d, rs.GEN_UNIFORM, 0x5EED0005)
    keys = torch.empty_like(keys_src)
    kbytes = keys.view(torch.uint8).view(n, kb)
    if argsort:
        vals_src = vals = None
        out = torch.empty(n, dtype=torch.int64, device="cuda")
    else:
        pos = torch.arange(n, dtype=torch.int64, device="cuda")
        vals_src = pos.view(torch.uint8).view(n, 8)[:, :vb].contiguous() if vb <= 8 else pos[:, None].expand(n, vb // 8).contiguous().view(torch.uint8).view(n, vb)
        del pos
        vals = torch.empty_like(vals_src)
    # the parent's way: one structured buffer of (key, value) elements; argsort: (key, u32 position)
    pvb = 4 if argsort else vb
    pd = rs.tuple_of(kname, pvb)
    pes = pd.elem_bytes
    buf = torch.empty((n, pes), dtype=torch.uint8, device="cuda")
    ptmp = torch.empty_like(buf)
    play = pd.layout()
    pos32 = torch.arange(n, dtype=torch.int32, device="cuda").view(torch.uint8).view(n, 4) if argsort else None
    bits = keys.view(torch.int32 if kb == 4 else torch.int64)
    flip = (-1 if d.key_kind != rs.KEY_FLOAT else torch.iinfo(bits.dtype).min) if desc else 0

    def parent():
        if desc:
            bits.bitwise_xor_(flip)
        if pes > kb + pvb:
            buf.zero_()
        buf[:, :kb] = kbytes
        buf[:, kb:kb + pvb] = pos32 if argsort else vals
        base.sort(buf.data_ptr(), ptmp.data_ptr(), n, play, s)
        if argsort:
            out.copy_(buf[:, kb:kb + 4].contiguous().view(torch.int32).view(n))
        else:
            kbytes.copy_(buf[:, :kb])
            vals.copy_(buf[:, kb:kb + pvb])
        if desc:
            bits.bitwise_xor_(flip)  # (argsort: the caller's keys put back as they were)

    # the floor: one array of already-joined elements of the size the new call sorts
    fd = rs.RadixDigits(es, 0, kb, d.key_kind)
    felems = torch.empty((n, es), dtype=torch.uint8, device="cuda")
    ftmp = torch.empty_like(felems)
    fsrc = torch.zeros((n, es), dtype=torch.uint8, device="cuda")
    fsrc[:, :kb] = keys_src.view(torch.uint8).view(n, kb)

    def new():
        if argsort:
            rs.radix_argsort(keys, descending=desc, out=out, ctx=ctx)
        else:
            rs.radix_sort_pairs(keys, vals, descending=desc, ctx=ctx)

    def floor():
        ctx.sort_device(felems.data_ptr(), ftmp.data_ptr(), n, fd, s)

    tkeys = keys.view(tview)

    def torch_way():
        if argsort:
            torch.argsort(tkeys, stable=True, descending=desc)
        else:
            r = torch.sort(tkeys, stable=True, descending=desc)
            vals[r.indices]

    # bytes the join and split kernels (route 2: and the copy and the gather) read and write
    if argsort:
        moved = n * (kb + es) + n * (es + 8)
    elif route == 1:
        moved = 2 * n * (kb + vb + es)
    else:
        moved = 2 * n * (kb + es) + 2 * n * vb + n * 4  # join, split, gather (the copy of the values is a memcpy node: not in join_split_ms)
    cbytes = moved // 2
    csrc = torch.empty(cbytes, dtype=torch.uint8, device="cuda")
    cdst = torch.empty_like(csrc)

    ways = {"new_ms": new, "parent_ms": parent, "floor_ms": floor, "torch_ms": torch_way, "copy_ms": lambda: cdst.copy_(csrc)}
    times = {w: [] for w in ways}
    other = {"new_ms": [], "floor_ms": []}
    for r in range(warmup + reps):
        for w, fn in ways.items():  # alternating: every way once per repetition
            keys.copy_(keys_src)
            if vals is not None:
                vals.copy_(vals_src)
            if w == "floor_ms":
                felems.copy_(fsrc)
            if w in other:
                ctx.profile(True)
            t = timed(fn, st)
            if w in other:
                o = ctx.profile_read()["other"][0]
                ctx.profile(False)
                if r >= warmup:
                    other[w].append(o)
            if r >= warmup:
                times[w].append(t)
    ctx.check()
    base.check()
    info = ctx.get_info(rs.INFO_LAST_PAIRS)
    rec = {"row": row, "log2n": k, "order": "descending" if desc else "ascending", "key_bytes": kb, "value_bytes": vb, "route": info & 0xFF,
           "joined_elem_bytes": (info >> 8) & 0xFF, "parent_elem_bytes": pes, "reps": reps}
    for w, v in times.items():
        rec[w] = round(median(v), 4)
    js = median(other["new_ms"]) - median(other["floor_ms"])
    rec["join_split_ms"] = round(js, 4)
    rec["moved_bytes"] = moved
    rec["frac_of_8TBps"] = round(moved / (js * 1e-3) / 8e12, 3) if js > 0 else None
    rec["copy_frac"] = round(2 * cbytes / (rec["copy_ms"] * 1e-3) / 8e12, 3)
    rec["join_split_vs_copy"] = round(rec["copy_ms"] / js, 3) if js > 0 else None
    rec["new_vs_parent"] = round(rec["parent_ms"] / rec["new_ms"], 2)
    rec["library"] = os.path.basename(rs._lib.lib_path())
    rec["baseline_library"] = os.path.basename(base.path)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=";".join(ROWS))
    ap.add_argument("--log2n", default="24,28")
    ap.add_argument("--orders", default="ascending;descending")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-library", default=os.environ.get("RSX_BASELINE_LIBRARY") or rs._lib.lib_path())
    ap.add_argument("--json", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()
    dev = torch.cuda.current_device()
    ctx = rs.Context(dev)
    base = Baseline(a.baseline_library, dev)
    sink = open(a.json, "a") if a.json else None
    for row in [x for x in a.rows.split(";") if x]:
        for k in (int(x) for x in a.log2n.split(",")):
            for order in [x for x in a.orders.split(";") if x]:
                rec = run_row(row, k, order == "descending", ctx, base, a.reps, a.warmup)
                line = json.dumps(rec)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
