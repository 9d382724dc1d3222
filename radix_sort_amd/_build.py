"""Builds librsx.so (the C-ABI HIP library) in-tree for gfx950.

`hipcc --offload-arch=gfx950` cross-compiles without a GPU; the resulting
radix_sort_amd/lib/librsx.so is git-ignored but travels to the GPU box.

The library is the translation units of UNITS below (one line each, with what it holds; rsx_es.hip once per element
size), compiled in parallel and linked into one shared object.  `python -m radix_sort_amd._build --variant NAME --es 4
-DX=1 ...` relinks a tuning variant (lib/v/NAME.so) that recompiles only the named size with the extra flags.
"""
from __future__ import annotations

import concurrent.futures
import os
import shutil
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIBDIR = os.path.join(_HERE, "lib")
OBJDIR = os.path.join(LIBDIR, "obj")
LIB = os.path.join(LIBDIR, "librsx.so")
ELEM_SIZES = (1, 2, 4, 8, 12, 16, 24, 32)
# (source, object name, extra flags): every translation unit of the library, in link order
UNITS = (
    ("rsx.hip", "rsx.o", ()),                # the C-ABI and the size-independent kernels
    ("rsx_pairs.hip", "rsx_pairs.o", ()),    # the join and split kernels of the key / value calls
    ("rsx_unique.hip", "rsx_unique.o", ()),  # the run kernels of rsx_unique_device and the kernels of rsx_compact_device
    ("rsx_scan.hip", "rsx_scan.o", ()),      # those of rsx_scan_by_key_device and, through rsx_reduce.hip, which it includes,
                                             # of rsx_reduce_by_key_device: one unit, the tile scan both calls launch built once
    ("rsx_lex.hip", "rsx_lex.o", ()),        # the join of several key columns: rsx_lexsort_device, rsx_sort_columns_device
    ("rsx_search.hip", "rsx_search.o", ()),  # the kernel of rsx_search_sorted_device
    ("rsx_merge.hip", "rsx_merge.o", ()),    # the kernels of rsx_merge_device
    ("rsx_setops.hip", "rsx_setops.o", ()),  # the kernel of rsx_setop_device
) + tuple(("rsx_es.hip", f"rsx_es{es}.o", (f"-DRSX_ES={es}",)) for es in ELEM_SIZES)  # the sort kernels, once per element size
# what the library is stale against: every unit, every file beside them that one of them includes (the headers and
# rsx_reduce.hip), and the public header
DEPS = sorted({src for src, _obj, _flags in UNITS} | {"rsx_reduce.hip"}) + sorted(f for f in os.listdir(CSRC) if f.endswith(".hpp")) + \
    [os.path.join("..", "..", "include", "rsx.h")]
CXXFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (need ROCm to build librsx.so)")


def stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in DEPS)


def _compile(job):
    src, obj, flags, verbose = job
    cmd = [hipcc()] + CXXFLAGS + flags + ["-c", os.path.join(CSRC, src), "-o", obj]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd, cwd=CSRC)
    return obj


def _objects(extra, only_es, objdir, verbose, reuse_from=None):
    """Compiles the translation units (in parallel); returns the object list.  With `only_es`, the
    other sizes' objects are taken from `reuse_from` (the main build) instead of being recompiled."""
    os.makedirs(objdir, exist_ok=True)
    jobs, objs = [], []
    for src, name, flags in UNITS:
        if only_es is None or any(f"-DRSX_ES={es}" in flags for es in only_es):
            obj = os.path.join(objdir, name)
            jobs.append((src, obj, list(flags) + list(extra), verbose))
        else:
            obj = os.path.join(reuse_from, name)
        objs.append(obj)
    workers = min(len(jobs), max(1, (os.cpu_count() or 2)))
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(_compile, jobs))
    return objs


def _link(objs, out, verbose):
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs + ["-lpthread"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd, cwd=CSRC)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not stale():
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    extra = os.environ.get("RSX_CXXFLAGS", "").split()
    objs = _objects(extra, None, OBJDIR, verbose)
    _link(objs, LIB, verbose)
    return LIB


def build_variant(name: str, only_es, flags, verbose: bool = False) -> str:
    """lib/v/NAME.so: the main build's objects with the named element sizes recompiled under `flags`
    (load it with RSX_LIBRARY=...).  Flags that the host unit reads too (tile geometry: -DRSX_KPT*, -DRSX_WG*)
    need `--es all`, which recompiles every unit."""
    if stale():
        build(force=True, verbose=verbose)
    vdir = os.path.join(LIBDIR, "v")
    os.makedirs(vdir, exist_ok=True)
    objs = _objects(flags, None if only_es is None else tuple(only_es), os.path.join(vdir, "obj_" + name), verbose,
                    reuse_from=OBJDIR)
    out = os.path.join(vdir, name + ".so")
    _link(objs, out, verbose)
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    if "--variant" in argv:
        i = argv.index("--variant")
        name = argv[i + 1]
        rest = argv[:i] + argv[i + 2:]
        es = [4]
        if "--es" in rest:
            j = rest.index("--es")
            es = None if rest[j + 1] == "all" else [int(x) for x in rest[j + 1].split(",")]  # all: host unit too
            rest = rest[:j] + rest[j + 2:]
        print(build_variant(name, es, rest, verbose=True))
    else:
        print(build(force=True, verbose=True))
