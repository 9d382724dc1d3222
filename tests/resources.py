"""What hipcc reports about the kernels of one translation unit at compile time (no GPU needed): registers, spills,
scratch, occupancy and static LDS, the budgets the *_resources tests hold."""
from __future__ import annotations

import functools
import os
import re
import subprocess
import tempfile

from radix_sort_amd import _build

_REMARK = re.compile(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                     r"LDS Size \[bytes/block\]): (\d+)")


@functools.lru_cache(maxsize=None)
def kernel_resources(source, flags=()):
    """{mangled kernel name: {remark: int}} of csrc/`source` compiled with the library's flags plus `flags` (a tuple)."""
    with tempfile.TemporaryDirectory() as d:
        cmd = [_build.hipcc()] + _build.CXXFLAGS + list(flags) + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                                  os.path.join(_build.CSRC, source), "-o", os.path.join(d, "o.o")]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        m = _REMARK.search(line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out
