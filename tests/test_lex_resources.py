"""Register budget of the join kernel of several key columns (no GPU needed: hipcc reports it at compile time; the
method of tests/test_reduce_resources.py).

rsx_lex_join_kernel is a streaming kernel: at most 64 bytes of elements per thread, one or two compound keys put
together by shifts, the columns read from the kernel arguments by a wave-uniform loop.  Nothing in it has a reason to
leave the registers -- in particular the byte offset of a column inside the compound key, a run-time value, must not
turn the key into an array in scratch memory -- so any spill and any scratch, in any instantiation, is a defect: the
bounds are 0."""
import os
import re

from radix_sort_amd import _build
from resources import kernel_resources

WIDTHS = (1, 2, 4, 8, 16)


def test_the_unit_is_part_of_the_library():
    assert "rsx_lex.hip" in _build.DEPS and "rsx_lex_kernels.hpp" in _build.DEPS
    blob = open(_build.build(), "rb").read()
    assert b"rsx_lex_join_kernel" in blob


def test_join_kernels_use_no_scratch():
    res = kernel_resources("rsx_lex.hip")
    kernels = {n: r for n, r in res.items() if "rsx_lex_join_kernel" in n}
    seen = []
    for name, r in kernels.items():
        print(name, r)
        assert "VGPRs" in r and "ScratchSize [bytes/lane]" in r, (name, r)
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        m = re.search(r"ILi(\d+)ELb([01])EE", name)  # <W, GATHER> of the mangled name
        assert m, name
        seen.append((int(m.group(1)), int(m.group(2))))
    assert sorted(seen) == sorted((w, g) for w in WIDTHS for g in (0, 1)), seen
    assert not [n for n in res if "rsx_lex" in n and n not in kernels], "a kernel of the unit that this test does not know"


def test_the_argument_struct_is_bounded_in_the_code():
    """The columns travel by value in the kernel arguments; the header asserts their size against the argument segment
    (test_join_kernels_use_no_scratch compiles that assertion)."""
    src = open(os.path.join(_build.CSRC, "rsx_lex_kernels.hpp")).read()
    m = re.search(r"static_assert\(sizeof\(LexArgs\) \+ (\d+) <= (\d+),", src)
    assert m and int(m.group(2)) <= 4096 and int(m.group(1)) >= 32  # 32: the five other arguments of the kernel
    assert re.search(r"static_assert\(sizeof\(LexColumn\) == 32 && sizeof\(LexArgs\) == 32 \* LEX_MAX_COLUMNS \+ 8", src)
    assert "__launch_bounds__(256)" in src and "__shared__" not in src and "atomic" not in src
