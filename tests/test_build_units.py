"""CPU: the library is rebuilt when any of its sources is newer than it (_build.stale), so DEPS has to name every one of
them -- a header that is missing there goes stale silently."""
import os

from radix_sort_amd import _build


def test_every_source_file_of_the_library_is_a_dependency():
    sources = sorted(f for f in os.listdir(_build.CSRC) if f.endswith((".hip", ".hpp")))
    assert sources and not [f for f in sources if f not in _build.DEPS], (sources, _build.DEPS)
    assert os.path.join("..", "..", "include", "rsx.h") in _build.DEPS
    for d in _build.DEPS:
        assert os.path.isfile(os.path.join(_build.CSRC, d)), d
