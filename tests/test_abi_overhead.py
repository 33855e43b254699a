"""gf_overhead_update at the drop-in boundary: declared in include/gangfit.h, exported by libgangfit.so, bound in
gangfit/_native.py, and counted in DESIGN.md's table of the deliverables (section 0, row (b))."""
import ctypes
import os
import re

from gangfit import _native, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "gangfit.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gf_[a-z0-9_]+)\s*\(", text)))


def test_overhead_update_is_declared_exported_and_bound():
    assert "gf_overhead_update" in _declared_symbols()
    lib = ctypes.CDLL(build.build_native())
    assert hasattr(lib, "gf_overhead_update")
    assert "gf_overhead_update" in _native.EXPORTED_SYMBOLS
    L = _native.load()
    assert L.gf_overhead_update.restype is ctypes.c_int32 and len(L.gf_overhead_update.argtypes) == 6


def test_design_counts_the_header_symbols():
    row = next(line for line in open(os.path.join(REPO, "DESIGN.md")) if line.startswith("| (b) |"))
    m = re.search(r"(\d+) `gf_\*` symbols", row)
    assert m, row
    assert int(m.group(1)) == len(_declared_symbols())
