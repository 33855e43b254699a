"""gf_cluster_update at the drop-in boundary: declared in include/gangfit.h, exported by libgangfit.so, bound in
gangfit/_native.py and wrapped by Context.cluster_update; the argument checks that need no launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import gangfit
from gangfit import _native, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(REPO, "include", "gangfit.h")).read()


def test_cluster_update_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "gf_cluster_update" in re.findall(r"\b(gf_[a-z0-9_]+)\s*\(", text)
    lib = ctypes.CDLL(build.build_native())
    assert hasattr(lib, "gf_cluster_update")
    assert "gf_cluster_update" in _native.EXPORTED_SYMBOLS
    L = _native.load()
    assert L.gf_cluster_update.restype is ctypes.c_int32 and len(L.gf_cluster_update.argtypes) == 9


def test_the_declaration_sits_next_to_the_overhead_update_with_its_nine_arguments():
    text = _header()
    decl = re.search(r"int gf_cluster_update\((.*?)\);", text, flags=re.S)
    assert decl, "no declaration"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "n_rows", "node", "alloc_cpu_milli", "alloc_mem_bytes", "alloc_gpu",
                                                          "node_flags", "zone_of_node", "name_rank"]
    assert text.index("int gf_overhead_update(") < decl.start() < text.index("int gf_generation(")


def test_a_null_context_is_invalid():
    L = _native.load()
    assert L.gf_cluster_update(None, 0, None, None, None, None, None, None, None) == _native.GF_ERR_INVALID
    one = np.zeros(1, dtype=np.int64)
    node = np.zeros(1, dtype=np.uint32)
    assert L.gf_cluster_update(None, 1, _native.ptr(node), _native.ptr(one), _native.ptr(one), _native.ptr(one), _native.ptr(node), None,
                               None) == _native.GF_ERR_INVALID


class _Recorder:
    """stands in for the library: records what Context.cluster_update hands to the entry point"""

    def __init__(self):
        self.calls = []

    def gf_cluster_update(self, *args):
        self.calls.append(args)
        return _native.GF_OK


def _wrapped(n_nodes):
    ctx = gangfit.Context.__new__(gangfit.Context)  # no device: only the marshalling runs
    ctx._lib, ctx._h, ctx._cluster_n, ctx.n_nodes = _Recorder(), None, n_nodes, 0
    return ctx


def test_the_wrapper_sends_columns_and_null_for_what_is_not_given():
    ctx = _wrapped(5)
    ctx.cluster_update([3, 1], [[1000, 2000, 0], [4000, 8000, 1]], [2, 3])
    (h, n_rows, node, cpu, mem, gpu, flags, zone, ranks), = ctx._lib.calls
    assert n_rows == 2 and zone is None and ranks is None and None not in (node, cpu, mem, gpu, flags)
    ctx.cluster_update([], np.zeros((0, 3)), [], name_rank=[4, 3, 2, 1, 0])  # a ranks-only call
    h, n_rows, node, cpu, mem, gpu, flags, zone, ranks = ctx._lib.calls[1]
    assert n_rows == 0 and ranks is not None and zone is None
    ctx.cluster_update([0], [[1, 1, 1]], [2], zone=[1])
    assert ctx._lib.calls[2][7] is not None


@pytest.mark.parametrize("kwargs", [
    dict(rows=[1, 2], alloc=[[1, 1, 1]], flags=[2, 2]),                      # one allocatable row for two nodes
    dict(rows=[1, 2], alloc=[[1, 1, 1], [2, 2, 2]], flags=[2]),              # one flag word for two nodes
    dict(rows=[1], alloc=[[1, 1, 1]], flags=[2], zone=[0, 1]),               # two zone ids for one node
    dict(rows=[1], alloc=[[1, 1, 1]], flags=[2], name_rank=[0, 1, 2]),       # ranks of another cluster size
])
def test_the_wrapper_refuses_columns_of_unequal_length(kwargs):
    ctx = _wrapped(5)
    with pytest.raises(AssertionError):
        ctx.cluster_update(**kwargs)
    assert ctx._lib.calls == []
