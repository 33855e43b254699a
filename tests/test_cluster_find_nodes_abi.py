"""gf_cluster_find_nodes at the drop-in boundary: declared in include/gangfit.h with its fourteen parameters, exported by
libgangfit.so, bound in gangfit/_native.py, refusing a NULL context before anything else (no GPU); and, on a device, every
refusal the header lists — each with its code, the outputs as preset and gf_generation unchanged."""
import ctypes
import os
import re

import numpy as np
import pytest

import cluster_find_nodes_cases as fc
import gangfit
from gangfit import _native, build
from gangfit import _native as N
from test_abi_overhead import REPO, _declared_symbols

PRESET = 0xABABABAB
PRESET64 = -0x0123456789ABCDEF


def test_cluster_find_nodes_is_declared_exported_and_bound():
    assert "gf_cluster_find_nodes" in _declared_symbols()
    lib = ctypes.CDLL(build.build_native())
    assert hasattr(lib, "gf_cluster_find_nodes")
    assert "gf_cluster_find_nodes" in _native.EXPORTED_SYMBOLS
    L = _native.load()
    assert L.gf_cluster_find_nodes.restype is ctypes.c_int32 and len(L.gf_cluster_find_nodes.argtypes) == 14
    assert hasattr(gangfit.Context, "cluster_find_nodes")


def test_the_declared_signature():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gangfit.h")).read(), flags=re.S)
    m = re.search(r"int\s+gf_cluster_find_nodes\s*\(([^)]*)\)\s*;", text)
    assert m is not None
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["gf_ctx *ctx", "int chained", "uint32_t n_sets", "const uint64_t *set_words", "const uint32_t *create_rank",
                      "uint32_t n_req", "const int64_t *exe", "const int32_t *k", "const uint32_t *req_set", "gf_find_result *results",
                      "uint32_t *exec_nodes", "uint64_t exec_nodes_cap", "uint32_t *reserved_adds", "int64_t *residual_out"]


def test_a_null_context_is_invalid():
    L = _native.load()
    exe, k, rank = np.zeros((1, 3), dtype=np.int64), np.ones(1, dtype=np.int32), np.zeros(1, dtype=np.uint32)
    res, out = np.full((1, 2), PRESET, dtype=np.uint32), np.full(2, PRESET, dtype=np.uint32)
    rc = L.gf_cluster_find_nodes(None, 1, 0, None, N.ptr(rank), 1, N.ptr(exe), N.ptr(k), None, N.ptr(res), N.ptr(out), 1, None, None)
    assert rc == _native.GF_ERR_INVALID and (res == PRESET).all() and (out == PRESET).all()


class _Outputs:
    def __init__(self, n_req, n, cap):
        self.res = np.full((n_req, 2), PRESET, dtype=np.uint32)
        self.nodes = np.full(cap + 1, PRESET, dtype=np.uint32)
        self.adds = np.full((n_req, n), PRESET, dtype=np.uint32)
        self.residual = np.full((n, 3), PRESET64, dtype=np.int64)

    def untouched(self):
        return ((self.res == PRESET).all() and (self.nodes == PRESET).all() and (self.adds == PRESET).all()
                and (self.residual == PRESET64).all())


def _raw(ctx, o, chained=1, n_sets=0, words=None, rank=None, n_req=None, exe=None, k=None, req_set=None, cap=None, results=True,
         nodes=True):
    """the C entry point with the pointers as given (None = NULL): its return code"""
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)  # noqa: E731
    exe, k, words, rank, req_set = arr(exe, np.int64), arr(k, np.int32), arr(words, np.uint64), arr(rank, np.uint32), arr(req_set, np.uint32)
    n_req = (0 if k is None else len(k)) if n_req is None else n_req
    cap = len(o.nodes) - 1 if cap is None else cap
    return ctx._lib.gf_cluster_find_nodes(ctx._h, chained, n_sets, N.ptr(words), N.ptr(rank), n_req, N.ptr(exe), N.ptr(k), N.ptr(req_set),
                                          N.ptr(o.res) if results else None, N.ptr(o.nodes) if nodes else None, cap, N.ptr(o.adds),
                                          N.ptr(o.residual))


def _set(ctx, c):
    ctx.set_cluster(c["alloc"], c["flags"], c["name_rank"], overhead=c["overhead"])


@pytest.mark.gpu
def test_every_refusal_leaves_the_outputs_as_preset(gf_ctx):
    n = 70  # two words per row, six bits used in the last
    c = fc.cluster(5, n)
    exe = np.array([[1000, fc.GIB, 0], [250, 0, 0], [0, 0, 1], [0, 0, 0]], dtype=np.int64)
    k = np.array([3, 0, 2, 5], dtype=np.int32)
    rank = fc.create_rank("random", n, 5)
    o = _Outputs(len(k), n, int(k.sum()))
    halves = np.zeros((2, n), dtype=bool)
    halves[0, :40], halves[1, 40:] = True, True
    words = gangfit.pack_node_sets(halves, n)
    good = dict(rank=rank, exe=exe, k=k)

    def refused(code, what, ctx, **kw):
        before = ctx.generation()
        assert _raw(ctx, o, **{**good, **kw}) == code, what
        assert o.untouched(), what
        assert ctx.generation() == before, what

    with gangfit.Context(0) as fresh:  # no gf_cluster_set yet
        refused(N.GF_ERR_STATE, "no cluster", fresh)
    _set(gf_ctx, c)
    gf_ctx.build_snapshot_resident(want_orders=False)
    v = gf_ctx.view()
    try:
        refused(N.GF_ERR_STATE, "a view", v)
    finally:
        v.close()
    refused(N.GF_ERR_INVALID, "create_rank NULL", gf_ctx, rank=None)
    twice = rank.copy()
    twice[3] = twice[4]
    refused(N.GF_ERR_INVALID, "a rank twice", gf_ctx, rank=twice)
    large = rank.copy()
    large[int(np.argmax(rank))] = n
    refused(N.GF_ERR_INVALID, "a rank of n_nodes", gf_ctx, rank=large)
    for bad in (-1, 1 << 62):
        wrong = exe.copy()
        wrong[2, 1] = bad
        refused(N.GF_ERR_INVALID, f"a request of {bad}", gf_ctx, exe=wrong)
    for bad in (-1, fc.MAX_K + 1):
        wrong = k.copy()
        wrong[1] = bad
        refused(N.GF_ERR_INVALID, f"k = {bad}", gf_ctx, k=wrong, cap=1 << 40)
    refused(N.GF_ERR_INVALID, "req_set names no set", gf_ctx, n_sets=2, words=words, req_set=[0, 1, 2, 0])
    refused(N.GF_ERR_INVALID, "req_set NULL with sets", gf_ctx, n_sets=2, words=words, req_set=None)
    refused(N.GF_ERR_INVALID, "set_words NULL with sets", gf_ctx, n_sets=2, words=None, req_set=[0, 1, 1, 0])
    beyond = words.copy()
    beyond[1, -1] |= np.uint64(1) << np.uint64(n & 63)  # node 70 of a cluster of 70
    refused(N.GF_ERR_INVALID, "a bit at n_nodes", gf_ctx, n_sets=2, words=beyond, req_set=[0, 0, 0, 0])
    beyond = words.copy()
    beyond[0, -1] |= np.uint64(1) << np.uint64(63)
    refused(N.GF_ERR_INVALID, "a bit beyond n_nodes", gf_ctx, n_sets=2, words=beyond, req_set=[1, 1, 1, 1])
    overlap = halves.copy()
    overlap[1, 39] = True  # node 39 in both rows
    refused(N.GF_ERR_INVALID, "overlapping rows, chained", gf_ctx, n_sets=2, words=gangfit.pack_node_sets(overlap, n), req_set=[0, 1, 1, 0])
    refused(N.GF_ERR_INVALID, "exe NULL", gf_ctx, exe=None)
    refused(N.GF_ERR_INVALID, "k NULL", gf_ctx, k=None, n_req=4)
    refused(N.GF_ERR_INVALID, "results NULL", gf_ctx, results=False)
    refused(N.GF_ERR_CAPACITY, "exec_nodes too small", gf_ctx, cap=int(k.sum()) - 1)
    refused(N.GF_ERR_CAPACITY, "exec_nodes NULL", gf_ctx, nodes=False)
    # ... and what it serves: overlapping rows when not chained, equal rows under two numbers when chained, the same pointers valid
    assert _raw(gf_ctx, o, chained=0, n_sets=2, words=gangfit.pack_node_sets(overlap, n), req_set=[0, 1, 1, 0], **good) == N.GF_OK
    assert not o.untouched()
    same = gangfit.pack_node_sets(np.stack([halves[0], halves[1], halves[0]]), n)
    assert _raw(gf_ctx, o, n_sets=3, words=same, req_set=[0, 1, 2, 0], **good) == N.GF_OK
    # no request: GF_OK, nothing written, even with nothing to point at
    o = _Outputs(len(k), n, int(k.sum()))
    assert _raw(gf_ctx, o, n_req=0, **good) == N.GF_OK and o.untouched()
    assert gf_ctx._lib.gf_cluster_find_nodes(gf_ctx._h, 1, 0, None, None, 0, None, None, None, None, None, 0, None, None) == N.GF_OK



@pytest.mark.gpu
def test_unusable_resident_usage_or_overhead_is_a_state_error():
    """What a gf_usage_apply / gf_overhead_update that failed half way leaves behind (option update_fault): the call refuses until
    gf_usage_reset / gf_cluster_set have replaced what is unknown."""
    n = 20
    c = fc.cluster(6, n)
    exe, k, rank = np.array([[1000, fc.GIB, 0]], dtype=np.int64), np.array([2], dtype=np.int32), fc.create_rank("identity", n, 0)
    with gangfit.Context(0) as ctx:
        _set(ctx, c)
        for fault, what in ((1, "usage"), (2, "overhead")):
            o = _Outputs(1, n, 2)
            assert _raw(ctx, o, rank=rank, exe=exe, k=k) == N.GF_OK and not o.untouched()
            ctx.set_option("update_fault", fault)
            o = _Outputs(1, n, 2)
            before = ctx.generation()
            assert _raw(ctx, o, rank=rank, exe=exe, k=k) == N.GF_ERR_STATE and what in ctx.last_error()
            assert o.untouched() and ctx.generation() == before
            if fault == 1:
                ctx.usage_reset()
            else:
                _set(ctx, c)
