"""gf_cluster_executor_fit at the drop-in boundary: declared in include/gangfit.h with its twelve parameters, exported by
libgangfit.so, bound in gangfit/_native.py, refusing a NULL context before anything else (no GPU); and, on a device, every
refusal the header lists — each with its code, nothing changed and node_out as preset."""
import ctypes
import os
import re

import numpy as np
import pytest

import cluster_executor_cases as xc
import gangfit
from gangfit import _native, build
from gangfit import _native as N
from test_abi_overhead import REPO, _declared_symbols

PRESET = 0xABABABAB


def test_cluster_executor_fit_is_declared_exported_and_bound():
    assert "gf_cluster_executor_fit" in _declared_symbols()
    lib = ctypes.CDLL(build.build_native())
    assert hasattr(lib, "gf_cluster_executor_fit")
    assert "gf_cluster_executor_fit" in _native.EXPORTED_SYMBOLS
    L = _native.load()
    assert L.gf_cluster_executor_fit.restype is ctypes.c_int32 and len(L.gf_cluster_executor_fit.argtypes) == 12


def test_the_declared_signature():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gangfit.h")).read(), flags=re.S)
    m = re.search(r"int\s+gf_cluster_executor_fit\s*\(([^)]*)\)\s*;", text)
    assert m is not None
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["gf_ctx *ctx", "int minimal_fragmentation", "uint32_t n_sets", "const uint64_t *set_words", "uint32_t n_req",
                      "const int64_t *exe", "const uint32_t *req_set", "const uint32_t *hosts_app", "const uint32_t *node_zone",
                      "const uint32_t *req_zone", "const uint32_t *exec_label_rank", "uint32_t *node_out"]


def test_a_null_context_is_invalid():
    L = _native.load()
    exe = np.zeros((1, 3), dtype=np.int64)
    out = np.full(1, PRESET, dtype=np.uint32)
    rc = L.gf_cluster_executor_fit(None, 0, 0, None, 1, _native.ptr(exe), None, None, None, None, None, _native.ptr(out))
    assert rc == _native.GF_ERR_INVALID and out[0] == PRESET


def _raw(ctx, mf=0, n_sets=0, words=None, n_req=None, exe=None, req_set=None, hosts=None, node_zone=None, req_zone=None, label=None,
         out=None):
    """the C entry point with the pointers as given (None = NULL): its return code"""
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)  # noqa: E731
    exe, words, req_set, hosts = arr(exe, np.int64), arr(words, np.uint64), arr(req_set, np.uint32), arr(hosts, np.uint32)
    node_zone, req_zone, label = arr(node_zone, np.uint32), arr(req_zone, np.uint32), arr(label, np.uint32)
    n_req = (0 if exe is None else len(exe.reshape(-1, 3))) if n_req is None else n_req
    return ctx._lib.gf_cluster_executor_fit(ctx._h, mf, n_sets, N.ptr(words), n_req, N.ptr(exe), N.ptr(req_set), N.ptr(hosts),
                                            N.ptr(node_zone), N.ptr(req_zone), N.ptr(label), N.ptr(out))


def _set(ctx, c):
    ctx.set_cluster(c["alloc"], c["flags"], c["name_rank"], overhead=c["overhead"], zone=c["zone"], n_zones=c["n_zones"])


@pytest.mark.gpu
def test_every_refusal_leaves_the_answers_as_preset(gf_ctx):
    n = 70  # two words per row, six bits used in the last
    c = xc.cluster(5, n, "three")
    exe = xc.requests(5, n_req=4)
    out = np.full(len(exe), PRESET, dtype=np.uint32)
    full = gangfit.pack_node_sets(np.ones((2, n), dtype=bool), n)

    def refused(code, what, ctx, **kw):
        before = ctx.generation()
        assert _raw(ctx, out=out, **{"exe": exe, **kw}) == code, what
        assert (out == PRESET).all(), what
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
    for bad in (-1, 1 << 62):
        wrong = exe.copy()
        wrong[2, 1] = bad
        refused(N.GF_ERR_INVALID, f"a request of {bad}", gf_ctx, exe=wrong)
    refused(N.GF_ERR_INVALID, "req_set names no set", gf_ctx, n_sets=2, words=full, req_set=[0, 1, 2, 0])
    refused(N.GF_ERR_INVALID, "req_set NULL with sets", gf_ctx, n_sets=2, words=full, req_set=None)
    refused(N.GF_ERR_INVALID, "set_words NULL with sets", gf_ctx, n_sets=2, words=None, req_set=[0, 1, 1, 0])
    beyond = full.copy()
    beyond[1, -1] |= np.uint64(1) << np.uint64(n & 63)  # node 70 of a cluster of 70
    refused(N.GF_ERR_INVALID, "a bit at n_nodes", gf_ctx, n_sets=2, words=beyond, req_set=[0, 0, 0, 0])
    beyond = full.copy()
    beyond[0, -1] |= np.uint64(1) << np.uint64(63)
    refused(N.GF_ERR_INVALID, "a bit beyond n_nodes", gf_ctx, n_sets=2, words=beyond, req_set=[1, 1, 1, 1])
    refused(N.GF_ERR_INVALID, "node_zone without req_zone", gf_ctx, node_zone=c["zone"])
    any_zone = c["zone"].copy()
    any_zone[n - 1] = xc.ANY
    refused(N.GF_ERR_INVALID, "a node_zone entry GF_ANY_ZONE", gf_ctx, node_zone=any_zone, req_zone=[0, 1, 2, xc.ANY])
    assert _raw(gf_ctx, exe=None, n_req=4, out=out) == N.GF_ERR_INVALID and (out == PRESET).all()
    assert _raw(gf_ctx, exe=exe, out=None) == N.GF_ERR_INVALID
    # ... and what it serves: the same pointers, valid
    assert _raw(gf_ctx, exe=exe, n_sets=2, words=full, req_set=[0, 1, 1, 0], node_zone=c["zone"], req_zone=[0, 1, 2, xc.ANY], out=out) == N.GF_OK
    assert (out != PRESET).all()
    # no request: GF_OK, nothing written, even with nothing to point at
    out[:] = PRESET
    assert _raw(gf_ctx, exe=exe, n_req=0, out=out) == N.GF_OK and (out == PRESET).all()
    assert gf_ctx._lib.gf_cluster_executor_fit(gf_ctx._h, 0, 0, None, 0, None, None, None, None, None, None, None) == N.GF_OK
    # more than 64 zones
    wide = dict(c, zone=(np.arange(n) % 65).astype(np.uint32), n_zones=65)
    _set(gf_ctx, wide)
    refused(N.GF_ERR_UNSUPPORTED, "65 zones", gf_ctx)
    refused(N.GF_ERR_UNSUPPORTED, "65 zones, minimal fragmentation", gf_ctx, mf=1)


@pytest.mark.gpu
def test_a_removal_below_zero_entries_is_refused_and_the_count_follows_every_update():
    """A removal that takes a node's entry count below zero is refused like one that takes a sum below zero — the sums of an
    all-zero entry cannot tell —, and leaves the resident usage usable; the call then still answers."""
    c, res_node, res_req, kw, right, wrong = xc.case_zero_valued_entry()
    with gangfit.Context(0) as ctx:
        _set(ctx, c)
        with pytest.raises(N.GangfitError) as e:
            ctx.usage_apply(res_node, res_req, -1)  # never added
        assert e.value.code == N.GF_ERR_INVALID
        assert ctx.cluster_executor_fit(kw["exe"]).tolist() == [wrong]  # no entry: the overhead counts once
        ctx.usage_apply(res_node, res_req, +1)
        assert ctx.cluster_executor_fit(kw["exe"]).tolist() == [right]
        ctx.usage_apply(res_node, res_req, -1)
        assert ctx.cluster_executor_fit(kw["exe"]).tolist() == [wrong]
        ctx.usage_apply(res_node, res_req, +1)
        ctx.usage_reset()
        assert ctx.cluster_executor_fit(kw["exe"]).tolist() == [wrong]
