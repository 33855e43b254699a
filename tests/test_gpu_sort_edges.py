"""priority_sort_kernel (csrc/gangfit_snapshot.hip) at the edges of its key widths, pass counts, segment geometry and trailing
zeros: the cases of tests/sort_edges.py built on the device and compared bit for bit with oracle/pysnapshot.py — the free
values, and the driver and executor lists.  tests/test_sort_edges_cpu.py proves that each case reaches its arm and that the
comparison tells a memory field one bit too narrow, a reversed tie-break and a dropped cpu group from the right order.  No
decisions are run here: the order is the object (the packers on built snapshots: tests/test_gpu_snapshot_magnitudes.py)."""
import numpy as np
import pytest

import sort_edges as se
from oracle import pysnapshot as ps

CASES = se.cases()
BY_NAME = {c[0]: c for c in CASES}
IDS = [c[0] for c in CASES]
FAMILY = {c[0]: c[1] for c in CASES}
SCALARS_ONLY = 512  # bytes device -> host of a build that stays on the device (the order outputs not counted)
_REF = {}


def _reference(name, ready):
    """oracle.pysnapshot.build of a case, computed once per session and left unchanged."""
    if (name, ready) not in _REF:
        inputs = BY_NAME[name][2]
        avail, _, D, X = ps.build(**(se.all_ready(inputs) if ready else inputs))
        for a in (avail, D, X):
            a.setflags(write=False)
        _REF[(name, ready)] = (avail, D, X)
    return _REF[(name, ready)]


def _first_difference(got, want):
    m = min(len(got), len(want))
    d = np.nonzero(got[:m] != want[:m])[0]
    at = int(d[0]) if len(d) else m
    return f"first difference at position {at}: got {got[at:at + 4].tolist()}, want {want[at:at + 4].tolist()} (lengths {len(got)}, {len(want)})"


def _check(ctx, name, ready, D, X, route=1):
    inputs, promise = BY_NAME[name][2], BY_NAME[name][3]
    avail, rD, rX = _reference(name, ready)
    assert np.array_equal(ctx.snapshot()[0], avail), name
    assert np.array_equal(D, rD), f"{name} drivers: {_first_difference(D, rD)}"
    assert np.array_equal(X, rX), f"{name} executors: {_first_difference(X, rX)}"
    if ready:  # both lists are the whole priority order
        assert len(D) == len(X) == promise["n"]
    info = ctx.build_info()
    if route == 1:
        assert info[:3] == (1, 1 if inputs["driver_label_rank"] is not None else 0, 0), (name, info)
        assert info[3] <= SCALARS_ONLY, (name, info)
    else:
        assert info[0] == 2, (name, info)


def _build(ctx, name, ready):
    inputs = BY_NAME[name][2]
    return ctx.build_snapshot(**(se.all_ready(inputs) if ready else inputs))


@pytest.mark.gpu
@pytest.mark.parametrize("ready", [True, False], ids=["all-ready", "drawn-flags"])
@pytest.mark.parametrize("name", IDS)
def test_device_order_at_the_edges(gf_ctx, name, ready):
    D, X = _build(gf_ctx, name, ready)
    _check(gf_ctx, name, ready, D, X)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in IDS if FAMILY[n] in ("widths", "labels")])
def test_host_finalized_route_installs_the_same_order(gf_ctx, name):
    gf_ctx.set_option("snapshot_finalize_host", 1)
    try:
        D, X = _build(gf_ctx, name, False)
        _check(gf_ctx, name, False, D, X, route=2)
    finally:
        gf_ctx.set_option("snapshot_finalize_host", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in IDS if FAMILY[n] in ("widths", "trailing-zeros")])
def test_resident_path_sorts_from_the_resident_sums(gf_ctx, name):
    """gf_cluster_set, the case's reservation entries through gf_usage_apply, then gf_snapshot_build_resident without any entry:
    the free values come from the resident sums."""
    c = BY_NAME[name][2]
    gf_ctx.set_cluster(c["alloc"], c["node_flags"], c["name_rank"], overhead=c["overhead"], zone=c["zone"], n_zones=c["n_zones"])
    gf_ctx.usage_apply(c["res_node"], c["res_req"], +1)
    D, X = gf_ctx.build_snapshot_resident(resident_usage=True)
    _check(gf_ctx, name, False, D, X)


# (case, every node ready) — None: sixty-four equal nodes of one zone, built in the test: one pass of the one-bit zone field
SEQUENCE = (("n65537", True),                       # 65 537 nodes, 2 passes
            ("label-first-skipped-max255", False),  # 3 groups (the first skipped) + a two-pass label group: 11 passes at 4 097
            ("n1", True),                           # one node, one pass
            ("c22-m40-z3", False),                  # one 64-bit group, 8 passes
            (None, True),
            ("c0-m62-z4", False),                   # 3 groups, the first skipped: 9 passes
            ("n8193", True),                        # 8 193 nodes, 2 passes
            ("c22-m40-z3", False))                  # ... and the 64-bit group again: its first answer


@pytest.mark.gpu
def test_builds_back_to_back_leave_nothing_behind(gf_ctx):
    """Builds of different pass count, group count and size follow each other on the session's context: the count tables, the
    three key / perm buffers beyond a smaller n and the range words of one build must not reach the next."""
    rng = np.random.default_rng(64)
    equal = dict(alloc=np.tile(np.array([[16000, 64 << 30, 0]], dtype=np.int64), (64, 1)),
                 node_flags=np.full(64, ps.READY | ps.DRIVER_CANDIDATE, dtype=np.uint32),
                 name_rank=rng.permutation(64).astype(np.uint32), zone=np.zeros(64, dtype=np.uint32), n_zones=1)
    assert se.plan([16000] * 64, [64 << 30] * 64, 1)["groups"] == [1]
    first = {}
    for step, (name, ready) in enumerate(SEQUENCE):
        if name is None:
            D, X = gf_ctx.build_snapshot(**equal)
            by_name = np.argsort(equal["name_rank"])
            assert np.array_equal(ps.build(**equal)[2], by_name)
            assert np.array_equal(D, by_name) and np.array_equal(X, by_name), f"step {step}: {_first_difference(D, by_name)}"
            assert gf_ctx.build_info()[:3] == (1, 0, 0)
            continue
        D, X = _build(gf_ctx, name, ready)
        _check(gf_ctx, name, ready, D, X)
        if name in first:
            assert np.array_equal(D, first[name][0]) and np.array_equal(X, first[name][1])
        first.setdefault(name, (D, X))
