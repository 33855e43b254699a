"""The other consumers of a layout that gf_snapshot_build_resident_set installed — the resident worker, single executors, findNodes,
the efficiencies — against a context that holds only the members (tests/snapshot_sets.py maps the indices back).

In a file of its own, on contexts of its own: a test that starts the resident worker makes streams, and where a launch lands next
to a resident worker depends on the streams a process has made (tests/test_gpu_worker.py); this file sorts behind every test
that looks at that."""
import numpy as np
import pytest

import gangfit
import snapshot_sets as ss
from gangfit import workloads as wl
from oracle import binding as ob


@pytest.mark.gpu
def test_other_consumers_of_the_layout():
    with gangfit.Context(0) as ctx, gangfit.Context(0) as members_ctx:
        try:
            _other_consumers(ctx, members_ctx)
        finally:
            ctx.worker_stop()


def _other_consumers(gf_ctx, members_ctx):
    n = 300
    rng = np.random.default_rng(10)
    c = ss.cluster(1000, n, 120, 3)
    members = rng.random(n) < 0.5
    ss.install(gf_ctx, c, resident=True)
    D, X = ss.build_set(gf_ctx, c, members, resident=True)
    r = ss.build(c, members)
    M, m, i = r.M, len(r.M), r.inputs
    members_ctx.set_cluster(i["alloc"], i["node_flags"], i["name_rank"], overhead=i["overhead"], zone=i["zone"], n_zones=i["n_zones"])
    members_ctx.build_snapshot_resident(res_node=i["res_node"], res_req=i["res_req"])
    apps, oapps = ss.apps_for(m)
    for algo in (0, 1, 4):  # the resident worker reads the slot records: their node word is the cluster's index
        mine, ref = gf_ctx.worker_fit(algo, apps), ob.fit_independent(algo, r.avail_c, oapps, r.D_c, r.X_c, sched=r.sched_c, zone=i["zone"])
        assert np.array_equal(mine.results, ss.results_to_cluster(ref.results, M)), algo
        for a in np.nonzero(ref.results["has_capacity"])[0]:
            assert np.array_equal(mine.placement(int(a))[2], ss.to_cluster(ref.placement(int(a))[2], M)), (algo, a)
    exe = np.array([[1000, 4 * ss.GIB, 0], [8000, 64 * ss.GIB, 0], [1000, ss.GIB, 1], [200000, ss.GIB, 0]], dtype=np.int64)
    reserved = np.zeros((n, 3), dtype=np.int64)
    reserved[M[::3]] = [2000, 8 * ss.GIB, 0]
    reserved[~members] = [1 << 40, 1 << 50, 5]  # rows of non-members: never read
    for mf in (False, True):
        got = gf_ctx.executor_fit(exe, reserved=reserved, minimal_fragmentation=mf)
        want = members_ctx.executor_fit(exe, reserved=reserved[M], minimal_fragmentation=mf)
        assert np.array_equal(got, ss.to_cluster(want, M)), mf
    k = np.array([3, 40, 1], dtype=np.int32)
    got, want = gf_ctx.find_nodes(exe[:3], k), members_ctx.find_nodes(exe[:3], k)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], ss.to_cluster(want[1], M))
    for q in range(3):
        o, p = int(got[2][q]), int(got[0][q])
        assert np.array_equal(got[3][o:o + p], ss.to_cluster(want[3][o:o + p], M))
    assert np.array_equal(got[4][:, M], want[4]) and not got[4][:, ~members].any()
    ref = ob.fit_independent(0, r.avail_c, oapps, r.D_c, r.X_c, sched=r.sched_c, zone=i["zone"])
    a = int(np.nonzero(ref.results["has_capacity"])[0][0])
    drv, xs = int(ref.results[a]["driver_node"]), ref.placement(a)[2]
    w = wl.config(2, n_nodes=16, n_apps=min(64, 4 * m))
    eff = gf_ctx.packing_efficiencies(0, w.drv[a], w.exe[a], int(M[drv]), ss.to_cluster(xs, M))
    eff_c = members_ctx.packing_efficiencies(0, w.drv[a], w.exe[a], drv, xs)
    assert np.array_equal(eff[M], eff_c)  # (the rows of non-members are outside the contract)
