"""gf_cluster_fit_feasible: the UnschedulablePodMarker's empty-cluster question (internal/extender/unschedulablepods.go:132-166)
answered from the resident cluster columns.  Every packer's answer must equal, bit for bit, the CPU oracle on the snapshot
oracle/pysnapshot.py builds from the same inputs with no reservations — the selected nodes as driver AND executor candidates —
and gf_fit_feasible after a real gf_snapshot_build of those inputs on a second context; and the call must leave everything the
warm Filter lives on as it found it."""
import numpy as np
import pytest

import cluster_scan_cases as cs
import gangfit
from gangfit import _native as N
from gangfit import workloads as wl
from oracle import binding as ob
from oracle import pysnapshot as ps
from test_snapshot_build import GIB, _cluster

pytestmark = pytest.mark.gpu
FIFO = gangfit.GF_MODE_FIFO_CHAIN
TIGHT = gangfit.GF_ALGO_TIGHTLY_PACK
ZONE_AWARE = (cs.AZ_AWARE,) + cs.SINGLE_AZ
PRESET = 0xAB


@pytest.fixture(scope="module")
def second():
    """the context that really installs what the scan only imagines"""
    with gangfit.Context(0) as ctx:
        yield ctx


def _everyone(c):
    return np.full(len(c["alloc"]), ps.READY | ps.DRIVER_CANDIDATE, dtype=np.uint32)


def _set_cluster(ctx, c):
    # the cluster's own flags and resident overhead are NOT what the scan reads: candidates and overhead come with the call
    ctx.set_cluster(c["alloc"], np.zeros(len(c["alloc"]), dtype=np.uint32), c["name_rank"], overhead=None, zone=c["zone"],
                    n_zones=c["n_zones"])


def _installed(second, c, select, over, algo, apps):
    second.build_snapshot(c["alloc"], cs.flags_of(select), c["name_rank"], overhead=over, zone=c["zone"], n_zones=c["n_zones"],
                          want_orders=False)
    return second.fit_feasible(algo, apps).astype(np.uint8)


def _raw(ctx, algo, over_cols, select, apps, out, n_apps=None):
    """the C entry point with the pointers as given (None = NULL): its return code"""
    cols = [None if col is None else np.ascontiguousarray(col, dtype=np.int64) for col in over_cols]
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.uint8)
    return ctx._lib.gf_cluster_fit_feasible(ctx._h, algo, *[N.ptr(col) for col in cols], N.ptr(sel),
                                            len(apps) if n_apps is None else n_apps, N.ptr(apps), N.ptr(out))


@pytest.mark.parametrize("n_zones", cs.ZONE_COUNTS)
@pytest.mark.parametrize("n", cs.NODE_COUNTS)
def test_every_packer_equals_the_oracle_and_an_installed_snapshot(gf_ctx, second, n, n_zones):
    seed = cs.seed_of(n, n_zones)
    c = cs.cluster(seed, n, n_zones)
    drv, exe, k = cs.applications(seed, c)
    apps = gangfit.make_apps(drv, exe, k)
    _set_cluster(gf_ctx, c)
    everyone = np.ones(n, dtype=bool)
    without_a_zone = c["zone"] != c["zone"][n // 2]
    nobody = np.zeros(n, dtype=bool)
    for over in (None, c["overhead"]):
        ref = cs.reference(c, everyone, drv, exe, k, overhead=over)
        for algo in cs.ALGOS:
            # the K edges of cluster_scan_cases.applications: 0, above the total, the driver's node counted after the driver, gpu
            # executors on the gpu minority — the oracle alone must answer both ways often enough for the comparison to mean something
            assert ref[algo].sum() >= 5 and (ref[algo] == 0).sum() >= 5, (n, n_zones, algo, int(ref[algo].sum()))
            for n_apps in (70, 7, 1):
                got = gf_ctx.cluster_fit_feasible(algo, apps[:n_apps], overhead=over).astype(np.uint8)
                assert got.tobytes() == ref[algo][:n_apps].tobytes(), (n, n_zones, algo, n_apps, over is not None)
            assert _installed(second, c, everyone, over, algo, apps).tobytes() == ref[algo].tobytes(), (n, n_zones, algo)
        # a selection that leaves out a whole zone; "every node" spelled out; one that leaves out every node
        ref_part = cs.reference(c, without_a_zone, drv, exe, k, overhead=over)
        for algo in cs.ALGOS:
            got = gf_ctx.cluster_fit_feasible(algo, apps, overhead=over, node_select=without_a_zone).astype(np.uint8)
            assert got.tobytes() == ref_part[algo].tobytes(), (n, n_zones, algo, "without a zone")
            got = gf_ctx.cluster_fit_feasible(algo, apps, overhead=over, node_select=everyone).astype(np.uint8)
            assert got.tobytes() == ref[algo].tobytes(), (n, n_zones, algo, "everyone")
            got = gf_ctx.cluster_fit_feasible(algo, apps, overhead=over, node_select=nobody)
            assert not got.any(), (n, n_zones, algo, "nobody")
        for algo in (TIGHT, cs.SINGLE_AZ[0], cs.SINGLE_AZ[1]) if without_a_zone.any() else ():
            assert _installed(second, c, without_a_zone, over, algo, apps).tobytes() == ref_part[algo].tobytes(), (n, n_zones, algo)


def test_an_overhead_above_the_allocatable_serves_the_plain_packers_only(gf_ctx, second):
    n, n_zones = 65, 3
    seed = cs.seed_of(n, n_zones)
    c = cs.cluster(seed, n, n_zones)
    drv, exe, k = cs.applications(seed, c)
    apps = gangfit.make_apps(drv, exe, k)
    over = c["overhead"].copy()
    over[7] = c["alloc"][7] + np.array([1000, 0, 0])      # cpu short by one core: a negative available quantity
    over[64] = c["alloc"][64] + np.array([0, GIB, 0])     # ... and memory, in the second chunk
    _set_cluster(gf_ctx, c)
    everyone = np.ones(n, dtype=bool)
    ref = cs.reference(c, everyone, drv, exe, k, overhead=over)
    for algo in cs.PLAIN:
        assert ref[algo].sum() >= 5 and (ref[algo] == 0).sum() >= 5
        got = gf_ctx.cluster_fit_feasible(algo, apps, overhead=over).astype(np.uint8)
        assert got.tobytes() == ref[algo].tobytes(), algo
        assert _installed(second, c, everyone, over, algo, apps).tobytes() == ref[algo].tobytes(), algo
    cols = [over[:, j] for j in range(3)]
    for algo in ZONE_AWARE:
        out = np.full(len(apps), PRESET, dtype=np.uint8)
        assert _raw(gf_ctx, algo, cols, None, apps, out) == N.GF_ERR_UNSUPPORTED, algo
        assert (out == PRESET).all(), algo


def test_refusals_leave_the_answers_as_preset(gf_ctx):
    n, n_zones = 64, 3
    seed = cs.seed_of(n, n_zones)
    c = cs.cluster(seed, n, n_zones)
    drv, exe, k = cs.applications(seed, c)
    apps = gangfit.make_apps(drv, exe, k)[:7]
    good = [c["overhead"][:, j] for j in range(3)]
    none = [None, None, None]
    out = np.full(len(apps), PRESET, dtype=np.uint8)

    def refused(code, what, ctx, algo, cols, use_apps):
        assert _raw(ctx, algo, cols, None, use_apps, out) == code, what
        assert (out == PRESET).all(), what

    with gangfit.Context(0) as fresh:  # no gf_cluster_set yet
        refused(N.GF_ERR_STATE, "no cluster", fresh, TIGHT, none, apps)
    _set_cluster(gf_ctx, c)
    gf_ctx.build_snapshot_resident(node_flags=_everyone(c), want_orders=False)
    v = gf_ctx.view()
    try:
        refused(N.GF_ERR_STATE, "a view", v, TIGHT, none, apps)
    finally:
        v.close()
    for missing in range(3):
        cols = list(good)
        cols[missing] = None
        refused(N.GF_ERR_INVALID, f"overhead column {missing} NULL", gf_ctx, TIGHT, cols, apps)
    for bad in (-1, 1 << 61):
        cols = [col.copy() for col in good]
        cols[1][n - 1] = bad
        refused(N.GF_ERR_INVALID, f"an overhead of {bad}", gf_ctx, TIGHT, cols, apps)
    for bad_k in (-1, N.GF_MAX_K + 1):
        wrong = apps.copy()
        wrong["k"][3] = bad_k
        refused(N.GF_ERR_INVALID, f"k = {bad_k}", gf_ctx, TIGHT, good, wrong)
    no_request = apps.copy()
    no_request["drv"][5] = [0, 0, 1]  # neither cpu nor memory: chooseBestResult's average could be 0
    for algo in ZONE_AWARE:
        refused(N.GF_ERR_UNSUPPORTED, "a driver without cpu and memory", gf_ctx, algo, good, no_request)
    for algo in cs.PLAIN:  # ... which the plain packers do not look at
        assert _raw(gf_ctx, algo, good, None, no_request, np.zeros(len(apps), dtype=np.uint8)) == N.GF_OK
    # more than 64 zones
    wide = dict(c, zone=(np.arange(n) % 65).astype(np.uint32), n_zones=65)
    _set_cluster(gf_ctx, wide)
    for algo in ZONE_AWARE:
        refused(N.GF_ERR_UNSUPPORTED, "65 zones", gf_ctx, algo, good, apps)
    ref = cs.reference(wide, np.ones(n, dtype=bool), drv[:7], exe[:7], k[:7], overhead=c["overhead"])
    for algo in cs.PLAIN:
        assert gf_ctx.cluster_fit_feasible(algo, apps, overhead=c["overhead"]).astype(np.uint8).tobytes() == ref[algo].tobytes()
    # no application: GF_OK, nothing written, even with nothing to point at
    assert _raw(gf_ctx, TIGHT, good, None, apps, out, n_apps=0) == N.GF_OK and (out == PRESET).all()
    assert gf_ctx._lib.gf_cluster_fit_feasible(gf_ctx._h, TIGHT, None, None, None, None, 0, None, None) == N.GF_OK


def test_the_scan_leaves_the_warm_filter_alone():
    n = 2500
    c = _cluster(95, n, 300, 3, with_overhead=True, labels=False)
    w = wl.config(2, n_nodes=16, n_apps=48)
    flags = np.ones(len(w.k), dtype=np.uint32)
    apps, oapps = gangfit.make_apps(w.drv, w.exe, w.k, flags), ob.make_apps(w.drv, w.exe, w.k, flags)
    select = np.random.default_rng(5).random(n) < 0.7
    with gangfit.Context(0) as ctx:
        ctx.set_cluster(c["alloc"], c["node_flags"], c["name_rank"], overhead=c["overhead"], zone=c["zone"], n_zones=c["n_zones"])
        ctx.usage_apply(c["res_node"], c["res_req"], +1)
        D, X = ctx.build_snapshot_resident(resident_usage=True)
        first = ctx.fit_batch(FIFO, TIGHT, apps)  # the Filter
        ref = ob.fit_fifo_chain(TIGHT, ctx.snapshot()[0], oapps, D, X)
        assert first.failed_at == ref.failed_at and np.array_equal(first.results, ref.results)

        def state():
            avail, sched = ctx.snapshot()
            return ctx.generation(), avail.tobytes(), sched.tobytes(), ctx.residual().tobytes(), ctx.chain_cache_stats()

        before = state()
        scan_ref = cs.reference(c, select, w.drv, w.exe, w.k, overhead=c["overhead"])
        for algo in cs.ALGOS:  # the marker's minute: every packer, on other overhead and candidates than the installed ones
            got = ctx.cluster_fit_feasible(algo, apps, overhead=c["overhead"], node_select=select).astype(np.uint8)
            assert got.tobytes() == scan_ref[algo].tobytes(), algo
        assert state() == before, "the scan moved a generation, the snapshot, the residual table or the chain cache"
        ctx.chain_cache_stats(reset=True)
        again = ctx.fit_batch(FIFO, TIGHT, apps)  # the same Filter: a resume, not a replay
        chains, resumed, evaluated, skipped = ctx.chain_cache_stats()
        assert (chains, resumed) == (1, 1) and skipped > 0, (chains, resumed, evaluated, skipped)
        assert again.failed_at == first.failed_at and again.results.tobytes() == first.results.tobytes()
        assert again.exec_nodes.tobytes() == first.exec_nodes.tobytes()
        assert ctx.residual().tobytes() == before[3]


def test_a_multi_device_context_answers_from_its_first_device():
    n, n_zones = 130, 3
    seed = cs.seed_of(n, n_zones)
    c = cs.cluster(seed, n, n_zones)
    drv, exe, k = cs.applications(seed, c)
    apps = gangfit.make_apps(drv, exe, k)
    ref = cs.reference(c, np.ones(n, dtype=bool), drv, exe, k, overhead=c["overhead"])
    with gangfit.Context(devices=[0] * 3) as g:
        _set_cluster(g, c)
        for algo in cs.ALGOS:
            assert g.cluster_fit_feasible(algo, apps, overhead=c["overhead"]).astype(np.uint8).tobytes() == ref[algo].tobytes(), algo
