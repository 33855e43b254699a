"""GPU parity at the edges of the quantity contract (include/gangfit.h: available in (-2^62, 2^62), requests in [0, 2^62),
K in [0, GF_MAX_K]), on the problems of tests/magnitudes.py: every packer, both modes, every context of the stress harness,
bit for bit against the oracle — where the kernels' reciprocal estimates, fix-ups, clamps, 64-bit division branches,
narrow-domain bounds and float64 roundings decide.  `python -m pytest tests/test_gpu_magnitudes.py -m gpu`."""
import numpy as np
import pytest

import gangfit
import magnitudes as mg
import stress_lib
from oracle import binding as ob
from oracle import pysnapshot as ps

pytestmark = pytest.mark.gpu

IND, FIFO = gangfit.GF_MODE_INDEPENDENT, gangfit.GF_MODE_FIFO_CHAIN
ALGOS = (0, 1, 2, 3, 4, 5)
CONTEXTS = stress_lib.CONTEXTS + (("independent-zones", {"zoned_fused": 0}),)
INVALID = gangfit._native.GF_ERR_INVALID


@pytest.fixture(scope="module")
def ctxs():
    cs = {name: gangfit.Context(0, options=opts) for name, opts in CONTEXTS}
    yield cs
    for c in cs.values():
        c.close()


def _install(ctx, p):
    avail, sched, zone, D, X = p[:5]
    ctx.set_snapshot(avail, sched)
    ctx.set_zones(zone)
    ctx.set_orders(D, X)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _refs(regime, p):
    avail, sched, zone, D, X, drv, exe, k, flags = p
    apps = ob.make_apps(drv, exe, k, flags)
    cf = mg.CLOSED_FORM[regime]
    return {algo: (ob.fit_independent(algo, avail, apps, D, X, closed_form=cf, sched=sched, zone=zone),
                   ob.fit_fifo_chain(algo, avail, apps, D, X, closed_form=cf, sched=sched, zone=zone)) for algo in ALGOS}


_REFS = {}


def _cases(regime):
    """The regime's cases with the oracle's answers, computed once per module run."""
    if regime not in _REFS:
        _REFS[regime] = [(name, p, route, _refs(regime, p)) for name, p, route in mg.cases(regime)]
    return _REFS[regime]


@pytest.mark.parametrize("regime", mg.REGIMES)
def test_every_packer_and_context_bit_exact(ctxs, regime):
    """Results, placements, failed_at and residuals of all six packers in both modes, gf_fit_feasible, and the averages
    chooseBestResult compares, in the stress harness's contexts plus the four-kernel zone route.  Guards cap_dim
    (gangfit_kernels.hip: estimate, +-1 fix-up, clamp at k + 1), cap_dim_full (gangfit_minfrag.inc, 64-bit division past 2^40),
    the wide chain kernels (fit_fifo_chain_kernel, fit_fifo_generic_kernel) on tables without a narrow form, prepare_app's
    hand-off at a scaled 2^30, node_efficiency's int64 -> float64 roundings and its small_cpu shortcut
    (gangfit_fifo_zoned.inc), and minimal fragmentation's (K + MaxInt) / 2 wrap."""
    feasible = 0
    for name, p, _, refs in _cases(regime):
        apps = gangfit.make_apps(*p[5:9])
        for cname, ctx in ctxs.items():
            _install(ctx, p)
            for algo in ALGOS:
                where = f"{regime} {name} ctx={cname} algo={algo}"
                ind, fifo = refs[algo]
                gpu = ctx.fit_batch(IND, algo, apps)
                assert stress_lib.same(gpu, ind, False) is None, where
                assert np.array_equal(ctx.fit_feasible(algo, apps), ind.results["has_capacity"].astype(bool)), where
                if algo != 2:
                    assert np.array_equal(_bits(ctx.avg_packing_efficiency(algo, apps, gpu)), _bits(ind.avg_eff)), where
                gpu = ctx.fit_batch(FIFO, algo, apps)
                assert stress_lib.same(gpu, fifo, True) is None, where
                assert np.array_equal(ctx.residual(), fifo.avail_after), where
                feasible += int(ind.results["has_capacity"].sum())
    assert feasible > 0


@pytest.mark.parametrize("regime", mg.REGIMES)
def test_per_node_efficiencies(ctxs, regime):
    """gf_packing_efficiencies (PackingResult.PackingEfficiencies) of a few placements per case: node_efficiency's
    Value() rounding of milli-cpus and its conversions of quantities past 2^53."""
    ctx = ctxs["default"]
    checked = 0
    for name, p, _, refs in _cases(regime)[:3]:
        avail, sched, zone, D, X, drv, exe, k, flags = p
        _install(ctx, p)
        ind = refs[0][0]
        for a in np.nonzero(ind.results["has_capacity"])[0][:3]:
            _, d, ex = ind.placement(int(a))
            want, _ = ob.packing_efficiency(avail, sched, drv[a], exe[a], d, ex)
            got = ctx.packing_efficiencies(0, drv[a], exe[a], d, ex)
            assert np.array_equal(_bits(got), _bits(want)), f"{regime} {name} app {a}"
            checked += 1
    assert checked > 0


@pytest.mark.parametrize("regime", mg.REGIMES)
def test_single_executors_and_find_nodes(ctxs, regime):
    """gf_executor_fit, first fit and minimal fragmentation (with `reserved` and hosts_app: capacities are cap_dim_full's
    unclamped quotients, up to 2^62 — the 64-bit division branch), and gf_find_nodes chained with its reserved_adds."""
    ctx = ctxs["default"]
    rng = np.random.default_rng(11 + mg.REGIMES.index(regime))
    for name, p, _, _ in _cases(regime)[:3]:
        avail, sched, zone, D, X, drv, exe, k, flags = p
        n = len(avail)
        _install(ctx, p)
        req = np.concatenate([exe, drv])[:24]
        reserved = np.where(rng.random((n, 3)) < 0.5, 0, rng.integers(0, 1 << 62, size=(n, 3)) >> rng.integers(0, 62, size=(n, 3)))
        hosts = rng.random((len(req), n)) < 0.05
        for mf in (False, True):
            for r in (None, reserved):
                got = ctx.executor_fit(req, reserved=r, minimal_fragmentation=mf, hosts=hosts if mf else None)
                want = [ob.executor_fit(avail, e, X, reserved=r, minimal_fragmentation=mf, hosts=hosts[i] if mf else None)
                        for i, e in enumerate(req)]
                assert got.tolist() == want, f"{regime} {name} minimal_fragmentation={mf} reserved={r is not None}"
        fk = np.clip(k, 1, 64).astype(np.int32)
        placed, last, off, nodes, adds = ctx.find_nodes(exe, fk, chained=True)
        ref = ob.find_nodes(avail, exe, fk, X[X < n], chained=True)
        assert np.array_equal(placed, ref.placed) and np.array_equal(adds, ref.adds), f"{regime} {name}"
        assert np.array_equal(ctx.residual(), ref.avail_after), f"{regime} {name}"


@pytest.mark.parametrize("regime", mg.REGIMES)
def test_two_shards_of_one_device(regime):
    """A context over device 0 twice: the node-range sharded steps of all six packers (gangfit_shard.inc) — the partial
    capacity sums and int32 deltas of the tightly-pack family, the count rows, the scaled-domain capacities and the
    designated-shard walk of the minimal-fragmentation family — at these magnitudes.  The context must still be sharding
    afterwards: a self-check that "disagreed" is answered right by the first device and would otherwise hide there."""
    with gangfit.Context(devices=[0, 0]) as g:
        assert g.shard_count() == 2
        for name, p, _, refs in _cases(regime):
            _install(g, p)
            apps = gangfit.make_apps(*p[5:9])
            for algo in ALGOS:
                assert stress_lib.same(g.fit_batch(IND, algo, apps), refs[algo][0], False) is None, f"{regime} {name} algo={algo}"
        assert g.shard_count() == 2, g.last_error()


def test_snapshot_build_near_2_62(gf_ctx):
    """gf_snapshot_build with allocatable just below 2^62 and reservations of up to 2^59 (per-node sums plus overhead below
    2^62, what its range check admits) against oracle/pysnapshot.build, then one chain of every packer family on the
    built snapshot."""
    rng = np.random.default_rng(62)
    n = 400
    top = np.int64(mg.QMAX)
    alloc = np.stack([top - rng.integers(0, 1 << 40, size=n), top - rng.integers(0, 1 << 61, size=n),
                      rng.integers(0, 9, size=n)], axis=1).astype(np.int64)
    alloc[::7, 1] = rng.integers(0, 1 << 30, size=len(alloc[::7]))  # small nodes the reservations overcommit
    overhead = np.stack([rng.integers(0, 1 << 60, size=n), rng.integers(0, 1 << 60, size=n), np.zeros(n, dtype=np.int64)],
                        axis=1).astype(np.int64)
    overhead[::7, 1] = rng.integers(0, alloc[::7, 1] + 1)  # schedulable stays >= 0: a negative one disables the efficiencies
    res_node = np.repeat(np.arange(n + 2), 2).astype(np.uint32)  # two entries per node, two to unknown nodes
    res_req = np.stack([rng.integers(0, 1 << 59, size=len(res_node)), rng.integers(0, 1 << 59, size=len(res_node)),
                        rng.integers(0, 2, size=len(res_node))], axis=1).astype(np.int64)
    flags = np.full(n, ps.READY | ps.DRIVER_CANDIDATE, dtype=np.uint32)
    flags[::11] = ps.READY
    ranks = rng.permutation(n).astype(np.uint32)
    D, X = gf_ctx.build_snapshot(alloc, flags, ranks, overhead=overhead, res_node=res_node, res_req=res_req)
    avail, sched, rD, rX = ps.build(alloc, flags, ranks, overhead=overhead, res_node=res_node, res_req=res_req)
    got_avail, got_sched = gf_ctx.snapshot()
    assert np.array_equal(got_avail, avail) and np.array_equal(got_sched, sched)
    assert np.array_equal(D, rD) and np.array_equal(X, rX)
    assert avail.max() > 1 << 61 and avail.min() < -(1 << 58)
    a = 20
    drv = np.stack([rng.integers(0, 1 << 61, size=a), rng.integers(0, 1 << 61, size=a), np.zeros(a, dtype=np.int64)], axis=1)
    exe = np.stack([rng.integers(1, 1 << 60, size=a), rng.integers(0, 1 << 60, size=a), rng.integers(0, 2, size=a)], axis=1)
    k = rng.integers(0, 50, size=a).astype(np.int32)
    flags_a = np.ones(a, dtype=np.uint32)
    apps = gangfit.make_apps(drv, exe, k, flags_a)
    for algo in (0, 1, 2, 4):
        gpu = gf_ctx.fit_batch(FIFO, algo, apps)
        ref = ob.fit_fifo_chain(algo, avail, ob.make_apps(drv, exe, k, flags_a), rD, rX, sched=sched,
                                zone=np.zeros(n, dtype=np.uint32))
        assert stress_lib.same(gpu, ref, True) is None, f"algo={algo}"
        assert np.array_equal(gf_ctx.residual(), ref.avail_after)
        assert ref.results["has_capacity"].any()


def test_narrow_edge_routes(ctxs):
    """Which kernel serves each narrow-edge FIFO chain, every packer.  The witness is gf_chain_cache_stats out[0]: chain_commit
    (gangfit_api_fit.cpp) counts a chain only when chain_plan proved every request narrow (narrow_units) on an LDS chain
    route; a chain that runs on the wide kernels — or is handed to them by prepare_app — is never counted.  A table or request
    scaling to 2^30-1 must take the LDS chain, its twin at 2^30 the wide kernel; a unit refinement landing on room = (2^30-1) /
    nmax stays narrow, one past it does not."""
    ctx = ctxs["default"]
    seen = set()
    for name, p, route, refs in _cases("narrow-edge"):
        if route is None:
            continue
        _install(ctx, p)
        apps = gangfit.make_apps(*p[5:9])
        for algo in ALGOS:
            ctx.chain_cache_stats(reset=True)
            gpu = ctx.fit_batch(FIFO, algo, apps)
            assert stress_lib.same(gpu, refs[algo][1], True) is None, f"{name} algo={algo}"
            assert np.array_equal(ctx.residual(), refs[algo][1].avail_after)
            committed = ctx.chain_cache_stats()[0]
            assert committed == (1 if route == "lds" else 0), f"{name} algo={algo}: {committed} LDS chains for route {route}"
            seen.add(route)
    assert seen == {"lds", "wide"}


def test_argument_edges(gf_ctx):
    """2^62-1 is a quantity, 2^62 is not; GF_MAX_K is a gang size, GF_MAX_K+1 is not — in every entry point that takes them
    (gf_snapshot_set, check_app / check_apps of the fits and efficiencies, gf_executor_fit's request and reserved checks,
    gf_find_nodes)."""
    Q, BAD = mg.QMAX, 1 << 62

    def refused(fn, *args, **kw):
        with pytest.raises(gangfit.GangfitError) as e:
            fn(*args, **kw)
        assert e.value.code == INVALID, e.value

    avail = np.array([[Q, Q, Q], [-Q, -Q, -Q], [Q, 0, 1], [0, Q, 0]], dtype=np.int64)
    sched = np.maximum(avail, 0)
    gf_ctx.set_snapshot(avail, sched)
    gf_ctx.set_zones(np.zeros(4, dtype=np.uint32))
    gf_ctx.set_orders([0, 1, 2, 3], [3, 2, 1, 0])
    for row in ([BAD, 0, 0], [0, -BAD, 0]):
        refused(gf_ctx.set_snapshot, np.array([row, [1, 1, 1]], dtype=np.int64))
    refused(gf_ctx.set_snapshot, avail, np.array([[BAD, 0, 0]] + [[1, 1, 1]] * 3, dtype=np.int64))
    gf_ctx.set_snapshot(avail, sched)
    gf_ctx.set_zones(np.zeros(4, dtype=np.uint32))
    gf_ctx.set_orders([0, 1, 2, 3], [3, 2, 1, 0])
    good = gangfit.make_apps([[Q, 0, 0], [0, 0, 0]], [[0, Q, 0], [1, 1, 0]], [1, mg.GF_MAX_K])
    ref = ob.fit_independent(0, avail, ob.make_apps([[Q, 0, 0], [0, 0, 0]], [[0, Q, 0], [1, 1, 0]], [1, mg.GF_MAX_K]),
                             [0, 1, 2, 3], [3, 2, 1, 0], sched=sched)
    for algo in ALGOS:
        out = gf_ctx.fit_batch(IND, algo, good)
        if algo == 0:
            assert stress_lib.same(out, ref, False) is None
        gf_ctx.fit_batch(FIFO, algo, good)
        gf_ctx.fit_feasible(algo, good)
    gf_ctx.avg_packing_efficiency(0, good, gf_ctx.fit_batch(IND, 0, good))
    gf_ctx.executor_fit([[Q, 0, 0], [0, Q, Q]], reserved=np.full((4, 3), Q), minimal_fragmentation=True)
    gf_ctx.find_nodes([[Q, 0, 0]], [mg.GF_MAX_K])
    bads = [([[BAD, 0, 0]], [[0, 0, 0]], [1]), ([[0, 0, 0]], [[0, 0, BAD]], [1]), ([[0, 0, 0]], [[1, 0, 0]], [mg.GF_MAX_K + 1])]
    for drv, exe, k in bads:
        apps = gangfit.make_apps(drv, exe, k)
        for algo in ALGOS:
            refused(gf_ctx.fit_batch, IND, algo, apps)
            refused(gf_ctx.fit_batch, FIFO, algo, apps)
            refused(gf_ctx.fit_feasible, algo, apps)
        refused(gf_ctx.spark_binpack, 0, drv[0], exe[0], k[0])
        refused(gf_ctx.worker_fit, 0, apps)
        res = gangfit.BatchOut(np.zeros(1, dtype=gangfit._native.RESULT_DTYPE), np.zeros(1, dtype=np.uint64),
                               np.zeros(0, dtype=np.uint32))
        refused(gf_ctx.avg_packing_efficiency, 0, apps, res)
        refused(gf_ctx.packing_efficiencies, 0, drv[0], exe[0], 0, np.zeros(k[0], dtype=np.uint32))
    for mf in (False, True):
        refused(gf_ctx.executor_fit, [[BAD, 0, 0]], minimal_fragmentation=mf)
        refused(gf_ctx.executor_fit, [[1, 0, 0]], reserved=np.full((4, 3), BAD), minimal_fragmentation=mf)
    refused(gf_ctx.find_nodes, [[0, BAD, 0]], [1])
    refused(gf_ctx.find_nodes, [[1, 0, 0]], [mg.GF_MAX_K + 1])
