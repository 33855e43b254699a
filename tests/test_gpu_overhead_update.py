"""gf_overhead_update: the overhead rows of the resident cluster (internal/extender/overhead.go:91-153 — per node, the summed
requests of every pod without a reservation) are replaced by rows while the resident usage sums stay.  After every update the
snapshot built from the resident state must equal the numpy restatement (oracle/pysnapshot.py) on the live overhead columns and,
bit for bit, what a fresh context builds from those columns; decisions on top of it equal the oracle's."""
import numpy as np
import pytest

import gangfit
from gangfit import _native as N
from gangfit import workloads as wl
from oracle import binding as ob
from oracle import pysnapshot as ps
from test_gpu_group import split  # noqa: F401  (fixture: both GANGFIT_TEST_GROUP_SPLIT modes)
from test_gpu_parity import _assert_same
from test_snapshot_build import GIB, _cluster

pytestmark = pytest.mark.gpu
IND, FIFO = gangfit.GF_MODE_INDEPENDENT, gangfit.GF_MODE_FIFO_CHAIN
TIGHT, SINGLE_AZ_TIGHT = gangfit.GF_ALGO_TIGHTLY_PACK, gangfit.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK


def _set_cluster(ctx, c, overhead):
    ctx.set_cluster(c["alloc"], c["node_flags"], c["name_rank"], overhead=overhead, zone=c["zone"], n_zones=c["n_zones"])


def _rows(rng, m):
    """m overhead rows in the value range of test_snapshot_build._cluster"""
    return np.stack([rng.integers(0, 8, size=m) * 250, rng.integers(0, 16, size=m) * (GIB // 4), np.zeros(m, dtype=np.int64)],
                    axis=1).astype(np.int64)


def _apps():
    w = wl.config(2, n_nodes=16, n_apps=48)
    flags = np.ones(len(w.k), dtype=np.uint32)
    return gangfit.make_apps(w.drv, w.exe, w.k, flags), ob.make_apps(w.drv, w.exe, w.k, flags)


def _raw_update(ctx, nodes, cols):
    """the C entry point with the pointers as given (None = NULL): its return code"""
    nodes = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.uint32)
    cols = [None if c is None else np.ascontiguousarray(c, dtype=np.int64) for c in cols]
    n = len(nodes) if nodes is not None else len(next(c for c in cols if c is not None))
    return ctx._lib.gf_overhead_update(ctx._h, n, N.ptr(nodes), *[N.ptr(c) for c in cols])


@pytest.mark.parametrize("installed_with_columns", [True, False])
def test_updates_match_the_restatement_and_a_fresh_build(installed_with_columns):
    n = 2500
    c = _cluster(91, n, 300, 3, with_overhead=True, labels=False)
    rng = np.random.default_rng(23)
    live = c["overhead"].copy() if installed_with_columns else np.zeros((n, 3), dtype=np.int64)
    apps, oapps = _apps()
    with gangfit.Context(0) as ctx, gangfit.Context(0) as fresh:
        _set_cluster(ctx, c, live.copy() if installed_with_columns else None)
        ctx.usage_apply(c["res_node"], c["res_req"], +1)  # ~300 reservations, K + 1 entries each
        again = None

        def one_row():
            nonlocal again
            again = int(rng.integers(0, n))
            return np.array([again]), _rows(rng, 1) + np.array([[250, GIB // 4, 0]])  # (never the row it replaces by accident)

        def a_few_hundred():
            return rng.permutation(n)[:317], _rows(rng, 317)

        def every_row():
            return rng.permutation(n), _rows(rng, n)

        def back_to_zero():
            nodes = rng.permutation(n)[:900]
            return nodes, np.zeros((900, 3), dtype=np.int64)

        def named_again():  # the row of round one, in a later call, with other values
            return np.array([again, (again + 1) % n]), _rows(rng, 2) + np.array([[500, GIB, 0]])

        for make in (one_row, a_few_hundred, every_row, back_to_zero, named_again):
            nodes, rows = make()
            ctx.overhead_update(nodes, rows)
            live[nodes] = rows
            D, X = ctx.build_snapshot_resident(resident_usage=True)
            cc = dict(c, overhead=live)
            avail, sched, rD, rX = ps.build(**cc)
            got_avail, got_sched = ctx.snapshot()
            assert np.array_equal(got_avail, avail) and np.array_equal(got_sched, sched), make.__name__
            assert np.array_equal(D, rD) and np.array_equal(X, rX), make.__name__
            fD, fX = fresh.build_snapshot(**cc)
            f_avail, f_sched = fresh.snapshot()
            assert got_avail.tobytes() == f_avail.tobytes() and got_sched.tobytes() == f_sched.tobytes(), make.__name__
            assert D.tobytes() == fD.tobytes() and X.tobytes() == fX.tobytes(), make.__name__
            for algo in (TIGHT, SINGLE_AZ_TIGHT):
                gpu = ctx.fit_batch(FIFO, algo, apps)
                ref = ob.fit_fifo_chain(algo, avail, oapps, rD, rX, sched=sched, zone=c["zone"])
                assert gpu.failed_at == ref.failed_at and np.array_equal(gpu.results, ref.results), (make.__name__, algo)
                assert np.array_equal(ctx.residual(), ref.avail_after), (make.__name__, algo)


def test_resident_usage_survives_an_update(gf_ctx):
    n = 2500
    c = _cluster(92, n, 300, 3, with_overhead=True, labels=False)
    rng = np.random.default_rng(29)
    _set_cluster(gf_ctx, c, c["overhead"])
    gf_ctx.usage_apply(c["res_node"], c["res_req"], +1)
    gf_ctx.build_snapshot_resident(resident_usage=True, want_orders=False)
    g0 = gf_ctx.generation()
    nodes = rng.permutation(n)[:400]
    rows = _rows(rng, 400)
    gf_ctx.overhead_update(nodes, rows)
    g1 = gf_ctx.generation()
    assert g1[2] == g0[2], "the usage generation moved"
    assert g1[1] > g0[1], "the cluster generation did not move"
    assert g1[0] == g0[0], "the snapshot epoch moved before any build"
    live = c["overhead"].copy()
    live[nodes] = rows
    D, X = gf_ctx.build_snapshot_resident(resident_usage=True)
    assert gf_ctx.generation()[0] > g1[0]
    avail, sched, rD, rX = ps.build(**dict(c, overhead=live))
    got_avail, got_sched = gf_ctx.snapshot()
    assert np.array_equal(got_avail, avail) and np.array_equal(got_sched, sched)
    assert np.array_equal(D, rD) and np.array_equal(X, rX)
    # the usage part is still in there: without the reservations the restatement differs
    no_usage, _, _, _ = ps.build(**dict(c, overhead=live, res_node=None, res_req=None))
    assert not np.array_equal(got_avail, no_usage)
    # an empty update is GF_OK and changes nothing, not even the generation
    gen = gf_ctx.generation()
    gf_ctx.overhead_update(np.zeros(0, dtype=np.uint32), np.zeros((0, 3), dtype=np.int64))
    assert gf_ctx.generation() == gen


def test_refusals_leave_the_state_alone(gf_ctx):
    n = 1200
    c = _cluster(93, n, 150, 2, with_overhead=True, labels=False)
    _set_cluster(gf_ctx, c, c["overhead"])
    gf_ctx.usage_apply(c["res_node"], c["res_req"], +1)
    D0, X0 = gf_ctx.build_snapshot_resident(resident_usage=True)
    before = [a.copy() for a in gf_ctx.snapshot()]
    gen = gf_ctx.generation()
    one = np.array([1000], dtype=np.int64)
    ok3 = [np.array([1000, 2000, 3000], dtype=np.int64)] * 3
    refused = {
        "a node out of range": ([3, n, 5], ok3),
        "the first node out of range": ([n + 7], [one, one, one]),
        "a duplicate node": ([3, 9, 3], ok3),
        "a negative value": ([4], [one, -one, one]),
        "a value of 2^61": ([4], [one, one, np.array([1 << 61], dtype=np.int64)]),
        "a NULL column": ([4], [one, None, one]),
        "a NULL node column": (None, [one, one, one]),
    }
    for what, (nodes, cols) in refused.items():
        assert _raw_update(gf_ctx, nodes, cols) == N.GF_ERR_INVALID, what
        assert gf_ctx.generation() == gen, what
    D1, X1 = gf_ctx.build_snapshot_resident(resident_usage=True)
    after = gf_ctx.snapshot()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    assert np.array_equal(D1, D0) and np.array_equal(X1, X0)
    # on a view: GF_ERR_STATE, like every installer
    v = gf_ctx.view()
    try:
        with pytest.raises(gangfit.GangfitError) as e:
            v.overhead_update([4], [[1000, 1000, 0]])
        assert e.value.code == N.GF_ERR_STATE
    finally:
        v.close()
    # before gf_cluster_set: GF_ERR_STATE
    with gangfit.Context(0) as fresh:
        with pytest.raises(gangfit.GangfitError) as e:
            fresh.overhead_update([0], [[1, 1, 1]])
        assert e.value.code == N.GF_ERR_STATE
    D2, X2 = gf_ctx.build_snapshot_resident(resident_usage=True)
    assert np.array_equal(gf_ctx.snapshot()[0], before[0]) and np.array_equal(D2, D0)


def test_sums_that_could_wrap_are_refused_through_an_update(gf_ctx):
    """test_snapshot_build.test_sums_that_could_wrap_are_refused with the large value arriving as an overhead row: usage +
    overhead of one node may never reach 2^62.  Either the update is refused or the gf_usage_apply / build that would cross the
    bound is; a wrapped snapshot is never built."""
    n = 8
    alloc = np.tile(np.array([[64000, 256 * GIB, 0]], dtype=np.int64), (n, 1))
    flags = np.full(n, ps.READY | ps.DRIVER_CANDIDATE, dtype=np.uint32)
    ranks = np.arange(n, dtype=np.uint32)
    big = np.int64(1) << 60
    zero3 = np.zeros(3, dtype=np.uint32)
    three_big = np.tile(np.array([[1000, big, 0]], dtype=np.int64), (3, 1))

    def built():
        gf_ctx.build_snapshot_resident(resident_usage=True, want_orders=False)
        return gf_ctx.snapshot()[0]

    for installed_with_columns in (True, False):
        over0 = np.tile(np.array([[250, GIB, 0]], dtype=np.int64), (n, 1)) if installed_with_columns else None
        live = over0.copy() if installed_with_columns else np.zeros((n, 3), dtype=np.int64)
        # (a) the usage is there first (3 x 2^60 on node 0), then an overhead row of 2^60 on the same node: 2^62
        gf_ctx.set_cluster(alloc, flags, ranks, overhead=over0)
        gf_ctx.usage_apply(zero3, three_big, +1)
        try:
            gf_ctx.overhead_update([0], [[0, big, 0]])
            took = True
        except gangfit.GangfitError as e:
            assert e.code == N.GF_ERR_INVALID
            took = False
        if took:  # then nothing more may be added, and the build must not wrap
            live[0] = [0, big, 0]
            with pytest.raises(gangfit.GangfitError):
                gf_ctx.usage_apply(np.zeros(1, dtype=np.uint32), np.array([[0, 1, 0]], dtype=np.int64), +1)
        want, _, _, _ = ps.build(alloc, flags, ranks, overhead=live, res_node=zero3, res_req=three_big)
        try:
            got = built()
        except gangfit.GangfitError as e:
            assert took and e.code == N.GF_ERR_INVALID
        else:
            assert np.array_equal(got, want) and (got > -(1 << 62)).all()
        # (b) the overhead row first (2^60 on node 3), then usage that would reach 2^62 with it: the usage is refused
        live = over0.copy() if installed_with_columns else np.zeros((n, 3), dtype=np.int64)
        gf_ctx.set_cluster(alloc, flags, ranks, overhead=over0)
        gf_ctx.overhead_update([3], [[0, big, 0]])
        live[3] = [0, big, 0]
        with pytest.raises(gangfit.GangfitError) as e:
            gf_ctx.usage_apply(np.full(3, 3, dtype=np.uint32), three_big, +1)
        assert e.value.code == N.GF_ERR_INVALID
        two = three_big[:2]
        gf_ctx.usage_apply(np.full(2, 3, dtype=np.uint32), two, +1)  # 2 x 2^60 + 2^60 < 2^62: fine
        want, _, _, _ = ps.build(alloc, flags, ranks, overhead=live, res_node=np.full(2, 3, dtype=np.uint32), res_req=two)
        assert np.array_equal(built(), want)
        # ... and with the entries travelling (gf_snapshot_build_resident's own check reads the same bound)
        with pytest.raises(gangfit.GangfitError) as e:
            gf_ctx.build_snapshot_resident(res_node=np.full(3, 3, dtype=np.uint32), res_req=three_big, want_orders=False)
        assert e.value.code == N.GF_ERR_INVALID
        # the bound may be loose but never too small: the row replaced by a small one, the bound still refuses or allows —
        # what is built is right either way
        gf_ctx.overhead_update([3], [[0, GIB, 0]])
        live[3] = [0, GIB, 0]
        want, _, _, _ = ps.build(alloc, flags, ranks, overhead=live, res_node=np.full(2, 3, dtype=np.uint32), res_req=two)
        assert np.array_equal(built(), want)


def test_multi_device_context(split):  # noqa: F811
    n = 2500
    c = _cluster(94, n, 300, 3, with_overhead=True, labels=False)
    rng = np.random.default_rng(31)
    w = wl.config(2, n_nodes=16, n_apps=64)
    apps, oapps = gangfit.make_apps(w.drv, w.exe, w.k), ob.make_apps(w.drv, w.exe, w.k)
    with gangfit.Context(devices=[0] * 3) as g:
        assert g.shard_count() == 3
        for installed_with_columns in (True, False):
            live = c["overhead"].copy() if installed_with_columns else np.zeros((n, 3), dtype=np.int64)
            _set_cluster(g, c, live.copy() if installed_with_columns else None)
            g.usage_apply(c["res_node"], c["res_req"], +1)
            for m in (1, 600):
                nodes, rows = rng.permutation(n)[:m], _rows(rng, m) + np.array([[250, 0, 0]])
                g0 = g.generation()
                g.overhead_update(nodes, rows)
                assert g.generation()[1] > g0[1] and g.generation()[2] == g0[2]
                live[nodes] = rows
                D, X = g.build_snapshot_resident(resident_usage=True)
                avail, sched, rD, rX = ps.build(**dict(c, overhead=live))
                got_avail, got_sched = g.snapshot()
                assert np.array_equal(got_avail, avail) and np.array_equal(got_sched, sched)
                assert np.array_equal(D, rD) and np.array_equal(X, rX)
                ref = ob.fit_independent(TIGHT, avail, oapps, rD, rX)
                assert 0 < ref.results["has_capacity"].sum()
                _assert_same(g.fit_batch(IND, TIGHT, apps), ref, apps)   # sharded; the first batch of a snapshot checks itself
                _assert_same(g.fit_batch(IND, TIGHT, apps), ref, apps)
                assert g.shard_count() == 3, "the context stopped sharding: a sharded batch disagreed with one device"
        with pytest.raises(gangfit.GangfitError) as e:  # a refusal reaches no device
            g.overhead_update([1, 1], [[1, 1, 0], [2, 2, 0]])
        assert e.value.code == N.GF_ERR_INVALID
        g.build_snapshot_resident(resident_usage=True, want_orders=False)
        assert np.array_equal(g.snapshot()[0], avail)


def test_the_chain_cache_survives_an_update_until_the_build():
    with gangfit.Context(0) as ctx:
        _chain_cache_case(ctx)


def _chain_cache_case(gf_ctx):
    n = 2500
    c = _cluster(95, n, 300, 3, with_overhead=True, labels=False)
    rng = np.random.default_rng(37)
    _set_cluster(gf_ctx, c, c["overhead"])
    gf_ctx.usage_apply(c["res_node"], c["res_req"], +1)
    D, X = gf_ctx.build_snapshot_resident(resident_usage=True)
    avail, sched = gf_ctx.snapshot()
    apps, oapps = _apps()
    ref_old = ob.fit_fifo_chain(TIGHT, avail, oapps, D, X)
    out = gf_ctx.fit_batch(FIFO, TIGHT, apps[:-1])  # the previous Filter's chain: one application shorter
    assert np.array_equal(out.results, ref_old.results[:-1])
    nodes = rng.permutation(n)[:500]
    rows = _rows(rng, 500) + np.array([[4000, 8 * GIB, 0]])  # enough to move decisions once it is built
    gf_ctx.overhead_update(nodes, rows)
    # no build yet: the installed snapshot did not change, the next chain resumes and answers for the OLD overhead
    gf_ctx.chain_cache_stats(reset=True)
    out = gf_ctx.fit_batch(FIFO, TIGHT, apps)
    chains, resumed, evaluated, skipped = gf_ctx.chain_cache_stats()
    assert (chains, resumed) == (1, 1) and skipped > 0, (chains, resumed, evaluated, skipped)
    assert out.failed_at == ref_old.failed_at and np.array_equal(out.results, ref_old.results)
    # after the build: a full replay on the new snapshot, equal to the oracle on the restatement
    live = c["overhead"].copy()
    live[nodes] = rows
    D2, X2 = gf_ctx.build_snapshot_resident(resident_usage=True)
    avail2, sched2, rD, rX = ps.build(**dict(c, overhead=live))
    assert np.array_equal(gf_ctx.snapshot()[0], avail2) and np.array_equal(D2, rD) and np.array_equal(X2, rX)
    gf_ctx.chain_cache_stats(reset=True)
    out = gf_ctx.fit_batch(FIFO, TIGHT, apps)
    chains, resumed, evaluated, skipped = gf_ctx.chain_cache_stats()
    assert (chains, resumed, skipped) == (1, 0, 0)
    ref_new = ob.fit_fifo_chain(TIGHT, avail2, oapps, rD, rX)
    assert out.failed_at == ref_new.failed_at and np.array_equal(out.results, ref_new.results)
    assert np.array_equal(gf_ctx.residual(), ref_new.avail_after)
