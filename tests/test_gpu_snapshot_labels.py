"""gf_snapshot_build* with label ranks (driver- / executor-prioritized-node-label, internal/sort/nodesorting.go:161-199): the
re-sort runs as one more key group of the priority sort, and the slot tables are built on the device whenever both lists are
still subsequences of that one order (gangfit_label_plan.h, LabelMerge); otherwise the host route installs them.  Either way the
snapshot, the two lists and every decision equal the restatement in oracle/pysnapshot.py and the oracle's decisions on it;
gf_snapshot_build_info says which route a build took."""
import numpy as np
import pytest

import gangfit
from gangfit import workloads as wl
from oracle import binding as ob
from oracle import pysnapshot as ps

GIB = 1 << 30
U = ps.UNRANKED
INDEPENDENT, FIFO = gangfit.GF_MODE_INDEPENDENT, gangfit.GF_MODE_FIFO_CHAIN
PACKERS = (0, 1, 2, 4, 5)
SIZES = [1, 5, 64, 65, 130, 1000, 4097]  # 64 | 65: the chunk edge; 130: a ragged last chunk; 4097: sort segments grow past 64
SCALARS_ONLY = 512  # bytes: "a few hundred at most" — nothing of size O(n_nodes) came back


def _cluster(seed, n, n_rr, n_zones, with_overhead=True):
    """The generator of tests/test_snapshot_build.py (same shapes), without label ranks."""
    rng = np.random.default_rng(seed)
    shape = rng.integers(0, 4, size=n)
    alloc = np.stack([np.array([16, 32, 64, 96])[shape] * 1000, np.array([64, 128, 256, 384])[shape] * GIB,
                      np.where(rng.random(n) < 0.1, 8, 0)], axis=1).astype(np.int64)
    overhead = None
    if with_overhead:
        overhead = np.stack([rng.integers(0, 8, size=n) * 250, rng.integers(0, 16, size=n) * (GIB // 4),
                             np.zeros(n, dtype=np.int64)], axis=1).astype(np.int64)
    ks = rng.integers(1, 25, size=n_rr)
    res_node = rng.integers(0, n + 3, size=int(ks.sum())).astype(np.uint32)
    res_req = np.stack([rng.choice([1000, 2000, 4000], size=len(res_node)), rng.choice([4, 8, 16], size=len(res_node)) * GIB,
                        (rng.random(len(res_node)) < 0.02).astype(np.int64)], axis=1).astype(np.int64).reshape(-1, 3)
    flags = (np.where(rng.random(n) < 0.05, ps.UNSCHEDULABLE, 0) | np.where(rng.random(n) < 0.95, ps.READY, 0) |
             np.where(rng.random(n) < 0.8, ps.DRIVER_CANDIDATE, 0)).astype(np.uint32)
    name_rank = rng.permutation(n).astype(np.uint32)
    zone = rng.integers(0, n_zones, size=n).astype(np.uint32)
    return dict(alloc=alloc, node_flags=flags, name_rank=name_rank, overhead=overhead, res_node=res_node, res_req=res_req,
                zone=zone, n_zones=n_zones, driver_label_rank=None, exec_label_rank=None)


def _family(c, family, rng):
    """The four label configurations whose two lists stay subsequences of one order."""
    n = len(c["alloc"])
    f = c["node_flags"]
    if family == "a":    # both lists use the same label
        el = rng.choice([0, 1, 2, U], size=n).astype(np.uint32)
        return dict(c, driver_label_rank=el.copy(), exec_label_rank=el)
    if family == "b":    # executors re-sorted; the driver candidates all carry one value of that label
        el = rng.choice([0, 1, 2, U], size=n).astype(np.uint32)
        flags = (f & ~np.uint32(ps.DRIVER_CANDIDATE)) | np.where(el == 1, ps.DRIVER_CANDIDATE, 0).astype(np.uint32)
        return dict(c, node_flags=flags, exec_label_rank=el)
    if family == "c":    # drivers re-sorted; the ready nodes all carry one value of that label
        dl = rng.choice([0, 1, U], size=n).astype(np.uint32)
        flags = (f & ~np.uint32(ps.READY)) | np.where(dl == 0, ps.READY, 0).astype(np.uint32)
        return dict(c, node_flags=flags, driver_label_rank=dl)
    dl = rng.choice([0, 1, U], size=n).astype(np.uint32)  # "d": two labels, one a monotone function of the other
    el = np.where(dl == U, U, dl.astype(np.uint64) * 2 + 3).astype(np.uint32)
    return dict(c, driver_label_rank=dl, exec_label_rank=el)


def _same_relative_order(D, X):
    """The two lists agree on the order of the nodes they share (<=> both are subsequences of one order)."""
    return np.array_equal(D[np.isin(D, X)], X[np.isin(X, D)])


def _no_group_expected(c):
    """No array re-sorts anything: each is absent or holds one value on every node."""
    return all(r is None or len(np.unique(r)) <= 1 for r in (c["driver_label_rank"], c["exec_label_rank"]))


def _check_snapshot(ctx, c, D, X):
    avail, sched, rD, rX = ps.build(**c)
    got_avail, got_sched = ctx.snapshot()
    assert np.array_equal(got_avail, avail)
    assert np.array_equal(got_sched, sched)
    assert np.array_equal(D, rD) and np.array_equal(X, rX)
    return avail, sched, rD, rX


def _check_decisions(ctx, c, avail, sched, rD, rX):
    n = len(avail)
    w = wl.config(2, n_nodes=16, n_apps=min(64, 4 * n))
    apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    oapps = ob.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    for algo in PACKERS:
        gpu = ctx.fit_batch(INDEPENDENT, algo, apps)
        ref = ob.fit_independent(algo, avail, oapps, rD, rX, sched=sched, zone=c["zone"])
        assert np.array_equal(gpu.results, ref.results), algo
        gpu = ctx.fit_batch(FIFO, algo, apps)
        ref = ob.fit_fifo_chain(algo, avail, oapps, rD, rX, sched=sched, zone=c["zone"])
        assert gpu.failed_at == ref.failed_at and np.array_equal(gpu.results, ref.results), algo
        assert np.array_equal(ctx.residual(), ref.avail_after), algo


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["a", "b", "c", "d"])
@pytest.mark.parametrize("n_zones", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_mergeable_label_families_stay_on_the_device(gf_ctx, n, n_zones, family):
    c = _cluster(1000 + n + n_zones, n, min(n, 300), n_zones, with_overhead=(n % 2 == 0))
    c = _family(c, family, np.random.default_rng(7 * n + n_zones + ord(family)))
    _, _, oD, oX = ps.build(**c)
    assert _same_relative_order(oD, oX)  # precondition: the case cannot pass through the host fallback unnoticed
    D, X = gf_ctx.build_snapshot(**c)
    info = gf_ctx.build_info()
    print("build_info", n, n_zones, family, info)
    assert info[:3] == (1, 0 if _no_group_expected(c) else 1, 0) and info[3] <= SCALARS_ONLY
    avail, sched, rD, rX = _check_snapshot(gf_ctx, c, D, X)
    _check_decisions(gf_ctx, c, avail, sched, rD, rX)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 130, 1000])
def test_conflicting_lists_fall_back_to_the_host(gf_ctx, n):
    c = _cluster(2000 + n, n, min(n, 300), 3)
    rng = np.random.default_rng(n)
    for _ in range(64):  # independent draws; at n = 5 a draw can merge by chance: take the first that does not
        c["driver_label_rank"] = rng.choice([0, 1, U], size=n).astype(np.uint32)
        c["exec_label_rank"] = rng.choice([0, 1, 2, U], size=n).astype(np.uint32)
        _, _, oD, oX = ps.build(**c)
        if not _same_relative_order(oD, oX):
            break
    assert not _same_relative_order(oD, oX)
    D, X = gf_ctx.build_snapshot(**c)
    info = gf_ctx.build_info()
    print("build_info", n, info)
    assert info[0] == 2 and info[1] == 1 and info[2] == 1
    avail, sched, rD, rX = _check_snapshot(gf_ctx, c, D, X)
    _check_decisions(gf_ctx, c, avail, sched, rD, rX)


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", ["all-unranked", "all-equal", "wide", "single-ranked"])
def test_rank_values(gf_ctx, ranks):
    n = 1000
    c = _cluster(3000 + len(ranks), n, 300, 3)
    rng = np.random.default_rng(len(ranks))
    plain_D, plain_X = gf_ctx.build_snapshot(**c)
    assert gf_ctx.build_info()[:3] == (1, 0, 0)
    if ranks == "all-unranked":
        r = np.full(n, U, dtype=np.uint32)
    elif ranks == "all-equal":
        r = np.full(n, 7, dtype=np.uint32)
    elif ranks == "wide":  # more than 256 distinct ranks up to 2^32 - 2: four label passes; ties keep the priority order
        values = np.unique(rng.integers(0, 0xFFFFFFFE, size=300, dtype=np.uint64))
        assert len(values) > 256
        r = rng.choice(values, size=n).astype(np.uint32)
        r[rng.random(n) < 0.1] = U
        r[:2] = (0, 0xFFFFFFFE)
    else:
        r = np.full(n, U, dtype=np.uint32)
        r[int(rng.integers(0, n))] = 3
    c = dict(c, driver_label_rank=r, exec_label_rank=r.copy())
    D, X = gf_ctx.build_snapshot(**c)
    info = gf_ctx.build_info()
    grouped = ranks in ("wide", "single-ranked")
    assert info[:3] == (1, 1 if grouped else 0, 0) and info[3] <= SCALARS_ONLY
    avail, sched, rD, rX = _check_snapshot(gf_ctx, c, D, X)
    if not grouped:
        assert np.array_equal(D, plain_D) and np.array_equal(X, plain_X)
    else:  # nodes of equal rank keep the priority order (the unlabelled lists)
        for got, plain in ((D, plain_D), (X, plain_X)):
            pos = np.empty(n, dtype=np.int64)
            pos[plain] = np.arange(len(plain))
            rk = r[got].astype(np.int64)
            assert (np.diff(rk) >= 0).all()
            same = np.diff(rk) == 0
            assert (np.diff(pos[got])[same] > 0).all()
    _check_decisions(gf_ctx, c, avail, sched, rD, rX)


@pytest.mark.gpu
def test_resident_path_with_labels(gf_ctx):
    n = 3000
    c = _cluster(77, n, 500, 3)
    rng = np.random.default_rng(5)
    el = rng.choice([0, 1, 2, U], size=n).astype(np.uint32)
    gf_ctx.set_cluster(c["alloc"], c["node_flags"], c["name_rank"], overhead=c["overhead"], zone=c["zone"], n_zones=c["n_zones"])
    gf_ctx.usage_apply(c["res_node"], c["res_req"], +1)
    g0 = gf_ctx.generation()
    gf_ctx.build_snapshot_resident(resident_usage=True, want_orders=False)  # the unlabelled build: how the generations move
    g1 = gf_ctx.generation()
    step = tuple(b - a for a, b in zip(g0, g1))
    assert gf_ctx.build_info()[:3] == (1, 0, 0)
    w = wl.config(2, n_nodes=16, n_apps=128)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    oapps = ob.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    for rep in range(3):
        flags = c["node_flags"].copy()
        if rep:  # this request's NodeNames: other driver candidates
            flags = (flags & ~np.uint32(ps.DRIVER_CANDIDATE)) | np.where(rng.random(n) < 0.5, ps.DRIVER_CANDIDATE, 0).astype(np.uint32)
        before = gf_ctx.generation()
        D, X = gf_ctx.build_snapshot_resident(resident_usage=True, node_flags=flags if rep else None, driver_label_rank=el,
                                              exec_label_rank=el)
        assert tuple(b - a for a, b in zip(before, gf_ctx.generation())) == step
        info = gf_ctx.build_info()
        assert info[:3] == (1, 1, 0) and info[3] <= SCALARS_ONLY
        cc = dict(c, node_flags=flags, driver_label_rank=el, exec_label_rank=el)
        avail, sched, rD, rX = _check_snapshot(gf_ctx, cc, D, X)
        ref = ob.fit_fifo_chain(0, avail, oapps, rD, rX)
        gf_ctx.chain_cache_stats(reset=True)
        for again in range(2):  # the second identical Filter resumes from the first one's checkpoints
            gpu = gf_ctx.fit_batch(FIFO, 0, apps)
            assert gpu.failed_at == ref.failed_at and np.array_equal(gpu.results, ref.results)
        chains, resumed, evaluated, skipped = gf_ctx.chain_cache_stats()
        assert (chains, resumed) == (2, 1), (chains, resumed, evaluated, skipped)


@pytest.mark.gpu
def test_switches(gf_ctx):
    n = 1000
    c = _family(_cluster(4000, n, 300, 3), "a", np.random.default_rng(1))
    plain = dict(c, driver_label_rank=None, exec_label_rank=None)
    gf_ctx.build_snapshot(**plain)
    assert gf_ctx.build_info()[:3] == (1, 0, 0)  # today's behaviour
    D1, X1 = gf_ctx.build_snapshot(**c)
    assert gf_ctx.build_info()[:3] == (1, 1, 0)
    avail, sched, rD, rX = _check_snapshot(gf_ctx, c, D1, X1)
    w = wl.config(2, n_nodes=16, n_apps=64)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    on_device = [gf_ctx.fit_batch(FIFO, algo, apps) for algo in PACKERS]
    gf_ctx.set_option("snapshot_finalize_host", 1)
    try:
        D2, X2 = gf_ctx.build_snapshot(**c)
        info = gf_ctx.build_info()
        assert info[:3] == (2, 0, 0) and info[3] > 6 * 8 * n
        _check_snapshot(gf_ctx, c, D2, X2)
        for algo, dev in zip(PACKERS, on_device):
            host = gf_ctx.fit_batch(FIFO, algo, apps)
            assert host.failed_at == dev.failed_at and np.array_equal(host.results, dev.results)
    finally:
        gf_ctx.set_option("snapshot_finalize_host", 0)
    _check_decisions(gf_ctx, c, avail, sched, rD, rX)  # (on the host-built layout of the same lists)
    # two shards on a repeated device id: builds with labels, answers like one device
    oapps = ob.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    with gangfit.Context(devices=[0, 0]) as g:
        Dg, Xg = g.build_snapshot(**c)
        assert g.build_info()[:3] == (1, 1, 0)
        assert np.array_equal(Dg, rD) and np.array_equal(Xg, rX)
        for algo in (0, 4):
            gpu = g.fit_batch(INDEPENDENT, algo, apps)
            ref = ob.fit_independent(algo, avail, oapps, rD, rX, sched=sched, zone=c["zone"])
            assert np.array_equal(gpu.results, ref.results)
    with gangfit.Context(0) as fresh:
        assert fresh.build_info() == (0, 0, 0, 0)
        with fresh.view() as v:
            fresh.build_snapshot(**c)
            assert v.build_info() == fresh.build_info() and v.build_info()[:3] == (1, 1, 0)


@pytest.mark.gpu
def test_executor_label_only_reports_its_route(gf_ctx):
    """The shape of the host mirror's device check (host/tests/host_test.cpp): executors prefer "spot" over "on-demand", a third
    of the nodes carry neither, and the driver candidates are the request's NodeNames, drawn independently of the label."""
    n = 300
    c = _cluster(0x5EED, n, 120, 3)
    rng = np.random.default_rng(8)
    c["exec_label_rank"] = rng.choice([0, 1, U], size=n).astype(np.uint32)
    D, X = gf_ctx.build_snapshot(**c)
    avail, sched, rD, rX = _check_snapshot(gf_ctx, c, D, X)
    route, grouped, fell_back, d2h = gf_ctx.build_info()
    assert route in (1, 2) and grouped == 1 and fell_back == (1 if route == 2 else 0)
    if not _same_relative_order(rD, rX):
        assert route == 2  # lists that conflict cannot have been installed from one order
    assert (d2h <= SCALARS_ONLY) == (route == 1)
    _check_decisions(gf_ctx, c, avail, sched, rD, rX)
