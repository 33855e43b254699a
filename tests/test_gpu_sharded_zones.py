"""GPU parity of the node-range sharded batch for the zone-aware tightly-pack packers (single-az-tightly-pack, az-aware-tightly-pack):
the shard steps once per candidate view (every zone of the evaluation list, plus the plain order for az-aware) and the finish step
that computes every zone's average efficiency and chooses (csrc/gangfit_shard.inc), driven by gangfit/sharded.py (a thread group
of shards on cuda:0) and inside the library (a multi-device context with a repeated device id).  Against the oracle, one-device
gf_fit_batch (fit_zoned_fused_kernel) and the averages bit for bit.  `python -m pytest tests -m gpu`."""
import ctypes as C
import threading

import numpy as np
import pytest

import gangfit
from gangfit import sharded
from gangfit import workloads as wl
from oracle import binding as ob
from test_gpu_group import split  # noqa: F401  (fixture: both GANGFIT_TEST_GROUP_SPLIT modes)
from test_gpu_parity import _assert_same
from test_gpu_zones import AZA, GIB, O_ALGO, SAZ, _bits, _setup, _zoned_problem

pytestmark = pytest.mark.gpu
IND = gangfit.GF_MODE_INDEPENDENT
N = gangfit._native


def _run(world, algo, avail, sched, zone, D, X, apps):
    """`world` shards of cuda:0 as a thread group, one gf_ctx each; every rank's answer."""
    import torch

    torch.cuda.init()  # (one thread initialises the runtime: see tests/test_gpu_sharded.py)
    group = sharded.ThreadGroup(world)
    outs, errs = [None] * world, []

    def work(r):
        try:
            with gangfit.Context(0) as ctx:
                _setup(ctx, avail, sched, zone, D, X)
                eng = sharded.HipShardEngine(ctx, r, world, "cuda:0")
                outs[r] = sharded.sharded_fit(eng, group.comm(r), algo, apps)
        except Exception as e:
            errs.append(e)
            group._barrier.abort()

    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    if errs:
        raise errs[0]
    return outs


def _check(world, algo, avail, sched, zone, D, X, drv, exe, k):
    """Every rank's sharded answer == the oracle == one device, and the averages chooseBestResult compared, bit for bit."""
    apps = gangfit.make_apps(drv, exe, k)
    ref = ob.fit_independent(O_ALGO[algo], avail, ob.make_apps(drv, exe, k), D, X, closed_form=True, sched=sched, zone=zone)
    with gangfit.Context(0) as ctx:
        _setup(ctx, avail, sched, zone, D, X)
        one = ctx.fit_batch(IND, algo, apps)
        _assert_same(one, ref, apps)
        for out in _run(world, algo, avail, sched, zone, D, X, apps):
            _assert_same(out, ref, apps)
            assert np.array_equal(out.results, one.results) and np.array_equal(out.exec_nodes, one.exec_nodes)
            assert np.array_equal(_bits(ctx.avg_packing_efficiency(algo, apps, out)), _bits(ref.avg_eff))
    return ref


def _az_major(avail, zone):
    order = wl.reference_node_order(avail, zone)
    return order, order.copy()


@pytest.mark.parametrize("algo", [SAZ, AZA])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [5, 64, 130, 1000])
def test_shards_of_one_gpu_match_oracle(algo, world, n):
    rng = np.random.default_rng(5100 + 31 * world + algo + n)
    feasible = 0
    for layout in ("merged", "identical"):
        for n_zones in (1, 3, 5):
            tight = bool(rng.integers(0, 2))
            avail, sched, zone, D, X, drv, exe, k = _zoned_problem(rng, n, 90, tight, layout, n_zones)
            ref = _check(world, algo, avail, sched, zone, D, X, drv, exe, k)  # zone ids interleaved over the order
            feasible += int(ref.results["has_capacity"].sum())
            D2, X2 = _az_major(avail, zone)  # the reference's own order: every zone one stretch of it
            ref = _check(world, algo, avail, sched, zone, D2, X2, drv, exe, k)
            feasible += int(ref.results["has_capacity"].sum())
    if n >= 64:
        assert feasible > 0


@pytest.mark.parametrize("algo", [SAZ, AZA])
@pytest.mark.parametrize("world", [2, 5])
@pytest.mark.parametrize("n", [700, 3000])
def test_gpu_gangs_inside_zones(algo, world, n):
    """Gangs of gpu executors on clusters whose gpu nodes are a minority: each view packs them from its zone's sub-slots of the
    compact gpu table (placements map sub-slot -> slot), cut at the shards' sub-slot ranges."""
    rng = np.random.default_rng(7300 + 13 * algo + world + n)
    for az_major in (False, True):
        avail, sched, zone, D, X, drv, exe, k = _zoned_problem(rng, n, 140, bool(rng.integers(0, 2)), "merged", 3)
        has = rng.random(n) < 0.12
        avail[:, 2] = np.where(has, rng.integers(1, 9, size=n), rng.integers(-1, 1, size=n))
        sched[:, 2] = np.maximum(avail[:, 2], 0) + rng.integers(0, 3, size=n)
        exe[:, 2] = np.where(rng.random(len(exe)) < 0.7, rng.integers(1, 4, size=len(exe)), 0)
        drv[:, 2] = np.where(rng.random(len(drv)) < 0.3, 1, 0)
        k = np.where(rng.random(len(k)) < 0.7, np.minimum(k, rng.integers(0, 30, size=len(k))), k).astype(np.int32)
        if az_major:
            D, X = _az_major(avail, zone)
        _check(world, algo, avail, sched, zone, D, X, drv, exe, k)


@pytest.mark.parametrize("algo", [SAZ, AZA])
def test_long_gangs_take_both_averages(algo):
    """Gangs longer than kRunBlocks * 64 executors and gangs on more than kRunMax nodes: the finish step takes the entry-wise
    average where the run-wise one does not apply, as the one-launch kernel does."""
    rng = np.random.default_rng(9300 + algo)
    n, a = 2000, 120
    sched = np.zeros((n, 3), dtype=np.int64)
    sched[:, 0] = rng.integers(8, 65, size=n) * 1000
    sched[:, 1] = rng.integers(16, 257, size=n) * GIB
    used = rng.random((n, 2)) * 0.6
    avail = sched.copy()
    avail[:, 0] -= (used[:, 0] * sched[:, 0]).astype(np.int64) // 250 * 250
    avail[:, 1] -= (used[:, 1] * sched[:, 1]).astype(np.int64)
    zone = rng.integers(0, 3, size=n).astype(np.uint32)
    drv = np.zeros((a, 3), dtype=np.int64)
    exe = np.zeros((a, 3), dtype=np.int64)
    drv[:, 0] = rng.integers(1, 5, size=a) * 500
    drv[:, 1] = rng.integers(1, 9, size=a) * GIB
    exe[:, 0] = rng.integers(1, 9, size=a) * 250
    exe[:, 1] = rng.integers(1, 17, size=a) * (GIB // 2)
    k = rng.choice([1, 7, 64, 65, 300, 512, 513, 700], size=a).astype(np.int32)
    D, X = _az_major(avail, zone)
    _check(3, algo, avail, sched, zone, D, X, drv, exe, k)


def test_choice_tie_break_fallback_and_zero_requests():
    """The cases of test_gpu_zones.test_zone_choice_and_tie_break through four shards: the better zone wins, equal zones tie to
    the first zone of the driver order, az-aware falls back to the plain pack, and a zero request (average 0.0) is no zone's result."""
    drv1, exe1 = np.array([[1000, GIB, 0]]), np.array([[1000, GIB, 0]])
    two = np.array([2], dtype=np.int32)
    cases = [
        ([[16000, 64 * GIB, 0], [16000, 64 * GIB, 0], [4000, 8 * GIB, 0]], [[16000, 64 * GIB, 0], [16000, 64 * GIB, 0], [8000, 16 * GIB, 0]],
         [0, 0, 1], [0, 1, 2], [0, 1, 2], drv1, exe1),
        ([[4000, 8 * GIB, 0], [4000, 8 * GIB, 0]], [[8000, 16 * GIB, 0], [8000, 16 * GIB, 0]], [5, 9], [1, 0], [1, 0], drv1, exe1),
        ([[2000, 8 * GIB, 0], [2000, 8 * GIB, 0]], [[4000, 8 * GIB, 0], [4000, 8 * GIB, 0]], [0, 1], [0, 1], [0, 1], drv1, exe1),
        ([[4000, 8 * GIB, 0], [4000, 8 * GIB, 0]], [[4000, 8 * GIB, 0], [4000, 8 * GIB, 0]], [0, 0], [0, 1], [0, 1],
         np.zeros((1, 3)), np.zeros((1, 3))),
    ]
    # (az-aware: no zone above 0.0 -> the plain pack, in the last case too)
    want = {SAZ: [(1, 2), (1, 1), (0, None), (0, None)], AZA: [(1, 2), (1, 1), (1, 0), (1, 0)]}
    for algo in (SAZ, AZA):
        for (avail, sched, zone, D, X, drv, exe), (ok, driver) in zip(cases, want[algo]):
            avail, sched = np.array(avail, dtype=np.int64), np.array(sched, dtype=np.int64)
            ref = _check(4, algo, avail, sched, np.array(zone, dtype=np.uint32), np.array(D, dtype=np.uint32),
                         np.array(X, dtype=np.uint32), np.asarray(drv, dtype=np.int64), np.asarray(exe, dtype=np.int64), two)
            assert int(ref.results["has_capacity"][0]) == ok
            if ok:
                assert int(ref.results["driver_node"][0]) == driver


@pytest.mark.parametrize("algo", [SAZ, AZA])
def test_zone_without_drivers_and_zones_inside_one_shard(algo):
    """A zone with executor candidates but no driver candidate (it is evaluated and never fits), zones that lie inside one shard's
    range, and more shards than zones."""
    rng = np.random.default_rng(9500 + algo)
    for n in (300, 1500):
        avail, sched, zone, _, _, drv, exe, k = _zoned_problem(rng, n, 120, False, "merged", 3)
        zone = (np.arange(n) * 3 // n).astype(np.uint32)  # 0, 1, 2 in three blocks of node ids
        D, X = _az_major(avail, zone)
        D = D[zone[D] != zone[D[0]]]  # the first zone of the order hosts executors only
        for world in (2, 8):
            _check(world, algo, avail, sched, zone, D, X, drv, exe, k)


@pytest.mark.parametrize("algo", [SAZ, AZA])
@pytest.mark.parametrize("n_dev", [2, 3, 8])
def test_group_shards_zone_aware_batches(algo, n_dev, split):
    """One context over n_dev device ids (all cuda:0): a zone-aware independent batch is sharded inside the library and comes
    back as the oracle's, with the context still sharding."""
    rng = np.random.default_rng(9700 + 17 * n_dev + algo)
    with gangfit.Context(devices=[0] * n_dev) as g:
        for n in (130, 1000):
            for az_major in (False, True):
                avail, sched, zone, D, X, drv, exe, k = _zoned_problem(rng, n, 150, bool(rng.integers(0, 2)), "merged", 3)
                if az_major:
                    D, X = _az_major(avail, zone)
                _setup(g, avail, sched, zone, D, X)
                apps = gangfit.make_apps(drv, exe, k)
                ref = ob.fit_independent(O_ALGO[algo], avail, ob.make_apps(drv, exe, k), D, X, closed_form=True, sched=sched, zone=zone)
                _assert_same(g.fit_batch(IND, algo, apps), ref, apps)
                _assert_same(g.fit_batch(IND, algo, apps), ref, apps)  # (the second batch of a snapshot: no self-check)
                assert g.shard_count() == n_dev, g.last_error()


def _fault_problem():
    rng = np.random.default_rng(9900)
    avail, sched, zone, _, _, drv, exe, k = _zoned_problem(rng, 1000, 150, False, "merged", 3)
    D, X = _az_major(avail, zone)
    ref = {a: ob.fit_independent(O_ALGO[a], avail, ob.make_apps(drv, exe, k), D, X, closed_form=True, sched=sched, zone=zone)
           for a in (SAZ, AZA)}
    return avail, sched, zone, D, X, drv, exe, k, ref


def _same(out, ref):
    return np.array_equal(out.results, ref.results) and all(
        np.array_equal(out.placement(int(a))[2], ref.placement(int(a))[2]) for a in np.nonzero(ref.results["has_capacity"])[0])


@pytest.mark.parametrize("algo", [SAZ, AZA])
def test_group_really_shards_zone_aware_batches(algo, monkeypatch):
    """Without the self-check, a dropped placement reduction (option group_fault = 1) must spoil a zone-aware batch: proof that
    the other devices' shards produced part of it — a batch served by the first device alone would come back right."""
    monkeypatch.setenv("GANGFIT_TEST_GROUP_SPLIT", "1")
    avail, sched, zone, D, X, drv, exe, k, ref = _fault_problem()
    apps = gangfit.make_apps(drv, exe, k)
    with gangfit.Context(devices=[0] * 4) as g:
        _setup(g, avail, sched, zone, D, X)
        g.set_option("group_verify", 0)
        g.set_option("group_fault", 1)
        assert ref[algo].results["has_capacity"].any()
        assert not _same(g.fit_batch(IND, algo, apps), ref[algo])


@pytest.mark.parametrize("algo", [SAZ, AZA])
def test_zone_aware_batch_is_self_checked_after_a_plain_one(algo, monkeypatch):
    """The self-check runs per packer family: a plain batch that the fault cannot spoil (no executors: nothing to reduce) verifies
    the plain family on the snapshot; the first zone-aware batch is still answered by the first device as well, so the same fault
    gives the right answers, says "disagreed" and stops the sharding."""
    monkeypatch.setenv("GANGFIT_TEST_GROUP_SPLIT", "1")
    avail, sched, zone, D, X, drv, exe, k, ref = _fault_problem()
    apps = gangfit.make_apps(drv, exe, k)
    k0 = np.zeros_like(k)
    with gangfit.Context(devices=[0] * 4) as g:
        _setup(g, avail, sched, zone, D, X)
        g.set_option("group_fault", 1)
        plain = ob.fit_independent(0, avail, ob.make_apps(drv, exe, k0), D, X, closed_form=True)
        _assert_same(g.fit_batch(IND, 0, gangfit.make_apps(drv, exe, k0)), plain, gangfit.make_apps(drv, exe, k0))
        assert g.shard_count() == 4, g.last_error()
        _assert_same(g.fit_batch(IND, algo, apps), ref[algo], apps)
        assert g.shard_count() == 1 and "disagreed" in g.last_error()
        _assert_same(g.fit_batch(IND, algo, apps), ref[algo], apps)  # served by the first device from now on


@pytest.mark.parametrize("congested", [False, True])
def test_config4_size_eight_shards(congested):
    """BASELINE config 4's size (50 000 nodes x 10 000 apps), three zones in the reference's AZ-major order, eight shards of one
    device: the same answer as one device."""
    w = wl.config(4)
    snap = wl.make_snapshot(50000, 0x5EED0004, 0.93, 1.0) if congested else w.snapshot
    zone = (wl.splitmix64(0xA3, len(snap.avail), 9) % np.uint64(3)).astype(np.uint32)
    order = wl.reference_node_order(snap.avail, zone)
    apps = gangfit.make_apps(w.drv, w.exe, w.k)
    for algo in (SAZ, AZA):
        with gangfit.Context(0) as ctx:
            _setup(ctx, snap.avail, snap.sched, zone, order, order)
            one = ctx.fit_batch(IND, algo, apps)
        for out in _run(8, algo, snap.avail, snap.sched, zone, order, order, apps)[:1]:
            assert np.array_equal(out.results, one.results) and np.array_equal(out.exec_nodes, one.exec_nodes)


def _layout(ctx, algo, half=11):
    rec, words, red = C.c_uint32(), C.c_uint64(), C.c_uint64()
    rc = ctx._lib.gf_shard_layout(ctx._h, algo, half, C.byref(rec), C.byref(words), C.byref(red))
    return rc, (rec.value, words.value, red.value)


def _partials_rc(ctx, algo):
    return ctx._lib.gf_shard_partials_dev(ctx._h, algo, 0, None, None, None)


def test_layout_and_refusals():
    rng = np.random.default_rng(9950)
    avail, sched, zone, D, X, drv, exe, k = _zoned_problem(rng, 400, 10, False, "merged", 3)
    with gangfit.Context(0) as ctx:
        _setup(ctx, avail, sched, zone, D, X)
        assert _layout(ctx, 0) == (0, (1, 22, 11)) and _layout(ctx, 1) == (0, (1, 22, 22))
        assert _layout(ctx, SAZ) == (0, (3, 33, 33)) and _layout(ctx, AZA) == (0, (4, 44, 44))
        for algo in (N.GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION, N.GF_ALGO_MINIMAL_FRAGMENTATION):
            assert _layout(ctx, algo)[0] == N.GF_ERR_UNSUPPORTED and _partials_rc(ctx, algo) == N.GF_ERR_UNSUPPORTED
        with pytest.raises(gangfit.GangfitError) as e:
            sharded.ShardedBatch(sharded.HipShardEngine(ctx, 0, 2, "cuda:0"), sharded.SingleComm(),
                                 N.GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION, gangfit.make_apps(drv, exe, k))
        assert e.value.code == N.GF_ERR_UNSUPPORTED
        # general layout
        ctx.set_orders([0, 1, 2], [2, 1, 0])
        for algo in (SAZ, AZA):
            assert _layout(ctx, algo)[0] == N.GF_ERR_UNSUPPORTED and _partials_rc(ctx, algo) == N.GF_ERR_UNSUPPORTED
        # more than 64 candidate views: 64 zones are 65 views for az-aware, 65 zones for single-AZ
        every = np.arange(len(avail), dtype=np.uint32)
        for nz, bad, good in ((64, AZA, SAZ), (65, SAZ, None)):
            _setup(ctx, avail, sched, (every % nz).astype(np.uint32), every, every)
            assert _layout(ctx, bad)[0] == N.GF_ERR_UNSUPPORTED and _partials_rc(ctx, bad) == N.GF_ERR_UNSUPPORTED
            if good is not None:
                assert _layout(ctx, good) == (0, (nz, nz * 11, nz * 11))
        # zones without the schedulable columns
        ctx.set_snapshot(avail)
        ctx.set_zones(zone)
        ctx.set_orders(X, X)
        for algo in (SAZ, AZA):
            assert _layout(ctx, algo)[0] == N.GF_ERR_UNSUPPORTED and _partials_rc(ctx, algo) == N.GF_ERR_UNSUPPORTED
