"""The resident worker on the zone-aware tightly-pack packers (single-az-tightly-pack, az-aware-tightly-pack): every answer
bit for bit what a launch (gf_fit_batch) and the CPU oracle give, tickets in flight, installs, refusals, co-residency.
`python -m pytest tests -m gpu`."""
import time

import numpy as np
import pytest

import gangfit
import kats
import magnitudes
from gangfit import _native as N
from gangfit import workloads as wl
from oracle import binding as ob
from test_gpu_parity import _assert_same
from test_gpu_zones import _zoned_problem

pytestmark = pytest.mark.gpu

IND = gangfit.GF_MODE_INDEPENDENT
TIGHT = gangfit.GF_ALGO_TIGHTLY_PACK
SAZ, AZA = gangfit.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK, gangfit.GF_ALGO_AZ_AWARE_TIGHTLY_PACK
SAZ_MF = gangfit.GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION
O_ALGO = {SAZ: ob.ALGO_SINGLE_AZ_TIGHTLY_PACK, AZA: ob.ALGO_AZ_AWARE_TIGHTLY_PACK, TIGHT: 0}
GIB = kats.GIB


def _setup(ctx, avail, sched, zone, D, X):
    ctx.set_snapshot(avail, sched)
    if zone is not None:
        ctx.set_zones(zone)
    ctx.set_orders(D, X)


def _same(a, b):
    return np.array_equal(a.results, b.results) and np.array_equal(a.exec_nodes, b.exec_nodes)


def _check(ctx, algo, avail, sched, zone, D, X, drv, exe, k):
    """Installs the problem; worker == launch bit for bit (results and exec_nodes), both == the oracle.  Returns the oracle's answer."""
    _setup(ctx, avail, sched, zone, D, X)
    apps = gangfit.make_apps(drv, exe, k)
    launch = ctx.fit_batch(IND, algo, apps)
    worker = ctx.worker_fit(algo, apps)
    assert np.array_equal(worker.results, launch.results)
    for a in np.nonzero(launch.results["has_capacity"])[0]:  # (an infeasible record's slice is unspecified on both sides)
        assert np.array_equal(worker.placement(int(a))[2], launch.placement(int(a))[2])
    ref = ob.fit_independent(O_ALGO[algo], np.asarray(avail, dtype=np.int64), ob.make_apps(drv, exe, k), D, X, closed_form=True,
                             sched=np.asarray(sched, dtype=np.int64), zone=np.asarray(zone, dtype=np.uint32))
    _assert_same(worker, ref, apps)
    _assert_same(launch, ref, apps)
    return ref


@pytest.mark.parametrize("layout", ["general", "merged"])
@pytest.mark.parametrize("algo", [SAZ, AZA])
@pytest.mark.parametrize("n", [64, 200, 1000])
def test_worker_parity_random(gf_ctx, algo, n, layout):
    rng = np.random.default_rng(41 * algo + n + 7 * len(layout))
    seen = set()
    for tight_cluster in (True, False):
        for n_zones in (1, 3, 5):
            a = 130
            avail, sched, zone, D, X, drv, exe, k = _zoned_problem(rng, n, a, tight_cluster, layout, n_zones)
            drv[:4] = 0  # drivers that ask for nothing; with executors that ask for nothing either, a zone of unused nodes has
            exe[:2] = 0  # average 0.0 and turns the gang down (test_choice_and_tie_break_on_the_worker pins that)
            k[4:8] = 0
            drv[6:8] = 1 << 40  # K = 0 and a driver that fits nowhere
            if not tight_cluster:  # long gangs: K > 512, placements over more than 63 nodes (the entry-wise averages)
                exe[8:12] = [250, 1, 0]         # small executors: the gang fits a zone
                exe[12:16] = [750000, 1, 0]     # one executor per node at the most, more executors than nodes: it fits nowhere
                k[8:16] = rng.integers(3 * n + 520, 3 * n + 900, size=8)
                k[16:20] = rng.integers(1, 4, size=4)  # small gangs of gpu executors
                exe[16:20, 2] = 1
            ref = _check(gf_ctx, algo, avail, sched, zone, D, X, drv, exe, k)
            feas = ref.results["has_capacity"] != 0
            for name, m in (("gpu", (exe[:, 2] > 0) & (k > 0)), ("k0", k == 0), ("long", k > 512), ("any", np.ones(a, dtype=bool))):
                seen.update((name, bool(f)) for f in feas[m])
    want = {(kind, f) for kind in ("any", "gpu", "k0", "long") for f in (True, False)}
    assert want <= seen, want - seen


@pytest.mark.parametrize("case", kats.REFERENCE_PINNED, ids=[c["name"] for c in kats.REFERENCE_PINNED])
def test_reference_pinned_through_the_worker(gf_ctx, case):
    """T1 / T3 / T4 of the reference select single-az-tightly-pack on one zone."""
    avail = np.array(case["avail"], dtype=np.int64)
    _setup(gf_ctx, avail, avail, np.zeros(len(avail), dtype=np.uint32), case["D"], case["X"])
    out = gf_ctx.worker_fit(SAZ, gangfit.make_apps([case["drv"]], [case["exe"]], [case["k"]]))
    ok, d, ex = out.placement(0)
    assert bool(ok) == case["feasible"]
    if ok:
        assert d == case["driver"] and ex.tolist() == case["execs"]
    else:
        assert out.results["driver_node"][0] == gangfit.GF_NO_NODE and out.results["exec_len"][0] == 0


def _one(ctx, algo, drv, exe, k):
    out = ctx.worker_fit(algo, gangfit.make_apps([drv], [exe], [k]))
    launch = ctx.fit_batch(IND, algo, gangfit.make_apps([drv], [exe], [k]))
    assert np.array_equal(out.results, launch.results)
    ok, d, ex = out.placement(0)
    return bool(ok), int(d), ex.tolist()


def test_choice_and_tie_break_on_the_worker(gf_ctx):
    sched = [[16000, 64 * GIB, 0], [16000, 64 * GIB, 0], [8000, 16 * GIB, 0]]
    avail = [[16000, 64 * GIB, 0], [16000, 64 * GIB, 0], [4000, 8 * GIB, 0]]
    _setup(gf_ctx, avail, sched, [0, 0, 1], [0, 1, 2], [0, 1, 2])
    assert _one(gf_ctx, SAZ, [1000, GIB, 0], [1000, GIB, 0], 2) == (True, 2, [2, 2])  # zone 1: average Max 7/8 beats 3/16
    sched2 = [[8000, 16 * GIB, 0], [8000, 16 * GIB, 0]]
    avail2 = [[4000, 8 * GIB, 0], [4000, 8 * GIB, 0]]
    _setup(gf_ctx, avail2, sched2, [5, 9], [1, 0], [0, 1])
    assert _one(gf_ctx, SAZ, [1000, GIB, 0], [1000, GIB, 0], 2) == (True, 1, [1, 1])  # exactly equal: the first zone of the list
    # no single zone fits: az-aware falls back to the plain order, single-az says no
    sched3 = [[4000, 8 * GIB, 0], [4000, 8 * GIB, 0]]
    avail3 = [[2000, 8 * GIB, 0], [2000, 8 * GIB, 0]]
    _setup(gf_ctx, avail3, sched3, [0, 1], [0, 1], [0, 1])
    assert not _one(gf_ctx, SAZ, [1000, GIB, 0], [1000, GIB, 0], 2)[0]
    assert _one(gf_ctx, AZA, [1000, GIB, 0], [1000, GIB, 0], 2) == (True, 0, [0, 1])
    # ... and only then: a gang that fits zone 1 stays in zone 1 although the plain order would start on node 0
    assert _one(gf_ctx, AZA, [1000, GIB, 0], [1000, GIB, 0], 1) == _one(gf_ctx, SAZ, [1000, GIB, 0], [1000, GIB, 0], 1)
    # a feasible zone with average 0.0 is not better than the worst: no capacity
    full = [[4000, 8 * GIB, 0], [4000, 8 * GIB, 0]]
    _setup(gf_ctx, full, full, [0, 0], [0, 1], [0, 1])
    assert not _one(gf_ctx, SAZ, [0, 0, 0], [0, 0, 0], 2)[0]


@pytest.mark.parametrize("layout", ["merged", "general"])
def test_choice_in_the_efficiency_regime(gf_ctx, layout):
    """tests/magnitudes.py's `efficiency` regime through the worker: zone 1 is zone 0's exact twin (equal averages: the first
    zone of the evaluation list is taken), zone 2 its twin one ulp of efficiency higher (the higher average is taken), on
    quantities whose float64 conversions round."""
    rng = np.random.default_rng(0xEFF)
    avail, sched, zone, D, X, drv, exe, k, _ = magnitudes.problem("efficiency", rng, layout, 3)
    for algo in (SAZ, AZA):
        ref = _check(gf_ctx, algo, avail, sched, zone, D, X, drv, exe, k)
        assert ref.results["has_capacity"].any()


@pytest.mark.parametrize("host_outputs", [False, True])
@pytest.mark.parametrize("sets", [1, 4])
def test_tickets_in_flight(sets, host_outputs):
    import torch

    ctx = gangfit.Context(0, options={"worker_sets": sets})
    try:
        w = wl.headline(3000, 400, seed=0x20AE)
        s = w.snapshot
        zone = (wl.splitmix64(0xB1, len(s.avail), 9) % np.uint64(3)).astype(np.uint32)
        _setup(ctx, s.avail, s.sched, zone, s.driver_order, s.exec_order)
        dev = torch.device("cuda:0")
        rng = np.random.default_rng(17 + sets)
        queues = []
        for q in range(5):  # different queues
            pick = rng.permutation(400)[: 400 - 31 * q]
            kk = w.k[pick].copy()
            kk[::40] = 30000  # (more executors than the cluster holds: their pre-filled placements must stay as they were)
            apps, total_k = gangfit.with_offsets(gangfit.make_apps(w.drv[pick], w.exe[pick], kk))
            queues.append((apps, total_k))
        max_k = max(q[1] for q in queues)
        for algo in (SAZ, AZA):
            want = [ctx.fit_batch(IND, algo, q[0]) for q in queues]
            assert any((x.results["has_capacity"] == 0).any() for x in want) and any(x.results["has_capacity"].any() for x in want)
            d_apps = [torch.from_numpy(q[0].view(np.uint8).copy()).to(dev) for q in queues]
            for n_batches in (1, 20, 150):
                if host_outputs:
                    res = [torch.zeros(400 * 16, dtype=torch.uint8).pin_memory() for _ in range(n_batches)]
                    exe = [torch.full((max_k + 1,), -7, dtype=torch.int32).pin_memory() for _ in range(n_batches)]
                else:
                    res = [torch.zeros(400 * 16, dtype=torch.uint8, device=dev) for _ in range(n_batches)]
                    exe = [torch.full((max_k + 1,), -7, dtype=torch.int32, device=dev) for _ in range(n_batches)]
                torch.cuda.synchronize()
                flags = N.GF_WORKER_HOST_OUTPUTS if host_outputs else 0
                batches = [(len(queues[i % 5][0]), d_apps[i % 5].data_ptr(), res[i].data_ptr(), exe[i].data_ptr(), queues[i % 5][1], flags)
                           for i in range(n_batches)]
                first = ctx.worker_submit_dev(algo, batches)
                ctx.worker_wait(first, n_batches)
                ctx.worker_stop()  # (torch's default stream would wait for a resident worker: its copies below)
                for i in range(n_batches):
                    apps, total_k = queues[i % 5]
                    got_r = res[i].cpu().numpy()[: len(apps) * 16].view(N.RESULT_DTYPE)
                    got_x = exe[i].cpu().numpy().view(np.uint32)
                    assert np.array_equal(got_r, want[i % 5].results), (n_batches, i)
                    for a in range(len(apps)):
                        lo, hi = int(apps["exec_off"][a]), int(apps["exec_off"][a]) + int(apps["k"][a])
                        if got_r["has_capacity"][a]:
                            assert np.array_equal(got_x[lo:hi], want[i % 5].exec_nodes[lo:hi]), (n_batches, i, a)
                        else:  # nothing is written before the choice: the caller's words are untouched
                            assert (got_x[lo:hi] == np.uint32(0xFFFFFFF9)).all(), (n_batches, i, a)
            st = ctx.worker_stats()
            assert st["posted"] == st["complete"]
        # a bounded stream leaves by itself
        ctx.worker_stop()
        res = [torch.zeros(400 * 16, dtype=torch.uint8, device=dev) for _ in range(6)]
        exe = [torch.zeros(max_k + 1, dtype=torch.int32, device=dev) for _ in range(6)]
        torch.cuda.synchronize()
        arr = ctx.worker_batches([(len(queues[i % 5][0]), d_apps[i % 5].data_ptr(), res[i].data_ptr(), exe[i].data_ptr(), queues[i % 5][1])
                                  for i in range(6)], leave_after=True)
        first = ctx.worker_submit_prepared(SAZ, arr)
        ctx.worker_wait(first, 6)
        deadline = time.perf_counter() + 2.0
        while ctx.worker_stats()["resident"] and time.perf_counter() < deadline:
            time.sleep(0.001)
        assert not ctx.worker_stats()["resident"]
        want0 = ctx.fit_batch(IND, SAZ, queues[0][0])
        assert np.array_equal(res[0].cpu().numpy()[: len(queues[0][0]) * 16].view(N.RESULT_DTYPE), want0.results)
    finally:
        ctx.close()


def test_installs_and_packer_changes():
    ctx = gangfit.Context(0, options={"worker_idle_us": 200000})
    try:
        w = wl.headline(3000, 300, seed=0x51)
        s = w.snapshot
        apps = gangfit.make_apps(w.drv, w.exe, w.k)
        zone_a = (wl.splitmix64(0xC1, len(s.avail), 9) % np.uint64(3)).astype(np.uint32)
        zone_b = (wl.splitmix64(0xC2, len(s.avail), 9) % np.uint64(5)).astype(np.uint32)
        _setup(ctx, s.avail, s.sched, zone_a, s.driver_order, s.exec_order)
        # (the launch's answer first: what is resident below is the worker alone)
        want_a = ctx.fit_batch(IND, SAZ, apps)
        first = ctx.worker_fit(SAZ, apps)
        assert _same(first, want_a)
        assert ctx.worker_stats()["resident"]
        ctx.set_zones(zone_b)  # an install: the resident worker leaves, the next batch answers for the new zones
        ctx.set_orders(s.driver_order, s.exec_order)
        assert not ctx.worker_stats()["resident"]
        second = ctx.worker_fit(SAZ, apps)
        ref = ob.fit_independent(O_ALGO[SAZ], s.avail, ob.make_apps(w.drv, w.exe, w.k), s.driver_order, s.exec_order,
                                 closed_form=True, sched=s.sched, zone=zone_b)
        _assert_same(second, ref, apps)
        assert not np.array_equal(first.results, second.results) or not np.array_equal(first.exec_nodes, second.exec_nodes)
        launched = {algo: ctx.fit_batch(IND, algo, apps) for algo in (TIGHT, SAZ, AZA)}
        for algo in (TIGHT, SAZ, AZA, TIGHT):  # packer changes on one context, no worker_stop in between
            assert _same(ctx.worker_fit(algo, apps), launched[algo]), algo
            assert ctx.worker_stats()["resident"]
        st = ctx.worker_stats()
        assert st["posted"] == st["complete"] == 6  # every ticket of this context
        ctx.worker_stop()
    finally:
        ctx.close()


def _refused(ctx, algo, apps, code):
    with pytest.raises(gangfit.GangfitError) as e:
        ctx.worker_fit(algo, apps)
    assert e.value.code == code, (e.value.code, code)


def test_refusals():
    ctx = gangfit.Context(0)
    try:
        w = wl.headline(500, 10, seed=1)
        s = w.snapshot
        apps = gangfit.make_apps(w.drv, w.exe, w.k)
        _setup(ctx, s.avail, s.sched, None, s.driver_order, s.exec_order)  # no zones installed
        _refused(ctx, SAZ, apps, N.GF_ERR_UNSUPPORTED)
        _refused(ctx, AZA, apps, N.GF_ERR_UNSUPPORTED)
        zone3 = (np.arange(500) % 3).astype(np.uint32)
        ctx.set_snapshot(s.avail)  # no schedulable columns
        ctx.set_zones(zone3)
        ctx.set_orders(s.driver_order, s.exec_order)
        _refused(ctx, SAZ, apps, N.GF_ERR_STATE)
        _refused(ctx, AZA, apps, N.GF_ERR_STATE)
        _setup(ctx, s.avail, s.sched, (np.arange(500) % 64).astype(np.uint32), s.driver_order, s.exec_order)
        _refused(ctx, AZA, apps, N.GF_ERR_UNSUPPORTED)  # 64 zones + the plain order: 65 views
        assert _same(ctx.worker_fit(SAZ, apps), ctx.fit_batch(IND, SAZ, apps))  # ... while single-az with 64 zones is served
        _setup(ctx, s.avail, s.sched, (np.arange(500) % 65).astype(np.uint32), s.driver_order, s.exec_order)
        _refused(ctx, SAZ, apps, N.GF_ERR_UNSUPPORTED)  # 65 zones
        _setup(ctx, s.avail, s.sched, zone3, s.driver_order, s.exec_order)
        _refused(ctx, SAZ_MF, apps, N.GF_ERR_UNSUPPORTED)
        v = ctx.view()
        _refused(v, SAZ, apps, N.GF_ERR_UNSUPPORTED)
        v.close()
        assert _same(ctx.worker_fit(SAZ, apps), ctx.fit_batch(IND, SAZ, apps))
        ctx.worker_stop()
    finally:
        ctx.close()


def test_a_fifo_chain_and_a_launch_start_next_to_a_worker_resident_on_single_az():
    """The zone-aware instances keep the worker's register budget (104 VGPRs): a FIFO chain and a gf_fit_batch of a plain packer
    start next to the resident worker without waiting for it to idle out."""
    ctx = gangfit.Context(0, options={"worker_idle_us": 500000})
    try:
        w = wl.headline(5000, 300, seed=0xFEED)
        s = w.snapshot
        zone = (wl.splitmix64(0xD1, len(s.avail), 9) % np.uint64(3)).astype(np.uint32)
        _setup(ctx, s.avail, s.sched, zone, s.driver_order, s.exec_order)
        apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
        want = ctx.fit_batch(gangfit.GF_MODE_FIFO_CHAIN, TIGHT, apps)
        want_ind = ctx.fit_batch(IND, SAZ, apps)
        want_tight = ctx.fit_batch(IND, TIGHT, apps)
        ctx.set_option("chain_cache", 0)  # the chain below replays
        assert _same(ctx.worker_fit(SAZ, apps), want_ind)
        assert ctx.worker_stats()["resident"]
        t0 = time.perf_counter()
        got = ctx.fit_batch(gangfit.GF_MODE_FIFO_CHAIN, TIGHT, apps)
        dt = time.perf_counter() - t0
        assert ctx.worker_stats()["resident"]  # ... and it is still there
        assert _same(got, want) and got.failed_at == want.failed_at
        assert dt < 0.1, dt  # (half a second would be the worker's idle period)
        t0 = time.perf_counter()
        got_ind = ctx.fit_batch(IND, TIGHT, apps)  # (as in the test this one copies)
        dt = time.perf_counter() - t0
        assert ctx.worker_stats()["resident"]
        assert _same(got_ind, want_tight)
        assert dt < 0.1, dt
        ctx.worker_stop()
    finally:
        ctx.close()


def test_headline_size_on_the_worker(gf_ctx):
    """10 000 nodes x 1 000 applications, three zones in AZ-major order, both packers, against the closed-form oracle."""
    w = wl.headline(10000, 1000)
    s = w.snapshot
    zone = (wl.splitmix64(0xA2, len(s.avail), 9) % np.uint64(3)).astype(np.uint32)
    # AZ-major: the priority order regrouped by zone (stable), as a cluster sorted by zone first presents it
    D = np.asarray(s.driver_order)[np.argsort(zone[s.driver_order], kind="stable")]
    X = np.asarray(s.exec_order)[np.argsort(zone[s.exec_order], kind="stable")]
    for algo in (SAZ, AZA):
        ref = _check(gf_ctx, algo, s.avail, s.sched, zone, D, X, w.drv, w.exe, w.k)
        assert ref.results["has_capacity"].mean() > 0.5
