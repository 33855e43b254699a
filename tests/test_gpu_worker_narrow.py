"""The resident worker's tightly-pack decisions in the snapshot's scaled int32 domain (gangfit_worker.inc: scale_record,
NarrowView, NarrowApp) next to its int64 path: every case compares the worker's result records and placements byte for byte
with gf_fit_batch on the same context AND with the literal oracle.  An application takes the scaled path when the snapshot has
a scaled form, every request of it is an exact multiple of its dimension's unit below 2^30 units and it is no gang of gpu
executors on a cluster with the compact gpu table; the cases put applications on both sides of each of those conditions, next
to each other in one ticket.  `python -m pytest tests/test_gpu_worker_narrow.py -m gpu`."""
import numpy as np
import pytest

import gangfit
import magnitudes as mg
import stress_lib
from gangfit import workloads as wl
from oracle import binding as ob

pytestmark = pytest.mark.gpu

TIGHT = gangfit.GF_ALGO_TIGHTLY_PACK
IND = gangfit.GF_MODE_INDEPENDENT
HOST_OUTPUTS = gangfit._native.GF_WORKER_HOST_OUTPUTS
GIB, MIB = 1 << 30, 1 << 20


@pytest.fixture(scope="module")
def ctx():
    c = gangfit.Context(0)
    yield c
    c.close()


def _submit(ctx, apps, host_outputs):
    """One ticket through gf_worker_submit_dev: (results, exec_nodes) as numpy arrays.  Device-resident outputs, or — with
    GF_WORKER_HOST_OUTPUTS — outputs in pinned host memory."""
    import torch

    dev = torch.device("cuda:0")
    apps_off, total_k = gangfit.with_offsets(apps)
    n = len(apps_off)
    d_apps = torch.from_numpy(apps_off.view(np.uint8).copy()).to(dev)
    if host_outputs:
        res = torch.zeros(n * 16, dtype=torch.uint8).pin_memory()
        ex = torch.zeros(total_k + 1, dtype=torch.int32).pin_memory()
    else:
        res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        ex = torch.zeros(total_k + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # torch fills on ITS stream; the worker does not wait for it
    first = ctx.worker_submit_dev(TIGHT, [(n, d_apps.data_ptr(), res.data_ptr(), ex.data_ptr(), total_k,
                                           HOST_OUTPUTS if host_outputs else 0)])
    ctx.worker_wait(first, 1)
    ctx.worker_stop()
    torch.cuda.synchronize()
    return (res.cpu().numpy().view(gangfit._native.RESULT_DTYPE).copy(), ex.cpu().numpy().view(np.uint32).copy(), apps_off)


def _check(ctx, avail, D, X, drv, exe, k, flags=None, where="", closed_form=False, submit=True):
    """Installs the problem; the worker (blocking call with pinned outputs, and tickets with device-resident and with pinned
    outputs) against the launch path and the literal oracle.  Returns the oracle's answer."""
    ctx.set_snapshot(avail)
    ctx.set_orders(D, X)
    flags = np.ones(len(k), dtype=np.uint32) if flags is None else flags
    apps = gangfit.make_apps(drv, exe, k, flags)
    ref = ob.fit_independent(TIGHT, avail, ob.make_apps(drv, exe, k, flags), D, X, closed_form=closed_form)
    launch = ctx.fit_batch(IND, TIGHT, apps)
    assert stress_lib.same(launch, ref, False) is None, where
    wk = ctx.worker_fit(TIGHT, apps)
    assert wk.results.tobytes() == launch.results.tobytes(), where
    assert stress_lib.same(wk, ref, False) is None, where
    feasible = np.nonzero(ref.results["has_capacity"])[0]
    for a in feasible:
        assert np.array_equal(wk.placement(int(a))[2], launch.placement(int(a))[2]), f"{where} app {a}"
    if submit:
        for host_outputs in (False, True):
            res, ex, apps_off = _submit(ctx, apps, host_outputs)
            assert res.tobytes() == launch.results.tobytes(), f"{where} host_outputs={host_outputs}"
            for a in feasible:  # (device-resident outputs: the placements of a gang that does not fit are unspecified)
                off, n = int(apps_off["exec_off"][a]), int(apps_off["k"][a])
                assert np.array_equal(ex[off:off + n], ref.placement(int(a))[2]), f"{where} host_outputs={host_outputs} app {a}"
    return ref


def test_headline_at_size(ctx):
    """10 000 nodes x 1 000 applications: cpu in 100 m, memory in 256 MiB, every request a multiple — all scaled but the gangs
    of gpu executors (5 %, the compact table)."""
    w = wl.headline()
    s = w.snapshot
    ref = _check(ctx, s.avail, s.driver_order, s.exec_order, w.drv, w.exe, w.k, where="headline")
    assert 0 < int(ref.results["has_capacity"].sum())


def test_forms_alternate_within_a_ticket(ctx):
    """Neighbouring applications of one wavefront alternate between the paths: every other request is off its unit by one
    byte of memory or one milli-core (executor or driver), the rest are multiples."""
    w = wl.headline(3000, 640, seed=0xA17)
    s = w.snapshot
    drv, exe = w.drv.copy(), w.exe.copy()
    a = np.arange(len(w.k))
    exe[a % 4 == 1, 1] += 1  # unit + 1 byte
    exe[a % 8 == 3, 0] -= 1  # one milli-core off
    drv[a % 8 == 7, 1] += 1
    drv[a % 16 == 5, 0] += 1
    ref = _check(ctx, s.avail, s.driver_order, s.exec_order, drv, exe, w.k, where="mixed forms")
    has = ref.results["has_capacity"].astype(bool)
    assert has[a % 2 == 1].any() and has[a % 2 == 0].any()


@pytest.mark.parametrize("regime", ["bytes", "narrow-edge", "huge", "max-k"])
def test_magnitude_regimes(ctx, regime):
    """tests/magnitudes.py: `bytes` has no scaled table (everything on int64); narrow-edge puts scaled magnitudes of exactly
    2^30 - 1 into the table and the requests, and their twins one unit past; huge and max-k are the int64 path's and the K
    clamp's edges."""
    feasible = 0
    for name, p, _ in mg.cases(regime):
        avail, sched, zone, D, X, drv, exe, k, flags = p
        ref = _check(ctx, avail, D, X, drv, exe, k, flags, where=f"{regime} {name}", closed_form=mg.CLOSED_FORM[regime],
                     submit=name.endswith("/1z"))
        feasible += int(ref.results["has_capacity"].sum())
    assert feasible > 0


def _small_cluster(rng, n=200, gpus=True):
    """cpu in 250 m, memory in MiB (odd multiples keep the units), a gpu on some nodes; the executor and driver orders are
    one order (merged layout)."""
    cpu = rng.integers(-2, 64, size=n) * 250
    mem = (rng.integers(1, 1 << 11, size=n) * 2 - 1) * MIB
    gpu = np.where(rng.random(n) < 0.2, rng.integers(0, 9, size=n), 0) if gpus else np.zeros(n, dtype=np.int64)
    avail = np.stack([cpu, mem, gpu], axis=1).astype(np.int64)
    order = wl.reference_node_order(avail)
    return avail, order, order.copy()


def test_request_shapes(ctx):
    """Zero request dimensions (never limit), K = 0, K = 1, an infeasible gang, gangs of gpu executors (the compact table,
    int64) next to scaled ones."""
    rng = np.random.default_rng(0x5CA1)
    avail, D, X = _small_cluster(rng)
    rows = [  # drv, exe, k
        ([250, 64 * MIB, 0], [0, 0, 0], 1000),             # nothing limits: every executor on the first node
        ([250, 64 * MIB, 0], [500, 0, 0], 40),             # memory never limits
        ([250, 64 * MIB, 0], [0, 128 * MIB, 0], 40),       # cpu never limits
        ([0, 0, 0], [250, MIB, 0], 0),                     # K = 0
        ([0, 0, 0], [250, MIB, 0], 1),                     # K = 1
        ([1000, 256 * MIB, 0], [1000, 512 * MIB, 0], 1),
        ([250, 64 * MIB, 0], [16000, 4096 * MIB, 0], 4000),  # infeasible: K beyond the cluster
        ([250, 64 * MIB, 0], [250, 64 * MIB, 1], 3),       # gpu executors
        ([250, 64 * MIB, 1], [250, 64 * MIB, 2], 2),
        ([250, 64 * MIB, 0], [250, 64 * MIB, 1], 500),     # gpu executors, infeasible
        ([64000, 0, 0], [250, MIB, 0], 2),                 # no driver candidate fits
        ([250, 64 * MIB, 0], [250, 64 * MIB + 1, 0], 5),   # not a multiple
    ]
    rows = rows * 3 + [([250 * int(rng.integers(0, 9)), int(rng.integers(0, 65)) * MIB, 0],
                        [250 * int(rng.integers(0, 9)), int(rng.integers(0, 513)) * MIB, int(rng.random() < 0.2)],
                        int(rng.integers(0, 120))) for _ in range(92)]
    drv = np.array([r[0] for r in rows], dtype=np.int64)
    exe = np.array([r[1] for r in rows], dtype=np.int64)
    k = np.array([r[2] for r in rows], dtype=np.int32)
    ref = _check(ctx, avail, D, X, drv, exe, k, where="request shapes")
    has = ref.results["has_capacity"]
    assert has[0] == 1 and has[3] == 1 and has[6] == 0 and has[10] == 0


def test_driver_on_an_executor_node_and_the_fallback(ctx):
    """The driver's reservation lands on a node the executors use (a -= drv in the scaled domain), and a gang whose first
    driver candidate sits where the executors were needed: wave_fallback picks a later candidate."""
    n = 130
    avail = np.zeros((n, 3), dtype=np.int64)
    avail[:, 0] = 250  # a quarter core: no driver of 1000 m, no executor of 2000 m
    avail[:, 1] = 3 * MIB
    # node 5 (first in the order) holds the driver and exactly two executors — or three executors without the driver
    avail[5] = [6250, 96 * MIB, 0]
    avail[77] = [1000, 16 * MIB, 0]   # a later driver candidate that holds no executor
    avail[100] = [8000, 64 * MIB, 0]  # two more executors
    order = np.concatenate([[5], np.setdiff1d(np.arange(n), [5])]).astype(np.uint32)
    drv = np.array([[250, MIB, 0], [1000, 16 * MIB, 0], [1000, 16 * MIB, 0], [1000, 16 * MIB, 0]], dtype=np.int64)
    exe = np.array([[2000, 32 * MIB, 0]] * 4, dtype=np.int64)
    k = np.array([4, 4, 5, 6], dtype=np.int32)
    ref = _check(ctx, avail, order, order.copy(), drv, exe, k, where="fallback")
    # apps 0, 1: driver and two executors on node 5, two on node 100.  app 2: with the driver on node 5 there are four places;
    # three on node 5 + two on node 100 once the driver moves to node 77.  app 3: six executors do not exist
    assert ref.results["has_capacity"].tolist() == [1, 1, 1, 0]
    assert int(ref.results["driver_node"][0]) == 5 and int(ref.results["driver_node"][2]) == 77
    # the same on the general layout (driver order != executor order)
    dorder = order[::-1].copy()
    _check(ctx, avail, dorder, order.copy(), drv, exe, k, where="fallback, general layout")


def test_congested_scans_run_past_group_0(ctx):
    """Usage ~ U[0.95, 1]: about half of the gangs do not fit, the scans walk the whole executor order (three groups of 64
    chunks at 10 000 nodes) and the driver-candidate fallback."""
    w = wl.headline(10000, 160, seed=0xC0DE, congested=True)
    s = w.snapshot
    ref = _check(ctx, s.avail, s.driver_order, s.exec_order, w.drv, w.exe, w.k, where="congested")
    has = ref.results["has_capacity"]
    assert 0 < int(has.sum()) < len(has)


def test_selftest_covers_the_scaled_arithmetic(ctx):
    """gf_selftest case (d): narrow_magic_lane against narrow_magic, the scaled cap3 against plain quotients, scale_word
    against a 64-bit divide on multiples, their neighbours, quotients of 2^30 - 1 and 2^30 and negative words."""
    assert ctx.selftest(seed=0x5EED, n_cases=4096) == 0
