"""The resident worker reads the operands of its rare paths from its argument segment where it uses them (gangfit_worker.inc,
OPERANDS).  What can go wrong is an operand read from the wrong place on a path a headline batch never takes, so ONE small
cluster and ONE batch of forty applications drive every such path — narrow and int64 decisions by the same wavefront, the
sparse pack, the fallback, K = 0, an infeasible gang, cooperative emission — for every packer the worker serves, with device and
host destinations, counters, the general layout and a snapshot without the int32 twin; then two snapshots one after the other on
one context and a stream that wraps the round words.  Every answer is compared bit for bit with gf_fit_batch_dev on the same
inputs, through a bounded stream (GF_WORKER_LEAVE_AFTER).  `python -m pytest tests -m gpu`."""
import numpy as np
import pytest

import gangfit
from gangfit import _native as N

pytestmark = pytest.mark.gpu

IND = gangfit.GF_MODE_INDEPENDENT
TIGHT, EVEN, MINFRAG = gangfit.GF_ALGO_TIGHTLY_PACK, gangfit.GF_ALGO_DISTRIBUTE_EVENLY, gangfit.GF_ALGO_MINIMAL_FRAGMENTATION
SAZ, AZA = gangfit.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK, gangfit.GF_ALGO_AZ_AWARE_TIGHTLY_PACK
ZONED = (SAZ, AZA)
GIB = 1 << 30
# the batch's named applications (the rest are small gangs in whole units)
A_ODD, A_GPU, A_FALLBACK, A_K0, A_INFEASIBLE, A_RUN, A_ODD_GPU = 3, 7, 11, 13, 17, 19, 23


def _cluster(n_nodes, seed=0x0A9):
    """n_nodes nodes in priority order 0, 1, ...: cpu in whole cores, memory in whole GiB, a gpu on every thirteenth node.  Node 0
    and the last node (the first driver candidate of the merged and of the general layout) hold exactly two of the fallback gang's
    executors and nothing to spare; the other nodes hold two and a driver."""
    rng = np.random.default_rng(seed)
    avail = np.zeros((n_nodes, 3), dtype=np.int64)
    avail[:, 0] = 1000 * rng.choice([64, 67, 72], size=n_nodes)  # (the units are the columns' gcds: one core, one GiB, one gpu)
    avail[:, 1] = GIB * rng.choice([64, 97, 128], size=n_nodes)
    avail[::13, 2] = rng.choice([1, 2, 4, 8], size=len(avail[::13]))
    avail[0] = (60000, 64 * GIB, 0)
    avail[1, :2] = (67000, 97 * GIB)
    avail[n_nodes - 1] = (60000, 64 * GIB, 0)
    avail[n_nodes - 2, :2] = (67000, 97 * GIB)
    avail[13, 2] = 1
    zone = (np.arange(n_nodes) % 3).astype(np.uint32)
    return avail, avail.copy(), zone


def _batch(avail, n_apps=40, seed=0xBA7):
    rng = np.random.default_rng(seed)
    drv = np.zeros((n_apps, 3), dtype=np.int64)
    exe = np.zeros((n_apps, 3), dtype=np.int64)
    drv[:, 0] = 1000 * rng.integers(1, 5, size=n_apps)
    drv[:, 1] = GIB * rng.integers(1, 5, size=n_apps)
    exe[:, 0] = 1000 * rng.integers(1, 9, size=n_apps)
    exe[:, 1] = GIB * rng.integers(1, 9, size=n_apps)
    k = rng.integers(1, 12, size=n_apps).astype(np.int32)
    drv[A_ODD], exe[A_ODD], k[A_ODD] = (1001, GIB, 0), (2000, 2 * GIB + 1, 0), 5            # no multiple of the units: the int64 path
    drv[A_GPU], exe[A_GPU], k[A_GPU] = (1000, GIB, 0), (2000, 2 * GIB, 1), 6                # a gang of gpu executors: the sparse pack
    drv[A_ODD_GPU], exe[A_ODD_GPU], k[A_ODD_GPU] = (1500, GIB, 1), (1001, GIB, 1), 3        # both
    # the fallback: executors of 30 cores, as many as the cluster holds WITHOUT a driver; a driver of 4 cores fits node 0 first and
    # costs it an executor, every other node has the 4 cores to spare
    exe[A_FALLBACK] = (30000, 8 * GIB, 0)
    drv[A_FALLBACK] = (4000, GIB, 0)
    k[A_FALLBACK] = int(np.minimum(avail[:, 0] // 30000, avail[:, 1] // (8 * GIB)).sum())
    k[A_K0] = 0
    exe[A_INFEASIBLE], k[A_INFEASIBLE] = (1000, GIB, 0), 100000
    drv[A_RUN], exe[A_RUN], k[A_RUN] = (1000, GIB, 0), (1000, GIB, 0), 40                   # forty on one node: cooperative emission
    return drv, exe, k


def _install(ctx, avail, sched, zone, layout="merged"):
    n = len(avail)
    order = np.arange(n, dtype=np.uint32)
    ctx.set_snapshot(avail, sched)
    ctx.set_zones(zone)
    if layout == "merged":
        ctx.set_orders(order, order)
    else:  # the two orders disagree: driver positions go through dslot
        ctx.set_orders(order[::-1].copy(), order)


class _Stream:
    """The batch on the device, the launch path's answer to it, and bounded streams of tickets of it through the worker."""

    def __init__(self, ctx, algo, drv, exe, k):
        import torch

        self.torch, self.ctx, self.algo = torch, ctx, algo
        self.dev = torch.device("cuda:0")
        self.apps, self.total_k = gangfit.with_offsets(gangfit.make_apps(drv, exe, k))
        self.n = len(self.apps)
        self.d_apps = torch.from_numpy(self.apps.view(np.uint8).copy()).to(self.dev)
        self.want_res, self.want_exec = self._outputs(False)
        torch.cuda.synchronize()
        ctx.fit_batch_dev(IND, algo, self.n, self.d_apps.data_ptr(), self.want_res.data_ptr(), self.want_exec.data_ptr(), self.total_k)
        torch.cuda.synchronize()
        self.res = self.want_res.cpu().numpy().view(N.RESULT_DTYPE)
        self.exec_nodes = self.want_exec.cpu().numpy().view(np.uint32)

    def _outputs(self, host):
        t = self.torch
        if host:
            return t.zeros(self.n * 16, dtype=t.uint8).pin_memory(), t.zeros(self.total_k + 1, dtype=t.int32).pin_memory()
        return t.zeros(self.n * 16, dtype=t.uint8, device=self.dev), t.zeros(self.total_k + 1, dtype=t.int32, device=self.dev)

    def placement(self, a):
        lo = int(self.apps["exec_off"][a])
        return self.exec_nodes[lo:lo + int(self.apps["k"][a])]

    def run(self, n_tickets, host=False, leave_after=True):
        outs = [self._outputs(host) for _ in range(n_tickets)]
        self.torch.cuda.synchronize()
        flags = N.GF_WORKER_HOST_OUTPUTS if host else 0
        arr = self.ctx.worker_batches([(self.n, self.d_apps.data_ptr(), r.data_ptr(), e.data_ptr(), self.total_k, flags) for r, e in outs],
                                      leave_after=leave_after)
        first = self.ctx.worker_submit_prepared(self.algo, arr)
        self.ctx.worker_wait(first, n_tickets)
        self.ctx.worker_stop()
        self.torch.cuda.synchronize()
        for i, (r, e) in enumerate(outs):
            got_r = r.cpu().numpy().view(N.RESULT_DTYPE)
            got_e = e.cpu().numpy().view(np.uint32)
            assert np.array_equal(got_r, self.res), (i, np.nonzero(got_r != self.res)[0][:8])
            # An infeasible record's slice is unspecified: a launch and the worker's direct emission (tightly-pack, device
            # destination) leave what they tried there, a worker that answers through its private slice leaves the caller's words alone.
            if self.algo != TIGHT or host:
                for a in np.nonzero(self.res["has_capacity"])[0]:
                    lo = int(self.apps["exec_off"][a])
                    hi = lo + int(self.apps["k"][a])
                    assert np.array_equal(got_e[lo:hi], self.exec_nodes[lo:hi]), (i, a)
            else:
                assert np.array_equal(got_e, self.exec_nodes), (i, np.nonzero(got_e != self.exec_nodes)[0][:8])


def _assert_categories(s, algo, avail, zone, drv, exe, k, merged=True):
    """Every category of the batch is there, read from the LAUNCH path's answers (s: a _Stream of packer `algo`)."""
    unit = [int(np.gcd.reduce(avail[:, j][avail[:, j] != 0])) for j in range(3)]
    whole = np.array([all(int(v) % u == 0 for v, u in zip(np.concatenate([drv[a], exe[a]]), unit * 2)) for a in range(len(k))])
    ok = s.res["has_capacity"] != 0
    assert whole.sum() >= 30 and ok[whole].sum() >= 25                                 # requests in whole units (narrow decisions)
    assert not whole[A_ODD] and ok[A_ODD] and not whole[A_ODD_GPU] and ok[A_ODD_GPU]   # no multiple of the units (int64 decisions)
    assert ok[A_GPU] and (avail[s.placement(A_GPU), 2] > 0).all()                      # packed on gpu nodes
    assert ok[A_K0] and s.res["exec_len"][A_K0] == 0
    assert not ok[A_INFEASIBLE]
    run = s.placement(A_RUN)
    assert ok[A_RUN] and len(run) == 40
    if algo in (TIGHT, SAZ, AZA):
        assert np.max(np.bincount(run)) > 16                                           # more than sixteen in a row on one node
    if algo in ZONED:  # a single zone was chosen wherever one zone holds the gang
        assert len(set(zone[s.placement(A_RUN)])) == 1 and len(set(zone[s.placement(A_GPU)])) == 1
    # the fallback gang: as many executors as the WHOLE cluster holds without a driver, and the first driver candidate that fits is
    # a node that loses an executor to its driver — the next candidate is taken.  No single zone holds it: single-az refuses it.
    first_fit = 0 if merged else len(avail) - 1
    assert (avail[first_fit] >= drv[A_FALLBACK]).all()
    if algo == SAZ:
        assert not ok[A_FALLBACK]
    else:
        assert ok[A_FALLBACK] and s.res["exec_len"][A_FALLBACK] == k[A_FALLBACK]
        if algo in (TIGHT, EVEN, AZA):
            assert s.res["driver_node"][A_FALLBACK] == (1 if merged else len(avail) - 2)


N_NODES = 130  # three chunks of 64 slots, the last one ragged


@pytest.mark.parametrize("algo", [TIGHT, EVEN, MINFRAG, SAZ, AZA])
def test_one_cluster_drives_every_path(algo):
    avail, sched, zone = _cluster(N_NODES)
    drv, exe, k = _batch(avail)
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail, sched, zone)
        s = _Stream(ctx, algo, drv, exe, k)
        _assert_categories(s, algo, avail, zone, drv, exe, k)
        s.run(3)             # device destinations
        s.run(3, host=True)  # a private slice and the copy-out
    finally:
        ctx.close()


def test_counters_are_the_launch_paths():
    avail, sched, zone = _cluster(N_NODES)
    drv, exe, k = _batch(avail)
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail, sched, zone)
        ctx.scan_stats(enable=True, reset=True)
        s = _Stream(ctx, TIGHT, drv, exe, k)  # (one launch)
        want = ctx.scan_stats(enable=True, reset=True)
        assert want[0] > 0 and want[1] > 0
        s.run(2)
        got = ctx.scan_stats(enable=True, reset=True)
        assert got == (2 * want[0], 2 * want[1])
        ctx.scan_stats(enable=False)
    finally:
        ctx.close()


@pytest.mark.parametrize("algo", [TIGHT, EVEN, SAZ])
def test_general_layout(algo):
    avail, sched, zone = _cluster(N_NODES)
    drv, exe, k = _batch(avail)
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail, sched, zone, layout="general")
        s = _Stream(ctx, algo, drv, exe, k)
        _assert_categories(s, algo, avail, zone, drv, exe, k, merged=False)
        s.run(3)
        s.run(2, host=True)
    finally:
        ctx.close()


def test_snapshot_without_the_int32_twin():
    avail, sched, zone = _cluster(N_NODES)
    avail[5, 1] += 1  # one odd byte: the memory unit is 1 and 64 GiB is not below 2^30 units
    sched = avail.copy()
    # the layout's own criterion (fill_narrow, gangfit_slot_layout.h; tests/test_slot_layout_cpu.py pins it): the twin exists only when
    # every value is below 2^30 of its column's gcd
    assert int(np.gcd.reduce(avail[:, 1])) == 1 and int(avail[:, 1].max()) >= 1 << 30
    drv, exe, k = _batch(avail)
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail, sched, zone)
        s = _Stream(ctx, TIGHT, drv, exe, k)
        _assert_categories(s, TIGHT, avail, zone, drv, exe, k)
        s.run(3)
        s.run(2, host=True)
    finally:
        ctx.close()


@pytest.mark.parametrize("algo", [TIGHT, AZA])
def test_two_snapshots_one_after_the_other(algo):
    """Another node count is another n_chunks (3, then 5), other tables, other units: nothing of the first launch survives."""
    ctx = gangfit.Context(0)
    try:
        answers = []
        for n_nodes, seed in ((N_NODES, 1), (300, 2), (N_NODES, 1)):
            avail, sched, zone = _cluster(n_nodes, seed)
            if n_nodes == 300:
                avail[:, 0] += 500 * (np.arange(n_nodes) % 2)  # half cores: another cpu unit
                sched = avail.copy()
            drv, exe, k = _batch(avail)
            _install(ctx, avail, sched, zone)
            s = _Stream(ctx, algo, drv, exe, k)
            s.run(3)
            answers.append((s.res.copy(), s.exec_nodes.copy()))
        assert not np.array_equal(answers[0][1], answers[1][1])
        assert np.array_equal(answers[0][0], answers[2][0]) and np.array_equal(answers[0][1], answers[2][1])
    finally:
        ctx.close()


@pytest.mark.parametrize("leave_after", [True, False])
def test_a_stream_longer_than_the_ring(leave_after):
    """150 tickets on two sets of one workgroup: 75 rounds per wavefront wrap the eight count words nine times; the worker
    leaves by GF_WORKER_LEAVE_AFTER, and once by gf_worker_stop."""
    avail, sched, zone = _cluster(N_NODES)
    drv, exe, k = _batch(avail)
    ctx = gangfit.Context(0, options={"worker_sets": 2, "worker_blocks_per_set": 1})
    try:
        _install(ctx, avail, sched, zone)
        s = _Stream(ctx, TIGHT, drv, exe, k)
        s.run(150, leave_after=leave_after)
        assert ctx.worker_geometry() == (2, 1)
        st = ctx.worker_stats()
        assert st["posted"] == st["complete"] == 150 and not st["resident"]
    finally:
        ctx.close()



def test_chunks_behind_group_zero():
    """4 300 nodes are 68 chunks: four lie behind group 0 of the chunk index, where the narrow view asks each chunk on its own
    (chunk_may_hold: row c + n_chunks and c + 2 n_chunks of the maxima, the units).  The first 4 200 nodes are too small for any
    executor, so every gang is packed from chunks 65 .. 67."""
    n_nodes, small = 4300, 4200
    avail, sched, zone = _cluster(n_nodes)
    avail[:small, 0] = 500  # half a core: another cpu unit, and no executor fits
    avail[:small, 2] = 0
    avail[small + 13, 2] = 3
    sched = avail.copy()
    drv, exe, k = _batch(avail)
    drv[:, 0] = 500         # drivers fit the small nodes
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail, sched, zone)
        s = _Stream(ctx, TIGHT, drv, exe, k)
        ok = s.res["has_capacity"] != 0
        assert ok.sum() >= 30 and ok[A_RUN] and ok[A_GPU] and ok[A_ODD] and not ok[A_INFEASIBLE]
        assert all((s.placement(a) >= small).all() for a in np.nonzero(ok)[0])
        s.run(3)
        s.run(2, host=True)
    finally:
        ctx.close()
