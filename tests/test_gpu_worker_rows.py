"""Shape rows of the resident worker (csrc/gangfit_worker_rows.h; gangfit_worker.inc, tightly-pack instance): a workgroup that has
met one scaled executor request kRowSightings times keeps the first 64 nodes with room for it in LDS and decides later gangs of
that shape from the row.  Every ticket below answers what a launch (gf_fit_batch_dev) answers on the same records: the results
byte for byte, the placements of every feasible record word for word.  Small geometries (one workgroup, or 3 sets of 2) so that
few tickets take a workgroup past the threshold."""
import numpy as np
import pytest

import gangfit
from gangfit import workloads as wl
# (the launch's answers, the stream and the hand-made cluster are shared with tests/test_gpu_worker_rows_edges.py: one copy)
from worker_rows_cases import apps_of as _apps, edge_cluster as _edge_cluster, stream as _stream

pytestmark = pytest.mark.gpu

GIB = 1 << 30
K_ROWS, K_SIGHTINGS, GF_MAX_K = 40, 4, 1 << 20  # gangfit_worker_rows.h


def _install(ctx, avail, sched, d_order, x_order):
    ctx.set_snapshot(avail, sched)
    ctx.set_orders(d_order, x_order)


@pytest.fixture(scope="module")
def small():
    """wl.config(2, 300, 165): 21 executor shapes; 76 records whose driver sits inside the cut, 48 whose driver's node keeps no room
    for an executor (counted with the numpy model when this test was written)."""
    w = wl.config(2, n_nodes=300, n_apps=165)
    return w, _apps(w.drv, w.exe, w.k)


def _tickets_for(sets, bps, shape_id, n_apps):
    """Tickets after which, by the hand-out rule (workgroup bs of a set serves the applications 16 bsr + l + row * 16 bps of its
    round's ticket, bsr = (bs + round) mod bps), at least three quarters of all decisions come after their workgroup has seen
    their shape kRowSightings + 16 times: kRowSightings to count, and up to one decision of each of the sixteen wavefronts that goes
    by while the entry is claimed, or while the row is built (a wavefront never waits for a row)."""
    stride = 16 * bps
    n_shapes = int(shape_id.max()) + 1
    for rounds in range(1, 4000):
        late = total = 0
        for bs in range(bps):
            seen = np.zeros(n_shapes, dtype=np.int64)
            for r in range(rounds):
                bsr = (bs + r) % bps
                ids = [a for row in range(n_apps // stride + 1) for a in range(16 * bsr + row * stride, 16 * bsr + row * stride + 16) if a < n_apps]
                cnt = np.bincount(shape_id[ids], minlength=n_shapes)
                late += int(np.maximum(seen + cnt - np.maximum(seen, K_SIGHTINGS + 16), 0).sum())
                total += len(ids)
                seen += cnt
        if late * 4 >= total * 3:
            return rounds * sets
    raise AssertionError("no stream length found")


@pytest.mark.parametrize("sets,bps", [(1, 1), (3, 2)])
def test_a_stream_builds_rows_and_then_hits_them(small, sets, bps):
    w, apps = small
    s = w.snapshot
    _, sid = np.unique(w.exe, axis=0, return_inverse=True)
    n_tickets = _tickets_for(sets, bps, sid.ravel(), len(apps))
    ctx = gangfit.Context(0, options={"worker_sets": sets, "worker_blocks_per_set": bps})
    try:
        _install(ctx, s.avail, s.sched, s.driver_order, s.exec_order)
        feas = _stream(ctx, [apps] * n_tickets)[id(apps)]
        assert feas.any()
        assert ctx.worker_geometry() == (sets, bps)
        st = ctx.worker_row_stats()
        print("tickets", n_tickets, "row stats", st)
        assert st["built"] > 0 and st["built"] <= K_ROWS * sets * bps
        assert st["served"] * 2 >= n_tickets * len(apps), st
    finally:
        ctx.close()


def test_edges_of_a_row_on_a_hand_made_cluster():
    """One workgroup.  Per shape twenty K = 1 records per ticket take it past the threshold; the same ticket, posted five times,
    meets every edge with the row in place.  Shape A = 2 cpu / 8 GiB: capacity 4 on a small node, 8 on a big one; the first 64 qualifying
    slots are 2 .. 65: row total 256, 255 with a 1 cpu / 1 GiB driver on slot 2 (its node keeps 3)."""
    avail, sched, order = _edge_cluster()
    D, A, A2 = [1000, GIB, 0], [2000, 8 * GIB, 0], [2000, 4 * GIB, 0]
    B = [16000, 64 * GIB, 0]      # room on the ten big nodes only: a complete row of ten entries
    Z, Z1 = [0, 0, 0], [2000, 0, 0]  # nothing requested (every capacity is the clamp); one zero dimension
    DBIG = [9000, GIB, 0]         # a driver only a big node takes: slot 120, behind every cut below
    DALL = [8000, 32 * GIB, 0]    # a driver that leaves its small node no room at all (c_ds == 0)
    drv, exe, k = [], [], []

    def add(d, e, kk):
        drv.append(d), exe.append(e), k.append(kk)

    for shape in (A, A2, B, Z, Z1):
        for _ in range(20):
            add(D, shape, 1)
    add(D, A, 255)            # K == the corrected row total
    add(D, A, 256)            # one more: a 65th qualifying node exists — falls back, feasible
    add(D, B, 10)             # a complete row of ten: exactly its total ...
    add(D, B, 11)             # ... and one more: falls back, infeasible
    add(D, A, 0), add(D, A, 1)
    add(DBIG, A, 200)         # the driver behind the cut
    add(DALL, A, 252)         # the driver's capacity drops to zero: 63 entries of 4
    add(DALL, A, 253)         # ... and one more than they hold: falls back, feasible
    add(D, Z, GF_MAX_K)       # the capacity clamp with K == GF_MAX_K
    add(D, Z1, 300)
    add(D, A2, 500), add(D, A, 100)                 # two shapes that differ in one word only
    add(D, [2000, 8 * GIB + 1, 0], 7), add(D, A, 9)  # one byte off its unit (the int64 path, no lookup) between two row hits
    apps = _apps(drv, exe, k)
    ctx = gangfit.Context(0, options={"worker_sets": 1, "worker_blocks_per_set": 1})
    try:
        _install(ctx, avail, sched, order, order.copy())
        feas = _stream(ctx, [apps] * 5)[id(apps)]
        want = dict(zip(range(100, 115), [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]))
        assert {i: int(feas[i]) for i in want} == want
        st = ctx.worker_row_stats()
        print("row stats", st)
        assert 0 < st["built"] <= 5
        # The edges ran on the row path: 110 records of the ticket are decided by a row once it exists (all 115 but K == 0, the
        # request off its unit, and the three that fall back by design).  Sixteen wavefronts meet a new shape at once and only the
        # one that claims the entry counts, so the rows are in place during the second ticket at the latest: the last three tickets
        # are served in full; two of them are asked for.
        assert st["served"] >= 2 * 110, st
        # a driver that is no executor candidate: the executor order leaves out the node the small driver takes
        ctx.worker_stop()
        _install(ctx, avail, sched, order, order[order != 2].copy())
        _stream(ctx, [apps] * 3)
    finally:
        ctx.close()


def test_more_shapes_than_rows():
    avail, sched, order = _edge_cluster()
    shapes = [[1000 * c, m * GIB, 0] for c in range(1, 6) for m in range(1, 10)]
    assert len(shapes) == K_ROWS + 5
    drv, exe, k = [], [], []
    for i, e in enumerate(shapes):  # shape by shape: the first rows exist before the directory is full (a workgroup whose
        for rep in range(20):  # directory fills before it has built any row stops looking up); sixteen wavefronts meet a
            # new shape at once and only the claimant counts: records 17 .. 20 take the shape past the threshold
            drv.append([1000, GIB, 0]), exe.append(e), k.append(1 + (7 * i + 3 * rep) % 60)
    apps = _apps(drv, exe, k)
    ctx = gangfit.Context(0, options={"worker_sets": 1, "worker_blocks_per_set": 1})
    try:
        _install(ctx, avail, sched, order, order.copy())
        _stream(ctx, [apps] * 3)
        st = ctx.worker_row_stats()
        print("row stats", st)
        assert 0 < st["built"] <= K_ROWS and st["served"] > 0 and st["fell_back"] > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("host_outputs", [False, True], ids=["device", "pinned"])
def test_gpu_gangs_and_pinned_outputs(host_outputs):
    """Gangs of gpu executors, and nothing else, on a cluster that has the compact table of gpu nodes: the launch packs them from
    that table, the worker — once their shape has a row — from the row; and the same stream with its outputs in pinned host memory
    (the row path writes the private slice, the wavefront copies out).  A feasible gang of at most 63 executors is always covered by
    its row (64 entries of capacity >= 1, or every node with room at all; the driver's reservation empties one entry at most), so
    once the rows stand — sixteen shapes, six records of each per ticket: within the first five tickets — every such record is
    served: two tickets' worth of them is asked for, of ten tickets."""
    w = wl.headline(2000, 4000, seed=0x6E77)
    s = w.snapshot
    gpu = np.nonzero(w.exe[:, 2] > 0)[0][:96]
    assert len(gpu) == 96
    apps = _apps(w.drv[gpu], w.exe[gpu], w.k[gpu])
    ctx = gangfit.Context(0, options={"worker_sets": 1, "worker_blocks_per_set": 1})
    try:
        _install(ctx, s.avail, s.sched, s.driver_order, s.exec_order)
        feas = _stream(ctx, [apps] * 10, host_outputs=host_outputs)[id(apps)]
        covered = int((feas & (apps["k"] >= 1) & (apps["k"] <= 63)).sum())
        assert covered >= 32, covered
        st = ctx.worker_row_stats()
        print("row stats", st, "covered per ticket", covered)
        assert st["built"] > 0 and st["served"] >= 2 * covered, (st, covered)
    finally:
        ctx.close()


def test_a_second_snapshot_gets_its_own_rows(small):
    w, apps = small
    s = w.snapshot
    other = wl.make_snapshot(300, 0xB0B)
    ctx = gangfit.Context(0, options={"worker_sets": 1, "worker_blocks_per_set": 1})
    try:
        _install(ctx, s.avail, s.sched, s.driver_order, s.exec_order)
        a = _stream(ctx, [apps] * 8)[id(apps)]
        _install(ctx, other.avail, other.sched, other.driver_order, other.exec_order)
        b = _stream(ctx, [apps] * 8)[id(apps)]  # (compared with a launch on the second snapshot)
        assert a.any() and b.any()
        assert ctx.worker_row_stats()["built"] > 0
    finally:
        ctx.close()


def test_sixteen_wavefronts_meet_one_shape_at_once(small):
    """Tickets of sixteen identical records on one workgroup: every wavefront probes, counts, and — one of them — builds and
    publishes the same row while the others decide."""
    w, _ = small
    i = int(np.argmax(w.k))
    apps = _apps(np.repeat(w.drv[i:i + 1], 16, axis=0), np.repeat(w.exe[i:i + 1], 16, axis=0), np.repeat(w.k[i:i + 1], 16))
    s = w.snapshot
    ctx = gangfit.Context(0, options={"worker_sets": 1, "worker_blocks_per_set": 1})
    try:
        _install(ctx, s.avail, s.sched, s.driver_order, s.exec_order)
        _stream(ctx, [apps] * 40)
        st = ctx.worker_row_stats()
        print("row stats", st)
        assert st["built"] == 1 and st["served"] + st["fell_back"] == 40 * 16
    finally:
        ctx.close()
