"""Shape rows of the resident worker (csrc/gangfit_worker_rows.h; SHAPE ROWS in csrc/gangfit_worker.inc) where the code itself names
something special and tests/test_gpu_worker_rows.py does not go: rows built behind group 0 of the chunk index and across its
boundary, a driver behind group 0 next to a READY row, merged layouts in which both orders leave nodes out, the conditions under
which rows are off, and the ways a stream reaches the worker while rows are live.  The cases, and the reasons for their shapes, are
in tests/worker_rows_cases.py; tests/test_worker_rows_cases_cpu.py recomputes on the CPU every figure used here.

Every ticket answers what a launch (gf_fit_batch_dev) answers on the same records, results byte for byte and the placements of
feasible records word for word; on the deep cluster the launch is held against the CPU oracle first.  gf_worker_row_stats counts
since the context was created, over launches that have left: every figure below is a difference around a stream, read after
worker_stop.  `python -m pytest tests/test_gpu_worker_rows_edges.py -m gpu -s` prints them."""
import time

import numpy as np
import pytest

import gangfit
import worker_rows_cases as wc
from gangfit import _native as N
from gangfit import workloads as wl
from oracle import binding as ob
from worker_rows_cases import apps_of as _apps, launch_answers as _launch_answers, stream as _stream

pytestmark = pytest.mark.gpu

IND, TIGHT = gangfit.GF_MODE_INDEPENDENT, gangfit.GF_ALGO_TIGHTLY_PACK
ZERO = {"built": 0, "served": 0, "fell_back": 0}


@pytest.fixture(scope="module")
def consts(tmp_path_factory):
    """(kRowLen, kRows, kRowSightings, kCapClamp) of the header, through the CPU shim."""
    return wc.consts(wc.compile_shim(tmp_path_factory.mktemp("worker_rows_edges")))


@pytest.fixture(scope="module")
def small():
    """wl.config(2, 300, 165): 21 executor shapes (tests/test_gpu_worker_rows.py)."""
    w = wl.config(2, n_nodes=300, n_apps=165)
    return w, _apps(w.drv, w.exe, w.k)


def _install(ctx, avail, sched, d_order, x_order):
    ctx.set_snapshot(avail, sched)
    ctx.set_orders(d_order, x_order)


def _context(sets, bps, **options):
    return gangfit.Context(0, options={"worker_sets": sets, "worker_blocks_per_set": bps, **options})


def _moved(ctx, before):
    now = ctx.worker_row_stats()
    return {key: now[key] - before[key] for key in now}


def _sixteen(w):
    """Sixteen copies of the small batch's largest gang: one record per wavefront of a workgroup."""
    i = int(np.argmax(w.k))
    assert w.k[i] >= 1
    return _apps(np.repeat(w.drv[i:i + 1], 16, axis=0), np.repeat(w.exe[i:i + 1], 16, axis=0), np.repeat(w.k[i:i + 1], 16))


# ------------------------------------------------------------------------------------------------ 1. the deep cluster


@pytest.mark.parametrize("variant", wc.DEEP_VARIANTS)
def test_rows_behind_chunk_group_zero(variant):
    """One workgroup, the ticket of wc.deep_case posted five times.  (1) the launch is the oracle's; (2) every ticket is the
    launch's; (3) one to three rows; (4) served >= 2 S: sixteen wavefronts meet a new shape at once and only the claimant counts, so
    with twenty warm-up records per shape the rows stand during the second ticket at the latest, the last three tickets are served
    in full — S records each, and a DBIG record served from a row would be wrong in (2) — and two of them are asked for;
    (5) what must fall back does: F records in each of the last three tickets."""
    c = wc.deep_case(variant)
    apps = _apps(c.drv, c.exe, c.k)
    ref = ob.fit_independent(0, c.avail, ob.make_apps(c.drv, c.exe, c.k, np.zeros(len(c.k), dtype=np.uint32)), c.D, c.X, closed_form=True)
    ctx = _context(1, 1)
    try:
        _install(ctx, c.avail, c.sched, c.D, c.X)
        answers = _launch_answers(ctx, apps)
        res = answers[1].cpu().numpy().view(N.RESULT_DTYPE)
        placed = answers[2].cpu().numpy().view(np.uint32)
        assert np.array_equal(res, ref.results), np.nonzero(res != ref.results)[0][:8]
        for a in np.nonzero(ref.results["has_capacity"])[0]:
            lo = int(apps["exec_off"][a])
            assert np.array_equal(placed[lo:lo + int(c.k[a])], ref.placement(int(a))[2]), (variant, int(a), c.names[a])
        for a, (_, _, _, feasible, driver, _) in enumerate(c.edges, start=c.first_edge):  # (and the declared answers, once more)
            assert res["has_capacity"][a] == feasible and (not feasible or res["driver_node"][a] == driver), (variant, a)
        before = ctx.worker_row_stats()
        _stream(ctx, [apps] * 5, answers={id(apps): answers})
        assert ctx.worker_geometry() == (1, 1)
        st = _moved(ctx, before)
        print(f"deep cluster, {variant}: row stats {st}, S = {c.s}, F = {c.f}, records per ticket {len(apps)}")
        assert 1 <= st["built"] <= 3, st
        assert st["served"] >= 2 * c.s, (st, c.s)
        assert st["fell_back"] >= 3 * c.f, (st, c.f)
        assert st["served"] + st["fell_back"] <= 5 * int((c.k > 0).sum()), st  # a decision is counted once at the most
    finally:
        ctx.close()


# ------------------------------------------------------------------------- 2. where rows must be off, and the threshold


def test_a_bounded_stream_on_either_side_of_the_threshold(small, consts):
    """GF_WORKER_LEAVE_AFTER on two sets of one workgroup: kRowSightings * sets tickets are the shortest stream that looks rows up.
    One ticket less: the statistics do not move at all.  At the threshold every narrow decision with K > 0 is counted exactly once —
    one shape cannot fill the directory — and each of the two workgroups builds one row at the most."""
    w, _ = small
    s = w.snapshot
    apps = _sixteen(w)
    threshold = consts[2] * 2
    ctx = _context(2, 1)
    try:
        _install(ctx, s.avail, s.sched, s.driver_order, s.exec_order)
        answers = {id(apps): _launch_answers(ctx, apps)}
        before = ctx.worker_row_stats()
        _stream(ctx, [apps] * (threshold - 1), leave_after=True, answers=answers)
        assert ctx.worker_geometry() == (2, 1)
        below = _moved(ctx, before)
        before = ctx.worker_row_stats()
        _stream(ctx, [apps] * threshold, leave_after=True, answers=answers)
        at = _moved(ctx, before)
        print(f"bounded stream: {threshold - 1} tickets {below}, {threshold} tickets {at}")
        assert below == ZERO, below
        assert at["served"] + at["fell_back"] == threshold * 16 and at["built"] <= 2, at
        assert ctx.worker_stats()["launches"] == 2
    finally:
        ctx.close()


def test_the_counting_instance_keeps_the_launch_paths_counters(small):
    """gf_scan_stats on: the counting instance runs, however long the stream — forty tickets add forty times what one launch adds, and
    no row is looked up; off again, on the same context, the same stream builds rows."""
    w, apps = small
    s = w.snapshot
    ctx = _context(1, 1)
    try:
        _install(ctx, s.avail, s.sched, s.driver_order, s.exec_order)
        ctx.scan_stats(enable=True, reset=True)
        answers = {id(apps): _launch_answers(ctx, apps)}  # (one launch, counted)
        want = ctx.scan_stats(enable=True, reset=True)
        assert want[0] > 0 and want[1] > 0
        before = ctx.worker_row_stats()
        _stream(ctx, [apps] * 40, answers=answers)
        assert ctx.scan_stats(enable=True, reset=True) == (40 * want[0], 40 * want[1])
        assert _moved(ctx, before) == ZERO
        assert ctx.scan_stats(enable=False, reset=True) == (0, 0)
        _stream(ctx, [apps] * 40, answers=answers)
        st = _moved(ctx, before)
        print("counting instance, then the product instance:", st)
        assert st["built"] > 0 and st["served"] > 0, st
        assert ctx.scan_stats(enable=False, reset=False) == (0, 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("what", ["general-layout", "no-int32-twin"])
def test_long_streams_on_tables_without_rows(small, what):
    """The general layout (the driver order reversed: the driver step of a row decision is the merged one) and a snapshot without
    the int32 twin (one odd byte on one node: the memory unit is the byte and 2^30 units do not hold a node) never look a row up."""
    w, apps = small
    s = w.snapshot
    avail, sched, d_order = s.avail, s.sched, s.driver_order
    if what == "general-layout":
        d_order = np.ascontiguousarray(s.driver_order[::-1])
    else:
        avail = s.avail.copy()
        avail[5, 1] += 1
        assert int(np.gcd.reduce(np.abs(avail[:, 1]))) == 1 and int(avail[:, 1].max()) >= 1 << 30  # (fill_narrow's criterion)
    ctx = _context(1, 1)
    try:
        _install(ctx, avail, sched, d_order, s.exec_order)
        before = ctx.worker_row_stats()
        feas = _stream(ctx, [apps] * 40)[id(apps)]
        assert feas.any()
        assert _moved(ctx, before) == ZERO
    finally:
        ctx.close()


def test_shapes_that_never_repeat_switch_the_lookups_off(consts):
    """Six different tickets of 48 records, 288 executor requests in all and none of them twice: the directory is full within the
    first ticket and no shape is ever seen kRowSightings times, so no row is built or hit, and a wavefront that finds the directory
    full stops looking up (at most one lookup per record is counted until then)."""
    avail, sched, order = wc.edge_cluster()
    tickets = [_apps(*t) for t in wc.unique_shape_tickets()]
    assert len(tickets) == 6 and all(len(t) == 48 for t in tickets) and 48 > consts[1]
    ctx = _context(1, 1)
    try:
        _install(ctx, avail, sched, order, order.copy())
        before = ctx.worker_row_stats()
        feas = _stream(ctx, tickets)
        assert all(f.all() for f in feas.values())
        st = _moved(ctx, before)
        print("shapes that never repeat:", st)
        assert st["built"] == 0 and st["served"] == 0 and st["fell_back"] <= 6 * 48, st
    finally:
        ctx.close()


# ------------------------------------------------------------------- 3. how a stream reaches the worker, with rows live


def test_tickets_of_different_lengths_interleave(small, consts):
    """Slices of 1, 15, 16, 17, 33 and 165 records — less than a row of wavefronts, exactly one, one more, two and a ragged third, ten
    and a ragged eleventh — cycled to 72 tickets, more than the ring of 64, on three sets of two workgroups."""
    w, _ = small
    s = w.snapshot
    slices = [_apps(w.drv[:n], w.exe[:n], w.k[:n]) for n in (1, 15, 16, 17, 33, 165)]
    ctx = _context(3, 2)
    try:
        _install(ctx, s.avail, s.sched, s.driver_order, s.exec_order)
        before = ctx.worker_row_stats()
        feas = _stream(ctx, [slices[i % 6] for i in range(72)])
        assert ctx.worker_geometry() == (3, 2) and any(f.any() for f in feas.values())
        st = _moved(ctx, before)
        print("mixed tickets:", st)
        assert 0 < st["built"] <= consts[1] * 6 and st["served"] > 0, st
    finally:
        ctx.close()


def test_blocking_tickets_in_pinned_memory(small):
    """gf_worker_fit: records and answers in pinned host memory, one blocking ticket per call, twelve calls on one resident launch
    (an idle period of half a second: the worker stays)."""
    w, _ = small
    s = w.snapshot
    apps = gangfit.make_apps(w.drv, w.exe, w.k)
    ctx = _context(1, 1, worker_idle_us=500000)
    try:
        _install(ctx, s.avail, s.sched, s.driver_order, s.exec_order)
        want = ctx.fit_batch(IND, TIGHT, apps)
        assert want.results["has_capacity"].any()
        before = ctx.worker_row_stats()
        for call in range(12):
            got = ctx.worker_fit(TIGHT, apps)
            assert np.array_equal(got.results, want.results), call
            for a in np.nonzero(want.results["has_capacity"])[0]:
                assert np.array_equal(got.placement(int(a))[2], want.placement(int(a))[2]), (call, int(a))
        ctx.worker_stop()
        st = _moved(ctx, before)
        print("worker_fit:", st)
        assert st["built"] > 0 and st["served"] > 0, st
    finally:
        ctx.close()


def test_a_worker_that_idled_out_and_came_back(small):
    """An idle period of 10 us: the leader has left long before the second stream is posted 50 ms later, the worker is launched
    again and its workgroups start from an empty directory."""
    w, apps = small
    s = w.snapshot
    ctx = _context(1, 1, worker_idle_us=10)
    try:
        _install(ctx, s.avail, s.sched, s.driver_order, s.exec_order)
        answers = {id(apps): _launch_answers(ctx, apps)}
        before, launches = ctx.worker_row_stats(), ctx.worker_stats()["launches"]
        _stream(ctx, [apps] * 8, stop=False, answers=answers)
        time.sleep(0.05)
        _stream(ctx, [apps] * 8, answers=answers)
        assert ctx.worker_stats()["launches"] == launches + 2
        st = _moved(ctx, before)
        print("idle-out and relaunch:", st)
        assert st["built"] > 0, st
    finally:
        ctx.close()


def test_an_install_under_a_resident_worker(small):
    """tests/test_gpu_worker_rows.py::test_a_second_snapshot_gets_its_own_rows without the worker_stop in between: the install
    itself makes the resident worker leave (InstallGuard), and the next launch cuts its rows from the second snapshot."""
    w, apps = small
    s = w.snapshot
    other = wl.make_snapshot(300, 0xB0B)
    ctx = _context(1, 1, worker_idle_us=500000)
    try:
        _install(ctx, s.avail, s.sched, s.driver_order, s.exec_order)
        before = ctx.worker_row_stats()
        a = _stream(ctx, [apps] * 8, stop=False)[id(apps)]  # (an idle period of half a second: the worker is still there)
        _install(ctx, other.avail, other.sched, other.driver_order, other.exec_order)
        assert not ctx.worker_stats()["resident"]
        first = _moved(ctx, before)
        b = _stream(ctx, [apps] * 8)[id(apps)]  # (compared with a launch on the second snapshot)
        st = _moved(ctx, before)
        print("install under a resident worker: first launch", first, "both", st)
        assert a.any() and b.any()
        assert first["built"] > 0 and st["built"] > first["built"] and st["served"] > first["served"], (first, st)
        assert ctx.worker_stats()["launches"] == 2
    finally:
        ctx.close()
