"""gf_filter_efficiency on the device: the cluster-wide average packing efficiency selectDriverNode reports
(computeAvgPackingEfficiencyForResult, internal/extender/resource.go:372-381), taken against the FIFO chain's residual.

Three parts (the reference sums in map-range order, which is unspecified):
  exact   counts, GPU == 1.0 without gpu nodes, zeros for an infeasible result, and — on dyadic inputs, where every order of
          addition gives the same bits (test_filter_efficiency_cpu.py shows that for the oracle alone) — the oracle's own sum;
  tree    bit identity with the restatement of the device's summation tree (tests/filter_efficiency.py) on arbitrary inputs;
  bound   within 2 (n - 1) 2^-53 sum|e_i| / len of the oracle's sequential sum, per field.
`python -m pytest tests -m gpu`."""
import functools

import numpy as np
import pytest

import filter_efficiency as fe
import gangfit
from gangfit import _native as N
from oracle import binding as ob

pytestmark = pytest.mark.gpu

FIFO = gangfit.GF_MODE_FIFO_CHAIN
SIZES = [1, 63, 64, 65, 130, 4096, 4097]


@functools.lru_cache(maxsize=None)
def _reference(seed, n, dyadic, algo, n_apps=6, n_zones=1, gpus=True, cpu_request=None, mem_unit=1, merged=False):
    """The problem and the oracle's Filter on it: FIFO replay, the last application's placement, the residual before it."""
    p = fe.problem(seed, n, dyadic, n_apps=n_apps, n_zones=n_zones, gpus=gpus, cpu_request=cpu_request, mem_unit=mem_unit,
                   merged=merged)
    ref = ob.fit_fifo_chain(algo, p.avail, ob.make_apps(p.drv, p.exe, p.k, p.flags), p.D, p.X, sched=p.sched, zone=p.zone)
    return p, ref


def _install(ctx, p):
    ctx.set_snapshot(p.avail, p.sched)
    if p.zone is not None:
        ctx.set_zones(p.zone)
    ctx.set_orders(p.D, p.X)


def _chain(ctx, p, ref, algo):
    """The device's chain; its last result and placement, checked against the oracle's."""
    apps = gangfit.make_apps(p.drv, p.exe, p.k, p.flags)
    out = ctx.fit_batch(FIFO, algo, apps)
    assert out.failed_at == ref.failed_at and np.array_equal(out.results, ref.results)
    a = len(apps) - 1
    ok, d, ex = out.placement(a)
    assert np.array_equal(ex, ref.placement(a)[2])
    return apps[a], out.results[a], ok, d, ex


def _check(ctx, p, algo, app, res, d, ex, table, against="residual", members=None, exact=False):
    """One call against `table` (the oracle's residual, or the snapshot): counts, tree, bound — and the oracle's bits if exact."""
    avg, counts = ctx.filter_efficiency(algo, app, res, ex, against=against, members=members)
    eff = fe.node_efficiencies(algo, table, p.sched, app["drv"], app["exe"], d, ex)
    want, want_counts = fe.restate(eff, p.sched, members)
    assert counts == want_counts, (counts, want_counts)
    assert np.array_equal(fe.bits(avg), fe.bits(want)), (avg, want)
    oracle = fe.oracle_sum(algo, table, p.sched, app["drv"], app["exe"], d, ex, members)
    assert np.all(np.abs(avg - oracle) <= fe.reorder_bound(eff, p.sched, members)), (avg, oracle)
    if exact:
        assert np.array_equal(fe.bits(avg), fe.bits(oracle)), (avg, oracle)
    return avg, counts, eff


@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "arbitrary"])
@pytest.mark.parametrize("n", SIZES)
def test_lane_chunk_and_group_edges(gf_ctx, n, dyadic):
    """Every node a key, then member rows with empty words, a single bit, a full word, a ragged last word and no bit at all.
    The clusters hold a key in neither order, a negative efficiency, one above 1 and a node with nothing schedulable; the
    arbitrary ones request 1 500 m cpu (the Value() rounding)."""
    algo = gangfit.GF_ALGO_TIGHTLY_PACK if dyadic else gangfit.GF_ALGO_DISTRIBUTE_EVENLY
    p, ref = _reference(n, n, dyadic, algo, cpu_request=None if dyadic else 1500)
    _install(gf_ctx, p)
    app, res, ok, d, ex = _chain(gf_ctx, p, ref, algo)
    assert ok or n < 4
    if not ok:
        avg, counts = gf_ctx.filter_efficiency(algo, app, res, ex)
        assert avg.tolist() == [0.0, 0.0, 0.0, 0.0] and counts == (0, 0)
        return
    _, counts, eff = _check(gf_ctx, p, algo, app, res, d, ex, ref.avail_after, exact=dyadic)
    assert counts[0] == n
    if n >= 130:
        assert len(p.neither) > 0 and eff.min() < 0.0 and eff.max() > 1.0
    for members in fe.member_rows(n, n):
        _check(gf_ctx, p, algo, app, res, d, ex, ref.avail_after, members=members, exact=dyadic)


@pytest.mark.parametrize("algo", fe.ALL_ALGOS)
def test_every_packer(gf_ctx, algo):
    """Three zones for the zone-aware packers.  The minimal-fragmentation pair leaves the driver only in `reserved`."""
    p, ref = _reference(40 + algo, 200, False, algo, n_zones=3 if algo in fe.ZONE_AWARE else 1, cpu_request=1500)
    _install(gf_ctx, p)
    app, res, ok, d, ex = _chain(gf_ctx, p, ref, algo)
    assert ok and len(ex) == 3
    avg, _, _ = _check(gf_ctx, p, algo, app, res, d, ex, ref.avail_after)
    with_execs = ob.packing_efficiency(ref.avail_after, p.sched, app["drv"], app["exe"], d, ex)[0]
    same = np.array_equal(fe.bits(fe.restate(with_execs, p.sched)[0]), fe.bits(avg))
    assert same == fe.RESERVES_EXECUTORS[algo]


def test_chain_of_forty_residual_resume_and_snapshot(gf_ctx):
    """Forty applications cross the chain cache's checkpoint at 32; the same Filter again resumes at the tip.  (Merged orders and
    memory in 4 KiB units: the LDS chain kernel serves the chain, and with it the chain cache.)"""
    algo = gangfit.GF_ALGO_TIGHTLY_PACK
    p, ref = _reference(7, 300, False, algo, n_apps=40, cpu_request=1500, mem_unit=4096, merged=True)
    _install(gf_ctx, p)
    app, res, ok, d, ex = _chain(gf_ctx, p, ref, algo)
    assert ok and ref.results["has_capacity"][:-1].any()
    assert not np.array_equal(ref.avail_after, p.avail)  # an earlier driver was committed
    first, _, _ = _check(gf_ctx, p, algo, app, res, d, ex, ref.avail_after)
    stats = gf_ctx.chain_cache_stats()
    app2, res2, _, d2, ex2 = _chain(gf_ctx, p, ref, algo)
    assert gf_ctx.chain_cache_stats()[1] == stats[1] + 1 and gf_ctx.chain_cache_stats()[3] >= stats[3] + 32  # resumed past 32
    again, _, _ = _check(gf_ctx, p, algo, app2, res2, d2, ex2, ref.avail_after)
    assert np.array_equal(fe.bits(first), fe.bits(again))
    snap, _, _ = _check(gf_ctx, p, algo, app, res, d, ex, p.avail, against="snapshot")
    assert not np.array_equal(fe.bits(snap), fe.bits(first))
    assert np.array_equal(gf_ctx.residual(), ref.avail_after)  # gf_residual_get's table is as the chain left it


def test_key_in_neither_order_is_counted(gf_ctx):
    algo = gangfit.GF_ALGO_TIGHTLY_PACK
    p, ref = _reference(11, 130, True, algo)
    _install(gf_ctx, p)
    app, res, ok, d, ex = _chain(gf_ctx, p, ref, algo)
    assert ok and len(p.neither) > 0
    members = np.zeros(p.n, dtype=bool)
    members[p.neither] = True  # keys without a slot: the snapshot's own quantities
    _, counts, _ = _check(gf_ctx, p, algo, app, res, d, ex, ref.avail_after, members=members, exact=True)
    assert counts[0] == len(p.neither)
    members[d] = True
    _check(gf_ctx, p, algo, app, res, d, ex, ref.avail_after, members=members, exact=True)


def test_cluster_without_gpus(gf_ctx):
    algo = gangfit.GF_ALGO_DISTRIBUTE_EVENLY
    p, ref = _reference(13, 130, False, algo, gpus=False)
    _install(gf_ctx, p)
    app, res, ok, d, ex = _chain(gf_ctx, p, ref, algo)
    assert ok
    avg, counts, _ = _check(gf_ctx, p, algo, app, res, d, ex, ref.avail_after)
    assert avg[2] == 1.0 and counts == (130, 0)


def test_infeasible_result_gives_zeros(gf_ctx):
    algo = gangfit.GF_ALGO_TIGHTLY_PACK
    p, ref = _reference(17, 65, True, algo)
    _install(gf_ctx, p)
    app, res, ok, d, ex = _chain(gf_ctx, p, ref, algo)
    none = np.zeros(1, dtype=N.RESULT_DTYPE)
    none[0] = (0, gangfit.GF_NO_NODE, 0, 1)
    for against in ("residual", "snapshot"):
        avg, counts = gf_ctx.filter_efficiency(algo, app, none, None, against=against)
        assert avg.tolist() == [0.0, 0.0, 0.0, 0.0] and counts == (0, 0)


def test_a_view_serves_it(gf_ctx):
    algo = gangfit.GF_ALGO_TIGHTLY_PACK
    p, ref = _reference(19, 300, False, algo, n_apps=9)
    _install(gf_ctx, p)
    view = gf_ctx.view()
    try:
        app, res, ok, d, ex = _chain(view, p, ref, algo)
        assert ok
        _check(view, p, algo, app, res, d, ex, ref.avail_after)
        _check(view, p, algo, app, res, d, ex, p.avail, against="snapshot", members=fe.member_rows(300, 1)[-2])
    finally:
        view.close()


def _code(fn, *args, **kw):
    with pytest.raises(gangfit.GangfitError) as e:
        fn(*args, **kw)
    return e.value.code


def test_refusals_change_nothing(gf_ctx):
    algo = gangfit.GF_ALGO_TIGHTLY_PACK
    p, ref = _reference(23, 130, True, algo)
    # no FIFO chain yet on these orders: GF_ERR_STATE against the residual, exactly where gf_residual_get refuses
    _install(gf_ctx, p)
    app = gangfit.make_apps(p.drv[-1:], p.exe[-1:], p.k[-1:])[0]
    some = np.zeros(1, dtype=N.RESULT_DTYPE)
    some[0] = (1, int(p.D[0]), 0, 1)
    assert _code(gf_ctx.residual) == N.GF_ERR_STATE
    assert _code(gf_ctx.filter_efficiency, algo, app, some, None) == N.GF_ERR_STATE
    app, res, ok, d, ex = _chain(gf_ctx, p, ref, algo)
    assert ok
    before = (gf_ctx.generation(), gf_ctx.residual(), gf_ctx.chain_cache_stats())
    lib, h = gf_ctx._lib, gf_ctx._h
    a1 = np.ascontiguousarray(app, dtype=N.APP_DTYPE).reshape(1)
    r1 = np.ascontiguousarray(res, dtype=N.RESULT_DTYPE).reshape(1)
    x1 = np.ascontiguousarray(ex, dtype=np.uint32)
    o1 = np.zeros(4)
    for args in ((None, N.ptr(r1), N.ptr(x1), None, N.ptr(o1), None), (N.ptr(a1), None, N.ptr(x1), None, N.ptr(o1), None),
                 (N.ptr(a1), N.ptr(r1), N.ptr(x1), None, None, None)):
        assert lib.gf_filter_efficiency(h, algo, 1, *args) == N.GF_ERR_INVALID
    assert lib.gf_filter_efficiency(h, algo, 1, N.ptr(a1), N.ptr(r1), None, None, N.ptr(o1), None) == N.GF_ERR_INVALID  # k > 0
    for against in (2, -1):
        assert _code(gf_ctx.filter_efficiency, algo, app, res, ex, against=against) == N.GF_ERR_INVALID
    for k in (-1, N.GF_MAX_K + 1):
        bad = a1.copy()
        bad["k"] = k
        assert _code(gf_ctx.filter_efficiency, algo, bad, res, ex) == N.GF_ERR_INVALID
    words = np.zeros((p.n + 63) // 64, dtype=np.uint64)
    words[-1] = np.uint64(1) << np.uint64(p.n % 64)  # node n_nodes itself
    assert _code(gf_ctx.filter_efficiency, algo, app, res, ex, members=words) == N.GF_ERR_INVALID
    after = (gf_ctx.generation(), gf_ctx.residual(), gf_ctx.chain_cache_stats())
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2] == after[2]
    # ... and a call that is served changes none of it either
    _check(gf_ctx, p, algo, app, res, d, ex, ref.avail_after, exact=True)
    after = (gf_ctx.generation(), gf_ctx.residual(), gf_ctx.chain_cache_stats())
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2] == after[2]
    # no schedulable columns
    with gangfit.Context(0) as bare:
        bare.set_snapshot(p.avail)
        bare.set_orders(p.D, p.X)
        gen = bare.generation()
        assert _code(bare.filter_efficiency, algo, app, res, ex, against="snapshot") == N.GF_ERR_STATE
        assert bare.generation() == gen
