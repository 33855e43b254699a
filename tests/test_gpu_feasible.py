"""gf_fit_feasible: the feasibility-only independent batch (what UnschedulablePodMarker reads: `!packingResult.HasCapacity`,
internal/extender/unschedulablepods.go:132-166).  Same decision code as gf_fit_batch(GF_MODE_INDEPENDENT); only one byte per
application crosses the host link."""
import functools

import numpy as np
import pytest

import gangfit
from gangfit import workloads as wl
from oracle import binding as ob

pytestmark = pytest.mark.gpu
IND = gangfit.GF_MODE_INDEPENDENT


def _congested(n_nodes, n_apps, seed):
    w = wl.headline(n_nodes, n_apps, seed=seed, congested=True)  # about half of the gangs do not fit
    return w, w.snapshot


@pytest.mark.parametrize("algo", [0, 1, 2])
@pytest.mark.parametrize("n_nodes,n_apps", [(1, 1), (64, 5), (300, 96), (3000, 700)])
def test_feasible_equals_the_oracle_and_the_full_batch(gf_ctx, algo, n_nodes, n_apps):
    w, s = _congested(n_nodes, n_apps, 0xFEA5 + algo + n_nodes)
    gf_ctx.set_snapshot(s.avail, s.sched)
    gf_ctx.set_orders(s.driver_order, s.exec_order)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, w.flags)
    fits = gf_ctx.fit_feasible(algo, apps)
    full = gf_ctx.fit_batch(IND, algo, apps)
    ref = ob.fit_independent(algo, s.avail, ob.make_apps(w.drv, w.exe, w.k, w.flags), s.driver_order, s.exec_order)
    assert np.array_equal(fits, full.results["has_capacity"].astype(bool))
    assert np.array_equal(fits, ref.results["has_capacity"].astype(bool))
    if n_apps >= 96:
        assert fits.any() and not fits.all()


@pytest.mark.parametrize("algo", [3, 4, 5])
def test_feasible_zone_aware_packers(gf_ctx, algo):
    w, s = _congested(900, 150, 0xFEA6 + algo)
    zone = (wl.splitmix64(0xA7, len(s.avail), 9) % np.uint64(3)).astype(np.uint32)
    order = wl.reference_node_order(s.avail, zone)
    gf_ctx.set_snapshot(s.avail, s.sched)
    gf_ctx.set_zones(zone)
    gf_ctx.set_orders(order, order)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, w.flags)
    fits = gf_ctx.fit_feasible(algo, apps)
    full = gf_ctx.fit_batch(IND, algo, apps)
    assert np.array_equal(fits, full.results["has_capacity"].astype(bool))
    assert fits.any()


@pytest.mark.parametrize("algo", [3, 4, 5])
def test_feasible_zone_aware_without_the_averages(gf_ctx, algo):
    """fit_zoned_fused_kernel's feasibility instantiation skips a zone's average efficiency when it is certainly above 0 (no node's
    available quantity above its schedulable one — checked by gf_snapshot_set — and a driver that asks for cpu or memory).  The
    cases around that short cut, each against the full batch (which always computes the averages, single_az.go:75-97):
    drivers with and without cpu / memory requests, gangs of nothing at all on nodes nobody uses (every efficiency is exactly 0:
    chooseBestResult's strict '<' turns the application down although it fits), and a snapshot with one node whose available
    memory exceeds its schedulable memory (the short cut must switch itself off)."""
    w, s = _congested(1200, 200, 0xFEA9 + algo)
    zone = (wl.splitmix64(0xA7, len(s.avail), 9) % np.uint64(3)).astype(np.uint32)
    order = wl.reference_node_order(s.avail, zone)
    drv, exe, k = w.drv.copy(), w.exe.copy(), w.k.copy()
    drv[0::5] = 0                  # drivers that ask for nothing
    drv[1::5, 0] = 0               # ... for memory only
    drv[2::5, 1] = 0               # ... for cpu only
    exe[0::10] = 0
    k[0::10] = 3                   # gangs of nothing at all
    apps = gangfit.make_apps(drv, exe, k, w.flags)
    verdicts = []
    for variant in ("as generated", "empty nodes", "one node above its schedulable memory"):
        avail, sched = s.avail.copy(), s.sched.copy()
        if variant == "empty nodes":
            avail = sched.copy()   # nothing is used anywhere: a gang of nothing has efficiency 0 everywhere
        elif variant == "one node above its schedulable memory":
            avail[order[0], 1] = sched[order[0], 1] + 1
        gf_ctx.set_snapshot(avail, sched)
        gf_ctx.set_zones(zone)
        gf_ctx.set_orders(order, order)
        fits = gf_ctx.fit_feasible(algo, apps)
        full = gf_ctx.fit_batch(IND, algo, apps)
        assert np.array_equal(fits, full.results["has_capacity"].astype(bool)), variant
        verdicts.append(fits)
    # the quirk is there: on empty nodes the gangs of nothing with a driver of nothing are turned down
    nothing = (~drv.any(axis=1)) & (~exe.any(axis=1))
    assert nothing.any() and verdicts[1][~nothing].any()
    if algo != 3:  # (az-aware-tightly-pack falls back to the plain placement when no zone is chosen: az_aware_pack_tightly.go:33-37)
        assert not verdicts[1][nothing].any()


def test_feasible_rejects_what_the_batch_rejects(gf_ctx):
    w, s = _congested(64, 4, 3)
    gf_ctx.set_snapshot(s.avail, s.sched)
    gf_ctx.set_orders(s.driver_order, s.exec_order)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, w.flags)
    apps["k"][2] = -1
    with pytest.raises(gangfit.GangfitError) as e:
        gf_ctx.fit_feasible(0, apps)
    assert e.value.code == gangfit._native.GF_ERR_INVALID
    assert len(gf_ctx.fit_feasible(0, apps[:0])) == 0


def test_feasible_waiting_for_the_stream(gf_ctx):
    """feasible_announce = 0: the call waits for the stream instead of watching the bytes arrive; same answers, also when the
    two kinds of call alternate on one context (the announcing call returns before its kernel has ended)."""
    w, s = _congested(2000, 500, 17)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, w.flags)
    with gangfit.Context(0) as c:
        c.set_snapshot(s.avail, s.sched)
        c.set_orders(s.driver_order, s.exec_order)
        full = c.fit_batch(IND, 0, apps)
        want = full.results["has_capacity"].astype(bool)
        for rnd in range(6):
            c.set_option("feasible_announce", rnd & 1)
            assert np.array_equal(c.fit_feasible(0, apps), want)
            assert np.array_equal(c.fit_feasible(1, apps[: 100 + rnd]), c.fit_batch(IND, 1, apps[: 100 + rnd]).results["has_capacity"].astype(bool))
            again = c.fit_batch(IND, 0, apps)  # right behind an announcing call: placements of the full batch unchanged
            assert np.array_equal(again.results, full.results) and np.array_equal(again.exec_nodes, full.exec_nodes)


def test_feasible_without_mapped_staging(gf_ctx):
    """zero_copy = 0: records and answers travel by copies around the kernel; same answers."""
    w, s = _congested(500, 120, 11)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, w.flags)
    with gangfit.Context(0, options={"zero_copy": 0}) as c:
        c.set_snapshot(s.avail, s.sched)
        c.set_orders(s.driver_order, s.exec_order)
        a = c.fit_feasible(0, apps)
        assert np.array_equal(a, c.fit_batch(IND, 0, apps).results["has_capacity"].astype(bool))


@pytest.mark.parametrize("route", ["zoned_fused=0", "70 zones"])
@pytest.mark.parametrize("algo", [3, 4, 5])
def test_feasible_on_the_four_kernel_zone_route(algo, route):
    """Without the one-launch zone kernel (option zoned_fused = 0, or more than 63 zones) gf_fit_feasible runs the full batch on
    the four-kernel route and hands on its HasCapacity: against the oracle's."""
    from test_gpu_zones import _setup, _zoned_problem_all_evaluated
    oalgo = {3: ob.ALGO_AZ_AWARE_TIGHTLY_PACK, 4: ob.ALGO_SINGLE_AZ_TIGHTLY_PACK, 5: ob.ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION}[algo]
    opts, n_zones = ({"zoned_fused": 0}, 3) if route == "zoned_fused=0" else ({}, 70)
    rng = np.random.default_rng(4600 + algo + n_zones)
    with gangfit.Context(0, options=opts) as ctx:
        for layout in ("merged", "identical"):
            avail, sched, zone, D, X, drv, exe, k = _zoned_problem_all_evaluated(rng, 300, 60, layout == "merged", layout, n_zones)
            _setup(ctx, avail, sched, zone, D, X)
            ref = ob.fit_independent(oalgo, avail, ob.make_apps(drv, exe, k), D, X, sched=sched, zone=zone)
            fits = ctx.fit_feasible(algo, gangfit.make_apps(drv, exe, k))
            assert np.array_equal(fits, np.asarray(ref.results["has_capacity"]).astype(bool))
            assert fits.any()


# ---- the collection's word edges, its words between calls, the staging modes and the counters' slot.  One congested 130-node
# cluster (two full 64-slot chunks and a partial one) and one queue of 257 applications; a test takes a prefix of it — an
# independent decision does not depend on the rest of its batch, so the oracle's answers for the whole queue serve every prefix.
# Seed 0xFEA7, on the oracle: 74 of the 257 fit under each plain packer (72 of the first 255), 74 / 51 / 51 under packers 3 / 4 / 5
# on the three zones; applications 0 .. 4 answer 1 0 1 0 0 and 252 .. 256 answer 0 1 1 1 1, so the first and the last word of the
# collection both carry the two values.
_EDGE_SIZES = (2, 3, 4, 5, 255, 256, 257)  # byte positions within a word; both sides of one 64-lane pass of feasible_collect (256)


@functools.lru_cache(maxsize=None)
def _edge_problem():
    w, s = _congested(130, 257, 0xFEA7)
    zone = (wl.splitmix64(0xA7, len(s.avail), 9) % np.uint64(3)).astype(np.uint32)
    return w, s, zone, wl.reference_node_order(s.avail, zone), gangfit.make_apps(w.drv, w.exe, w.k, w.flags)


@functools.lru_cache(maxsize=None)
def _edge_oracle(algo):
    w, s, _, _, _ = _edge_problem()
    return ob.fit_independent(algo, s.avail, ob.make_apps(w.drv, w.exe, w.k, w.flags), s.driver_order, s.exec_order)


def _edge_install(ctx, algo):
    """The snapshot of _edge_problem as packer `algo` needs it (zones and the zone-ranked order for packers 3, 4, 5)."""
    _, s, zone, order, _ = _edge_problem()
    ctx.set_snapshot(s.avail, s.sched)
    if algo >= 3:
        ctx.set_zones(zone)
        ctx.set_orders(order, order)
    else:
        ctx.set_orders(s.driver_order, s.exec_order)


def _has_capacity(batch):
    return np.asarray(batch.results["has_capacity"]).astype(bool)


@pytest.mark.parametrize("n_apps", _EDGE_SIZES)
@pytest.mark.parametrize("algo", [0, 1, 2])
def test_feasible_word_edges_plain_packers(gf_ctx, algo, n_apps):
    apps = _edge_problem()[4][:n_apps]
    _edge_install(gf_ctx, algo)
    fits = gf_ctx.fit_feasible(algo, apps)
    assert np.array_equal(fits, _has_capacity(gf_ctx.fit_batch(IND, algo, apps)))
    assert np.array_equal(fits, _has_capacity(_edge_oracle(algo))[:n_apps])
    if n_apps >= 255:
        assert fits.any() and not fits.all()


@pytest.mark.parametrize("n_apps", _EDGE_SIZES)
@pytest.mark.parametrize("algo", [3, 4, 5])
def test_feasible_word_edges_zone_aware_packers(gf_ctx, algo, n_apps):
    apps = _edge_problem()[4][:n_apps]
    _edge_install(gf_ctx, algo)
    fits = gf_ctx.fit_feasible(algo, apps)
    assert np.array_equal(fits, _has_capacity(gf_ctx.fit_batch(IND, algo, apps)))
    if n_apps >= 255:
        assert fits.any() and not fits.all()


@pytest.mark.parametrize("algo", [0, 3])
def test_feasible_words_return_to_zero_between_calls(algo):
    """257 applications, then 3, then the full batch of the same 3, then 257 again, on one context: a collection word that a call
    left set, or an output that two routes shared, would show in the next answer."""
    apps = _edge_problem()[4]
    with gangfit.Context(0) as c:
        _edge_install(c, algo)
        first = c.fit_feasible(algo, apps)
        few = c.fit_feasible(algo, apps[:3])
        full = c.fit_batch(IND, algo, apps[:3])
        again = c.fit_feasible(algo, apps)
        assert first.any() and not first.all()
        assert np.array_equal(few, first[:3]) and np.array_equal(few, _has_capacity(full))
        assert np.array_equal(again, first)
        assert np.array_equal(first, _has_capacity(c.fit_batch(IND, algo, apps)))
        if algo < 3:
            ref = _edge_oracle(algo)
            assert np.array_equal(first, _has_capacity(ref))
            assert np.array_equal(full.results, ref.results[:3])
            for a in np.nonzero(_has_capacity(ref)[:3])[0]:
                assert np.array_equal(full.placement(int(a))[2], ref.placement(int(a))[2])
        else:  # the oracle of the zone-aware packer, on the same three applications
            w, s, zone, order, _ = _edge_problem()
            ref = ob.fit_independent(ob.ALGO_AZ_AWARE_TIGHTLY_PACK, s.avail, ob.make_apps(w.drv[:3], w.exe[:3], w.k[:3], w.flags[:3]),
                                     order, order, sched=s.sched, zone=zone)
            assert np.array_equal(full.results, ref.results)
            for a in np.nonzero(_has_capacity(ref))[0]:
                assert np.array_equal(full.placement(int(a))[2], ref.placement(int(a))[2])


@pytest.mark.parametrize("options", [{"feasible_announce": 0}, {"zero_copy": 0}], ids=["feasible_announce=0", "zero_copy=0"])
@pytest.mark.parametrize("algo", [1, 4])
def test_feasible_word_edges_in_both_staging_modes(algo, options):
    apps = _edge_problem()[4]
    with gangfit.Context(0, options=options) as c:
        _edge_install(c, algo)
        fits = c.fit_feasible(algo, apps)
        assert np.array_equal(fits, _has_capacity(c.fit_batch(IND, algo, apps)))
        if algo < 3:
            assert np.array_equal(fits, _has_capacity(_edge_oracle(algo)))
        assert fits.any() and not fits.all()


def test_scan_counters_arrive_and_feasible_leaves_them_alone():
    """The counters of a plain independent batch still arrive, and a feasibility call — whose collection words once travelled in
    the counters' parameter — neither counts nor disturbs them."""
    apps = _edge_problem()[4]
    with gangfit.Context(0) as c:
        _edge_install(c, 0)
        c.scan_stats(enable=True, reset=True)
        c.fit_batch(IND, 0, apps)
        counted = c.scan_stats(enable=True, reset=False)
        assert counted[0] > 0 and counted[1] > 0
        c.fit_feasible(0, apps)
        assert c.scan_stats(enable=True, reset=True) == counted
        c.fit_batch(IND, 0, apps)
        assert c.scan_stats(enable=True, reset=False) == counted
