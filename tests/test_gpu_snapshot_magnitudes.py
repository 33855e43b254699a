"""The parity battery of tests/test_gpu_magnitudes.py on snapshots installed through gf_snapshot_build, the path production takes:
the problems of tests/magnitudes.py as build inputs (tests/snapshot_inputs.py), so that the slot tables, chunk maxima, units,
largest scaled magnitudes, narrow table and zone masks a decision reads are the ones gangfit_snapshot.hip built on the device
(finalize_slots_kernel, finalize_reduce_kernel, finalize_narrow_zones_kernel) — and, with option "snapshot_finalize_host" = 1,
the ones the host builds from the same device-sorted columns.  Bit for bit against oracle/pysnapshot.build and the oracle's
decisions on that restated snapshot; the snapshot the library reports is compared, never used as a reference.
`python -m pytest tests/test_gpu_snapshot_magnitudes.py -m gpu`."""
import numpy as np
import pytest

import gangfit
import magnitudes as mg
import snapshot_inputs as si
import stress_lib
from oracle import binding as ob
from oracle import pysnapshot as ps
from test_snapshot_build import _cluster

pytestmark = pytest.mark.gpu

IND, FIFO = gangfit.GF_MODE_INDEPENDENT, gangfit.GF_MODE_FIFO_CHAIN
ALGOS = (0, 1, 2, 3, 4, 5)
SCALARS_ONLY = 512  # bytes: nothing of size O(n_nodes) came back from a build finalized on the device
SETTINGS = ((0, "device"), (1, "host"))  # option "snapshot_finalize_host"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _problems(regime):
    """[(name, problem, FIFO route or None)]: the regime's merged-layout cases; narrow-edge also at 64 nodes (on the device
    the sentinel slot then sits alone in a chunk of its own) and at 65 (a ragged last chunk)."""
    out = [(name, p, route) for name, p, route in mg.cases(regime) if "merged" in name]
    if regime == "narrow-edge":
        rng = np.random.default_rng(6465)
        for n in (64, 65):
            for v, route in mg.NARROW_VARIANTS:
                out.append((f"{v}/merged/3z/n{n}", mg.narrow_edge(rng, "merged", 3, v, n=n), route))
    return out


_REFS = {}


def _cases(regime, draw):
    """[(name, problem, route, build inputs, (avail, sched, D, X) of the restatement, {algo: (independent, FIFO)})], computed
    once per module run: the two finalize settings share the oracle's answers."""
    key = (regime, draw)
    if key not in _REFS:
        cf = mg.CLOSED_FORM[regime]
        out = []
        for i, (name, p, route) in enumerate(_problems(regime)):
            c = si.as_build_inputs(p, np.random.default_rng(100 + i), draw)
            avail, sched, D, X = ps.build(**c)
            apps = ob.make_apps(*p[5:9])
            refs = {algo: (ob.fit_independent(algo, avail, apps, D, X, closed_form=cf, sched=sched, zone=c["zone"]),
                           ob.fit_fifo_chain(algo, avail, apps, D, X, closed_form=cf, sched=sched, zone=c["zone"]))
                    for algo in ALGOS}
            out.append((name, p, route, c, (avail, sched, D, X), refs))
        _REFS[key] = out
    return _REFS[key]


def _build(ctx, c, setting, where):
    """One build under the current finalize setting: the route it reports, and snapshot and lists against the restatement."""
    D, X = ctx.build_snapshot(**c)
    info = ctx.build_info()
    if setting == 0:
        assert info[:3] == (1, 0, 0) and info[3] <= SCALARS_ONLY, (where, info)
    else:
        assert info[:3] == (2, 0, 0), (where, info)
    return D, X


def _check_tables(ctx, D, X, ref, where):
    avail, sched, rD, rX = ref
    got_avail, got_sched = ctx.snapshot()
    assert np.array_equal(got_avail, avail), where
    assert np.array_equal(got_sched, sched), where
    assert np.array_equal(D, rD) and np.array_equal(X, rX), where


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("setting,setting_name", SETTINGS)
@pytest.mark.parametrize("draw", si.CANDIDATES)
@pytest.mark.parametrize("regime", mg.REGIMES)
def test_every_packer_on_built_snapshots(gf_ctx, regime, draw, setting, setting_name, algo):
    """Snapshot and lists, then results, placements, failed_at and residuals of each of the six packers in both modes,
    gf_fit_feasible and the averages chooseBestResult compares (one packer per case: max-k's gangs of 2^20 take a second each).
    What only this path reaches: the per-chunk gcds of finalize_slots_kernel (its 32-bit rounds and, past 2^32, the 64-bit
    butterfly) folded by finalize_reduce_kernel into the units; the largest scaled
    magnitudes nmax that bound a batch's unit refinement (narrow_units); narrow_ok from finalize_narrow_zones_kernel at a scaled
    2^30 - 1 | 2^30; zone masks and the evaluation list over sparse zone ids; every node in a slot, candidate or not."""
    feasible = 0
    gf_ctx.set_option("snapshot_finalize_host", setting)
    try:
        for name, p, _, c, ref, refs in _cases(regime, draw):
            where = f"{regime} {name} {draw} finalize={setting_name}"
            D, X = _build(gf_ctx, c, setting, where)
            _check_tables(gf_ctx, D, X, ref, where)
            apps = gangfit.make_apps(*p[5:9])
            ind, fifo = refs[algo]
            gpu = gf_ctx.fit_batch(IND, algo, apps)
            assert stress_lib.same(gpu, ind, False) is None, (where, stress_lib.same(gpu, ind, False))
            assert np.array_equal(gf_ctx.fit_feasible(algo, apps), ind.results["has_capacity"].astype(bool)), where
            if algo != 2:
                assert np.array_equal(_bits(gf_ctx.avg_packing_efficiency(algo, apps, gpu)), _bits(ind.avg_eff)), where
            gpu = gf_ctx.fit_batch(FIFO, algo, apps)
            assert stress_lib.same(gpu, fifo, True) is None, (where, stress_lib.same(gpu, fifo, True))
            assert np.array_equal(gf_ctx.residual(), fifo.avail_after), where
            feasible += int(ind.results["has_capacity"].sum())
    finally:
        gf_ctx.set_option("snapshot_finalize_host", 0)
    assert feasible > 0


@pytest.mark.parametrize("draw,setting,setting_name", [("all", 0, "device"), ("all", 1, "host"), ("drawn", 0, "device")])
def test_narrow_edge_routes_on_built_snapshots(gf_ctx, draw, setting, setting_name):
    """The witness of test_gpu_magnitudes.test_narrow_edge_routes — gf_chain_cache_stats out[0] after one FIFO chain: 1 when
    chain_plan proved every request narrow on an LDS chain route, 0 when the wide kernels ran — on built snapshots.  With every
    node a candidate both finalize settings describe the same slot space, so units, nmax and narrow_ok must put every variant
    on the route magnitudes.NARROW_VARIANTS names: a unit one factor too coarse, or an nmax one too small, moves a refine-* or a
    *-bound twin across.  On the drawn candidates only the device setting is held to it: there every node has a slot, the
    edge nodes 0 .. 4 stay candidates, and the other nodes carry odd multiples of the unit below 2^13, so neither the units
    nor the bound move (the host layout scales by the candidates' values only)."""
    seen = set()
    gf_ctx.set_option("snapshot_finalize_host", setting)
    try:
        for name, p, route, c, ref, refs in _cases("narrow-edge", draw):
            assert route is not None
            where = f"{name} {draw} finalize={setting_name}"
            _build(gf_ctx, c, setting, where)
            apps = gangfit.make_apps(*p[5:9])
            for algo in ALGOS:
                gf_ctx.chain_cache_stats(reset=True)
                gpu = gf_ctx.fit_batch(FIFO, algo, apps)
                assert stress_lib.same(gpu, refs[algo][1], True) is None, (where, algo)
                committed = gf_ctx.chain_cache_stats()[0]
                print("route", where, "algo", algo, "committed", committed, "want", route)
                assert committed == (1 if route == "lds" else 0), f"{where} algo={algo}: {committed} LDS chains for route {route}"
                seen.add(route)
    finally:
        gf_ctx.set_option("snapshot_finalize_host", 0)
    assert seen == {"lds", "wide"}


_WIDE = {}


def _wide_gcd_case():
    """The "two-keys" inputs of test_snapshot_build.test_priority_sort_key_groups (5 000 nodes, odd 61-bit memory: every chunk of
    finalize_slots_kernel takes the 64-bit gcd butterfly, the units are 1 and the table has no narrow form) with 64 applications
    of magnitudes.bytes_regime's request shapes, and the oracle's answers for packers 0 and 4."""
    if not _WIDE:
        n, spread = 5000, "two-keys"
        rng = np.random.default_rng(len(spread))
        c = _cluster(900 + len(spread), n, 0, 3, with_overhead=False, labels=False)
        alloc = c["alloc"].copy()
        alloc[:, 1] = rng.integers(0, 1 << 61, size=n) | 1
        alloc[:, 0] = rng.integers(0, 1 << 20, size=n)
        c["alloc"] = alloc
        c["res_node"], c["res_req"] = np.zeros(0, dtype=np.uint32), np.zeros((0, 3), dtype=np.int64)
        drv, exe, k, flags = mg.bytes_regime(np.random.default_rng(61), "merged", 3, n=8, a=64)[5:9]
        avail, sched, D, X = ps.build(**c)
        oapps = ob.make_apps(drv, exe, k, flags)
        refs = {algo: (ob.fit_independent(algo, avail, oapps, D, X, sched=sched, zone=c["zone"]),
                       ob.fit_fifo_chain(algo, avail, oapps, D, X, sched=sched, zone=c["zone"])) for algo in (0, 4)}
        _WIDE.update(c=c, ref=(avail, sched, D, X), apps=(drv, exe, k, flags), refs=refs)
    return _WIDE


@pytest.mark.parametrize("setting,setting_name", SETTINGS)
def test_wide_gcd_branch_with_decisions(gf_ctx, setting, setting_name):
    w = _wide_gcd_case()
    assert (w["ref"][0][:, 1] >> 32).any() and (w["ref"][0][:, 1] & 1).all()  # 64-bit values, gcd 1: the precondition
    apps = gangfit.make_apps(*w["apps"])
    gf_ctx.set_option("snapshot_finalize_host", setting)
    try:
        where = f"two-keys finalize={setting_name}"
        D, X = _build(gf_ctx, w["c"], setting, where)
        _check_tables(gf_ctx, D, X, w["ref"], where)
        for algo in (0, 4):
            ind, fifo = w["refs"][algo]
            gpu = gf_ctx.fit_batch(IND, algo, apps)
            assert stress_lib.same(gpu, ind, False) is None, (where, algo)
            assert np.array_equal(_bits(gf_ctx.avg_packing_efficiency(algo, apps, gpu)), _bits(ind.avg_eff)), (where, algo)
            gf_ctx.chain_cache_stats(reset=True)
            gpu = gf_ctx.fit_batch(FIFO, algo, apps)
            assert stress_lib.same(gpu, fifo, True) is None, (where, algo)
            assert np.array_equal(gf_ctx.residual(), fifo.avail_after), (where, algo)
            assert gf_ctx.chain_cache_stats()[0] == 0, (where, algo)  # no narrow form: the wide kernels
            assert ind.results["has_capacity"].any(), (where, algo)
    finally:
        gf_ctx.set_option("snapshot_finalize_host", 0)
