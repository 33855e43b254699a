"""GPU parity behind chunk group zero of the priority orders, on the hollow fronts of tests/deep_orders.py: every entry point that
walks an order, bit for bit against the oracle (integers and float64 bit patterns only: no tolerance anywhere).  The suite's
other problems end their decisions in the first chunks; here nothing is decided before position p = 4 095, 4 096, 4 097 (68 and
132 chunks) or 8 191, 8 192, 8 193 (132 chunks).  What each front is there for:

  cleared          wave_decide's group-0 preload finding nothing (md == 0, pre.m == 0): `from = dc > kWave ? kWave * kWave : n_d`,
                   wave_first_fitting_driver started at (from / kWave) / kWave, chunk_group_mask of groups 1 and 2 in wave_tight_scan,
                   the other scans of gangfit_kernels.hip and the chain kernels.
  stale            the "stale maximum" arm: every front chunk admitted by its maxima, loaded and refused, in every scan.
  drivers-front    a driver from group 0's scalar masks with a ScanPre that holds no executor chunk: the executor scan leaves g == 0.
  executors-front  the driver from the generic search (ds >= p) with executors preloaded in group 0; pre.c == bd where the last
                   front chunk is the driver's; a gang that runs from group 0 across p.
  straddle         the running sum crossing a group boundary between two executors: K-1 at p-1 and K at p, an end on p-1, the
                   whole order and one more (tightly-pack's run, distribute-evenly's second pass, the capacity sums of the
                   minimal-fragmentation histograms and of the shards' partial sums).
  fallback         wave_fallback / wave_next_feasible_driver with driver positions past 4 096: S_d < K for seventy candidates, the
                   next feasible driver in a later chunk, and a gang no driver serves.
  gpu-gangs        the compact gpu table with p0_sub_known == false (driver from the generic search), the gpu nodes all in group 0
                   or all behind p, with sparse_gpu on and off.
  draining         the chains' LDS front, global tail and checkpoints once the front is used up mid-chain: the chain's own maxima
                   index is stale when the first application moves behind p.

Then the single executors (executor_fit_kernel<true>'s per-lane best across groups), findNodes (kFindAhead batches, a ragged 69th
chunk), the resident worker's narrow and wide decisions, and node-range shards whose cuts fall inside the front.
`python -m pytest tests/test_gpu_deep_orders.py -m gpu`."""
import numpy as np
import pytest

import deep_orders as do
import gangfit
import stress_lib
import test_gpu_sharded
import test_gpu_sharded_minfrag
import test_gpu_sharded_zones
from oracle import binding as ob
from test_find_nodes import _check_rebuild

pytestmark = pytest.mark.gpu

IND, FIFO = gangfit.GF_MODE_INDEPENDENT, gangfit.GF_MODE_FIFO_CHAIN
ALGOS = (0, 1, 2, 3, 4, 5)
CONTEXTS = stress_lib.CONTEXTS + (("independent-zones", {"zoned_fused": 0}), ("minfrag-matrix", {"minfrag_matrix": 1}))
# FIFO chains.  The default budget holds the whole table in LDS.  Budgets of 24 000 and 50 000 bytes end the LDS front inside the
# hollow front (a chunk block of the solo kernel is 784 bytes, a slot of the other LDS kernels 12: at most 4 032 slots, fewer
# next to the fixed tables), so every deep decision is taken in the global tail.  "tail-behind-p" sets, per packer and problem,
# the budget that keeps exactly do.tail_target(p) slots in LDS: position p and two more chunks in the LDS front, a global tail
# behind them.  do.chain_lds_slots restates the route's geometry and every case asserts where the boundary falls.
CHAIN_CONTEXTS = (("default", {}), ("generic", {"fifo_generic": 1}), ("lds-24000", {"lds_budget": 24000}),
                  ("lds-50000", {"lds_budget": 50000}), ("tail-behind-p", {}))
SINGLE_BOUNDS = do.BOUNDS + tuple((4370, p) for p in (4095, 4096, 4097))
_REFS, _OTHER = {}, {}


def _cases(front):
    """The front's cases with the oracle's answers (literal, every packer, both modes), computed once per module run."""
    if front not in _REFS:
        cs = do.cases(front)
        refs = do.references(cs, workers=16)
        _REFS[front] = [(name, p, info, refs[name]) for name, p, info in cs]
    return _REFS[front]


def _install(ctx, p):
    avail, sched, zone, D, X = p[:5]
    ctx.set_snapshot(avail, sched)
    ctx.set_zones(zone)
    ctx.set_orders(D, X)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctxs():
    cs = {name: gangfit.Context(0, options=opts) for name, opts in CONTEXTS}
    yield cs
    for c in cs.values():
        c.close()


@pytest.mark.parametrize("front", do.FRONTS)
def test_independent_batches(ctxs, front):
    """gf_fit_batch (results, driver nodes, placements), gf_fit_feasible and gf_avg_packing_efficiency of all six packers in
    the stress harness's contexts plus the four-kernel zone route and the capacity matrix."""
    for name, p, info, refs in _cases(front):
        apps = gangfit.make_apps(*p[5:9])
        for cname, ctx in ctxs.items():
            _install(ctx, p)
            for algo in ALGOS:
                where = f"{name} ctx={cname} algo={algo}"
                ind = refs[algo][0]
                gpu = ctx.fit_batch(IND, algo, apps)
                assert stress_lib.same(gpu, ind, False) is None, where
                assert np.array_equal(gpu.results["exec_len"], ind.results["exec_len"]), where
                assert np.array_equal(ctx.fit_feasible(algo, apps), ind.results["has_capacity"].astype(bool)), where
                if algo != 2:
                    assert np.array_equal(_bits(ctx.avg_packing_efficiency(algo, apps, gpu)), _bits(ind.avg_eff)), where


def _queue(p, how):
    """The problem's queue, without its last application, or followed by its first thirty applications again."""
    cols = p[5:9]
    if how == "short":
        cols = tuple(v[:-1] for v in cols)
    if how == "long":
        cols = tuple(np.concatenate([v, v[:30]]) for v in cols)
    return cols


@pytest.mark.parametrize("cname,options", CHAIN_CONTEXTS, ids=[c for c, _ in CHAIN_CONTEXTS])
@pytest.mark.parametrize("front", do.FRONTS)
def test_fifo_chains(front, cname, options):
    """gf_fit_batch's FIFO chain of all six packers: failed_at, results, placements and gf_residual_get against the oracle's
    full replay, for four queues in a row: the 40 applications; the queue without its last one; the 40 again; the 40 followed by
    30 more.  Every chain ends at application 36, which is not skippable, and each queue shares its first 36 applications
    with the chain before it.

    gf_chain_cache_stats tells the route and the resumes, and both are asserted for every packer in every context, from
    do.chain_lds_slots (route_of's geometry over the library's byte counts).  A chain on the wide or generic kernels —
    fifo_generic, the general layout, or zone and minimal-fragmentation tables that do not fit the budget — is never counted.
    A chain of an LDS kernel is, and it leaves checkpoints 32 applications apart when its whole table sits in LDS or it is
    the solo kernel (tightly-pack, distribute-evenly), else 128 apart: none in these queues (chain_plan).  With checkpoints,
    the second and third queue resume — from the cached chain's tip at application 36 when the whole table is in LDS, else
    from the checkpoint at 32, deciding the deep applications 32 .. 35 again — and the fourth, which ends in another block of
    32 than the tip, always restores the checkpoint at 32."""
    cases = _cases(front)
    for how in ("short", "long"):
        if (front, how) not in _OTHER:
            _OTHER[front, how] = do.references([(name, p[:5] + _queue(p, how), info) for name, p, info, _ in cases], workers=16,
                                               modes=(True,))
    with gangfit.Context(0, options=options) as ctx:
        device_lds = ctx.device_info()["lds_bytes_per_cu"]
        for name, p, info, refs in cases:
            _install(ctx, p)
            n_slots, nz, pp = int(max(info["dpos"].max(), info["xpos"].max())) + 2, do.n_eval_zones(p), info["p"]
            queues = [(gangfit.make_apps(*_queue(p, how)), refs if how is None else _OTHER[front, how][name])
                      for how in (None, "short", None, "long")]
            for algo in ALGOS:
                where = f"{name} ctx={cname} algo={algo}"
                budget = {"lds-24000": 24000, "lds-50000": 50000}.get(cname, device_lds)
                if cname == "tail-behind-p":
                    budget = do.chain_lds_slots(algo, None, n_slots, nz, target=do.tail_target(pp))
                    ctx.set_option("lds_budget", budget)
                lds = cname != "generic" and info["layout"] != "general"
                slots = do.chain_lds_slots(algo, budget, n_slots, nz) if lds else None
                if slots is not None:  # where the LDS front ends
                    if cname == "default":
                        assert slots >= n_slots, where
                    elif cname == "tail-behind-p":
                        assert pp < slots == do.tail_target(pp) < n_slots - 1, where
                    else:
                        assert slots < pp and slots <= 4032, where
                ctx.chain_cache_stats(reset=True)
                for step, (apps, other) in enumerate(queues):
                    ref = other[algo][1]
                    gpu = ctx.fit_batch(FIFO, algo, apps)
                    assert gpu.failed_at == ref.failed_at == do.LAST, (where, step)
                    assert stress_lib.same(gpu, ref, True) is None, (where, step)
                    assert np.array_equal(ctx.residual(), ref.avail_after), (where, step)
                committed, resumed = ctx.chain_cache_stats()[:2]
                print(f"{where}: LDS slots {slots} of {n_slots}, {committed} chains counted, {resumed} resumed")
                every_32 = slots is not None and (algo in (0, 1) or slots >= n_slots)
                assert (committed, resumed) == ((4, 3 if every_32 else 0) if slots is not None else (0, 0)), where


@pytest.mark.parametrize("n,p", SINGLE_BOUNDS)
def test_single_executors(gf_ctx, n, p):
    """gf_executor_fit and gf_executor_fit_zoned: first fit whose first fitting node is p-1, p and p+1; minimal fragmentation
    whose smallest capacity lies behind p, whose equal-capacity twin in an earlier group must win, whose hosting node behind p
    wins against smaller capacities in group 0 — plain, with `reserved`, and with a zone filter that removes all of group 0;
    and a batch of drawn requests over the same table."""
    avail, X, node_zone, shapes, hosts, reserved, what = do.executor_cases(n, p)
    rng = np.random.default_rng(n + p)
    extra = np.stack([rng.integers(0, 5, size=12) * do.CPU, rng.integers(0, 4, size=12) * 8 * do.GIB, rng.integers(0, 3, size=12)], axis=1)
    req = np.concatenate([shapes, extra]).astype(np.int64)
    hosts = np.concatenate([hosts, rng.random((len(extra), n)) < 0.001])
    gf_ctx.set_snapshot(avail)
    gf_ctx.set_zones(np.zeros(n, dtype=np.uint32))
    gf_ctx.set_orders(X, X)
    xpos = np.argsort(X)
    behind_p = dict(node_zone=node_zone, req_zone=np.ones(len(req), dtype=np.uint32))  # filterNodesToZone: zone 1 starts at p
    for mf, r, zoned in [(mf, r, z) for mf in (False, True) for r in (None, reserved) for z in (None, behind_p)]:
        order = X if zoned is None else X[node_zone[X] == 1]
        want = [ob.executor_fit(avail, e, order, reserved=r, minimal_fragmentation=mf, hosts=hosts[i] if mf else None)
                for i, e in enumerate(req)]
        got = gf_ctx.executor_fit(req, reserved=r, minimal_fragmentation=mf, hosts=hosts if mf else None, **(zoned or {}))
        where = f"n={n} p={p} minimal_fragmentation={mf} reserved={r is not None} zoned={zoned is not None}"
        assert got.tolist() == want, where
        key = ("min_frag" if mf else "first_fit") + ("_reserved" if r is not None else "") + ("_zoned" if zoned else "")
        for q, pos in what.get(key, {}).items():  # the answers the table was built for
            assert xpos[got[q]] == pos, (where, q)


@pytest.mark.parametrize("n,p", SINGLE_BOUNDS)
def test_find_nodes(gf_ctx, n, p):
    """gf_find_nodes, chained and not: K reached on p-1, p and p+1 behind a front of nodes that hold nothing — each still
    visited and charged one add —, a request that ends in the last, ragged chunk (at 4 370 nodes the 69th: no multiple of
    kFindAhead) and one that comes up an executor short; reserved_adds, the documented rebuild of `reserved`, the residual."""
    avail, X, exe, k, what = do.find_nodes_cases(n, p)
    gf_ctx.set_snapshot(avail)
    gf_ctx.set_zones(np.zeros(n, dtype=np.uint32))
    gf_ctx.set_orders(X, X)
    for chained in (False, True):
        want = ob.find_nodes(avail, exe, k, X, chained=chained)
        placed, last, off, nodes, adds = gf_ctx.find_nodes(exe, k, chained=chained)
        assert np.array_equal(placed, want.placed) and np.array_equal(adds, want.adds), (n, p, chained)
        for q in range(len(k)):
            o = int(off[q])
            assert np.array_equal(nodes[o:o + int(placed[q])], want.placement(q)), (n, p, chained, q)
            _check_rebuild(int(placed[q]), int(last[q]), int(k[q]), want.placement(q), want.adds[q], X)
        if chained:
            assert np.array_equal(gf_ctx.residual(), want.avail_after), (n, p)
        else:
            assert (adds[:, X[:p - 1]] == 1).all(), (n, p)


@pytest.mark.parametrize("front", ("cleared", "stale", "straddle", "fallback"))
def test_resident_worker(front):
    """gf_worker_fit, the packers the worker serves in every layout (tightly-pack, distribute-evenly, minimal fragmentation,
    az-aware tightly-pack), on tables in whole units — the narrow view's 16-byte slot records and its chunk maxima behind
    group 0 — and on the same problems with a bytes-grained memory column, where the table has no narrow form and every
    decision is the wide one."""
    bytes_grained = []
    for name, p, info, _ in _cases(front):
        if info["p"] in (4096, 8191):
            q, i = do.problem(front, info["n"], info["p"], info["layout"], info["n_zones"], variant=info["variant"], bytes_grained=True)
            assert int(np.gcd.reduce(np.abs(q[0][:, 1]))) == 1 and int(q[0][:, 1].max()) >= 1 << 30
            bytes_grained.append((name + "/bytes", q, i))
    refs = do.references(bytes_grained, workers=16, algos=(0, 1, 2, 3), modes=(False,))
    with gangfit.Context(0) as ctx:
        for name, p, info, ref in [c for c in _cases(front)] + [(nm, q, i, refs[nm]) for nm, q, i in bytes_grained]:
            _install(ctx, p)
            apps = gangfit.make_apps(*p[5:9])
            for algo in (0, 1, 2, 3):
                got = ctx.worker_fit(algo, apps)
                assert stress_lib.same(got, ref[algo][0], False) is None, f"{name} algo={algo}"
                assert stress_lib.same(ctx.fit_batch(IND, algo, apps), ref[algo][0], False) is None, f"{name} algo={algo}"
        ctx.worker_stop()


_SHARD_RUN = {"plain": ((0, 1), lambda w, algo, p, apps: test_gpu_sharded._run(w, algo, p[0], p[3], p[4], apps)),
              "zoned": ((3, 4), lambda w, algo, p, apps: test_gpu_sharded_zones._run(w, algo, *p[:5], apps)),
              "minfrag": ((2, 5), lambda w, algo, p, apps: test_gpu_sharded_minfrag._run(w, algo, *p[:5], apps))}


@pytest.mark.parametrize("family", sorted(_SHARD_RUN))
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("front", ("cleared", "straddle"))
def test_node_range_shards(front, world, family):
    """8 400 slots in two ranges of 4 200 — each with a group boundary of its own — and in three, whose cuts fall inside the
    hollow front: the partial capacity sums, count rows and designated-shard walks of gangfit_shard.inc, all six packers (the
    orders that merge: a general layout is refused)."""
    algos, run = _SHARD_RUN[family]
    ran = 0
    for name, p, info, refs in _cases(front):
        if info["n"] != 8400 or info["layout"] == "general":
            continue
        apps = gangfit.make_apps(*p[5:8])
        for algo in algos:
            for out in run(world, algo, p, apps):
                assert stress_lib.same(out, refs[algo][0], False) is None, f"{name} world={world} algo={algo}"
            ran += 1
    assert ran >= 6
