"""GPU parity of the gangfit/sharded.py route at the edges of the quantity contract (include/gangfit.h: available in
(-2^62, 2^62), requests in [0, 2^62), K in [0, GF_MAX_K]): one gf_ctx per rank, HipShardEngine over a ThreadGroup of shards of
cuda:0, on the problems of tests/magnitudes.py, all six packers, bit for bit against the oracle.  The minimal-fragmentation
family (shard_mf_counts_kernel, shard_mf_emit_kernel of csrc/gangfit_shard.inc) decides per range whether it has a histogram
form — mf_narrow_app's verdict, a scaled table, a capacity of 256 or more — and hands a batch entry some range flagged to ONE
designated shard (a mod n_shards), which walks the full order with unclamped 64-bit capacities; the witnesses below count, from
the oracle's answers, that both sides of those branches are reached.  tests/test_gpu_magnitudes.py::test_two_shards_of_one_device
is the same battery through the in-library multi-device context.  `python -m pytest tests/test_gpu_sharded_magnitudes.py -m gpu`;
the witnesses need the oracle only and run with the CPU suite."""
import math
import threading

import numpy as np
import pytest

import gangfit
import magnitudes as mg
import stress_lib
from gangfit import sharded
from test_gpu_magnitudes import _cases, _install  # (the regimes' cases with the oracle's answers: computed once per run)
from test_gpu_sharded_minfrag import _multi_level

ALGOS = (0, 1, 2, 3, 4, 5)
MF, SAZMF = sharded.MINFRAG_ALGOS
UNSUPPORTED = gangfit._native.GF_ERR_UNSUPPORTED
HIST_BINS = 256  # kMfHistBins: a capacity of this or more among a view's executor candidates flags its range
# eight shards for the regimes whose clusters are a few chunks: empty ranges, and the designated shard a % 8 often owns no node
SWEEPS = [(regime, world) for regime in mg.REGIMES for world in (2, 3) + ((8,) if regime in ("narrow-edge", "huge") else ())]


def _general(p):
    """The problem's orders do not merge: no one order has both as subsequences once unknown names and repeated driver candidates
    are dropped (plan_layout, csrc/gangfit_slot_layout.h), i.e. the nodes in both orders come in two different sequences.  What
    magnitudes.orders draws as "general" almost always is; max-k's 48 nodes with a handful of driver candidates are not always."""
    avail, D, X = p[0], p[3], p[4]
    xs = [int(v) for v in X if v < len(avail)]
    ds = list(dict.fromkeys(int(v) for v in D if v < len(avail)))
    return [v for v in ds if v in set(xs)] != [v for v in xs if v in set(ds)]


def _sweep(regime, world):
    """`world` threads, each with its ONE gf_ctx and HipShardEngine for the whole regime: every case installed in turn, every
    packer's batch run through the thread group.  -> per rank {(case, algo): BatchOut, or the code the batch was refused with}."""
    import torch

    torch.cuda.init()  # (one thread initialises the runtime: see tests/test_gpu_sharded.py)
    items = [(name, p, gangfit.make_apps(*p[5:9])) for name, p, _, _ in _cases(regime)]
    group = sharded.ThreadGroup(world)
    # (ranks that disagree about a refusal would part ways: the ones that were served must not wait for the others for ever)
    group._barrier = threading.Barrier(world, timeout=60)
    outs, errs = [{} for _ in range(world)], []

    def work(r):
        try:
            with gangfit.Context(0) as ctx:
                eng, comm = sharded.HipShardEngine(ctx, r, world, "cuda:0"), group.comm(r)
                for name, p, apps in items:
                    _install(ctx, p)
                    for algo in ALGOS:
                        batch = sharded.ShardedMinfragBatch if algo in sharded.MINFRAG_ALGOS else sharded.ShardedBatch
                        try:  # (a refusal comes from the layout query, on every rank alike, before any exchange)
                            b = batch(eng, comm, algo, apps)
                        except gangfit.GangfitError as e:
                            outs[r][name, algo] = e.code
                            continue
                        b.step()
                        outs[r][name, algo] = b.fetch()
        except Exception as e:
            errs.append(e)
            group._barrier.abort()

    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    if errs:
        raise next((e for e in errs if not isinstance(e, threading.BrokenBarrierError)), errs[0])
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("regime,world", SWEEPS)
def test_every_packer_on_every_rank_bit_exact(regime, world):
    """Orders that merge (the merged and identical layouts, and a general draw that happens to): every rank holds the oracle's
    results and placements, all six packers (sharded_fit's steps for tightly-pack, distribute-evenly and the two zone-aware
    tightly-pack packers, sharded_fit_minfrag's for the two minimal-fragmentation packers; the applications' flags travel on
    both sides).  General layouts: the batch is refused with GF_ERR_UNSUPPORTED on every rank; every regime has one."""
    outs = _sweep(regime, world)
    compared = refused = 0
    assert not any(_general(p) for name, p, _, _ in _cases(regime) if "general" not in name.split("/"))
    for name, p, _, refs in _cases(regime):
        for algo in ALGOS:
            for r in range(world):
                got, where = outs[r][name, algo], f"{regime} {name} algo={algo} rank {r} of {world}"
                if _general(p):
                    assert isinstance(got, int) and got == UNSUPPORTED, where
                    refused += 1
                else:
                    assert not isinstance(got, int), f"{where}: refused with {got}"
                    assert stress_lib.same(got, refs[algo][0], False) is None, where
                    compared += 1
    assert compared > 0 and refused > 0


# ---- witnesses, from the oracle's answers
def _capacities(avail, nodes, exe):
    """GetNodeCapacity (capacity.go:36-75) of `nodes` with nothing reserved, exact (Python integers; math.MaxInt = 2^63-1)."""
    out = []
    for n in nodes:
        caps = [(1 << 63) - 1 if e == 0 else (0 if v < 0 else v // e) for v, e in zip((int(x) for x in avail[n]), (int(x) for x in exe))]
        out.append(min(caps))
    return out


def _units(p):
    """The scaled table's units, fill_narrow's (csrc/gangfit_slot_layout.h): per dimension the gcd over the nodes either order
    names; None when a scaled magnitude reaches 2^30 — no scaled table."""
    avail, D, X = p[0], p[3], p[4]
    nodes = np.unique(np.concatenate([D[D < len(avail)], X[X < len(avail)]]))
    units = []
    for j in range(3):
        col = [abs(int(v)) for v in avail[nodes, j]]
        g = math.gcd(*col) or 1
        if max(col) // g >= 1 << 30:
            return None
        units.append(g)
    return units


def _must_walk(p, algo, a, placement):
    """The feasible gang `a` (k > 0) has no histogram form in some range, so the designated shard decided it, for one of the
    reasons shard_mf_counts_kernel knows: "table" — no scaled table —, "request" — a request that is no multiple of the table's
    units or scales to 2^30 or more (mf_narrow_app) —, "capacity" — an executor candidate of its view (every candidate for the
    plain packer, the chosen zone's for single-AZ) holds 256 executors or more with nothing reserved.  None: every range of any
    world keeps the histogram form (these clusters are far below 65 536 slots)."""
    avail, _, zone, _, X = p[:5]
    units = _units(p)
    if units is None:
        return "table"
    for v, u in zip([int(x) for x in p[5][a]] + [int(x) for x in p[6][a]], units * 2):
        if v % u or v // u >= 1 << 30:
            return "request"
    nodes = np.unique(X[X < len(avail)])
    if algo == SAZMF:
        nodes = nodes[zone[nodes] == zone[placement[0]]]
    return "capacity" if max(_capacities(avail, nodes, p[6][a])) >= HIST_BINS else None


def _census(regime):
    """(feasible minimal-fragmentation gangs compared, those of them with executors, those the designated shard must have
    decided, of those the ones with a zero dimension in the executor request, the others whose placement has runs of two
    lengths) over the regime's sharded cases."""
    feasible = with_execs = walked = walked_zero = multi = 0
    for name, p, _, refs in _cases(regime):
        if _general(p):
            continue
        for algo in (MF, SAZMF):
            ref = refs[algo][0]
            for a in np.nonzero(ref.results["has_capacity"])[0]:
                placement = ref.placement(int(a))[2]
                feasible += 1
                with_execs += int(len(placement) > 0)
                if len(placement) and _must_walk(p, algo, int(a), placement):
                    walked += 1
                    walked_zero += int((p[6][a] == 0).any())
                else:
                    multi += _multi_level(placement)
    return feasible, with_execs, walked, walked_zero, multi


@pytest.mark.parametrize("regime", mg.REGIMES)
def test_the_battery_reaches_both_routes(regime):
    """What test_every_packer_on_every_rank_bit_exact compares is not vacuous: every regime has feasible minimal-fragmentation
    gangs; bytes, huge and max-k hold feasible gangs only the designated-shard walk can have decided (bytes: all of them; huge
    and max-k: gangs whose executor request has a zero dimension, capacity math.MaxInt in it); narrow-edge holds gangs the
    histogram form spreads over levels of two capacities."""
    feasible, with_execs, walked, walked_zero, multi = _census(regime)
    print(f"{regime}: {feasible} feasible minimal-fragmentation gangs ({with_execs} with executors), {walked} on the "
          f"designated-shard route ({walked_zero} with a zero request dimension), {multi} over two run lengths")
    assert feasible >= 1
    if regime == "bytes":  # (no case has a scaled table; a gang without executors has nothing to place)
        assert all(_units(p) is None for _, p, _, _ in _cases(regime)) and walked == with_execs >= 1
    if regime in ("huge", "max-k"):
        assert walked_zero >= 1
    if regime == "narrow-edge":
        assert multi >= 1 and walked < feasible
