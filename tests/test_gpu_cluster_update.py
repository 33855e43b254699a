"""gf_cluster_update: node rows of the resident cluster changed in place.  The whole specification is an equivalence — after the
call every consumer of the resident columns answers exactly as on a fresh context that was given gf_cluster_set with the new
node side, this context's current overhead columns and gf_usage_apply(+1) of every entry it carries — so context A (set, usage,
overhead rows, then the update) is held to context B (state 1 from scratch) on every consumer, bit for bit; the all-groups
capacity scan is also held to the CPU oracle the way tests/cluster_scan_sets_cases.py holds it.  Sizes: the word and 64-word
group edges of the bit rows."""
import numpy as np
import pytest

import cluster_executor_cases as xc
import cluster_scan_cases as cs
import cluster_scan_sets_cases as ss
import gangfit
from gangfit import _native as N
from gangfit import workloads as wl
from oracle import pysnapshot as ps
from test_snapshot_build import GIB, _cluster

pytestmark = pytest.mark.gpu
IND, FIFO = gangfit.GF_MODE_INDEPENDENT, gangfit.GF_MODE_FIFO_CHAIN
TIGHT = gangfit.GF_ALGO_TIGHTLY_PACK
SIZES = (1, 63, 64, 65, 130, 4095, 4096, 4097, 4161)
ROWS = ("none", "first", "last", "partial_word", "every")
ZONES = 3


@pytest.fixture(scope="module")
def fresh_ctx():
    """context B: rebuilt from scratch in every case"""
    ctx = gangfit.Context(0)
    yield ctx
    ctx.close()


def _state(seed, n):
    """state 0: node side, overhead and reservation entries (some on nodes outside the cluster, some nodes overcommitted)"""
    c = _cluster(seed, n, max(2, min(300, n // 6)), ZONES, with_overhead=True, labels=False)
    return dict(alloc=c["alloc"], flags=c["node_flags"] & np.uint32(ps.READY | ps.UNSCHEDULABLE), name_rank=c["name_rank"], zone=c["zone"],
                overhead=c["overhead"], res_node=c["res_node"], res_req=c["res_req"])


def _rows_of(kind, n, rng):
    if kind == "none":
        return np.zeros(0, dtype=np.uint32)
    if kind == "first":
        return np.array([0], dtype=np.uint32)
    if kind == "last":
        return np.array([n - 1], dtype=np.uint32)
    if kind == "partial_word":  # the last word of the bit row, whatever part of it the cluster fills
        return np.array([64 * ((n - 1) // 64)], dtype=np.uint32)
    return rng.permutation(n).astype(np.uint32)  # every row, in no order


def _mutated(s, rows, rng):
    """state 1: on the named rows the allocatable goes up, down and to zero, readiness and the cordon flip, the zone moves"""
    out = dict(s, alloc=s["alloc"].copy(), flags=s["flags"].copy(), zone=s["zone"].copy())
    for i, r in enumerate(rows):
        kind = i % 4
        if kind == 0:
            out["alloc"][r] = 0
        elif kind == 1:
            out["alloc"][r] = s["alloc"][r] * 2 + [1000, GIB, 1]
        elif kind == 2:
            out["alloc"][r] = s["alloc"][r] // 2
        else:
            out["alloc"][r] = [48000, 192 * GIB, 8]
        out["flags"][r] = [ps.READY, 0, ps.READY | ps.UNSCHEDULABLE, ps.READY][int(rng.integers(0, 4))]
        out["zone"][r] = (int(s["zone"][r]) + int(rng.integers(0, ZONES))) % ZONES
    return out


def _send(ctx, s1, rows, with_zone=True, name_rank=None):
    ctx.cluster_update(rows, s1["alloc"][rows], s1["flags"][rows], zone=s1["zone"][rows] if with_zone else None, name_rank=name_rank)


def _set(ctx, s, overhead):
    ctx.set_cluster(s["alloc"], s["flags"], s["name_rank"], overhead=overhead, zone=s["zone"], n_zones=ZONES)


def _from_scratch(ctx, s, overhead):
    _set(ctx, s, overhead)
    ctx.usage_apply(s["res_node"], s["res_req"], +1)


def _questions(seed, n, s1, rows):
    """What both contexts are asked: a pure function of the size, the seed and state 1."""
    rng = np.random.default_rng(seed + 101)
    w = wl.config(2, n_nodes=16, n_apps=12)
    one = np.ones(len(w.k), dtype=np.uint32)
    member = rng.random(n) < 0.7
    member[rows[::2]] = False  # a member row that excludes some of the updated nodes
    sets = xc.node_sets(seed, n)
    scan_sets = np.stack([np.ones(n, dtype=bool), np.arange(n) % 2 == 0, rng.random(n) < 0.4])
    app_set = (np.arange(ss.n_apps_of(n)) % len(scan_sets)).astype(np.uint32)
    c1 = dict(alloc=s1["alloc"], zone=s1["zone"], n_zones=ZONES, name_rank=s1["name_rank"])
    drv, exe, k = ss.applications(seed, c1, scan_sets, app_set)
    xexe = xc.requests(seed, 24)
    fexe = np.tile(np.array([[1000, GIB, 0], [250, 0, 0], [0, 0, 1], [4000, 16 * GIB, 0]], dtype=np.int64), (3, 1))
    return dict(batch=gangfit.make_apps(w.drv, w.exe, w.k, one), chain=gangfit.make_apps(w.drv[:4], w.exe[:4], w.k[:4], one[:4]),
                member=member, req_flags=(s1["flags"] | np.where(rng.random(n) < 0.6, ps.DRIVER_CANDIDATE, 0)).astype(np.uint32),
                sets=sets, scan_sets=scan_sets, app_set=app_set, c1=c1, scan=(drv, exe, k), scan_apps=gangfit.make_apps(drv, exe, k),
                xexe=xexe, xset=rng.integers(0, len(sets), size=len(xexe)).astype(np.uint32), hosts=rng.random((len(xexe), n)) < 0.2,
                fexe=fexe, fk=rng.integers(0, 20, size=len(fexe)).astype(np.int32), fsets=np.stack([np.arange(n) % 3 == g for g in range(3)]),  # (a chained call: rows equal or disjoint)
                fset=rng.integers(0, 3, size=len(fexe)).astype(np.uint32),
                create_rank=rng.permutation(n).astype(np.uint32))


def _decisions(ctx, q):
    """a small independent batch and a 3 + 1 FIFO chain on the installed snapshot"""
    def placed(out):  # (the placement of an application without capacity is not defined)
        return [out.placement(int(a))[2].tobytes() for a in np.nonzero(out.results["has_capacity"])[0]]

    ind = ctx.fit_batch(IND, TIGHT, q["batch"])
    chain = ctx.fit_batch(FIFO, TIGHT, q["chain"])
    return [ind.results.tobytes(), placed(ind), chain.results.tobytes(), placed(chain), chain.failed_at, ctx.residual().tobytes()]


def _answers(ctx, s, q):
    """{consumer: everything it answers}, comparable with ==; `scan` keeps the arrays for the oracle"""
    out = {}

    def installed(D, X):
        avail, sched = ctx.snapshot()
        return [D.tobytes(), X.tobytes(), avail.tobytes(), sched.tobytes()]

    out["build, resident usage"] = installed(*ctx.build_snapshot_resident(resident_usage=True)) + _decisions(ctx, q)
    out["build, travelling entries"] = installed(*ctx.build_snapshot_resident(s["res_node"], s["res_req"]))
    out["build, request flags"] = installed(*ctx.build_snapshot_resident(resident_usage=True, node_flags=q["req_flags"]))
    out["build, the defaults again"] = installed(*ctx.build_snapshot_resident(resident_usage=True))
    out["set build, resident usage"] = installed(*ctx.build_snapshot_resident_set(q["member"], resident_usage=True)) + _decisions(ctx, q)
    out["set build, travelling entries"] = installed(*ctx.build_snapshot_resident_set(q["member"], s["res_node"], s["res_req"]))
    scan = {algo: ctx.cluster_fit_feasible_sets(algo, q["scan_apps"], q["scan_sets"], q["app_set"]).astype(np.uint8) for algo in cs.ALGOS}
    out["scan"] = [scan[algo].tobytes() for algo in cs.ALGOS]
    out["executor"] = [ctx.cluster_executor_fit(q["xexe"], sets=q["sets"], req_set=q["xset"]).tobytes(),
                       ctx.cluster_executor_fit(q["xexe"], True, sets=q["sets"], req_set=q["xset"], hosts=q["hosts"]).tobytes()]
    for chained in (True, False):
        placed, last, off, nodes, adds, residual = ctx.cluster_find_nodes(q["fexe"], q["fk"], q["create_rank"], sets=q["fsets"], req_set=q["fset"],
                                                                          chained=chained, want_adds=True, want_residual=True)
        defined = [nodes[int(o):int(o) + int(p)].tobytes() for o, p in zip(off, placed)]  # (behind placed[q]: not defined)
        out["find nodes, chained" if chained else "find nodes"] = [placed.tobytes(), last.tobytes(), adds.tobytes(), residual.tobytes(), defined]
    return out, scan


def _same(a, b, where):
    for consumer in b:
        assert a[consumer] == b[consumer], (where, consumer)


def _live_overhead(ctx, s, rng):
    """overhead rows replaced after the set: what the update must keep"""
    n = len(s["alloc"])
    live = s["overhead"].copy()
    nodes = rng.permutation(n)[: max(1, n // 5)]
    live[nodes] = np.stack([rng.integers(0, 8, size=len(nodes)) * 250, rng.integers(0, 16, size=len(nodes)) * (GIB // 4),
                            np.zeros(len(nodes), dtype=np.int64)], axis=1)
    ctx.overhead_update(nodes, live[nodes])
    return live


@pytest.mark.parametrize("rows_kind", ROWS)
@pytest.mark.parametrize("n", SIZES)
def test_an_updated_context_answers_like_a_fresh_one(gf_ctx, fresh_ctx, n, rows_kind):
    seed = 7000 + n
    rng = np.random.default_rng(seed)
    s0 = _state(seed, n)
    rows = _rows_of(rows_kind, n, rng)
    s1 = _mutated(s0, rows, rng)
    ranks = None
    if rows_kind in ("last", "every"):  # the name order travels with these: reversed
        s1["name_rank"] = (n - 1 - s0["name_rank"]).astype(np.uint32)
        ranks = s1["name_rank"]
    _from_scratch(gf_ctx, s0, s0["overhead"])
    live = _live_overhead(gf_ctx, s0, rng)
    gen = gf_ctx.generation()
    _send(gf_ctx, s1, rows, name_rank=ranks)
    after = gf_ctx.generation()
    sent = len(rows) > 0 or ranks is not None
    assert after == (gen[0], gen[1] + (1 if sent else 0), gen[2]), (gen, after)
    _from_scratch(fresh_ctx, s1, live)
    q = _questions(seed, n, s1, rows)
    got, scan = _answers(gf_ctx, s1, q)
    want, _ = _answers(fresh_ctx, s1, q)
    _same(got, want, (n, rows_kind))
    ref = ss.reference(q["c1"], q["scan_sets"], q["app_set"], *q["scan"])
    for algo in cs.ALGOS:
        assert scan[algo].tobytes() == ref[algo].tobytes(), (n, rows_kind, algo)


def test_every_kind_of_change_one_after_the_other(gf_ctx, fresh_ctx):
    """One context walks through the kinds of change; after each it is held to a fresh context on the state reached."""
    n, seed = 130, 4242
    rng = np.random.default_rng(seed)
    s = _state(seed, n)
    _from_scratch(gf_ctx, s, s["overhead"])
    live = _live_overhead(gf_ctx, s, rng)
    carrying = np.unique(s["res_node"][s["res_node"] < n])  # nodes with usage
    assert len(carrying) >= 4
    a, b = int(carrying[0]), int(carrying[1])
    # the zone order at state 0 (zones by free memory, cpu): the move below must change it
    order0 = _zone_order(s, live)
    heavy = np.nonzero(s["zone"] == order0[-1])[0]

    def step(where, rows, with_zone=True, name_rank=None, request_flags_first=False):
        rows = np.asarray(rows, dtype=np.uint32)
        q = _questions(seed, n, s, rows)
        if request_flags_first:  # the device's flag column holds a request's candidate flags when the update arrives
            gf_ctx.build_snapshot_resident(resident_usage=True, node_flags=q["req_flags"], want_orders=False)
        gen = gf_ctx.generation()
        _send(gf_ctx, s, rows, with_zone=with_zone, name_rank=name_rank)
        assert gf_ctx.generation() == (gen[0], gen[1] + 1, gen[2]), where
        _from_scratch(fresh_ctx, s, live)
        got, _ = _answers(gf_ctx, s, q)
        want, _ = _answers(fresh_ctx, s, q)
        _same(got, want, where)

    s = dict(s, alloc=s["alloc"].copy(), flags=s["flags"].copy(), zone=s["zone"].copy())
    s["alloc"][a] = s["alloc"][a] * 3
    step("allocatable up", [a], with_zone=False)
    s["alloc"][a] = s["alloc"][a] // 6
    step("allocatable down", [a], with_zone=False)
    keep = s["alloc"][[a, b]].copy()
    s["alloc"][[a, b]] = 0
    step("allocatable to zero", [a, b], with_zone=False)
    s["alloc"][[a, b]] = keep
    step("... and back", [b, a], with_zone=False)
    s["flags"][a] = 0  # GF_NODE_READY cleared on a node that carries usage
    s["flags"][b] = ps.READY | ps.UNSCHEDULABLE  # ... and the cordon set on another
    step("NotReady and cordoned, on nodes that carry usage", [a, b], with_zone=False)
    s["zone"][heavy] = order0[0]  # the zone with the most free memory empties into the one with the least
    assert _zone_order(s, live) != order0, "the move does not change the zone ranking"
    step("a zone move that changes the zone ranking", heavy)
    s["name_rank"] = (n - 1 - s["name_rank"]).astype(np.uint32)
    s["alloc"][a] += [500, 0, 0]
    step("name_rank reversed, with a row", [a], name_rank=s["name_rank"])
    s["name_rank"] = np.random.default_rng(3).permutation(n).astype(np.uint32)
    step("a ranks-only call", [], name_rank=s["name_rank"])
    s["flags"][a] = ps.READY
    s["flags"][b] = 0
    step("after a build that had uploaded request flags", [a, b], request_flags_first=True)
    # the defaults are the update's, not the request's: a build with node_flags == NULL selects them
    D, X = gf_ctx.build_snapshot_resident(resident_usage=True)
    avail, sched, rD, rX = ps.build(s["alloc"], s["flags"], s["name_rank"], overhead=live, res_node=s["res_node"], res_req=s["res_req"],
                                    zone=s["zone"], n_zones=ZONES)
    assert np.array_equal(D, rD) and np.array_equal(X, rX) and len(rD) == 0  # (no default flag names a driver candidate)
    assert np.array_equal(gf_ctx.snapshot()[0], avail) and a in X and b not in X


def _zone_order(s, overhead):
    free = s["alloc"] - overhead
    used = np.zeros_like(free)
    inside = s["res_node"] < len(free)
    np.add.at(used, s["res_node"][inside], s["res_req"][inside])
    free = free - used
    return sorted(range(ZONES), key=lambda z: (int(free[s["zone"] == z, 1].sum()), int(free[s["zone"] == z, 0].sum()), z))


def test_the_update_leaves_the_warm_filter_and_the_resident_worker_alone():
    n, seed = 2500, 95
    rng = np.random.default_rng(seed)
    s = _state(seed, n)
    w = wl.config(2, n_nodes=16, n_apps=40)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    flags = (s["flags"] | ps.DRIVER_CANDIDATE).astype(np.uint32)
    ctx = gangfit.Context(0, options={"worker_idle_us": 1000000})
    try:
        _from_scratch(ctx, s, s["overhead"])
        ctx.build_snapshot_resident(resident_usage=True, node_flags=flags, want_orders=False)
        first = ctx.fit_batch(FIFO, TIGHT, apps)  # the driver Filter's chain
        assert first.results["has_capacity"].any()
        # (the host's copy of the snapshot is fetched before the worker starts, as the Filter's callers do: fetching it is a
        #  device read of its own and not the update's business)
        before_snapshot = [a.tobytes() for a in ctx.snapshot()]
        before_residual = ctx.residual().tobytes()
        by_worker = ctx.worker_fit(TIGHT, apps)
        assert ctx.worker_stats()["resident"]
        gen, launches = ctx.generation(), ctx.worker_stats()["launches"]
        rows = rng.permutation(n)[:40].astype(np.uint32)
        s1 = _mutated(s, rows, rng)
        _send(ctx, s1, rows)
        assert ctx.generation() == (gen[0], gen[1] + 1, gen[2])
        assert [a.tobytes() for a in ctx.snapshot()] == before_snapshot and ctx.residual().tobytes() == before_residual
        ctx.chain_cache_stats(reset=True)
        again = ctx.fit_batch(FIFO, TIGHT, apps)  # the identical chain: a resume, on the snapshot that is still installed
        chains, resumed, evaluated, skipped = ctx.chain_cache_stats()
        assert (chains, resumed) == (1, 1) and skipped > 0, (chains, resumed, evaluated, skipped)
        assert again.results.tobytes() == first.results.tobytes() and again.exec_nodes.tobytes() == first.exec_nodes.tobytes()
        st = ctx.worker_stats()
        assert st["resident"] and st["launches"] == launches, (st, launches)
        assert ctx.worker_fit(TIGHT, apps).results.tobytes() == by_worker.results.tobytes()
        # the next build sees the new rows
        flags1 = (s1["flags"] | ps.DRIVER_CANDIDATE).astype(np.uint32)
        D, X = ctx.build_snapshot_resident(resident_usage=True, node_flags=flags1)
        avail, sched, rD, rX = ps.build(s1["alloc"], flags1, s1["name_rank"], overhead=s1["overhead"], res_node=s1["res_node"],
                                        res_req=s1["res_req"], zone=s1["zone"], n_zones=ZONES)
        got_avail, got_sched = ctx.snapshot()
        assert np.array_equal(got_avail, avail) and np.array_equal(D, rD) and np.array_equal(X, rX)
        assert (s1["alloc"][rows] == 0).all(axis=1).any() and (sched < 0).any()  # a row went to zero under its overhead:
        assert not got_sched.any()  # ... a negative schedulable value disables the efficiencies (gf_snapshot_get then reports 0)
        assert ctx.generation()[0] > gen[0]
        ctx.worker_stop()
    finally:
        ctx.close()


def _raw(ctx, n_rows, node, cols, flags, zone, ranks):
    """the C entry point with the pointers as given (None = NULL): its return code"""
    u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)  # noqa: E731
    cols = [None if c is None else np.ascontiguousarray(c, dtype=np.int64) for c in cols]
    node, flags, zone, ranks = u32(node), u32(flags), u32(zone), u32(ranks)
    return ctx._lib.gf_cluster_update(ctx._h, n_rows, N.ptr(node), *[N.ptr(c) for c in cols], N.ptr(flags), N.ptr(zone), N.ptr(ranks))


def test_refusals_leave_the_state_alone(gf_ctx):
    n, seed = 200, 93
    s = _state(seed, n)
    _from_scratch(gf_ctx, s, s["overhead"])
    q = _questions(seed, n, s, np.array([3], dtype=np.uint32))
    before, _ = _answers(gf_ctx, s, q)
    gen = gf_ctx.generation()
    one = np.array([1000], dtype=np.int64)
    three = [np.array([1000, 2000, 3000], dtype=np.int64)] * 3
    f1, f3 = np.array([ps.READY]), np.full(3, ps.READY)
    twice = np.arange(n)
    twice[5] = 6
    refused = {
        "a NULL allocatable column": (1, [4], [one, None, one], f1, None, None),
        "a NULL node column": (1, None, [one, one, one], f1, None, None),
        "a NULL flag column": (1, [4], [one, one, one], None, None, None),
        "a node at n_nodes": (3, [3, n, 5], three, f3, None, None),
        "a node beyond n_nodes": (1, [n + 7], [one, one, one], f1, None, None),
        "a node named twice": (3, [3, 9, 3], three, f3, None, None),
        "a negative allocatable": (1, [4], [one, -one, one], f1, None, None),
        "an allocatable of 2^62": (1, [4], [one, one, np.array([1 << 62], dtype=np.int64)], f1, None, None),
        "a zone id at n_zones": (3, [1, 2, 3], three, f3, [0, ZONES, 1], None),
        "ranks with a value twice": (0, None, [None] * 3, None, None, twice),
        "ranks with a value at n_nodes": (1, [4], [one, one, one], f1, [0], np.arange(1, n + 1)),
    }
    for what, (n_rows, node, cols, flags, zone, ranks) in refused.items():
        assert _raw(gf_ctx, n_rows, node, cols, flags, zone, ranks) == N.GF_ERR_INVALID, what
        assert gf_ctx.generation() == gen, what
    # nothing sent: GF_OK, nothing changes, nothing is bumped
    assert _raw(gf_ctx, 0, None, [None] * 3, None, None, None) == N.GF_OK
    assert gf_ctx.generation() == gen
    after, _ = _answers(gf_ctx, s, q)
    _same(after, before, "after the refusals")
    # on a view: GF_ERR_STATE, like every call that changes the resident cluster
    v = gf_ctx.view()
    try:
        with pytest.raises(gangfit.GangfitError) as e:
            v.cluster_update([4], [[1000, 1000, 0]], [ps.READY])
        assert e.value.code == N.GF_ERR_STATE
    finally:
        v.close()
    with gangfit.Context(0) as other:
        # before gf_cluster_set: GF_ERR_STATE
        with pytest.raises(gangfit.GangfitError) as e:
            other.cluster_update([0], [[1, 1, 1]], [ps.READY])
        assert e.value.code == N.GF_ERR_STATE
        # a cluster installed without zones: zone ids of 0 say nothing new, anything else needs gf_cluster_set
        other.set_cluster(s["alloc"], s["flags"], s["name_rank"], overhead=s["overhead"])
        other.usage_apply(s["res_node"], s["res_req"], +1)
        D0, X0 = other.build_snapshot_resident(resident_usage=True)
        snap0 = other.snapshot()[0]
        g0 = other.generation()
        assert _raw(other, 2, [4, 5], [three[0][:2]] * 3, f3[:2], [0, 1], None) == N.GF_ERR_INVALID
        assert other.generation() == g0
        D1, X1 = other.build_snapshot_resident(resident_usage=True)
        assert np.array_equal(D1, D0) and np.array_equal(X1, X0) and np.array_equal(other.snapshot()[0], snap0)
        assert _raw(other, 2, [4, 5], [s["alloc"][[4, 5], j] for j in range(3)], s["flags"][[4, 5]], [0, 0], None) == N.GF_OK
        D1, X1 = other.build_snapshot_resident(resident_usage=True)
        assert np.array_equal(D1, D0) and np.array_equal(X1, X0) and np.array_equal(other.snapshot()[0], snap0)
        # the resident cluster marked unknown (what an update that failed half way leaves): GF_ERR_STATE until gf_cluster_set
        other.set_option("update_fault", 2)
        with pytest.raises(gangfit.GangfitError) as e:
            other.cluster_update([0], [[1, 1, 1]], [ps.READY])
        assert e.value.code == N.GF_ERR_STATE
        _set(other, s, s["overhead"])
        other.cluster_update([0], [[1, 1, 1]], [ps.READY])
    after, _ = _answers(gf_ctx, s, q)
    _same(after, before, "at the end")


def test_a_multi_device_context_gives_every_device_the_rows(fresh_ctx):
    n, seed = 700, 94
    rng = np.random.default_rng(seed)
    s0 = _state(seed, n)
    rows = rng.permutation(n)[:90].astype(np.uint32)
    s1 = _mutated(s0, rows, rng)
    s1["name_rank"] = (n - 1 - s0["name_rank"]).astype(np.uint32)
    w = wl.config(2, n_nodes=16, n_apps=64)
    apps = gangfit.make_apps(w.drv, w.exe, w.k)
    flags1 = (s1["flags"] | ps.DRIVER_CANDIDATE).astype(np.uint32)
    with gangfit.Context(devices=[0] * 3) as g:
        assert g.shard_count() == 3
        _from_scratch(g, s0, s0["overhead"])
        gen = g.generation()
        _send(g, s1, rows, name_rank=s1["name_rank"])
        assert g.generation() == (gen[0], gen[1] + 1, gen[2])
        D, X = g.build_snapshot_resident(resident_usage=True, node_flags=flags1)
        _from_scratch(fresh_ctx, s1, s1["overhead"])
        fD, fX = fresh_ctx.build_snapshot_resident(resident_usage=True, node_flags=flags1)
        assert D.tobytes() == fD.tobytes() and X.tobytes() == fX.tobytes()
        assert [a.tobytes() for a in g.snapshot()] == [a.tobytes() for a in fresh_ctx.snapshot()]
        want = fresh_ctx.fit_batch(IND, TIGHT, apps)
        assert want.results["has_capacity"].any()
        for _ in range(2):  # sharded; the first batch of a snapshot checks itself against one device
            got = g.fit_batch(IND, TIGHT, apps)
            assert got.results.tobytes() == want.results.tobytes()
            for a in np.nonzero(want.results["has_capacity"])[0]:
                assert np.array_equal(got.placement(int(a))[2], want.placement(int(a))[2])
        assert g.shard_count() == 3, "the context stopped sharding: a sharded batch disagreed with one device"
        with pytest.raises(gangfit.GangfitError) as e:  # a refusal reaches no device
            g.cluster_update([1, 1], [[1, 1, 0], [2, 2, 0]], [ps.READY, ps.READY])
        assert e.value.code == N.GF_ERR_INVALID
        D2, X2 = g.build_snapshot_resident(resident_usage=True, node_flags=flags1)
        assert D2.tobytes() == D.tobytes() and X2.tobytes() == X.tobytes()
