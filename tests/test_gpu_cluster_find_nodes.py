"""gf_cluster_find_nodes: findNodes of the failover reconciler (internal/extender/failover.go:412-436, the chain's Sub :159)
answered from the resident cluster columns for every instance group in one call.  Results, placements, reserved_adds and
residual_out must equal the CPU oracle's on every row's own order (tests/cluster_find_nodes_cases.py) bit for bit and the
installing route's (gf_snapshot_set + gf_orders_set + gf_find_nodes per row) on a second context, and the call must leave
everything the warm driver Filter lives on as it found it."""
import numpy as np
import pytest

import cluster_find_nodes_cases as fc
import gangfit
from gangfit import workloads as wl
from oracle import binding as ob
from test_snapshot_build import _cluster

pytestmark = pytest.mark.gpu
FIFO = gangfit.GF_MODE_FIFO_CHAIN
IND = gangfit.GF_MODE_INDEPENDENT
TIGHT = gangfit.GF_ALGO_TIGHTLY_PACK


def _install(ctx, c):
    ctx.set_cluster(c["alloc"], c["flags"], c["name_rank"], overhead=c["overhead"])
    if len(c["res_node"]):
        ctx.usage_apply(c["res_node"], c["res_req"], +1)


def _call(ctx, c, chained):
    return ctx.cluster_find_nodes(c["exe"], c["k"], c["create_rank"], sets=c["sets"], req_set=c["req_set"], chained=chained,
                                  want_adds=True, want_residual=True)


def _equal(got, want, c, where):
    placed, last, off, nodes, adds, residual = got
    assert np.array_equal(placed, want["placed"]), where
    assert np.array_equal(last, want["last"]), where
    assert np.array_equal(off, want["off"]), where
    assert np.array_equal(adds, want["adds"]), where
    for q in range(len(placed)):  # (the entries behind placed[q] of a request's slice are not defined)
        o = int(off[q])
        assert np.array_equal(nodes[o:o + int(placed[q])], want["exec_nodes"][o:o + int(placed[q])]), (where, q)
    assert residual.dtype == np.int64 and np.array_equal(residual, want["residual"]), where


def _both_modes(ctx, c, where):
    _install(ctx, c)
    for chained in (True, False):
        _equal(_call(ctx, c, chained), fc.expected(c, chained=chained), c, where + ("chained" if chained else "independent",))


@pytest.mark.parametrize("n", fc.NODE_COUNTS)
@pytest.mark.parametrize("family", fc.FAMILIES)
def test_every_output_equals_the_oracle_on_the_rows_own_orders(gf_ctx, family, n):
    for rank_kind in fc.RANKS:
        _both_modes(gf_ctx, fc.case(family, n, rank_kind), (family, n, rank_kind))


def test_sixty_five_steps_and_one_node(gf_ctx):
    _both_modes(gf_ctx, fc.case_big(), ("eight", fc.BIG))


def test_k_max_with_an_all_zero_request_clamps_at_k(gf_ctx):
    c = fc.case_k_max()
    _both_modes(gf_ctx, c, ("k max",))
    placed, last, off, nodes, _, _ = _call(gf_ctx, c, True)
    assert placed[0] == fc.MAX_K and (nodes[: fc.MAX_K] == last[0]).all()


def test_rows_of_equal_content_are_one_group_when_chained(gf_ctx):
    """Two row numbers with the same nodes are the same instance group: their requests chain with each other."""
    c = fc.case("three", 130, "random")
    sets = np.concatenate([c["sets"], c["sets"][:1]])  # row 5 = row 0 once more
    twin = c["req_set"].copy()
    first = np.nonzero(twin == 0)[0]
    twin[first[::2]] = len(sets) - 1
    c2 = dict(c, sets=sets, req_set=twin)
    _install(gf_ctx, c2)
    _equal(_call(gf_ctx, c2, True), fc.expected(c, chained=True), c2, "twin rows")


@pytest.mark.parametrize("family,n", [("none", 257), ("three", 300), ("eight", 65), ("one", 1)])
def test_the_installing_route_on_a_second_context_answers_the_same(gf_ctx, family, n):
    """gf_snapshot_set(A) + gf_orders_set(O) + gf_find_nodes per row: find_nodes_kernel and cluster_find_nodes_kernel do not
    share their step's code, this holds them to each other."""
    c = fc.case(family, n, "random")
    A = fc.available(c)
    _install(gf_ctx, c)
    with gangfit.Context(0) as other:
        for chained in (True, False):
            placed, last, off, nodes, adds, residual = _call(gf_ctx, c, chained)
            table = A.copy()
            for member, qs in fc.groups(c):
                O = fc.order_of(c, member)
                if len(O) == 0:
                    assert not placed[qs].any() and (last[qs] == fc.NO).all() and not adds[qs].any()
                    continue
                other.set_snapshot(A)
                other.set_orders(O, O)
                p2, l2, o2, n2, a2 = other.find_nodes(c["exe"][qs], c["k"][qs], chained=chained)
                assert np.array_equal(placed[qs], p2) and np.array_equal(last[qs], l2) and np.array_equal(adds[qs], a2), (chained, qs)
                for i, q in enumerate(qs):
                    assert np.array_equal(nodes[int(off[q]):int(off[q]) + int(placed[q])], n2[int(o2[i]):int(o2[i]) + int(p2[i])])
                if chained:
                    table[O] = other.residual()[O]
            assert np.array_equal(residual, table), chained


def test_the_call_leaves_the_warm_filter_and_the_resident_worker_alone():
    n = 2500
    cl = _cluster(95, n, 300, 3, with_overhead=True, labels=False)
    w = wl.config(2, n_nodes=16, n_apps=40)
    flags = np.ones(len(w.k), dtype=np.uint32)
    apps, oapps = gangfit.make_apps(w.drv, w.exe, w.k, flags), ob.make_apps(w.drv, w.exe, w.k, flags)
    rng = np.random.default_rng(5)
    group = rng.integers(0, 3, size=n)
    c = dict(alloc=cl["alloc"], overhead=cl["overhead"], flags=cl["node_flags"], name_rank=cl["name_rank"], res_node=cl["res_node"],
             res_req=cl["res_req"], sets=np.stack([group == g for g in range(3)]), create_rank=rng.permutation(n).astype(np.uint32),
             req_set=rng.integers(0, 3, size=30).astype(np.uint32),
             exe=np.tile(np.array([[1000, fc.GIB, 0], [250, 0, 0], [0, 0, 1]], dtype=np.int64), (10, 1)),
             k=rng.integers(0, 60, size=30).astype(np.int32))
    ctx = gangfit.Context(0, options={"worker_idle_us": 1000000})
    try:
        ctx.set_cluster(cl["alloc"], cl["node_flags"], cl["name_rank"], overhead=cl["overhead"], zone=cl["zone"], n_zones=cl["n_zones"])
        ctx.usage_apply(cl["res_node"], cl["res_req"], +1)
        D, X = ctx.build_snapshot_resident(resident_usage=True)
        first = ctx.fit_batch(FIFO, TIGHT, apps)  # the driver Filter
        ref = ob.fit_fifo_chain(TIGHT, ctx.snapshot()[0], oapps, D, X)
        assert first.failed_at == ref.failed_at and np.array_equal(first.results, ref.results)
        by_worker = ctx.worker_fit(TIGHT, apps)
        assert ctx.worker_stats()["resident"]

        def state():
            avail, sched = ctx.snapshot()
            st = ctx.worker_stats()
            return (ctx.generation(), avail.tobytes(), sched.tobytes(), ctx.residual().tobytes(), ctx.chain_cache_stats(),
                    st["resident"], st["launches"])

        before = state()
        for chained in (True, False):
            _equal(_call(ctx, c, chained), fc.expected(c, chained=chained), c, ("next to the Filter", chained))
        assert state() == before, "the call moved a generation, the snapshot, the residual table, the chain cache or the worker"
        assert before[5], "the worker had left before the call"
        ctx.chain_cache_stats(reset=True)
        again = ctx.fit_batch(FIFO, TIGHT, apps)  # the same driver Filter: a resume, not a replay
        chains, resumed, evaluated, skipped = ctx.chain_cache_stats()
        assert (chains, resumed) == (1, 1) and skipped > 0, (chains, resumed, evaluated, skipped)
        assert again.results.tobytes() == first.results.tobytes() and again.exec_nodes.tobytes() == first.exec_nodes.tobytes()
        assert ctx.residual().tobytes() == before[3]
        st = ctx.worker_stats()
        assert st["resident"] and st["launches"] == before[6]
        assert ctx.worker_fit(TIGHT, apps).results.tobytes() == by_worker.results.tobytes()
        # the answer follows gf_usage_apply with no build in between
        extra_node = np.nonzero(c["sets"][0])[0][:50].astype(np.uint32)
        extra_req = np.tile(np.array([[500, fc.GIB // 2, 0]], dtype=np.int64), (len(extra_node), 1))
        ctx.usage_apply(extra_node, extra_req, +1)
        c2 = dict(c, res_node=np.concatenate([c["res_node"], extra_node]), res_req=np.concatenate([c["res_req"], extra_req]))
        _equal(_call(ctx, c2, True), fc.expected(c2, chained=True), c2, "after gf_usage_apply")
        assert ctx.generation()[0] == before[0][0], "an update installed something"
        ctx.worker_stop()
    finally:
        ctx.close()


def test_a_multi_device_context_answers_from_its_first_device():
    c = fc.case("three", 130, "reversed")
    with gangfit.Context(devices=[0] * 3) as g:
        _install(g, c)
        _equal(_call(g, c, True), fc.expected(c, chained=True), c, "three shards")
