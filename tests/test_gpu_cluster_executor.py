"""gf_cluster_executor_fit: the executor Filter (rescheduleExecutor, internal/extender/resource.go:594-703) answered from the
resident cluster columns.  Every answer must equal the CPU oracle's on the snapshot oracle/pysnapshot.py builds from the rows of S
alone (tests/cluster_executor_cases.py), and the call must leave everything the warm driver Filter lives on as it found it."""
import numpy as np
import pytest

import cluster_executor_cases as xc
import gangfit
import magnitudes as mg
import snapshot_inputs as si
from gangfit import workloads as wl
from oracle import binding as ob
from oracle import pysnapshot as ps
from test_snapshot_build import _cluster

pytestmark = pytest.mark.gpu
FIFO = gangfit.GF_MODE_FIFO_CHAIN
TIGHT = gangfit.GF_ALGO_TIGHTLY_PACK


def _install(ctx, c, res_node=None, res_req=None):
    ctx.set_cluster(c["alloc"], c["flags"], c["name_rank"], overhead=c.get("overhead"), zone=c.get("zone"), n_zones=c["n_zones"])
    if res_node is not None and len(res_node):
        ctx.usage_apply(res_node, res_req, +1)


def _both(ctx, c, res_node, res_req, where, **kw):
    """the device against the helper, both variants; returns the first-fit answers"""
    first = None
    for mf in (False, True):
        want = xc.expected(c, res_node, res_req, kw.get("sets"), kw.get("req_set"), kw["exe"], minimal_fragmentation=mf,
                           hosts=kw.get("hosts") if mf else None, node_zone=kw.get("node_zone"), req_zone=kw.get("req_zone"),
                           exec_label_rank=kw.get("exec_label_rank"))
        got = ctx.cluster_executor_fit(minimal_fragmentation=mf, **kw)
        assert got.tolist() == want, (where, "minimal fragmentation" if mf else "first fit")
        first = got if first is None else first
    return first


@pytest.mark.parametrize("zones", xc.ZONE_CONFIGS)
@pytest.mark.parametrize("n", xc.NODE_COUNTS)
def test_both_variants_equal_the_oracle_on_the_rows_of_s(gf_ctx, n, zones):
    seed = 1000 * n + xc.ZONE_CONFIGS.index(zones)
    rng = np.random.default_rng(seed + 3)
    c = xc.cluster(seed, n, zones)
    exe = xc.requests(seed, n_req=60 if n > 65 else 24)
    R = len(exe)
    _install(gf_ctx, c, c["res_node"], c["res_req"])
    sets = xc.node_sets(seed, n)
    req_set = rng.integers(0, len(sets), size=R).astype(np.uint32)
    hosts = rng.random((R, n)) < (0.3 if n < 100 else 0.03)
    own_ids = (0,) if c["zone"] is None else tuple(int(z) for z in np.unique(c["zone"]))
    # the cluster's own zone ids, one that holds no node, and "anywhere"
    req_zone = rng.choice(np.array(own_ids + (own_ids[-1] + 1, xc.ANY), dtype=np.uint32), size=R).astype(np.uint32)
    other_zone = rng.integers(0, 4, size=n).astype(np.uint32)  # topology.kubernetes.io/zone need not be the sorted label (quirk 7)
    other_req = rng.integers(0, 5, size=R).astype(np.uint32)   # (zone 4 holds no node)
    other_req[rng.random(R) < 0.2] = xc.ANY
    label = rng.integers(0, 3, size=n).astype(np.uint32)
    label[rng.random(n) < 0.3] = ps.UNRANKED
    where = (n, zones)
    got = _both(gf_ctx, c, c["res_node"], c["res_req"], where + ("every node",), exe=exe, hosts=hosts)
    assert (got == xc.NO).any() and (got != xc.NO).any(), where
    _both(gf_ctx, c, c["res_node"], c["res_req"], where + ("sets",), exe=exe, sets=sets, req_set=req_set, hosts=hosts)
    _both(gf_ctx, c, c["res_node"], c["res_req"], where + ("sets + own zones",), exe=exe, sets=sets, req_set=req_set, req_zone=req_zone)
    _both(gf_ctx, c, c["res_node"], c["res_req"], where + ("own zones",), exe=exe, req_zone=req_zone, exec_label_rank=label)
    _both(gf_ctx, c, c["res_node"], c["res_req"], where + ("sets + another label + ranks",), exe=exe, sets=sets, req_set=req_set,
          hosts=hosts, node_zone=other_zone, req_zone=other_req, exec_label_rank=label)
    # an empty row and an empty zone answer "no capacity", whatever the request
    nobody = gf_ctx.cluster_executor_fit(exe, sets=sets, req_set=np.full(R, 2, dtype=np.uint32))
    assert (nobody == xc.NO).all()
    nowhere = gf_ctx.cluster_executor_fit(exe, minimal_fragmentation=True, req_zone=np.full(R, own_ids[-1] + 1, dtype=np.uint32))
    assert (nowhere == xc.NO).all()


def test_equal_values_and_equal_zone_sums_fall_to_name_rank_and_zone_id(gf_ctx):
    """130 identical nodes alternate between two zones of 65: the zone sums are equal (the lower zone id ranks first), memory and
    cpu are equal everywhere (name_rank alone separates)."""
    n = 130
    rng = np.random.default_rng(9)
    c = dict(alloc=np.tile(np.array([[8000, 16 * xc.GIB, 1]], dtype=np.int64), (n, 1)), overhead=None,
             flags=np.full(n, ps.READY, dtype=np.uint32), name_rank=rng.permutation(n).astype(np.uint32),
             zone=((np.arange(n) + 1) % 2).astype(np.uint32), n_zones=2)  # node 0 is in zone 1
    _install(gf_ctx, c)
    exe = np.array([[1000, xc.GIB, 0], [1000, xc.GIB, 1], [9000, 1, 0]], dtype=np.int64)
    got = _both(gf_ctx, c, None, None, "equal", exe=exe)
    in_zone0 = np.nonzero(c["zone"] == 0)[0]
    assert got[0] == in_zone0[np.argmin(c["name_rank"][in_zone0])] and got[2] == xc.NO
    sets = np.zeros((1, n), dtype=bool)
    sets[0, 64:] = True  # 33 nodes of each zone: still equal sums, and nothing of the first step
    _both(gf_ctx, c, None, None, "equal, second half", exe=exe, sets=sets, req_set=[0, 0, 0])


@pytest.mark.parametrize("case", xc.CONSTRUCTED, ids=[f.__name__ for f in xc.CONSTRUCTED])
def test_constructed_cases(gf_ctx, case):
    c, res_node, res_req, kw, right, wrong = case()
    _install(gf_ctx, c, res_node, res_req)
    assert gf_ctx.cluster_executor_fit(**kw).tolist() == [right]


def test_a_battery_at_the_edges_of_the_quantity_contract(gf_ctx):
    """tests/snapshot_inputs.py's byte-granular problem on three sparse zones (ids 3, 10, 17 of 18), drawn candidates, through
    the RESIDENT usage: gf_usage_apply admits what sums below 2^62 over the whole cluster, which the `huge` regime's entries of
    2^61 - 1 per node do not."""
    name, p, _ = [t for t in mg.cases("bytes") if t[0] == "merged/3z"][0]
    b = si.as_build_inputs(p, np.random.default_rng(100), "drawn")
    c = dict(alloc=b["alloc"], overhead=None, flags=b["node_flags"], name_rank=b["name_rank"], zone=b["zone"], n_zones=b["n_zones"])
    n = len(c["alloc"])
    _install(gf_ctx, c, b["res_node"], b["res_req"])
    exe = np.asarray(p[6], dtype=np.int64)
    rng = np.random.default_rng(4)
    hosts = rng.random((len(exe), n)) < 0.05
    got = _both(gf_ctx, c, b["res_node"], b["res_req"], "bytes", exe=exe, hosts=hosts)
    assert (got != xc.NO).any()
    req_zone = rng.choice(np.array([3, 10, 17, 4, xc.ANY], dtype=np.uint32), size=len(exe)).astype(np.uint32)
    _both(gf_ctx, c, b["res_node"], b["res_req"], "bytes, zones", exe=exe, hosts=hosts, sets=xc.node_sets(1, n),
          req_set=rng.integers(0, 6, size=len(exe)).astype(np.uint32), req_zone=req_zone)
    # the largest quantities: one node at 2^62 - 1 allocatable, requests up to 2^62 - 1
    top = xc._plain([[mg.QMAX, mg.QMAX, mg.QMAX], [8000, 8 * xc.GIB, 0], [mg.QMAX, 1, 0]])
    _install(gf_ctx, top)
    exe = np.array([[mg.QMAX, mg.QMAX, mg.QMAX], [1, 1, 1], [0, 0, 0], [mg.QMAX, 1, 0], [1, mg.QMAX, 0], [3, 7, 0]], dtype=np.int64)
    _both(gf_ctx, top, None, None, "top", exe=exe)


def test_the_call_leaves_the_warm_filter_alone_and_follows_the_resident_state():
    n = 2500
    c = _cluster(95, n, 300, 3, with_overhead=True, labels=False)
    xcl = dict(alloc=c["alloc"], overhead=c["overhead"], flags=c["node_flags"], name_rank=c["name_rank"], zone=c["zone"],
               n_zones=c["n_zones"])
    w = wl.config(2, n_nodes=16, n_apps=48)
    flags = np.ones(len(w.k), dtype=np.uint32)
    apps, oapps = gangfit.make_apps(w.drv, w.exe, w.k, flags), ob.make_apps(w.drv, w.exe, w.k, flags)
    rng = np.random.default_rng(5)
    sets = np.stack([rng.random(n) < 0.7, rng.random(n) < 0.1])
    exe = xc.requests(3, n_req=12)
    req_set = rng.integers(0, 2, size=len(exe)).astype(np.uint32)
    req_zone = rng.choice(np.array([0, 1, 2, xc.ANY], dtype=np.uint32), size=len(exe)).astype(np.uint32)
    kw = dict(exe=exe, sets=sets, req_set=req_set, req_zone=req_zone)
    with gangfit.Context(0) as ctx:
        _install(ctx, xcl, c["res_node"], c["res_req"])
        D, X = ctx.build_snapshot_resident(resident_usage=True)
        first = ctx.fit_batch(FIFO, TIGHT, apps)  # the driver Filter
        ref = ob.fit_fifo_chain(TIGHT, ctx.snapshot()[0], oapps, D, X)
        assert first.failed_at == ref.failed_at and np.array_equal(first.results, ref.results)

        def state():
            avail, sched = ctx.snapshot()
            return ctx.generation(), avail.tobytes(), sched.tobytes(), ctx.residual().tobytes(), ctx.chain_cache_stats()

        before = state()
        answers = _both(ctx, xcl, c["res_node"], c["res_req"], "next to the Filter", **kw)  # executor Filters in between
        assert state() == before, "the call moved a generation, the snapshot, the residual table or the chain cache"
        ctx.chain_cache_stats(reset=True)
        again = ctx.fit_batch(FIFO, TIGHT, apps)  # the same driver Filter: a resume, not a replay
        chains, resumed, evaluated, skipped = ctx.chain_cache_stats()
        assert (chains, resumed) == (1, 1) and skipped > 0, (chains, resumed, evaluated, skipped)
        assert again.results.tobytes() == first.results.tobytes() and again.exec_nodes.tobytes() == first.exec_nodes.tobytes()
        assert ctx.residual().tobytes() == before[3]
        # the answer follows gf_usage_apply / gf_overhead_update with no build in between: fill the first answer's node
        q = int(np.nonzero((answers != xc.NO) & (exe.sum(axis=1) > 0))[0][0])
        node = int(answers[q])
        more_node = np.concatenate([c["res_node"], np.array([node], dtype=np.uint32)])
        more_req = np.concatenate([c["res_req"], c["alloc"][node:node + 1]])
        ctx.usage_apply([node], c["alloc"][node:node + 1], +1)
        moved = _both(ctx, xcl, more_node, more_req, "after gf_usage_apply", **kw)
        assert moved[q] != node
        ctx.usage_apply([node], c["alloc"][node:node + 1], -1)
        assert _both(ctx, xcl, c["res_node"], c["res_req"], "after the removal", **kw).tolist() == answers.tolist()
        over = xcl["overhead"].copy()
        over[node] = c["alloc"][node]
        ctx.overhead_update([node], over[node:node + 1])
        moved = _both(ctx, dict(xcl, overhead=over), c["res_node"], c["res_req"], "after gf_overhead_update", **kw)
        assert moved[q] != node
        assert ctx.generation()[0] == before[0][0], "an update installed something"


def test_a_build_with_request_flags_does_not_change_the_candidates(gf_ctx):
    """gf_snapshot_build_resident(node_flags) leaves a request's flags in the build's column: the executor candidates stay
    those of gf_cluster_set."""
    n = 130
    c = xc.cluster(77, n, "three")
    exe = xc.requests(77, n_req=24)
    _install(gf_ctx, c, c["res_node"], c["res_req"])
    request_flags = np.full(n, ps.UNSCHEDULABLE | ps.DRIVER_CANDIDATE, dtype=np.uint32)
    request_flags[: n // 2] = ps.READY | ps.DRIVER_CANDIDATE
    gf_ctx.build_snapshot_resident(node_flags=request_flags, resident_usage=True, want_orders=False)
    _both(gf_ctx, c, c["res_node"], c["res_req"], "after a build with request flags", exe=exe)


def test_a_multi_device_context_answers_from_its_first_device():
    n = 130
    c = xc.cluster(31, n, "three")
    exe = xc.requests(31, n_req=24)
    with gangfit.Context(devices=[0] * 3) as g:
        _install(g, c, c["res_node"], c["res_req"])
        _both(g, c, c["res_node"], c["res_req"], "three shards", exe=exe, sets=xc.node_sets(31, n),
              req_set=np.arange(len(exe), dtype=np.uint32) % 6)
