"""gf_cluster_fit_feasible_sets: the capacity scan for drivers of many instance groups in one call.  Every application's answer
must equal, bit for bit, the CPU oracle on the snapshot of its own node set, and what gf_cluster_fit_feasible answers on the same
context for that set by itself; a refusal leaves the output untouched; and the call leaves everything the warm Filter lives on as
it found it.  Sizes, set families and seeds: cluster_scan_sets_cases."""
import numpy as np
import pytest

import cluster_scan_cases as cs
import cluster_scan_sets_cases as ss
import gangfit
from gangfit import _native as N
from gangfit import workloads as wl
from oracle import binding as ob
from oracle import pysnapshot as ps
from test_snapshot_build import _cluster

pytestmark = pytest.mark.gpu
FIFO = gangfit.GF_MODE_FIFO_CHAIN
TIGHT = gangfit.GF_ALGO_TIGHTLY_PACK
ZONE_AWARE = (cs.AZ_AWARE,) + cs.SINGLE_AZ
PRESET = 0xAB


def _set_cluster(ctx, c):
    ctx.set_cluster(c["alloc"], np.zeros(len(c["alloc"]), dtype=np.uint32), c["name_rank"], overhead=None, zone=c["zone"],
                    n_zones=c["n_zones"])


def _raw(ctx, algo, over_cols, n_sets, words, app_set, apps, out, n_apps=None):
    """the C entry point with the pointers as given (None = NULL): its return code"""
    cols = [None if col is None else np.ascontiguousarray(col, dtype=np.int64) for col in over_cols]
    return ctx._lib.gf_cluster_fit_feasible_sets(ctx._h, algo, *[N.ptr(col) for col in cols], n_sets, N.ptr(words), N.ptr(app_set),
                                                 len(apps) if n_apps is None else n_apps, N.ptr(apps), N.ptr(out))


@pytest.mark.parametrize("n, n_zones, family", ss.CASES())
def test_every_packer_equals_the_oracle_and_the_one_set_scan(gf_ctx, n, n_zones, family):
    case = ss.case(n, n_zones, family)
    c, sets, app_set = case["c"], case["sets"], case["app_set"]
    apps = gangfit.make_apps(case["drv"], case["exe"], case["k"])
    for key, (yes, no) in ss.answers_both_ways(case).items():
        print(n, n_zones, family, key, yes, no)
        assert yes >= 5 and no >= 5, (n, n_zones, family, key, yes, no)  # the oracle alone answers both ways
    _set_cluster(gf_ctx, c)
    empty = ~sets.any(axis=1)[app_set]
    for over, ref in ((None, case["ref"]), (c["overhead"], case["ref_over"])):
        for algo in cs.ALGOS:
            got = gf_ctx.cluster_fit_feasible_sets(algo, apps, sets, app_set, overhead=over).astype(np.uint8)
            assert got.tobytes() == ref[algo].tobytes(), (n, n_zones, family, algo, over is not None)
            assert not got[empty].any()
            for s, row in enumerate(sets):  # the contract: the one-set entry point, set by set
                idx = np.nonzero(app_set == s)[0]
                if len(idx) == 0:
                    continue
                one = gf_ctx.cluster_fit_feasible(algo, apps[idx], overhead=over, node_select=row).astype(np.uint8)
                assert one.tobytes() == got[idx].tobytes(), (n, n_zones, family, algo, over is not None, s)


@pytest.mark.parametrize("n, family", [(130, "scattered"), (130, "many"), (ss.GROUP + 65, "second_group")])
def test_fewer_applications_and_another_order_of_the_sets(gf_ctx, n, family):
    case = ss.case(n, 3, family)
    c, sets, app_set = case["c"], case["sets"], case["app_set"]
    apps = gangfit.make_apps(case["drv"], case["exe"], case["k"])
    _set_cluster(gf_ctx, c)
    # the sets dealt round robin, in blocks (sorted by set), and shuffled: the answers travel with their applications
    orders = (np.arange(len(apps)), np.argsort(app_set, kind="stable"), np.random.default_rng(n).permutation(len(apps)))
    for algo in cs.ALGOS:
        ref = case["ref_over"][algo]
        for order in orders:
            got = gf_ctx.cluster_fit_feasible_sets(algo, apps[order], sets, app_set[order], overhead=c["overhead"]).astype(np.uint8)
            assert got.tobytes() == ref[order].tobytes(), (n, family, algo)
        for n_apps in (len(apps), 7, 1):  # (70 at 130 nodes; the group-edge sizes have 32: cluster_scan_sets_cases.n_apps_of)
            got = gf_ctx.cluster_fit_feasible_sets(algo, apps[:n_apps], sets, app_set[:n_apps], overhead=c["overhead"]).astype(np.uint8)
            assert got.tobytes() == ref[:n_apps].tobytes(), (n, family, algo, n_apps)


def test_refusals_leave_the_answers_as_preset(gf_ctx):
    n, n_zones = 65, 3
    case = ss.case(n, n_zones, "contiguous")
    c = case["c"]
    apps = gangfit.make_apps(case["drv"], case["exe"], case["k"])[:7]
    app_set = np.ascontiguousarray(case["app_set"][:7])
    words = gangfit.pack_node_sets(case["sets"], n)
    n_sets = len(words)
    good = [c["overhead"][:, j] for j in range(3)]
    none = [None, None, None]
    out = np.full(len(apps), PRESET, dtype=np.uint8)

    def refused(code, what, ctx, algo, cols, use_apps, use_sets=n_sets, use_words=words, use_app_set=app_set):
        assert _raw(ctx, algo, cols, use_sets, use_words, use_app_set, use_apps, out) == code, what
        assert (out == PRESET).all(), what

    with gangfit.Context(0) as fresh:  # no gf_cluster_set yet
        refused(N.GF_ERR_STATE, "no cluster", fresh, TIGHT, none, apps)
    _set_cluster(gf_ctx, c)
    gf_ctx.build_snapshot_resident(node_flags=np.full(n, ps.READY | ps.DRIVER_CANDIDATE, dtype=np.uint32), want_orders=False)
    v = gf_ctx.view()
    try:
        refused(N.GF_ERR_STATE, "a view", v, TIGHT, none, apps)
    finally:
        v.close()
    # ---- what the one-set entry point refuses
    for missing in range(3):
        cols = list(good)
        cols[missing] = None
        refused(N.GF_ERR_INVALID, f"overhead column {missing} NULL", gf_ctx, TIGHT, cols, apps)
    for bad in (-1, 1 << 61):
        cols = [col.copy() for col in good]
        cols[1][n - 1] = bad
        refused(N.GF_ERR_INVALID, f"an overhead of {bad}", gf_ctx, TIGHT, cols, apps)
    for bad_k in (-1, N.GF_MAX_K + 1):
        wrong = apps.copy()
        wrong["k"][3] = bad_k
        refused(N.GF_ERR_INVALID, f"k = {bad_k}", gf_ctx, TIGHT, good, wrong)
    no_request = apps.copy()
    no_request["drv"][5] = [0, 0, 1]  # ONE application whose average could be 0 refuses the whole call
    above = [col.copy() for col in good]
    above[0][64] = c["alloc"][64, 0] + 1000
    for algo in ZONE_AWARE:
        refused(N.GF_ERR_UNSUPPORTED, "a driver without cpu and memory", gf_ctx, algo, good, no_request)
        refused(N.GF_ERR_UNSUPPORTED, "an overhead above the allocatable", gf_ctx, algo, above, apps)
    for algo in cs.PLAIN:  # ... which the plain packers do not look at
        ok = np.zeros(len(apps), dtype=np.uint8)
        assert _raw(gf_ctx, algo, good, n_sets, words, app_set, no_request, ok) == N.GF_OK
        assert _raw(gf_ctx, algo, above, n_sets, words, app_set, apps, ok) == N.GF_OK
    # ---- the four of this entry point
    refused(N.GF_ERR_INVALID, "no set", gf_ctx, TIGHT, good, apps, use_sets=0)
    refused(N.GF_ERR_INVALID, "set_words NULL", gf_ctx, TIGHT, good, apps, use_words=None)
    refused(N.GF_ERR_INVALID, "app_set NULL", gf_ctx, TIGHT, good, apps, use_app_set=None)
    beyond = app_set.copy()
    beyond[6] = n_sets
    refused(N.GF_ERR_INVALID, "app_set[6] = n_sets", gf_ctx, TIGHT, good, apps, use_app_set=beyond)
    for row in range(n_sets):  # node 65 of a 65-node cluster: bit 1 of the last word
        stray = words.copy()
        stray[row, -1] |= np.uint64(1) << np.uint64(n % 64)
        refused(N.GF_ERR_INVALID, f"a bit at n_nodes in row {row}", gf_ctx, TIGHT, good, apps, use_words=stray)
    stray = words.copy()
    stray[0, -1] |= np.uint64(1) << np.uint64(63)
    refused(N.GF_ERR_INVALID, "the last bit of the last word", gf_ctx, TIGHT, good, apps, use_words=stray)
    # ---- more than 64 zones
    wide = dict(c, zone=(np.arange(n) % 65).astype(np.uint32), n_zones=65)
    _set_cluster(gf_ctx, wide)
    for algo in ZONE_AWARE:
        refused(N.GF_ERR_UNSUPPORTED, "65 zones", gf_ctx, algo, good, apps)
    # no application: GF_OK, nothing written, even with nothing to point at
    assert _raw(gf_ctx, TIGHT, good, n_sets, words, app_set, apps, out, n_apps=0) == N.GF_OK and (out == PRESET).all()
    assert gf_ctx._lib.gf_cluster_fit_feasible_sets(gf_ctx._h, TIGHT, None, None, None, 0, None, None, 0, None, None) == N.GF_OK
    # ... and the call still answers
    _set_cluster(gf_ctx, c)
    got = gf_ctx.cluster_fit_feasible_sets(TIGHT, apps, case["sets"], app_set, overhead=c["overhead"]).astype(np.uint8)
    assert got.tobytes() == case["ref_over"][TIGHT][:7].tobytes()


def test_the_sets_scan_leaves_the_warm_filter_alone():
    n = 2500
    c = _cluster(95, n, 300, 3, with_overhead=True, labels=False)
    w = wl.config(2, n_nodes=16, n_apps=48)
    flags = np.ones(len(w.k), dtype=np.uint32)
    apps, oapps = gangfit.make_apps(w.drv, w.exe, w.k, flags), ob.make_apps(w.drv, w.exe, w.k, flags)
    rng = np.random.default_rng(5)
    group = rng.integers(0, 4, size=n)
    sets = np.stack([group == 0, group == 1, (group == 2) | (group == 0), np.zeros(n, dtype=bool)])
    app_set = (np.arange(len(apps)) % len(sets)).astype(np.uint32)
    with gangfit.Context(0) as ctx:
        ctx.set_cluster(c["alloc"], c["node_flags"], c["name_rank"], overhead=c["overhead"], zone=c["zone"], n_zones=c["n_zones"])
        ctx.usage_apply(c["res_node"], c["res_req"], +1)
        D, X = ctx.build_snapshot_resident(resident_usage=True)
        first = ctx.fit_batch(FIFO, TIGHT, apps)  # the Filter
        ref = ob.fit_fifo_chain(TIGHT, ctx.snapshot()[0], oapps, D, X)
        assert first.failed_at == ref.failed_at and np.array_equal(first.results, ref.results)

        def state():
            avail, sched = ctx.snapshot()
            return ctx.generation(), avail.tobytes(), sched.tobytes(), ctx.residual().tobytes(), ctx.chain_cache_stats()

        before = state()
        scan_ref = ss.reference(c, sets, app_set, w.drv, w.exe, w.k, overhead=c["overhead"])
        for algo in cs.ALGOS:  # the marker's minute: every packer, every instance group, on other overhead and candidates
            got = ctx.cluster_fit_feasible_sets(algo, apps, sets, app_set, overhead=c["overhead"]).astype(np.uint8)
            assert got.tobytes() == scan_ref[algo].tobytes(), algo
        assert state() == before, "the scan moved a generation, the snapshot, the residual table or the chain cache"
        ctx.chain_cache_stats(reset=True)
        again = ctx.fit_batch(FIFO, TIGHT, apps)  # the same Filter: a resume, not a replay
        chains, resumed, evaluated, skipped = ctx.chain_cache_stats()
        assert (chains, resumed) == (1, 1) and skipped > 0, (chains, resumed, evaluated, skipped)
        assert again.failed_at == first.failed_at and again.results.tobytes() == first.results.tobytes()
        assert again.exec_nodes.tobytes() == first.exec_nodes.tobytes()
        assert ctx.residual().tobytes() == before[3]


def test_a_multi_device_context_answers_like_one_device():
    case = ss.case(130, 3, "overlapping")
    c = case["c"]
    apps = gangfit.make_apps(case["drv"], case["exe"], case["k"])
    with gangfit.Context(devices=[0] * 3) as g:
        _set_cluster(g, c)
        for algo in cs.ALGOS:
            got = g.cluster_fit_feasible_sets(algo, apps, case["sets"], case["app_set"], overhead=c["overhead"]).astype(np.uint8)
            assert got.tobytes() == case["ref_over"][algo].tobytes(), algo
