"""gf_snapshot_build_resident_set: the snapshot of a node set of the resident cluster.  The installed snapshot, the two orders and
every decision equal what a cluster of the members alone gets — oracle/pysnapshot.py on the compacted rows (tests/snapshot_sets.py),
the oracle's packers on that, and the library's own gf_cluster_set + gf_snapshot_build_resident on a second context that holds only
the members — with every node index mapped back to the cluster's.  The shapes are the edges, not the workload."""
import numpy as np
import pytest

import gangfit
import snapshot_sets as ss
from gangfit import _native as N
from oracle import binding as ob
from oracle import pysnapshot as ps

GIB = ss.GIB
U = ps.UNRANKED
INDEPENDENT, FIFO = gangfit.GF_MODE_INDEPENDENT, gangfit.GF_MODE_FIFO_CHAIN
PACKERS = (0, 1, 2, 4, 5)  # tightly-pack, distribute-evenly, minimal-fragmentation, single-az tightly-pack / minimal-fragmentation
PLAIN = (0, 1, 2)          # a FIFO chain of the single-az packers takes at most 63 zones (GF_ERR_UNSUPPORTED beyond, sets or not)


@pytest.fixture(scope="module")
def members_ctx():
    """The comparison context: it is only ever given the rows of the members."""
    ctx = gangfit.Context(0)
    yield ctx
    ctx.close()


def _check_decisions(ctx, r, n, tiny=False, packers=PACKERS, fifo=PACKERS):
    """fit_batch, independent and FIFO (the packers of `fifo`), against the oracle on the compacted snapshot with the indices
    mapped back."""
    apps, oapps = ss.apps_for(len(r.M), tiny)
    zone_c = r.inputs["zone"]
    for algo in packers:
        gpu = ctx.fit_batch(INDEPENDENT, algo, apps)
        ref = ob.fit_independent(algo, r.avail_c, oapps, r.D_c, r.X_c, sched=r.sched_c, zone=zone_c)
        assert np.array_equal(gpu.results, ss.results_to_cluster(ref.results, r.M)), algo
        for a in np.nonzero(ref.results["has_capacity"])[0]:
            assert np.array_equal(gpu.placement(int(a))[2], ss.to_cluster(ref.placement(int(a))[2], r.M)), (algo, a)
        if algo not in fifo:
            continue
        gpu = ctx.fit_batch(FIFO, algo, apps)
        ref = ob.fit_fifo_chain(algo, r.avail_c, oapps, r.D_c, r.X_c, sched=r.sched_c, zone=zone_c)
        assert gpu.failed_at == ref.failed_at and np.array_equal(gpu.results, ss.results_to_cluster(ref.results, r.M)), algo
        for a in np.nonzero(ref.results["has_capacity"])[0]:  # (the executor slice of an application without capacity is unspecified)
            assert np.array_equal(gpu.placement(int(a))[2], ss.to_cluster(ref.placement(int(a))[2], r.M)), (algo, a)
        assert np.array_equal(ctx.residual(), ss.rows_to_cluster(ref.avail_after, r.M, n)), algo  # zeros in the rows of non-members
        if len(r.M) == 0:
            assert not gpu.results["has_capacity"].any()


def _check(ctx, c, members, D, X, tiny=False, route=None, fifo=PACKERS):
    """Everything that is always compared.  Returns the reference."""
    n = len(c["alloc"])
    r = ss.build(c, members)
    m = len(r.M)
    assert np.array_equal(D, r.D) and np.array_equal(X, r.X)
    avail, sched = ctx.snapshot()
    assert avail.shape == (n, 3) and np.array_equal(avail, r.avail)  # the members' rows, zeros elsewhere
    assert np.array_equal(sched, r.sched)
    info, built = ctx.snapshot_set_info(), ctx.build_info()
    if route is not None:
        assert built[0] == route
    assert info[:2] == (1, m)
    if built[0] == 1:
        assert info[2] == m + 1 and info[3] == (m + 1 + 63) // 64  # non-members cost no slot
    else:
        assert built[0] == 2 and info[2] <= m + 1
    _check_decisions(ctx, r, n, tiny, fifo=fifo)
    return r


def _check_against_members_only(ctx, other, c, r, D, X, tiny=False, fifo=PACKERS):
    """The library's own build on a context that holds only the members: orders, rows, route and chains."""
    n, i = len(c["alloc"]), r.inputs
    other.set_cluster(i["alloc"], i["node_flags"], i["name_rank"], overhead=i["overhead"], zone=i["zone"], n_zones=i["n_zones"])
    oD, oX = other.build_snapshot_resident(res_node=i["res_node"], res_req=i["res_req"], driver_label_rank=i["driver_label_rank"],
                                           exec_label_rank=i["exec_label_rank"])
    assert np.array_equal(D, ss.to_cluster(oD, r.M)) and np.array_equal(X, ss.to_cluster(oX, r.M))
    assert other.build_info()[:3] == ctx.build_info()[:3]
    (avail, sched), (oavail, osched) = ctx.snapshot(), other.snapshot()
    assert np.array_equal(avail, ss.rows_to_cluster(oavail, r.M, n)) and np.array_equal(sched, ss.rows_to_cluster(osched, r.M, n))
    assert ctx.snapshot_set_info()[2:] == other.snapshot_set_info()[2:]  # the layout it would get alone
    assert other.snapshot_set_info()[:2] == (0, len(r.M))
    apps, _ = ss.apps_for(len(r.M), tiny)
    for algo in fifo:
        mine, theirs = ctx.fit_batch(FIFO, algo, apps), other.fit_batch(FIFO, algo, apps)
        assert mine.failed_at == theirs.failed_at and np.array_equal(mine.results, ss.results_to_cluster(theirs.results, r.M))
        for a in np.nonzero(theirs.results["has_capacity"])[0]:
            assert np.array_equal(mine.placement(int(a))[2], ss.to_cluster(theirs.placement(int(a))[2], r.M)), (algo, a)


def _pick(rng, n, m, layout):
    """m members of n nodes: one run that ends at the last node, or scattered with the last node among them."""
    if layout == "contiguous":
        return np.arange(n - m, n)
    if m == 0:
        return np.zeros(0, dtype=np.int64)
    return np.sort(np.concatenate([rng.choice(n - 1, size=m - 1, replace=False), [n - 1]]))


# ---- 1. the known answer
@pytest.mark.gpu
def test_known_answer_through_the_abi(gf_ctx, members_ctx):
    c, members, expected = ss.known_answer()
    c = {k: (np.asarray(v) if isinstance(v, list) else v) for k, v in c.items()}
    ss.install(gf_ctx, c, resident=False)
    D, X = gf_ctx.build_snapshot_resident()  # every node: the foreign zone-1 nodes put zone 0 first
    assert D.tolist()[:3] == [0, 2, 1] and gf_ctx.snapshot_set_info() == (0, 6, 7, 1)
    D, X = ss.build_set(gf_ctx, c, members, resident=False)
    assert D.tolist() == expected and X.tolist() == expected
    r = _check(gf_ctx, c, members, D, X, tiny=True, route=1)
    _check_against_members_only(gf_ctx, members_ctx, c, r, D, X, tiny=True)


# ---- 2. slot-chunk edges
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["contiguous", "scattered"])
@pytest.mark.parametrize("n,m", [(n, m) for n in (64, 65, 130) for m in (0, 1, 63, 64, 65, 128) if m <= n])
def test_slot_chunk_edges(gf_ctx, n, m, layout):
    """m + 1 slots fill exactly one chunk or spill into a second; the row's last word is full, one bit or two bits."""
    rng = np.random.default_rng(1000 * n + m)
    c = ss.cluster(100 + n + m, n, min(n, 40), 2, with_overhead=(m % 2 == 1))
    members = _pick(rng, n, m, layout)
    resident = layout == "scattered"  # entries that travel | the resident usage route
    ss.install(gf_ctx, c, resident)
    D, X = ss.build_set(gf_ctx, c, members, resident)
    _check(gf_ctx, c, members, D, X, route=2 if m == 0 else 1)


# ---- 3. the full set, and the NULL row
@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 1000])
def test_full_set_equals_the_parent_call(gf_ctx, n):
    c = ss.cluster(300 + n, n, min(n, 300), 3, labels=(n == 1000))
    labels = dict(driver_label_rank=c["driver_label_rank"], exec_label_rank=c["exec_label_rank"])
    ss.install(gf_ctx, c, resident=False)
    pD, pX = gf_ctx.build_snapshot_resident(res_node=c["res_node"], res_req=c["res_req"], **labels)
    parent = (gf_ctx.snapshot(), gf_ctx.build_info(), gf_ctx.snapshot_set_info())
    apps, _ = ss.apps_for(n)
    runs = [gf_ctx.fit_batch(FIFO, algo, apps) for algo in PACKERS]
    assert parent[2][0] == 0 and parent[2][1] == n
    for members in (np.ones(n, dtype=bool), None):
        D, X = ss.build_set(gf_ctx, c, members, resident=False)
        assert np.array_equal(D, pD) and np.array_equal(X, pX)
        snap, built, info = gf_ctx.snapshot(), gf_ctx.build_info(), gf_ctx.snapshot_set_info()
        assert np.array_equal(snap[0], parent[0][0]) and np.array_equal(snap[1], parent[0][1])
        assert built == parent[1]  # route, label group, merge check and the bytes that came back
        assert info == ((1 if members is not None else 0),) + parent[2][1:]
        for algo, before in zip(PACKERS, runs):
            now = gf_ctx.fit_batch(FIFO, algo, apps)
            assert now.failed_at == before.failed_at and np.array_equal(now.results, before.results)
            for a in np.nonzero(before.results["has_capacity"])[0]:
                assert np.array_equal(now.placement(int(a))[2], before.placement(int(a))[2])
        if members is not None:
            _check(gf_ctx, c, members, D, X)


# ---- 4. zones
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["zone-without-member", "members-in-one-zone", "65-zones", "513-zones"])
def test_zones(gf_ctx, members_ctx, case):
    rng = np.random.default_rng(len(case))
    if case == "65-zones":        # beyond 64 zones the sort does not rank them itself: zone_rank_kernel
        n, nz = 130, 65
    elif case == "513-zones":     # beyond 512 the zone sums are not combined in LDS
        n, nz = 600, 513
    else:
        n, nz = 200, 4
    c = ss.cluster(400 + n, n, 100, nz)
    if nz > 4:
        c["zone"][:nz] = rng.permutation(nz).astype(np.uint32)  # every zone id is in use
    members = rng.random(n) < 0.5
    if case == "zone-without-member":
        members &= c["zone"] != 1
    elif case == "members-in-one-zone":
        members = c["zone"] == 2
    assert 0 < members.sum() < n
    ss.install(gf_ctx, c, resident=True)
    D, X = ss.build_set(gf_ctx, c, members, resident=True)
    # the zones of the evaluation list: those that own a driver candidate and an executor candidate among the members
    ref = ss.build(c, members)
    evaluated = len(set(c["zone"][ref.D].tolist()) & set(c["zone"][ref.X].tolist()))
    assert (evaluated > 63) == (case == "513-zones")
    fifo = PLAIN if evaluated > 63 else PACKERS
    r = _check(gf_ctx, c, members, D, X, route=1, fifo=fifo)
    _check_against_members_only(gf_ctx, members_ctx, c, r, D, X, fifo=fifo)
    if evaluated > 63:  # the single-az chains are refused on the set's layout exactly as on the members' own
        apps, _ = ss.apps_for(len(r.M))
        for ctx in (gf_ctx, members_ctx):
            for algo in (4, 5):
                with pytest.raises(gangfit.GangfitError) as e:
                    ctx.fit_batch(FIFO, algo, apps)
                assert e.value.code == N.GF_ERR_UNSUPPORTED


# ---- 5. adversarial non-members
@pytest.mark.gpu
@pytest.mark.parametrize("resident", [False, True])
def test_adversarial_non_members(gf_ctx, resident):
    n = 200
    rng = np.random.default_rng(55)
    c = ss.cluster(500, n, 150, 3)
    members = rng.random(n) < 0.5
    members[:4] = (True, False, False, False)
    outside = np.nonzero(~members)[0]
    inside = np.nonzero(members)[0]
    third = len(outside) // 3
    # allocatable near 2^61: counted, the sort's memory and cpu fields would not fit one key with the zone field
    c["alloc"][outside[:third], 0] = (1 << 61) - rng.integers(1, 1000, size=third)
    c["alloc"][outside[:third], 1] = (1 << 61) - rng.integers(1, 1000, size=third) * GIB
    # ties with members in memory and cpu: the same rows, the same usage and overhead
    twins = rng.choice(inside, size=third)
    c["alloc"][outside[third:2 * third]] = c["alloc"][twins]
    c["overhead"][outside[third:2 * third]] = c["overhead"][twins]
    c["zone"][outside[third:2 * third]] = c["zone"][twins]
    # overhead above allocatable on a non-member: its schedulable value is negative
    c["overhead"][outside[-1]] = c["alloc"][outside[-1]] + [1000, GIB, 1]
    # entries on non-members, large ones among them
    extra = rng.choice(outside, size=64).astype(np.uint32)
    c["res_node"] = np.concatenate([c["res_node"], extra])
    c["res_req"] = np.concatenate([c["res_req"], np.tile(np.array([[1 << 40, 1 << 50, 3]], dtype=np.int64), (64, 1))])
    ss.install(gf_ctx, c, resident)
    D, X = ss.build_set(gf_ctx, c, members, resident)
    r = _check(gf_ctx, c, members, D, X, route=1)  # (single-az tightly-pack among the packers: the efficiencies are still served)
    assert np.array_equal(gf_ctx.snapshot()[1][r.M], r.sched_c) and r.sched_c.any()  # have_sched stayed set
    # the same cluster over every node: the negative schedulable value switches the efficiencies off there
    gf_ctx.build_snapshot_resident(res_node=None if resident else c["res_node"], res_req=None if resident else c["res_req"],
                                   resident_usage=resident)
    assert not gf_ctx.snapshot()[1].any()


# ---- 6. labels
def _same_relative_order(D, X):
    return np.array_equal(D[np.isin(D, X)], X[np.isin(X, D)])


@pytest.mark.gpu
@pytest.mark.parametrize("label_max", [0, 2, 254])
def test_labels_device_route(gf_ctx, members_ctx, label_max):
    """label_max + 1 is the key of "not ranked": 1, 3 and 255 are the last values before one more bit or one more pass."""
    n = 300
    rng = np.random.default_rng(600 + label_max)
    c = ss.cluster(600 + label_max, n, 120, 3)
    members = rng.random(n) < 0.5
    el = rng.integers(0, label_max + 1, size=n).astype(np.uint32)
    el[rng.random(n) < 0.3] = U
    el[np.nonzero(members)[0][:2]] = (label_max, U)
    el[~members] = 0  # non-members carry label rank 0
    c = dict(c, driver_label_rank=el.copy(), exec_label_rank=el)  # both lists use the same label: they merge
    ss.install(gf_ctx, c, resident=False)
    D, X = ss.build_set(gf_ctx, c, members, resident=False)
    assert gf_ctx.build_info()[:3] == (1, 1, 0)
    r = _check(gf_ctx, c, members, D, X, route=1)
    _check_against_members_only(gf_ctx, members_ctx, c, r, D, X)


@pytest.mark.gpu
def test_labels_conflicting_pair_ends_on_the_host_route(gf_ctx, members_ctx):
    n = 300
    rng = np.random.default_rng(66)
    c = ss.cluster(660, n, 120, 3)
    members = rng.random(n) < 0.5
    for _ in range(64):
        c["driver_label_rank"] = np.where(members, rng.choice([0, 1, U], size=n), 0).astype(np.uint32)
        c["exec_label_rank"] = np.where(members, rng.choice([0, 1, 2, U], size=n), 0).astype(np.uint32)
        r = ss.build(c, members)
        if not _same_relative_order(r.D, r.X):
            break
    assert not _same_relative_order(r.D, r.X)
    ss.install(gf_ctx, c, resident=True)
    D, X = ss.build_set(gf_ctx, c, members, resident=True)
    assert gf_ctx.build_info()[:3] == (2, 1, 1)
    r = _check(gf_ctx, c, members, D, X, route=2)
    _check_against_members_only(gf_ctx, members_ctx, c, r, D, X)


@pytest.mark.gpu
@pytest.mark.parametrize("labels", [False, True])
def test_option_snapshot_finalize_host(gf_ctx, labels):
    n = 300
    rng = np.random.default_rng(67)
    c = ss.cluster(670, n, 120, 3, labels=labels)
    members = rng.random(n) < 0.4
    c["overhead"][np.nonzero(~members)[0][0]] = c["alloc"][np.nonzero(~members)[0][0]] + 1  # sched_ok is decided over members only
    ss.install(gf_ctx, c, resident=False)
    gf_ctx.set_option("snapshot_finalize_host", 1)
    try:
        D, X = ss.build_set(gf_ctx, c, members, resident=False)
        assert gf_ctx.build_info()[:3] == (2, 0, 0)
        r = _check(gf_ctx, c, members, D, X, route=2)
        assert r.sched_c.any() and np.array_equal(gf_ctx.snapshot()[1][r.M], r.sched_c)
    finally:
        gf_ctx.set_option("snapshot_finalize_host", 0)


# ---- 7. switching the Filter's group on one context
@pytest.mark.gpu
def test_switching_groups(gf_ctx, members_ctx):
    n = 400
    rng = np.random.default_rng(7)
    c = ss.cluster(700, n, 200, 3, with_overhead=False)
    group = rng.integers(0, 3, size=n)
    A, B = group == 0, group == 1
    ss.install(gf_ctx, c, resident=True)
    over_nodes = rng.choice(n, size=50, replace=False).astype(np.uint32)
    over_rows = np.stack([rng.integers(1, 8, size=50) * 250, rng.integers(1, 16, size=50) * (GIB // 4), np.zeros(50, dtype=np.int64)], axis=1)
    gf_ctx.overhead_update(over_nodes, over_rows)
    c["overhead"] = np.zeros((n, 3), dtype=np.int64)
    c["overhead"][over_nodes] = over_rows
    apps, _ = ss.apps_for(100)
    gen = gf_ctx.generation()

    def build_and_check(members):
        nonlocal gen
        D, X = ss.build_set(gf_ctx, c, members, resident=True)
        now = gf_ctx.generation()
        assert now[0] > gen[0] and now[1:] == gen[1:]  # the snapshot epoch moves, the cluster and usage words do not
        gen = now
        r = _check(gf_ctx, c, members, D, X, route=1)
        _check_against_members_only(gf_ctx, members_ctx, c, r, D, X)  # a fresh cluster of the members, entries replayed
        gf_ctx.chain_cache_stats(reset=True)
        first, again = gf_ctx.fit_batch(FIFO, 0, apps), gf_ctx.fit_batch(FIFO, 0, apps)
        assert np.array_equal(first.results, again.results)
        assert gf_ctx.chain_cache_stats()[:2] == (2, 1)  # the build dropped the cache: the first chain replays, the second resumes
        assert gf_ctx.generation() == gen

    build_and_check(A)
    build_and_check(B)
    more = rng.integers(0, n, size=40).astype(np.uint32)
    more_req = np.tile(np.array([[2000, 8 * GIB, 0]], dtype=np.int64), (40, 1))
    gf_ctx.usage_apply(more, more_req, +1)
    now = gf_ctx.generation()
    assert now[0] == gen[0] and now[1] == gen[1] and now[2] == gen[2] + 1
    gen = now
    c["res_node"] = np.concatenate([c["res_node"], more])
    c["res_req"] = np.concatenate([c["res_req"], more_req])
    build_and_check(A)


# ---- 8. entries that travel / resident usage on the multi-device route and on a view
@pytest.mark.gpu
def test_multi_device_and_view(gf_ctx):
    n = 300
    rng = np.random.default_rng(8)
    c = ss.cluster(800, n, 100, 3)
    members = rng.random(n) < 0.5
    with gangfit.Context(devices=[0, 0]) as g:  # two shards on a repeated device id: every device builds the set
        for resident in (False, True):
            ss.install(g, c, resident)
            D, X = ss.build_set(g, c, members, resident)
            r = ss.build(c, members)
            assert np.array_equal(D, r.D) and np.array_equal(X, r.X)
            assert g.snapshot_set_info() == (1, len(r.M), len(r.M) + 1, (len(r.M) + 64) // 64)
            apps, oapps = ss.apps_for(len(r.M))
            for algo in (0, 4):
                gpu = g.fit_batch(INDEPENDENT, algo, apps)
                ref = ob.fit_independent(algo, r.avail_c, oapps, r.D_c, r.X_c, sched=r.sched_c, zone=r.inputs["zone"])
                assert np.array_equal(gpu.results, ss.results_to_cluster(ref.results, r.M))
    ss.install(gf_ctx, c, resident=False)
    D, X = ss.build_set(gf_ctx, c, members, resident=False)
    with gf_ctx.view() as v:
        assert v.snapshot_set_info() == gf_ctx.snapshot_set_info() and v.snapshot_set_info()[0] == 1


# ---- 9. one randomised case
@pytest.mark.gpu
def test_randomised_sets(gf_ctx, members_ctx):
    n = 4161
    rng = np.random.default_rng(0x5E75)
    c = ss.cluster(900, n, 1500, 3, labels=True)
    el = c["exec_label_rank"]
    c = dict(c, driver_label_rank=el.copy())  # one label for both lists: the device route
    group = rng.integers(0, 3, size=n)
    sets = [group == 0, group == 1, group == 2, (group == 0) | (rng.random(n) < 0.3)]
    ss.install(gf_ctx, c, resident=True)
    for k, members in enumerate(sets):
        resident = k % 2 == 0
        D, X = ss.build_set(gf_ctx, c, members, resident)
        r = _check(gf_ctx, c, members, D, X, route=1)
        assert len(r.M) > 64
        _check_against_members_only(gf_ctx, members_ctx, c, r, D, X)

