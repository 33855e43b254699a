"""GPU parity of the node-range sharded batch for the minimal-fragmentation packers (minimal-fragmentation,
single-az-minimal-fragmentation): the gf_shard_mf_* steps of include/gangfit.h (csrc/gangfit_shard.inc: count rows per range, one
plan from their sum, every range emits its own runs by prefix rank) driven by gangfit/sharded.py — a thread group of shards on
cuda:0 — and inside the library (a multi-device context with a repeated device id).  Against the oracle and one-device
gf_fit_batch; tests/test_sharded_minfrag_cpu.py is the same decomposition as a numpy model.  `python -m pytest tests -m gpu`."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import gangfit
from gangfit import sharded
from gangfit import workloads as wl
from oracle import binding as ob
from test_gpu_group import split  # noqa: F401  (fixture: both GANGFIT_TEST_GROUP_SPLIT modes)
from test_gpu_parity import _assert_same, _random_problem
from test_gpu_zones import _setup, _zoned_problem

pytestmark = pytest.mark.gpu
IND = gangfit.GF_MODE_INDEPENDENT
N = gangfit._native
MF, SAZMF = gangfit.GF_ALGO_MINIMAL_FRAGMENTATION, gangfit.GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION
O_ALGO = {MF: ob.ALGO_MINIMAL_FRAGMENTATION, SAZMF: ob.ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION}


def _run(world, algo, avail, sched, zone, D, X, apps):
    """`world` shards of cuda:0 as a thread group, one gf_ctx each; every rank's answer."""
    import torch

    torch.cuda.init()  # (one thread initialises the runtime: see tests/test_gpu_sharded.py)
    group = sharded.ThreadGroup(world)
    outs, errs = [None] * world, []

    def work(r):
        try:
            with gangfit.Context(0) as ctx:
                _setup(ctx, avail, sched, zone, D, X)
                eng = sharded.HipShardEngine(ctx, r, world, "cuda:0")
                outs[r] = sharded.sharded_fit_minfrag(eng, group.comm(r), algo, apps)
        except Exception as e:
            errs.append(e)
            group._barrier.abort()

    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    if errs:
        raise errs[0]
    return outs


def _ref(algo, avail, sched, zone, D, X, drv, exe, k):
    return ob.fit_independent(O_ALGO[algo], avail, ob.make_apps(drv, exe, k), D, X, sched=sched, zone=zone)


def _check(world, algo, avail, sched, zone, D, X, drv, exe, k, ref=None):
    """Every rank's sharded answer == the oracle's."""
    apps = gangfit.make_apps(drv, exe, k)
    if ref is None:
        ref = _ref(algo, avail, sched, zone, D, X, drv, exe, k)
    for out in _run(world, algo, avail, sched, zone, D, X, apps):
        _assert_same(out, ref, apps)
    return ref


# ---- 1. crafted clusters: 192 executor nodes in identity order, node i = [caps[i], 99, 0]; executor (1, 1, 0).  With a
#      driver-only node 192 (it merges in ahead of the executors: node i sits at slot i + 1) or D = X (node i at slot i).
def _crafted(caps_at, driver_only=True, extra=None):
    avail = np.zeros((193 if driver_only else 192, 3), dtype=np.int64)
    avail[:192, 1] = 99
    for s, c in caps_at.items():
        avail[s, 0] = c
    for s, row in (extra or {}).items():
        avail[s] = row
    X = np.arange(192, dtype=np.uint32)
    if driver_only:
        avail[192] = [1, 1, 0]
        return avail, np.array([192], dtype=np.uint32), X
    return avail, X.copy(), X


def _crafted_batch(world, avail, D, X, ks, drv=(1, 1, 0), exe=(1, 1, 0)):
    a = len(ks)
    drv, exe = np.tile(np.array(drv, dtype=np.int64), (a, 1)), np.tile(np.array(exe, dtype=np.int64), (a, 1))
    ref = _check(world, MF, avail, None, None, D, X, drv, exe, np.array(ks, dtype=np.int32))
    return [(bool(ref.results["has_capacity"][i]), int(ref.results["driver_node"][i]), ref.placement(i)[2].tolist()) for i in range(a)]


@pytest.mark.parametrize("world", [2, 3])
def test_doc_comment_example_across_shards(world):
    avail, D, X = _crafted({0: 1, 64: 1, 65: 3, 63: 5, 128: 5, 191: 17})
    got = _crafted_batch(world, avail, D, X, [6, 11, 15, 17, 19, 32, 33])
    want = [[63] * 5 + [0], [63] * 5 + [128] * 5 + [0], [63] * 5 + [128] * 5 + [65] * 3 + [0, 64], [191] * 17, [191] * 17 + [65, 65]]
    for (ok, d, ex), execs in zip(got, want):
        assert ok and d == 192 and ex == execs
    assert got[5][0] and sorted(set(got[5][2])) == [0, 63, 64, 65, 128, 191]  # 32: all six nodes
    assert not got[6][0]                                                      # 33: one more than the cluster holds


@pytest.mark.parametrize("world", [2, 3])
def test_one_level_in_three_shards(world):
    avail, D, X = _crafted({10: 5, 70: 5, 130: 5})
    got = _crafted_batch(world, avail, D, X, [7, 12, 15, 16])
    assert got[0][2] == [10] * 5 + [70, 70]  # the first undrained node of the last level lives in the next shard
    assert got[1][2] == [10] * 5 + [70] * 5 + [130, 130]
    assert got[2][2] == [10] * 5 + [70] * 5 + [130] * 5
    assert not got[3][0]


@pytest.mark.parametrize("world", [2, 3])
def test_driver_correction(world):
    avail, D, X = _crafted({}, driver_only=False, extra={0: [6, 99, 0], 100: [5, 99, 0]})
    (ok, d, ex), = _crafted_batch(world, avail, D, X, [5], drv=(1, 1, 0))
    assert ok and d == 0 and ex == [0] * 5    # 6 -> 5 with the driver on it: the first of the two fives
    (ok, d, ex), = _crafted_batch(world, avail, D, X, [5], drv=(0, 1, 0))
    assert ok and d == 0 and ex == [100] * 5  # stays 6: node 100 is the smallest sufficient
    # the driver lands in an EARLIER shard's range and drops its node a level: the later shards patch their prefix
    avail, D, X = _crafted({10: 5, 70: 5, 130: 5}, driver_only=False)
    for ok, d, _ in _crafted_batch(world, avail, D, X, [7, 12]):
        assert ok and d == 10


@pytest.mark.parametrize("world", [2, 3])
def test_k_zero_big_capacities_and_unscaled_requests(world):
    avail, D, X = _crafted({10: 5, 70: 5, 130: 5})
    (ok, d, ex), = _crafted_batch(world, avail, D, X, [0])
    assert ok and d == 192 and ex == []
    # a capacity of 256 or more in ONE shard's range only: every shard must take the designated-shard route, for every
    # application index (the designated shard is a mod n_shards)
    avail, D, X = _crafted({10: 5, 130: 5}, extra={70: [300, 999, 0]})
    got = _crafted_batch(world, avail, D, X, [4, 7, 290, 305, 4, 7, 311])
    assert [g[0] for g in got] == [True] * 6 + [False]
    assert got[0][2] == [10] * 4 and got[2][2] == [70] * 290
    # a request that is not a multiple of the table's units (every cpu value is a multiple of 30, the executor asks for 4)
    avail, D, X = _crafted({10: 30, 70: 30, 130: 30})
    got = _crafted_batch(world, avail, D, X, [3, 7, 15, 21, 22], exe=(4, 1, 0))  # capacities 7, 7, 7
    assert [g[0] for g in got] == [True] * 4 + [False] and got[1][2] == [10] * 7


# ---- 2. random parity: the generator of tests/test_gpu_minfrag.py::test_histogram_form_level_walks
@functools.lru_cache(maxsize=None)
def _level_walk_problem(n, cap_hi):
    """Whole small capacities, 5 % overcommitted nodes, 150 applications, a third of them one- or two-node gangs; the same
    cluster in three random zones.  With the oracle's answers: plain, zones interleaved, zones in AZ-major order (computed once
    per cluster, shared by the worlds)."""
    rng = np.random.default_rng(31337 + 17 * n + cap_hi)
    caps = rng.integers(0, cap_hi + 1, size=n)
    caps[rng.random(n) < 0.05] = -1
    avail = np.stack([caps, np.full(n, 1000), rng.integers(0, 2, size=n)], axis=1).astype(np.int64)
    order = rng.permutation(n).astype(np.uint32)
    a = 150
    total = int(np.maximum(caps, 0).sum())
    k = rng.integers(1, max(2, total), size=a)
    k[: a // 3] = rng.integers(1, max(2, min(total, 3 * cap_hi)), size=a // 3)
    k = np.minimum(k, 100000).astype(np.int32)
    drv = np.stack([rng.integers(0, 3, size=a), rng.integers(0, 50, size=a), np.zeros(a, dtype=np.int64)], axis=1).astype(np.int64)
    exe = np.stack([rng.integers(1, 3, size=a), rng.integers(0, 9, size=a), np.zeros(a, dtype=np.int64)], axis=1).astype(np.int64)
    zone = rng.integers(0, 3, size=n).astype(np.uint32)
    sched = np.maximum(avail, 1) + 5
    k3 = np.minimum(k, max(1, total // 4)).astype(np.int32)
    az = wl.reference_node_order(avail, zone).astype(np.uint32)
    refs = (_ref(MF, avail, None, None, order, order, drv, exe, k), _ref(SAZMF, avail, sched, zone, order, order, drv, exe, k3),
            _ref(SAZMF, avail, sched, zone, az, az, drv, exe, k3))
    return avail, sched, zone, order, az, drv, exe, k, k3, total, refs


SIZES = [(n, cap_hi) for n in (5, 65, 130, 700) for cap_hi in (3, 60, 300)]


@pytest.mark.parametrize("world", [2, 3, 8])  # (eight shards of three chunks: empty ranges)
@pytest.mark.parametrize("n,cap_hi", SIZES)
def test_shards_of_one_gpu_match_oracle(n, cap_hi, world):
    avail, sched, zone, order, az, drv, exe, k, k3, total, refs = _level_walk_problem(n, cap_hi)
    _check(world, MF, avail, None, None, order, order, drv, exe, k, refs[0])
    _check(world, SAZMF, avail, sched, zone, order, order, drv, exe, k3, refs[1])
    _check(world, SAZMF, avail, sched, zone, az, az, drv, exe, k3, refs[2])
    if total > 0:
        assert refs[0].results["has_capacity"].any()


def _multi_level(placement):
    """The placement drains nodes of at least two capacities completely: its runs before the last have two lengths."""
    p = np.asarray(placement)
    if len(p) == 0:
        return False
    starts = np.r_[0, np.nonzero(p[1:] != p[:-1])[0] + 1, len(p)]
    return len(set(np.diff(starts)[:-1].tolist())) >= 2


def test_the_battery_holds_multi_level_gangs():
    """Counted from the oracle's placements: what test_shards_of_one_gpu_match_oracle compares includes gangs over several levels."""
    multi = 0
    for n, cap_hi in SIZES:
        for ref in _level_walk_problem(n, cap_hi)[-1]:
            multi += sum(_multi_level(ref.placement(int(a))[2]) for a in np.nonzero(ref.results["has_capacity"])[0])
    assert multi >= 1


# ---- 3. gangs of gpu executors across ranges
@pytest.mark.parametrize("algo", [MF, SAZMF])
@pytest.mark.parametrize("world", [3, 8])
def test_gpu_gangs_across_ranges(algo, world):
    """The clusters of tests/test_gpu_sharded.py::test_gpu_gangs_take_the_ranges_part_of_the_compact_view: gpu nodes are a minority
    (the sparse gpu view exists) and sit in clumps of the priority order; gangs of gpu executors that fit, that do not, and
    whose driver lands on a gpu node."""
    rng = np.random.default_rng(777 + 13 * world + algo)
    seen = [0, 0]
    for n in (70, 700, 3000):
        for tight_cluster in (True, False):
            avail, D, X, drv, exe, k = _random_problem(rng, n, 200, tight_cluster, "merged")
            avail[:, 2] = 0
            pos = np.arange(len(X))
            clump = ((pos // max(1, len(X) // 9)) % 3 == 1) & (rng.random(len(X)) < 0.4)
            nodes = X[clump]
            nodes = nodes[nodes < n]
            avail[nodes, 2] = rng.integers(1, 9, size=len(nodes))
            exe[:, 2] = np.where(rng.random(len(exe)) < 0.7, rng.integers(1, 4, size=len(exe)), 0)
            drv[:, 2] = np.where(rng.random(len(drv)) < 0.3, 1, 0)
            small = rng.random(len(k)) < 0.75
            k = np.where(small, np.minimum(k, rng.integers(0, 40, size=len(k))), k).astype(np.int32)
            zone = rng.integers(0, 3, size=n).astype(np.uint32) if algo == SAZMF else None
            sched = np.maximum(avail, 0) + 5 if algo == SAZMF else None
            ref = _check(world, algo, avail, sched, zone, D, X, drv, exe, k)
            gpu_gang = (exe[:, 2] > 0) & (k > 0)
            seen[0] += int((ref.results["has_capacity"][gpu_gang] != 0).sum())
            seen[1] += int((ref.results["has_capacity"][gpu_gang] == 0).sum())
    assert seen[0] > 20 and seen[1] > 20


# ---- 4. headline size
@pytest.mark.parametrize("algo", [MF, SAZMF])
def test_headline_size_eight_shards(algo):
    """10 000 nodes x 1 000 applications, three zones in the reference's AZ-major order, eight shards of one device: rank 0's
    results and exec_nodes are one device's."""
    w = wl.headline(10000, 1000)
    s = w.snapshot
    zone = (wl.splitmix64(0xA4, len(s.avail), 9) % np.uint64(3)).astype(np.uint32)
    order = wl.reference_node_order(s.avail, zone).astype(np.uint32)
    apps = gangfit.make_apps(w.drv, w.exe, w.k)
    with gangfit.Context(0) as ctx:
        _setup(ctx, s.avail, s.sched, zone, order, order)
        one = ctx.fit_batch(IND, algo, apps)
    assert one.results["has_capacity"].mean() > 0.5
    out = _run(8, algo, s.avail, s.sched, zone, order, order, apps)[0]
    assert np.array_equal(out.results, one.results) and np.array_equal(out.exec_nodes, one.exec_nodes)


# ---- 5. layout and refusals
def _mf_layout(ctx, algo, half=11):
    rec, row, words, red = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    rc = ctx._lib.gf_shard_mf_layout(ctx._h, algo, half, C.byref(rec), C.byref(row), C.byref(words), C.byref(red))
    return rc, (rec.value, row.value, words.value, red.value)


def _refused(ctx, algo, code, apps):
    """The layout query and all four steps answer `code` for `algo` and say why; no step touches its device buffers."""
    import torch

    lib, h, n = ctx._lib, ctx._h, len(apps)
    d_apps = torch.from_numpy(gangfit.with_offsets(apps)[0].view(np.uint8).copy()).to("cuda:0")
    buf = {name: torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda:0") for name in ("part", "cnt", "drv", "res", "exec")}
    p = {name: C.c_void_p(t.data_ptr()) for name, t in buf.items()}
    da = C.c_void_p(d_apps.data_ptr())
    assert _mf_layout(ctx, algo)[0] == code and ctx.last_error()
    assert lib.gf_shard_mf_counts_dev(h, algo, n, da, p["part"], p["cnt"], None) == code
    assert lib.gf_shard_mf_drivers_dev(h, algo, n, da, p["part"], p["drv"], None) == code
    assert lib.gf_shard_mf_emit_dev(h, algo, n, da, p["part"], p["drv"], p["cnt"], p["res"], p["exec"], 64, None) == code
    assert lib.gf_shard_mf_finish_dev(h, algo, n, da, p["part"], p["drv"], p["res"], p["exec"], 64, None) == code
    torch.cuda.synchronize()
    for t in buf.values():
        assert bool((t == 0x5A).all())


def test_layout_and_refusals():
    rng = np.random.default_rng(9960)
    avail, sched, zone, D, X, drv, exe, k = _zoned_problem(rng, 400, 10, False, "merged", 3)
    k = np.minimum(k, 5).astype(np.int32)
    apps = gangfit.make_apps(drv, exe, k)
    with gangfit.Context(0) as ctx:
        _setup(ctx, avail, sched, zone, D, X)
        # records per application, bytes of a count row (256 uint16 counts), words of the placement buffer, words reduced
        assert _mf_layout(ctx, MF) == (0, (1, 512, 11, 11)) and _mf_layout(ctx, SAZMF) == (0, (3, 512, 33, 33))
        for algo in (N.GF_ALGO_TIGHTLY_PACK, N.GF_ALGO_DISTRIBUTE_EVENLY, N.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK, N.GF_ALGO_AZ_AWARE_TIGHTLY_PACK):
            _refused(ctx, algo, N.GF_ERR_UNSUPPORTED, apps)  # any other packer
        # the old entry points still refuse the minimal-fragmentation packers
        for algo in (MF, SAZMF):
            rec, words, red = C.c_uint32(), C.c_uint64(), C.c_uint64()
            assert ctx._lib.gf_shard_layout(ctx._h, algo, 11, C.byref(rec), C.byref(words), C.byref(red)) == N.GF_ERR_UNSUPPORTED
            assert ctx._lib.gf_shard_partials_dev(ctx._h, algo, 0, None, None, None) == N.GF_ERR_UNSUPPORTED
            with pytest.raises(gangfit.GangfitError) as e:
                sharded.ShardedBatch(sharded.HipShardEngine(ctx, 0, 2, "cuda:0"), sharded.SingleComm(), algo, apps)
            assert e.value.code == N.GF_ERR_UNSUPPORTED
        with pytest.raises(gangfit.GangfitError) as e:  # ... and the new batch refuses the others
            sharded.ShardedMinfragBatch(sharded.HipShardEngine(ctx, 0, 2, "cuda:0"), sharded.SingleComm(), 0, apps)
        assert e.value.code == N.GF_ERR_UNSUPPORTED
        # general slot layout
        ctx.set_orders([0, 1, 2], [2, 1, 0])
        for algo in (MF, SAZMF):
            _refused(ctx, algo, N.GF_ERR_UNSUPPORTED, apps)
        # more than 64 views
        every = np.arange(len(avail), dtype=np.uint32)
        _setup(ctx, avail, sched, (every % 65).astype(np.uint32), every, every)
        _refused(ctx, SAZMF, N.GF_ERR_UNSUPPORTED, apps)
        assert _mf_layout(ctx, MF)[0] == 0
        _setup(ctx, avail, sched, (every % 64).astype(np.uint32), every, every)
        assert _mf_layout(ctx, SAZMF) == (0, (64, 512, 64 * 11, 64 * 11))
        # single-AZ without the schedulable columns
        ctx.set_snapshot(avail)
        ctx.set_zones(zone)
        ctx.set_orders(X, X)
        _refused(ctx, SAZMF, N.GF_ERR_STATE, apps)
        assert _mf_layout(ctx, MF)[0] == 0
    with gangfit.Context(devices=[0, 0]) as g:  # a multi-device context runs the steps itself
        _setup(g, avail, sched, zone, D, X)
        for algo in (MF, SAZMF):
            _refused(g, algo, N.GF_ERR_UNSUPPORTED, apps)


# ---- 6. the in-library multi-device context
@pytest.mark.parametrize("algo", [MF, SAZMF])
@pytest.mark.parametrize("n_dev", [2, 3, 8])
def test_group_shards_minfrag_batches(algo, n_dev, split):
    """One context over n_dev device ids (all cuda:0): a minimal-fragmentation batch is sharded inside the library and comes back
    as the oracle's on the first (self-checked) and the second batch of a snapshot, with the context still sharding."""
    rng = np.random.default_rng(9800 + 17 * n_dev + algo)
    with gangfit.Context(devices=[0] * n_dev) as g:
        for n, cap_hi in ((130, 60), (700, 60), (700, 300)):  # the histogram form, and capacities beyond its last bin
            avail, sched, zone, order, az, drv, exe, k, k3, total, refs = _level_walk_problem(n, cap_hi)
            apps = gangfit.make_apps(drv, exe, k if algo == MF else k3)
            for D, ref in ((order, refs[0 if algo == MF else 1]),) + (((az, refs[2]),) if algo == SAZMF else ()):
                _setup(g, avail, sched, zone, D, D)
                _assert_same(g.fit_batch(IND, algo, apps), ref, apps)
                _assert_same(g.fit_batch(IND, algo, apps), ref, apps)  # (the second batch of a snapshot: no self-check)
                assert g.shard_count() == n_dev, g.last_error()
        avail, sched, zone, D, X, drv, exe, k = _zoned_problem(rng, 1000, 150, True, "merged", 3)  # driver-only, executor-only nodes
        _setup(g, avail, sched, zone, D, X)
        apps = gangfit.make_apps(drv, exe, k)
        ref = _ref(algo, avail, sched, zone, D, X, drv, exe, k)
        _assert_same(g.fit_batch(IND, algo, apps), ref, apps)
        _assert_same(g.fit_batch(IND, algo, apps), ref, apps)
        assert g.shard_count() == n_dev, g.last_error()


def _same(out, ref):
    return np.array_equal(out.results, ref.results) and all(
        np.array_equal(out.placement(int(a))[2], ref.placement(int(a))[2]) for a in np.nonzero(ref.results["has_capacity"])[0])


def _fault_problem(algo):
    avail, sched, zone, order, az, drv, exe, k, k3, total, refs = _level_walk_problem(700, 60)
    return avail, sched, zone, az, gangfit.make_apps(drv, exe, k if algo == MF else k3), _ref(
        algo, avail, sched, zone, az, az, drv, exe, k if algo == MF else k3)


@pytest.mark.parametrize("algo", [MF, SAZMF])
def test_group_really_shards_minfrag_batches(algo, monkeypatch):
    """Without the self-check, a dropped placement reduction (option group_fault = 1) must spoil the batch: proof that the other
    devices' shards produced part of it — a batch served by the first device alone would come back right."""
    monkeypatch.setenv("GANGFIT_TEST_GROUP_SPLIT", "1")
    avail, sched, zone, az, apps, ref = _fault_problem(algo)
    with gangfit.Context(devices=[0] * 4) as g:
        _setup(g, avail, sched, zone, az, az)
        g.set_option("group_verify", 0)
        g.set_option("group_fault", 1)
        assert (ref.results["has_capacity"] != 0).any()
        assert not _same(g.fit_batch(IND, algo, apps), ref)


@pytest.mark.parametrize("algo", [MF, SAZMF])
def test_minfrag_batch_is_self_checked_after_a_plain_one(algo, monkeypatch):
    """The self-check runs per packer family: a tightly-pack batch the fault cannot spoil (no executors: nothing to reduce)
    verifies the plain family on the snapshot; the first minimal-fragmentation batch is still answered by the first device as
    well, so the same fault gives the right answers, says "disagreed" and stops the sharding."""
    monkeypatch.setenv("GANGFIT_TEST_GROUP_SPLIT", "1")
    avail, sched, zone, az, apps, ref = _fault_problem(algo)
    k0 = np.zeros(len(apps), dtype=np.int32)
    with gangfit.Context(devices=[0] * 4) as g:
        _setup(g, avail, sched, zone, az, az)
        g.set_option("group_fault", 1)
        apps0 = gangfit.make_apps(apps["drv"], apps["exe"], k0)
        plain = ob.fit_independent(0, avail, ob.make_apps(apps["drv"], apps["exe"], k0), az, az, closed_form=True)
        _assert_same(g.fit_batch(IND, 0, apps0), plain, apps0)
        assert g.shard_count() == 4, g.last_error()
        _assert_same(g.fit_batch(IND, algo, apps), ref, apps)
        assert g.shard_count() == 1 and "disagreed" in g.last_error()
        _assert_same(g.fit_batch(IND, algo, apps), ref, apps)  # served by the first device from now on
