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
from test_sharded_minfrag_cpu import last_bin_expect, last_bin_flags, last_bin_model, last_bin_tables

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


def _flags(world, avail, D, X, apps):
    """The verdict of the counts step itself, [shard][application]: True where shard_mf_counts_kernel published "no histogram
    form" (fit_count of its record) for the plain packer's one view.  One context takes every shard's range in turn."""
    import torch

    torch.cuda.init()
    out = []
    with gangfit.Context(0) as ctx:
        _setup(ctx, avail, None, None, D, X)
        for r in range(world):
            eng = sharded.HipShardEngine(ctx, r, world, "cuda:0")
            b = sharded.ShardedMinfragBatch(eng, sharded.SingleComm(), MF, apps)
            assert b.records == 1
            with eng.stream_context():
                mine = eng.mf_counts(MF, b.d_apps, b.n_apps, b.records, b.row_bytes)
                part = mine[: b.n_apps * 16].cpu().numpy().view(np.int64).reshape(b.n_apps, 2)
            out.append(part[:, 1] != 0)
    return np.stack(out)


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
#      The scaled table's units are the gcds of its columns (fill_narrow, csrc/gangfit_slot_layout.h) and a request that is not a
#      multiple of them has no histogram form: node 192 = [1, 1, 0] keeps them at 1, and without it nodes 1 = [0, 1, 0] and
#      2 = [1, 0, 0] do, which hold no executor and no driver that asks for cpu.  _hist_form asserts the kernel's verdict.
def _crafted(caps_at, driver_only=True, extra=None):
    avail = np.zeros((193 if driver_only else 192, 3), dtype=np.int64)
    avail[:192, 1] = 99
    if not driver_only:
        avail[1], avail[2] = [0, 1, 0], [1, 0, 0]
    for s, c in caps_at.items():
        avail[s, 0] = c
    for s, row in (extra or {}).items():
        avail[s] = row
    X = np.arange(192, dtype=np.uint32)
    if driver_only:
        avail[192] = [1, 1, 0]
        return avail, np.array([192], dtype=np.uint32), X
    return avail, X.copy(), X


def _hist_form(world, avail, D, X, drv, exe, k, want=False):
    """The counts step flags the ranges `want` says (one flag for all: a bool; per shard: a list) for every gang with executors:
    a crafted case that means the histogram form must not walk for a reason of its own making, and the other way round."""
    k = np.asarray(k)
    got = _flags(world, avail, D, X, gangfit.make_apps(drv, exe, k))[:, k > 0]
    want = np.broadcast_to(np.asarray(want, dtype=bool).reshape(-1, 1), got.shape)
    assert np.array_equal(got, want), got.astype(int).tolist()


def _crafted_batch(world, avail, D, X, ks, drv=(1, 1, 0), exe=(1, 1, 0), flagged=False):
    a = len(ks)
    drv, exe = np.tile(np.array(drv, dtype=np.int64), (a, 1)), np.tile(np.array(exe, dtype=np.int64), (a, 1))
    _hist_form(world, avail, D, X, drv, exe, ks, flagged)
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
    got = _crafted_batch(world, avail, D, X, [4, 7, 290, 305, 4, 7, 311], flagged=[s == (0 if world == 2 else 1) for s in range(world)])
    assert [g[0] for g in got] == [True] * 6 + [False]
    assert got[0][2] == [10] * 4 and got[2][2] == [70] * 290
    # a request that is not a multiple of the table's units: every cpu value is a multiple of 30 — the driver-only node's and the
    # driver's request as well —, the executor asks for 4.  Every range says so, whatever its capacities
    avail, D, X = _crafted({10: 30, 70: 30, 130: 30})
    avail[192] = [30, 1, 0]
    got = _crafted_batch(world, avail, D, X, [3, 7, 15, 21, 22], drv=(30, 1, 0), exe=(4, 1, 0), flagged=True)  # capacities 7, 7, 7
    assert [g[0] for g in got] == [True] * 4 + [False] and got[1][2] == [10] * 7


# ---- 1b. the last bin of a count row: the tables of tests/test_sharded_minfrag_cpu.py::last_bin_tables — a node of 255 (histogram
#      form) or 256 executors (its range flags every gang: the designated shard walks) in ONE range, with the driver on a node of
#      its own or on that very node, 256 -> 255 (still flagged) and 255 -> 254 (c0 = 255 patched out of the row's last bin)
def _last_bin_problem(table):
    avail, D, X, drv, ks, plain = table
    a = len(ks)
    drv_a, exe_a = np.tile(np.array(drv, dtype=np.int64), (a, 1)), np.tile(np.array([1, 1, 0], dtype=np.int64), (a, 1))
    return (np.array(avail, dtype=np.int64), np.array(D, dtype=np.uint32), np.array(X, dtype=np.uint32), drv_a, exe_a,
            np.array(ks, dtype=np.int32))


def _last_bin_batch(run, table):
    """`run(avail, D, X, drv, exe, k) -> the oracle's answer` after comparing a route with it; then what the table expects."""
    ref = run(*_last_bin_problem(table))
    last_bin_expect([ref.placement(i) for i in range(len(table[4]))], table[1][0], table[5])


@pytest.mark.parametrize("world", [2, 3])
def test_capacity_255_and_256_in_one_range(world):
    """With the kernel's own verdict per range: 255 keeps the histogram form in every range, with the driver's node at 255 -> 254
    too; 256 flags the ranges that hold such a node and no other, 256 -> 255 included."""
    for table in last_bin_tables():
        flags = last_bin_flags(last_bin_model(table), world)  # (the model lays the slots out as the device does)
        assert any(flags) == (table[0][70][0] == 256) and not all(flags)
        _hist_form(world, *_last_bin_problem(table), flags)
        _last_bin_batch(lambda avail, D, X, drv, exe, k: _check(world, MF, avail, None, None, D, X, drv, exe, k), table)


def _group_batch(g, avail, D, X, drv, exe, k, ref=None):
    """The batch on the multi-device context `g`, against the oracle; the context is still sharding afterwards."""
    apps = gangfit.make_apps(drv, exe, k)
    if ref is None:
        ref = _ref(MF, avail, None, None, D, X, drv, exe, k)
    _setup(g, avail, None, None, D, X)
    _assert_same(g.fit_batch(IND, MF, apps), ref, apps)  # (the first batch of a snapshot: self-checked)
    _assert_same(g.fit_batch(IND, MF, apps), ref, apps)
    assert g.shard_count() == 2, g.last_error()
    return ref


def test_capacity_255_and_256_in_one_range_in_library(split):
    with gangfit.Context(devices=[0, 0]) as g:
        for table in last_bin_tables():
            _last_bin_batch(lambda *problem: _group_batch(g, *problem), table)


# ---- 1c. the size of a range: thin tables of 2046 and 2047 chunks, two shards.  Identity executor order; four driver candidates
#      (slots 0, 65 471, 65 472, 130 943: the first slot, either side of the boundary between the ranges, the last slot of 2046
#      chunks) that a driver's MEMORY request chooses between — candidate i holds i + 1, every other node 1 — while executors ask
#      for cpu only; a driver that asks for its node's whole cpu drops the node's capacity to 0.
#        2046 chunks   both ranges are 1023 chunks and keep the histogram form.  Every node holds 1: a uint16 bin of 65 472, a
#                      summed bin of 130 944.  Every node holds 255 (node 1: 254, so that the cpu column's unit stays 1): the
#                      second range's capacity sum is 65 472 x 255, the bound shard_mf_counts_kernel's comment claims.
#        2047 chunks   the second range is 1024 chunks = 65 536 slots: flagged, every gang goes to the designated shard although
#                      every capacity is 1.
RANGE_DRIVERS = (0, 65471, 65472, 130943)
GF_MAX_K = 1 << 20


@functools.lru_cache(maxsize=None)
def _range_table(chunks, cap):
    """(avail, D, X, drv, exe, k, the oracle's answer: computed once per table, shared by the routes).  Gangs of 65 472 executors
    (a range's worth at capacity 1), 65 473 (the first node of the next range), 70 000, 130 944 and 130 945 (one more than 2046
    chunks of capacity 1 hold), and 2^20 where the table holds them; drivers on each of the four candidates, keeping their
    node's capacity (cpu 0) or taking it.  The oracle is the literal packer; for the gang that does not fit, the closed form
    as well."""
    n = chunks * 64
    avail = np.zeros((n, 3), dtype=np.int64)
    avail[:, 0], avail[:, 1] = cap, 1
    if cap > 1:
        avail[1, 0] = cap - 1
    avail[list(RANGE_DRIVERS), 1] = np.arange(1, 5)
    X = np.arange(n, dtype=np.uint32)
    D = np.array(RANGE_DRIVERS, dtype=np.uint32)
    total = int(avail[:, 0].sum())
    # (k, the driver's candidate, whether the driver takes its node's cpu)
    gangs = [(65472, 0, False), (65473, 0, False), (70000, 0, True), (65472, 1, True), (65472, 2, True), (65473, 1, True),
             (70000, 3, True), (130944, 0, False), (130943, 2, True), (130945, 3, False)]
    if total > GF_MAX_K:
        gangs += [(GF_MAX_K, 0, False), (GF_MAX_K, 0, True), (GF_MAX_K, 3, True)]
    drv = np.array([[cap if takes else 0, cand + 1, 0] for _, cand, takes in gangs], dtype=np.int64)
    exe = np.tile(np.array([1, 0, 0], dtype=np.int64), (len(gangs), 1))
    k = np.array([g[0] for g in gangs], dtype=np.int32)
    ref = _ref(MF, avail, None, None, D, X, drv, exe, k)
    misfit = [i for i in range(len(gangs)) if not ref.results["has_capacity"][i]]
    assert misfit == ([9] if total < 130945 else [])
    for i in misfit:
        cf = ob.fit_independent(O_ALGO[MF], avail, ob.make_apps(drv[i:i + 1], exe[i:i + 1], k[i:i + 1]), D, X, closed_form=True)
        assert not cf.results["has_capacity"][0]
    fits = np.nonzero(ref.results["has_capacity"])[0]
    assert [int(ref.results["driver_node"][i]) for i in fits] == [RANGE_DRIVERS[gangs[i][1]] for i in fits]
    return avail, D, X, drv, exe, k, ref


def _range_rows(avail, chunks, world=2):
    """The count rows of the ranges as the counts step takes them (nothing reserved; executors ask for one cpu)."""
    cuts = [chunks * s // world * 64 for s in range(world + 1)]
    return np.stack([np.bincount(np.clip(avail[lo:hi, 0], 0, 256), minlength=257) for lo, hi in zip(cuts, cuts[1:])])


RANGE_TABLES = [(2046, 1), (2046, 255), (2047, 1)]


@pytest.mark.parametrize("chunks,cap", RANGE_TABLES)
def test_range_of_1023_and_1024_chunks(chunks, cap):
    avail, D, X, drv, exe, k, ref = _range_table(chunks, cap)
    rows = _range_rows(avail, chunks)
    if chunks == 2046:  # what the rows hold: the largest uint16 bin, the largest summed bin, the largest capacity sum of a range
        assert rows[:, 1:256].max() == 65472 and rows.sum(axis=0)[1:256].max() == (130944 if cap == 1 else 130943)
        assert max(int((r[:256] * np.arange(256)).sum()) for r in rows) == 65472 * cap
    else:
        assert chunks * 64 - chunks // 2 * 64 == 65536  # the second range: one chunk too many for uint16 counts
    _hist_form(2, avail, D, X, drv, exe, k, [False, chunks == 2047])  # (the kernel's verdict: 1024 chunks are flagged, 1023 not)
    apps = gangfit.make_apps(drv, exe, k)
    for out in _run(2, MF, avail, None, None, D, X, apps):
        _assert_same(out, ref, apps)


@pytest.mark.parametrize("chunks,cap", RANGE_TABLES)
def test_range_of_1023_and_1024_chunks_in_library(chunks, cap, split):
    avail, D, X, drv, exe, k, ref = _range_table(chunks, cap)
    with gangfit.Context(devices=[0, 0]) as g:
        _group_batch(g, avail, D, X, drv, exe, k, ref)


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
