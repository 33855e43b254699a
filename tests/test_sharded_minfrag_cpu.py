"""The node-range sharded minimal-fragmentation batch as a numpy model: the specification the shard_mf_* kernels of
csrc/gangfit_shard.inc are read against (in the manner of tests/test_lane_algorithms.py).  Per range of the priority order a
capacity sum and a COUNT ROW (how many executor candidates of the range have capacity c, c = 1 .. 255, nothing reserved); from
the gathered rows every shard derives the same picture — the winning driver slot, the counts with the driver's node moved
from [c0] to [c1], its own prefix (the rows of the ranges before it, patched when the driver lies in one of them), the plan of
team_minfrag_hist — and emits, by prefix rank, only the runs of its own range.  Each placement entry is written by exactly one
shard, so the sum over shards of the zero-initialised buffers is the placement.  Checked against the oracle
(minimal_fragmentation.go:59-137) over crafted clusters and a few hundred random ones, worlds 1 to 8."""
import numpy as np
import pytest

from oracle import binding as ob
from oracle import pyoracle as po

BINS = 256          # capacities below this are counted; a larger one anywhere -> "no histogram form"
MF = ob.ALGO_MINIMAL_FRAGMENTATION


class Table:
    """The merged slot layout: `slots` = node ids in priority order, xcand / dcand = executor / driver candidate flags."""

    def __init__(self, avail, slots, xcand, dcand, units=(1, 1, 1)):
        self.avail = np.asarray(avail, dtype=np.int64)
        self.slots = [int(s) for s in slots]
        self.xcand, self.dcand = list(xcand), list(dcand)
        self.units = units
        self.chunks = (len(self.slots) + 63) // 64

    def range_of(self, shard, world):  # slots [lo, hi) of the shard: whole 64-slot chunks
        lo, hi = self.chunks * shard // world, self.chunks * (shard + 1) // world
        return lo * 64, min(hi * 64, len(self.slots))

    def cap(self, j, exe, reserved=(0, 0, 0)):  # GetNodeCapacity of slot j (capacity.go:59-75); 0 for a non-candidate
        if not self.xcand[j]:
            return 0
        return po.get_node_capacity(self.avail[self.slots[j]], reserved, exe)

    def scaled(self, drv, exe):  # mf_narrow_app: the requests are multiples of the table's units
        return all(int(v) % u == 0 for v, u in zip(list(drv) + list(exe), list(self.units) * 2))


def merged_slots(D, X):
    """plan_layout's merged order (csrc/gangfit_slot_layout.h) of a driver and an executor order without unknown or repeated
    names: (node of slot, executor candidate flags, driver candidate flags).  A driver-only node goes in ahead of the executors
    it precedes."""
    slots, xcand, dcand, i, j = [], [], [], 0, 0
    while i < len(D) or j < len(X):
        if i < len(D) and j < len(X) and D[i] == X[j]:
            slots, xcand, dcand, i, j = slots + [D[i]], xcand + [True], dcand + [True], i + 1, j + 1
        elif i < len(D) and D[i] not in X:
            slots, xcand, dcand, i = slots + [D[i]], xcand + [False], dcand + [True], i + 1
        else:
            assert j < len(X) and X[j] not in D, "the orders do not merge"
            slots, xcand, dcand, j = slots + [X[j]], xcand + [True], dcand + [False], j + 1
    return slots, xcand, dcand


def column_units(avail, slots):
    """fill_narrow's units of the scaled table: per dimension the gcd of the slots' values (1 for a column of zeros).  A request
    that is not a multiple of them has no histogram form on the device, whatever its capacities are."""
    cols = np.abs(np.asarray(avail, dtype=np.int64)[list(slots)])
    return tuple(int(np.gcd.reduce(cols[:, j])) or 1 for j in range(3))


def counts_step(T, shard, world, drv, exe, K):
    """-> (S, flag, row): S = sum over the range of min(cap, K), row[c] = nodes of the range with capacity c."""
    lo, hi = T.range_of(shard, world)
    row = np.zeros(BINS, dtype=np.int64)
    S, flag = 0, not T.scaled(drv, exe) or hi - lo >= 65536
    if K == 0:
        return 0, flag, row
    for j in range(lo, hi):
        c = T.cap(j, exe)
        S += min(c, K)
        if c >= BINS:
            flag = True
        elif c > 0:
            row[c] += 1
    if flag:
        row[:] = 0
    return S, flag, row


def drivers_step(T, shard, world, drv, exe, K, S):
    """The first driver candidate of the range with fit && S - c0 + c1 >= K (tightly-pack's rule), or None."""
    if S < K:
        return None
    lo, hi = T.range_of(shard, world)
    for j in range(lo, hi):
        a = T.avail[T.slots[j]]
        if not T.dcand[j] or po.greater_than(drv, a):
            continue
        c0, c1 = min(T.cap(j, exe), K), min(T.cap(j, exe, drv), K)
        if S - c0 + c1 >= K:
            return j
    return None


def plan(cn, K):
    """team_minfrag_hist's plan on the counts cn[c] (driver already moved): ({level: (nodes drained, output offset)},
    target) with target = (level, rank, offset, copies) of the ONE node that takes everything or what is left, or None."""
    levels = [c for c in range(1, BINS) if cn[c]]
    max_cap = levels[-1]
    top = BINS
    if K < max_cap:  # "avoid mostly empty nodes" (:68-78)
        target = (K + max_cap) // 2
        if sum(cn[c] * min(c, K) for c in levels if c < target) >= K:
            top = target

    def smallest_at_least(need, below):
        return next((c for c in levels if need <= c < below), None)

    R, drained = K, {}
    cf = smallest_at_least(R, top)
    if cf is not None:
        return drained, (cf, 0, 0, K)
    while True:
        m = max(c for c in levels if c < top)  # :113
        q = min(cn[m], R // m)                 # :120
        drained[m] = (q, K - R)
        R -= q * m
        if R == 0:
            return drained, None
        if q < cn[m]:  # R < m: the smallest capacity >= R below, else the first undrained node of this level
            cf = smallest_at_least(R, m)
            return drained, ((cf, 0, K - R, R) if cf is not None else (m, q, K - R, R))
        top = m  # :130
        cf = smallest_at_least(R, top)
        if cf is not None:
            return drained, (cf, 0, K - R, R)


def emit_step(T, shard, world, a, drv, exe, K, d, flags, rows):
    """This shard's slice of the placement: K entries, node + 1 where it writes, 0 elsewhere."""
    out = np.zeros(K, dtype=np.int64)
    if any(flags):  # one designated shard decides over the FULL order with the literal packer
        if shard == a % world:
            avail = {T.slots[j]: list(T.avail[T.slots[j]]) for j in range(len(T.slots))}
            order = [T.slots[j] for j in range(len(T.slots)) if T.xcand[j]]
            nodes, ok = po.minimal_fragmentation(list(exe), K, order, avail, {T.slots[d]: list(drv)})
            assert ok
            out[:] = np.asarray(nodes) + 1
        return out
    lo, hi = T.range_of(shard, world)
    cn = np.sum(rows, axis=0)
    pre = np.sum(rows[:shard], axis=0) if shard else np.zeros(BINS, dtype=np.int64)
    c0, c1 = T.cap(d, exe), T.cap(d, exe, drv)  # every shard reads slot d itself
    for c, delta in ((c0, -1), (c1, +1)):
        if c > 0:
            cn[c] += delta
            if d < lo:
                pre[c] += delta
    drained, target = plan(cn, K)
    seen = pre.copy()
    for j in range(lo, hi):  # pass 2 over the own range, the driver reserved at d
        c = T.cap(j, exe, drv if j == d else (0, 0, 0))
        if c <= 0:
            continue
        rank = seen[c]
        seen[c] += 1
        if c in drained and rank < drained[c][0]:
            at = drained[c][1] + rank * c
            assert not out[at:at + c].any()
            out[at:at + c] = T.slots[j] + 1
        if target is not None and (c, rank) == target[:2]:
            out[target[2]:target[2] + target[3]] = T.slots[j] + 1
    return out


def model_fit(T, world, a, drv, exe, K):
    """(feasible, driver node, executor nodes) of one application by `world` shards."""
    first = [counts_step(T, s, world, drv, exe, K) for s in range(world)]          # -- all-gather of sums and rows --
    S = sum(f[0] for f in first)
    found = [drivers_step(T, s, world, drv, exe, K, S) for s in range(world)]     # -- all-gather --
    found = [j for j in found if j is not None]
    if not found:
        return False, None, None
    d = min(found)
    if K == 0:
        return True, T.slots[d], np.zeros(0, dtype=np.int64)
    flags, rows = [f[1] for f in first], np.stack([f[2] for f in first])
    outs = [emit_step(T, s, world, a, drv, exe, K, d, flags, rows) for s in range(world)]
    for i in range(K):  # every entry is written by exactly one shard
        assert sum(1 for o in outs if o[i]) == 1, (i, K)
    return True, T.slots[d], np.sum(outs, axis=0) - 1                             # -- all-reduce(SUM), finish --


def _check(avail, D, X, T, drv, exe, K, worlds, a=0):
    ok, rd, rex = ob.spark_binpack(MF, avail, drv, exe, K, D, X)
    for world in worlds:
        got = model_fit(T, world, a, drv, exe, K)
        assert got[0] == ok, (world, K)
        if ok:
            assert got[1] == rd and got[2].tolist() == rex.tolist(), (world, K, got[2].tolist(), rex.tolist())
    return ok, rd, rex


# ---- crafted clusters: 192 executor nodes in identity order, node i = [caps[i], 99, 0], executor (1, 1, 0)
def _crafted(caps_at, driver_only=True, extra=None):
    caps = np.zeros(192, dtype=np.int64)
    for s, c in caps_at.items():
        caps[s] = c
    avail = [[int(c), 99, 0] for c in caps]
    if not driver_only:  # (as tests/test_gpu_sharded_minfrag.py::_crafted: nodes that keep the scaled table's units at 1)
        avail[1], avail[2] = [0, 1, 0], [1, 0, 0]
    for s, row in (extra or {}).items():
        avail[s] = row
    X = list(range(192))
    if driver_only:  # the driver goes to a node of its own, last in the merged order
        avail.append([1, 1, 0])
        return avail, [192], X, Table(avail, X + [192], [True] * 192 + [False], [False] * 192 + [True])
    return avail, X, X, Table(avail, X, [True] * 192, [True] * 192)


EXE = DRV = [1, 1, 0]
WORLDS = (1, 2, 3, 8)


def test_doc_comment_example_across_shards():
    avail, D, X, T = _crafted({0: 1, 64: 1, 65: 3, 63: 5, 128: 5, 191: 17})
    want = {6: [63] * 5 + [0], 11: [63] * 5 + [128] * 5 + [0], 15: [63] * 5 + [128] * 5 + [65] * 3 + [0, 64],
            17: [191] * 17, 19: [191] * 17 + [65, 65]}
    for K, execs in want.items():
        ok, rd, rex = _check(avail, D, X, T, DRV, EXE, K, WORLDS)
        assert ok and rd == 192 and rex.tolist() == execs
    ok, _, rex = _check(avail, D, X, T, DRV, EXE, 32, WORLDS)
    assert ok and sorted(set(rex.tolist())) == [0, 63, 64, 65, 128, 191]
    assert not _check(avail, D, X, T, DRV, EXE, 33, WORLDS)[0]


def test_one_level_in_three_shards():
    avail, D, X, T = _crafted({10: 5, 70: 5, 130: 5})
    want = {7: [10] * 5 + [70, 70],  # the first undrained node of the last level lives in the next shard
            12: [10] * 5 + [70] * 5 + [130, 130], 15: [10] * 5 + [70] * 5 + [130] * 5}
    for K, execs in want.items():
        ok, _, rex = _check(avail, D, X, T, DRV, EXE, K, WORLDS)
        assert ok and rex.tolist() == execs
    assert not _check(avail, D, X, T, DRV, EXE, 16, WORLDS)[0]


def test_driver_correction():
    avail, D, X, T = _crafted({}, driver_only=False, extra={0: [6, 99, 0], 100: [5, 99, 0]})
    ok, rd, rex = _check(avail, D, X, T, [1, 1, 0], EXE, 5, WORLDS)
    assert ok and rd == 0 and rex.tolist() == [0] * 5      # 6 -> 5 with the driver: the first of the two fives
    ok, rd, rex = _check(avail, D, X, T, [0, 1, 0], EXE, 5, WORLDS)
    assert ok and rd == 0 and rex.tolist() == [100] * 5    # stays 6: the five is the smallest sufficient
    # the driver lands in an EARLIER shard's range and drops its node a level: the later shards patch their prefix
    avail, D, X, T = _crafted({10: 5, 70: 5, 130: 5}, driver_only=False)
    for K in (7, 12):
        ok, rd, _ = _check(avail, D, X, T, DRV, EXE, K, WORLDS)
        assert ok and rd == 10


def test_k_zero_big_capacities_and_unscaled_requests():
    avail, D, X, T = _crafted({10: 5, 70: 5, 130: 5})
    ok, rd, rex = _check(avail, D, X, T, DRV, EXE, 0, WORLDS)
    assert ok and rd == 192 and len(rex) == 0
    # a capacity of 256 or more in ONE range only: every shard must take the designated-shard route
    avail, D, X, T = _crafted({10: 5, 130: 5}, extra={70: [300, 999, 0]})
    for a in range(3):
        for K in (4, 7, 290, 305):
            assert _check(avail, D, X, T, DRV, EXE, K, WORLDS, a=a)[0]
    # a request that is not a multiple of the table's units (cpu in units of 2)
    avail, D, X, T = _crafted({10: 10, 70: 10, 130: 10})
    T.units = (2, 1, 1)
    for K in (3, 7):
        assert _check(avail, D, X, T, DRV, [3, 1, 0], K, WORLDS, a=1)[0]


# ---- the last bin of a count row (tests/test_gpu_sharded_minfrag.py runs the same tables through the kernels)
def last_bin_tables():
    """[(avail, D, X, driver request, gang sizes, plain)]: the crafted cluster with nodes 10 and 130 at 5 and node 70 at 255 —
    the row's last bin — or 256, which flags node 70's range alone.  The driver sits on node 192, or on node 70 itself (D = [70]):
    256 -> 255 is still flagged (the counts are taken with nothing reserved), 255 -> 254 patches c0 = 255 out of the last bin, a
    driver that asks for no cpu patches it out and in again.  Gangs that land on node 70 alone, that drain it and go on, the
    cluster's sum, and (last) one more.  plain = False: nodes 140 and 150 hold cap - 1 and cap as well, in a later range than
    node 70: their ranks in their levels depend on the prefix patch for a driver in an EARLIER range.
    Nodes 0 = [0, 1, 0] and 1 = [1, 0, 0] hold no executor and keep every column's unit at 1 (column_units): without them the
    requests of 1 would have no scaled form and every gang would walk, 255 or 256."""
    out = []

    def cluster(caps):
        avail = [[0, 99, 0] for _ in range(192)]
        avail[0], avail[1] = [0, 1, 0], [1, 0, 0]
        for node, c in caps.items():
            avail[node] = [c, 99 if c == 5 else 999, 0]
        return avail

    for cap in (255, 256):
        for on_70, drv in ((False, [1, 1, 0]), (True, [1, 1, 0]), (True, [0, 1, 0])):
            avail = cluster({10: 5, 130: 5, 70: cap})
            if not on_70:
                avail.append([1, 1, 0])
            total = cap + 10 - (1 if on_70 and drv[0] else 0)
            ks = [4, 100, cap - 2, cap - 1, cap, cap + 1, cap + 5, total - 1, total, total + 1]
            out.append((avail, [70] if on_70 else [192], list(range(192)), drv, ks, True))
        avail = cluster({10: 5, 130: 5, 70: cap, 140: cap - 1, 150: cap})
        total = 3 * cap - 2 + 10  # node 70 gives cap - 1 with the driver on it
        ks = [cap - 1, cap, 2 * cap - 2, 2 * cap - 1, 2 * cap, 3 * cap - 2, 3 * cap - 1, total - 1, total, total + 1]
        out.append((avail, [70], list(range(192)), [1, 1, 0], ks, False))
    return out


def last_bin_expect(got, driver, plain):
    """got[i] = (feasible, driver node, executor nodes) of gang i of a table of last_bin_tables, already compared with the oracle."""
    assert [bool(g[0]) for g in got] == [True] * (len(got) - 1) + [False]
    assert all(g[1] == driver for g in got[:-1])
    if plain:  # (K + max) / 2 admits the fives for the small gang only
        assert list(got[0][2]) == [10] * 4 and list(got[1][2]) == [70] * 100 and sorted(set(got[-2][2])) == [10, 70, 130]
    else:
        assert sorted(set(got[-2][2])) == [10, 70, 130, 140, 150]


def last_bin_model(table):
    """The table as the device lays it out — the merged order, the scaled table's units — and the verdict that is the point of
    it: the requests have a scaled form, so only a capacity of 256 can flag a range."""
    avail, D, X, drv, ks, plain = table
    slots, xcand, dcand = merged_slots(D, X)
    T = Table(avail, slots, xcand, dcand, units=column_units(avail, slots))
    assert T.units == (1, 1, 1) and T.scaled(drv, EXE)
    return T


def last_bin_flags(T, world):
    """Which ranges must say "no histogram form": those with an executor candidate of 256 or more, nothing reserved."""
    return [any(T.cap(j, EXE) >= BINS for j in range(*T.range_of(s, world))) for s in range(world)]


def test_capacity_255_and_256_in_one_range():
    for table in last_bin_tables():
        avail, D, X, drv, ks, plain = table
        T = last_bin_model(table)
        for world in (2, 3):  # 256 flags exactly the ranges that hold such a node, 255 none — whatever the driver will reserve
            flags = last_bin_flags(T, world)
            assert [counts_step(T, s, world, drv, EXE, 100)[1] for s in range(world)] == flags
            assert any(flags) == (avail[70][0] == 256) and not all(flags)
        last_bin_expect([_check(avail, D, X, T, drv, EXE, K, WORLDS, a=i) for i, K in enumerate(ks)], D[0], plain)


# ---- the size of a range: 2047 chunks in two shards = 1023 and 1024 chunks; 65 536 slots are one too many for uint16 counts
def test_range_of_65536_slots_is_flagged():
    n = 2047 * 64
    avail = np.ones((n, 3), dtype=np.int64)
    X = list(range(n))
    T = Table(avail, X, [True] * n, [j in (0, 65471, 65472, n - 1) for j in range(n)])
    exe, drv = [1, 0, 0], [1, 1, 0]
    assert T.range_of(0, 2) == (0, 65472) and T.range_of(1, 2) == (65472, n)
    S, flag, row = counts_step(T, 0, 2, drv, exe, 70000)
    assert (S, flag) == (65472, False) and row[1] == 65472 and row.sum() == 65472
    S, flag, row = counts_step(T, 1, 2, drv, exe, 70000)
    assert (S, flag) == (65536, True) and not row.any()
    assert [counts_step(T, s, 3, drv, exe, 70000)[1] for s in range(3)] == [False] * 3  # 682, 682 and 683 chunks
    # a few gangs through the whole model: the flag of ONE range sends them to the designated shard, capacities of 1 or not
    for a, K in enumerate((3, 70)):
        ok, rd, rex = _check(avail, [0, 65471, 65472, n - 1], X, T, drv, exe, K, (2,), a=a)
        assert ok and rd == 0 and rex.tolist() == list(range(1, K + 1))


def _merged_problem(rng, n, cap_hi):
    caps = rng.integers(0, cap_hi + 1, size=n)
    caps[rng.random(n) < 0.05] = -1  # overcommitted nodes
    avail = np.stack([caps, np.full(n, 1000), rng.integers(0, 2, size=n)], axis=1).astype(np.int64)
    order = rng.permutation(n)
    xflag, dflag = rng.random(n) < 0.85, rng.random(n) < 0.7
    dflag[int(rng.integers(0, n))] = True
    xflag[int(rng.integers(0, n))] = True
    D, X = order[dflag].astype(np.uint32), order[xflag].astype(np.uint32)
    return avail, D, X, Table(avail, order, xflag, dflag), int(np.maximum(caps, 0).sum())


@pytest.mark.parametrize("seed", range(8))
def test_random_clusters_match_oracle(seed):
    """~300 clusters x applications: whole small capacities, overcommitted nodes, driver-only and executor-only nodes, gangs one
    node takes and gangs over many levels; cap_hi 300 puts capacities beyond the last bin."""
    rng = np.random.default_rng(8800 + seed)
    feasible = multi = 0
    for n in (5, 65, 130, 200, 450):
        for cap_hi in (3, 60, 300):
            avail, D, X, T, total = _merged_problem(rng, n, cap_hi)
            for a in range(3):
                K = int(rng.integers(1, max(2, min(total, 3 * cap_hi)))) if a else int(rng.integers(0, max(2, total + 2)))
                drv = [int(rng.integers(0, 3)), int(rng.integers(0, 50)), 0]
                exe = [int(rng.integers(1, 3)), int(rng.integers(0, 9)), 0]
                ok, _, rex = _check(avail, D, X, T, drv, exe, K, [int(w) for w in rng.choice(np.arange(1, 9), 3, replace=False)], a)
                feasible += ok
                multi += ok and len(set(rex.tolist())) > 2
    assert feasible > 10 and multi > 3
