"""Inputs of the empty-cluster capacity scan tests (gf_cluster_fit_feasible): small clusters with scattered zone ids, seventy
applications whose executor counts sit on the edges of the cluster's capacity, and the reference answer — the CPU oracle on the
snapshot oracle/pysnapshot.py builds from the same inputs with no reservations and the selected nodes as driver AND executor
candidates.  `predicate` restates what the scan computes (order-free) in Python integers; it only places the executor counts
of the generated applications on the edges and is itself checked against the oracle on the CPU (test_cluster_scan_abi.py)."""
import numpy as np

from oracle import binding as ob
from oracle import pysnapshot as ps

GIB = 1 << 30
PLAIN = (0, 1, 2)          # tightly-pack, distribute-evenly, minimal-fragmentation
AZ_AWARE = 3               # az-aware-tightly-pack: the plain answer
SINGLE_AZ = (4, 5)         # single-az-tightly-pack, single-az-minimal-fragmentation
ALGOS = PLAIN + (AZ_AWARE,) + SINGLE_AZ
NODE_COUNTS = (1, 63, 64, 65, 130)
ZONE_COUNTS = (1, 3, 64)
N_APPS = 70


def seed_of(n, n_zones):
    """Seeds at which the ORACLE alone answers at least five applications each way for every packer, with and without the
    overhead (searched once on the CPU; the tests assert it again on every run)."""
    return 1000 * n + 10 * n_zones


def cluster(seed, n, n_zones):
    rng = np.random.default_rng(seed)
    shape = rng.integers(0, 4, size=n)
    gpu = np.where(rng.random(n) < 0.15, 8, 0)
    if n >= 8:
        gpu[int(rng.integers(0, n))] = 8  # a gpu minority, never empty
    alloc = np.stack([np.array([16, 32, 64, 96])[shape] * 1000, np.array([64, 128, 256, 384])[shape] * GIB, gpu], axis=1).astype(np.int64)
    over = np.stack([rng.integers(0, 8, size=n) * 250, rng.integers(0, 16, size=n) * (GIB // 4), np.zeros(n, dtype=np.int64)],
                    axis=1).astype(np.int64)
    zone = rng.integers(0, n_zones, size=n).astype(np.uint32)  # scattered, not AZ-major
    return dict(alloc=alloc, overhead=over, zone=zone, n_zones=n_zones, name_rank=rng.permutation(n).astype(np.uint32))


def _caps(avail, exe, k):
    """min(capacity, k) per node: the add-one-then-compare loop of the packers in closed form"""
    c = np.full(len(avail), k, dtype=np.int64)
    for j in range(3):
        if exe[j] > 0:
            c = np.minimum(c, avail[:, j] // exe[j])
    return np.where((avail < 0).any(axis=1), 0, c)


def predicate(c, select, drv, exe, k, per_zone, overhead=None):
    """(answer, S, best S - cap + cap') of the plain order, or of the best zone by itself"""
    avail_all = c["alloc"] if overhead is None else c["alloc"] - overhead
    drv = np.asarray(drv, dtype=np.int64)
    select = np.asarray(select) != 0
    best_s, best_total = 0, -1
    for z in (range(c["n_zones"]) if per_zone else [None]):
        avail = avail_all[select if z is None else select & (c["zone"] == z)]
        caps = _caps(avail, exe, k)
        s = int(caps.sum())
        fits = (avail >= drv).all(axis=1)
        if fits.any():
            total = int((s - caps[fits] + _caps(avail[fits] - drv, exe, k)).max())
            if total > best_total:
                best_s, best_total = s, total
    return best_total >= k, best_s, best_total


def applications(seed, c, n_apps=N_APPS):
    """Seventy applications for the cluster WITHOUT its overhead (the same ones are asked with it).  Executor counts on the edges: 0, 1, exactly what fits behind the best driver candidate and one more (a gang that fits only
    once the driver's node is counted after the driver: the plain sum alone would take it), the same per zone, far above the
    cluster's total; gpu executors for a fifth of them."""
    rng = np.random.default_rng(seed + 7)
    n = len(c["alloc"])
    everyone = np.ones(n, dtype=bool)
    drv = np.stack([rng.choice([500, 1000, 2000, 4000], size=n_apps), rng.choice([1, 2, 4, 8], size=n_apps) * GIB,
                    (rng.random(n_apps) < 0.1).astype(np.int64)], axis=1).astype(np.int64)
    exe = np.stack([rng.choice([1000, 2000, 4000, 8000], size=n_apps), rng.choice([2, 4, 8, 16, 32], size=n_apps) * GIB,
                    (rng.random(n_apps) < 0.2).astype(np.int64)], axis=1).astype(np.int64)
    exe[3, 1] = 0  # a dimension that never limits
    exe[4, 0] = 0
    k = np.zeros(n_apps, dtype=np.int64)
    for a in range(n_apps):
        d, e = [int(v) for v in drv[a]], [int(v) for v in exe[a]]
        _, s, total = predicate(c, everyone, d, e, 1 << 20, per_zone=False)
        _, zs, ztotal = predicate(c, everyone, d, e, 1 << 20, per_zone=True)
        edges = [0, 1, total, total + 1, s, ztotal, ztotal + 1, 3 * s + 5, total // 2, int(rng.integers(0, max(s, 1) + 1)), 2, zs]
        k[a] = min(max(edges[a % len(edges)], 0), 1 << 20)
    return drv, exe, k.astype(np.int32)


def flags_of(select):
    return np.where(np.asarray(select) != 0, ps.READY | ps.DRIVER_CANDIDATE, 0).astype(np.uint32)


def reference(c, select, drv, exe, k, overhead=None):
    """{algo: HasCapacity bytes} from the oracle on the restated snapshot: no reservations, the selected nodes in both lists"""
    avail, sched, D, X = ps.build(c["alloc"], flags_of(select), c["name_rank"], overhead=overhead, zone=c["zone"], n_zones=c["n_zones"])
    oapps = ob.make_apps(drv, exe, k)
    out = {}
    for algo in ALGOS:
        r = ob.fit_independent(algo, avail, oapps, D, X, sched=sched, zone=c["zone"])
        out[algo] = (r.results["has_capacity"] != 0).astype(np.uint8)
    return out
