"""What gf_cluster_executor_fit must answer, from the CPU oracle alone: the installing route (oracle.pysnapshot.build +
oracle.binding.executor_fit) given only the rows of S — the nodes of the request's set that pass its zone test.

A helper module, not a test file; tests/test_cluster_executor_cpu.py checks what it promises.

`reserved`, the map the reference subtracts on this path: first-fit — a node's overhead once more when at
least one reservation entry names the node (resource.go:642; an entry of all zeros counts); minimal fragmentation — every
node's overhead (GetNodeCapacities' reservedResources, resource.go:682).
"""
import numpy as np

from oracle import binding as ob
from oracle import pysnapshot as ps

GIB = 1 << 30
NO = 0xFFFFFFFF
ANY = 0xFFFFFFFF
QMAX = (1 << 62) - 1
NODE_COUNTS = (1, 63, 64, 65, 130, 700, 3000)
ZONE_CONFIGS = ("one", "three", "sparse")
SPARSE_IDS = (3, 10, 17)  # n_zones = 18: the ids in between (and 0 .. 2) are empty


def expected(c, res_node, res_req, sets, req_set, exe, minimal_fragmentation=False, hosts=None, node_zone=None, req_zone=None,
             exec_label_rank=None):
    """One cluster node index (NO = no capacity) per request.  c: dict with alloc (n, 3), overhead (n, 3) or None, flags,
    name_rank, zone (or None) and n_zones; res_node / res_req: the reservation entries the resident usage holds; sets:
    (n_sets, n) truth values or None = every node; the rest as Context.cluster_executor_fit takes them."""
    alloc = np.asarray(c["alloc"], dtype=np.int64).reshape(-1, 3)
    n = len(alloc)
    over = np.zeros_like(alloc) if c.get("overhead") is None else np.asarray(c["overhead"], dtype=np.int64).reshape(-1, 3)
    flags = np.asarray(c["flags"], dtype=np.uint32)
    name_rank = np.asarray(c["name_rank"], dtype=np.uint32)
    zone = np.zeros(n, dtype=np.uint32) if c.get("zone") is None else np.asarray(c["zone"], dtype=np.uint32)
    rn = np.zeros(0, dtype=np.int64) if res_node is None else np.asarray(res_node, dtype=np.int64)
    rr = np.zeros((0, 3), dtype=np.int64) if res_req is None else np.asarray(res_req, dtype=np.int64).reshape(-1, 3)
    inside = rn < n  # entries on nodes outside the cluster are ignored
    rn, rr = rn[inside], rr[inside]
    entries = np.bincount(rn, minlength=n)
    test_zone = zone if node_zone is None else np.asarray(node_zone, dtype=np.uint32)
    exe = np.asarray(exe, dtype=np.int64).reshape(-1, 3)
    out, built = [], {}
    for q in range(len(exe)):
        member = np.ones(n, dtype=bool) if sets is None else np.asarray(sets[int(req_set[q])]) != 0
        Q = ANY if req_zone is None else int(req_zone[q])
        if Q != ANY:
            member = member & (test_zone == Q)
        idx = np.nonzero(member)[0]
        if len(idx) == 0:
            out.append(NO)
            continue
        key = member.tobytes()
        if key not in built:  # the snapshot of S: what NodeSchedulingMetadataForNodes + PotentialNodes make of getNodes(nodeNames)
            local = np.full(n, -1, dtype=np.int64)
            local[idx] = np.arange(len(idx))
            keep = member[rn]
            avail, _, _, X = ps.build(alloc[idx], flags[idx], name_rank[idx], overhead=over[idx], res_node=local[rn[keep]],
                                      res_req=rr[keep], zone=zone[idx], n_zones=int(c["n_zones"]),
                                      exec_label_rank=None if exec_label_rank is None else np.asarray(exec_label_rank)[idx])
            built[key] = (avail, X)
        avail, X = built[key]
        if minimal_fragmentation:
            reserved = over[idx]
        else:
            reserved = over[idx] * (entries[idx] > 0)[:, None]
        h = None if hosts is None else np.asarray(hosts[q], dtype=bool)[idx].astype(np.uint8)
        r = ob.executor_fit(avail, exe[q], X, reserved=reserved, minimal_fragmentation=minimal_fragmentation, hosts=h)
        out.append(NO if r == NO else int(idx[r]))
    return out


def cluster(seed, n, zones):
    """A cluster of n nodes with everything the resident columns can hold: drawn flags, overhead on most nodes (above the
    allocatable on a few: negative available), reservation entries (all-zero ones and ones outside the cluster among them),
    blocks of nodes with equal (memory, cpu) that only name_rank separates, a few values at the top of the quantity contract."""
    rng = np.random.default_rng(seed)
    alloc = np.stack([rng.choice([4000, 8000, 16000], size=n), rng.choice([8, 16, 32], size=n) * GIB,
                      rng.choice([0, 0, 1, 4], size=n)], axis=1).astype(np.int64)
    over = np.stack([rng.integers(0, 4, size=n) * 250, rng.integers(0, 5, size=n) * (GIB // 4), np.zeros(n, dtype=np.int64)],
                    axis=1).astype(np.int64)
    over[rng.random(n) < 0.2] = 0
    too_much = rng.random(n) < 0.05
    over[too_much, 0] = alloc[too_much, 0] + 1000  # negative available cpu
    if n > 4:
        alloc[n - 1] = [QMAX, QMAX, 7]  # the largest allocatable the contract admits
    n_res = int(rng.integers(n, 3 * n + 2))
    res_node = rng.integers(0, n + max(1, n // 20), size=n_res).astype(np.uint32)  # (some beyond the cluster: ignored)
    res_req = np.stack([rng.choice([0, 500, 1000], size=n_res), rng.choice([0, GIB // 2, GIB], size=n_res),
                        rng.choice([0, 0, 0, 1], size=n_res)], axis=1).astype(np.int64)
    res_req[rng.random(n_res) < 0.15] = 0  # entries of all zeros: the node is a key of the usage map all the same
    res_node[0], res_req[0] = int(rng.integers(0, n)), 0  # (at least one of them, on a node of the cluster)
    flags = (np.where(rng.random(n) < 0.85, ps.READY, 0) | np.where(rng.random(n) < 0.5, ps.DRIVER_CANDIDATE, 0) |
             np.where(rng.random(n) < 0.08, ps.UNSCHEDULABLE, 0)).astype(np.uint32)
    flags[0], over[0] = ps.READY | ps.DRIVER_CANDIDATE, [250, GIB // 4, 0]  # node 0 is always a candidate with something left
    if zones == "one":
        zone, n_zones = None, 1
    elif zones == "three":
        zone, n_zones = rng.integers(0, 3, size=n).astype(np.uint32), 3
    elif zones == "sparse":
        zone, n_zones = rng.choice(SPARSE_IDS, size=n).astype(np.uint32), max(SPARSE_IDS) + 1
    else:
        raise ValueError(zones)
    return dict(alloc=alloc, overhead=over, flags=flags, name_rank=rng.permutation(n).astype(np.uint32), zone=zone,
                n_zones=n_zones, res_node=res_node, res_req=res_req)


def requests(seed, n_req=60):
    """Executor requests from "fits everywhere" to "fits nowhere", zero dimensions and the contract's largest among them."""
    rng = np.random.default_rng(seed + 7)
    exe = np.stack([rng.choice([0, 250, 1000, 3000, 7000, 15000], size=n_req), rng.choice([0, 1, GIB, 6 * GIB, 15 * GIB, 31 * GIB], size=n_req),
                    rng.choice([0, 0, 0, 1, 4], size=n_req)], axis=1).astype(np.int64)
    exe[0] = [0, 0, 0]            # every capacity math.MaxInt
    exe[1 % n_req] = [17000, 1, 0]  # above every ordinary node's cpu
    exe[2 % n_req] = [1, (1 << 61) + 1, 0]
    exe[3 % n_req] = [QMAX, QMAX, QMAX]
    return exe


def node_sets(seed, n):
    """Rows: every node, a random half, nobody, one node, two overlapping thirds."""
    rng = np.random.default_rng(seed + 11)
    sets = np.zeros((6, n), dtype=bool)
    sets[0] = True
    sets[1] = rng.random(n) < 0.5
    sets[3, int(rng.integers(0, n))] = True
    sets[4, : (2 * n + 2) // 3] = True
    sets[5, n // 3:] = True
    return sets


# ---- three constructed cases, each with two candidate answers that provably differ: (cluster, entries, kwargs, right, wrong)

def _plain(alloc, overhead=None, zone=None, n_zones=1):
    n = len(alloc)
    return dict(alloc=np.asarray(alloc, dtype=np.int64), overhead=overhead, flags=np.full(n, ps.READY, dtype=np.uint32),
                name_rank=np.arange(n, dtype=np.uint32), zone=zone, n_zones=n_zones)


def case_subset_zone_ranks():
    """(a) Zone 0 = {n0: 50 GiB, n1: 60 GiB}, zone 1 = {n2: 100 GiB}.  The whole cluster ranks zone 1 (100) before zone 0 (110):
    its order is n2, n0, n1.  The subset {n0, n2} ranks zone 0 (50) before zone 1 (100): n0, n2.  Everything fits, so the answer
    is n0; filtering the whole cluster's order would have said n2."""
    c = _plain([[8000, 50 * GIB, 0], [8000, 60 * GIB, 0], [8000, 100 * GIB, 0]], zone=np.array([0, 0, 1], dtype=np.uint32), n_zones=2)
    kw = dict(sets=np.array([[1, 0, 1]], dtype=bool), req_set=[0], exe=[[1000, GIB, 0]])
    return c, None, None, kw, 0, 2


def case_zero_valued_entry():
    """(b) n0: 10 GiB allocatable, 4 GiB overhead, ONE reservation entry of all zeros; n1: 20 GiB, nothing.  A 5 GiB executor
    fits n0's allocatable - overhead (6 GiB) but not allocatable - 2 * overhead (2 GiB): the entry makes n0 a key of the usage
    map, the overhead counts twice, the answer is n1.  The usage SUMS of n0 are zero: they alone would have said n0."""
    c = _plain([[8000, 10 * GIB, 0], [8000, 20 * GIB, 0]], overhead=np.array([[0, 4 * GIB, 0], [0, 0, 0]], dtype=np.int64))
    kw = dict(sets=None, req_set=None, exe=[[1000, 5 * GIB, 0]])
    return c, np.array([0], dtype=np.uint32), np.zeros((1, 3), dtype=np.int64), kw, 1, 0


def case_hosting_beats_capacity():
    """(c) Minimal fragmentation: n0 hosts the application and holds 5 executors, n1 does not and holds 2.  Hosting comes
    first: n0; by capacity alone it would have been n1."""
    c = _plain([[5000, 32 * GIB, 0], [2000, 32 * GIB, 0]])
    kw = dict(sets=None, req_set=None, exe=[[1000, GIB, 0]], minimal_fragmentation=True, hosts=np.array([[1, 0]], dtype=bool))
    return c, None, None, kw, 0, 1


CONSTRUCTED = (case_subset_zone_ranks, case_zero_valued_entry, case_hosting_beats_capacity)
