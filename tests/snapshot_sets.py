"""Node sets of a resident cluster as inputs of gf_snapshot_build_resident_set (Context.build_snapshot_resident_set): the
compaction of a cluster to the members of a set and the mapping of what is computed on the compact rows back to cluster indices,
once, for every test of the feature.

A helper module, not a test file; tests/test_snapshot_sets_cpu.py checks what it promises.

The reference of every comparison is code that knows nothing of sets: oracle/pysnapshot.py::build on compact(c, members), the
oracle's packers on its result, and the library's own gf_cluster_set + gf_snapshot_build_resident on a context that holds only the
members.  compact() is the definition of include/gangfit.h in executable form:

  rows of M = the members in ascending cluster index; the same zone ids and n_zones; name ranks = the rank among members of the
  cluster's name_rank; only the reservation entries that name a member (renamed); the members' flag and label-rank rows.
"""
from dataclasses import dataclass

import numpy as np

from oracle import pysnapshot as ps

NO_NODE = 0xFFFFFFFF
CAND = ps.READY | ps.DRIVER_CANDIDATE


def member_index(members, n):
    """Index list or boolean mask -> the members in ascending cluster index (int64)."""
    mem = np.asarray(members)
    if mem.dtype == np.bool_:
        assert mem.shape == (n,)
        return np.nonzero(mem)[0].astype(np.int64)
    idx = np.unique(mem.astype(np.int64).reshape(-1))
    assert len(idx) == 0 or (idx[0] >= 0 and idx[-1] < n)
    return idx


def compact(c, members):
    """Keyword arguments of oracle.pysnapshot.build / Context.build_snapshot for the members of cluster c alone."""
    alloc = np.asarray(c["alloc"], dtype=np.int64).reshape(-1, 3)
    n = len(alloc)
    M = member_index(members, n)
    m = len(M)
    where = np.full(n, -1, dtype=np.int64)  # cluster index -> member index
    where[M] = np.arange(m)
    name_rank = np.asarray(c["name_rank"], dtype=np.int64)[M]
    rank = np.empty(m, dtype=np.int64)
    rank[np.argsort(name_rank, kind="stable")] = np.arange(m)
    res_node = res_req = None
    if c.get("res_node") is not None and len(c["res_node"]):
        rn = np.asarray(c["res_node"], dtype=np.int64)
        rr = np.asarray(c["res_req"], dtype=np.int64).reshape(-1, 3)
        keep = rn < n
        keep[keep] = where[rn[keep]] >= 0
        res_node = where[rn[keep]].astype(np.uint32)
        res_req = rr[keep]

    def rows(a, dtype):
        return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=dtype)[M])

    zone = c.get("zone")
    return dict(alloc=alloc[M], node_flags=rows(c["node_flags"], np.uint32), name_rank=rank.astype(np.uint32),
                overhead=rows(None if c.get("overhead") is None else np.asarray(c["overhead"]).reshape(-1, 3), np.int64),
                res_node=res_node, res_req=res_req, zone=rows(zone, np.uint32), n_zones=c.get("n_zones", 1),
                driver_label_rank=rows(c.get("driver_label_rank"), np.uint32),
                exec_label_rank=rows(c.get("exec_label_rank"), np.uint32))


@dataclass
class SetRef:
    M: np.ndarray        # members, ascending cluster index
    inputs: dict         # compact(c, members)
    avail_c: np.ndarray  # (m, 3) of the members alone
    sched_c: np.ndarray
    D_c: np.ndarray      # orders in member indices
    X_c: np.ndarray
    avail: np.ndarray    # (n, 3): the members' rows, zeros elsewhere
    sched: np.ndarray
    D: np.ndarray        # orders in cluster indices
    X: np.ndarray


def build(c, members):
    """oracle.pysnapshot.build on the members alone, and its result in the cluster's indices."""
    n = len(np.asarray(c["alloc"]).reshape(-1, 3))
    M = member_index(members, n)
    inputs = compact(c, M)
    if len(M):
        avail_c, sched_c, D_c, X_c = ps.build(**inputs)
    else:
        avail_c = sched_c = np.zeros((0, 3), dtype=np.int64)
        D_c = X_c = np.zeros(0, dtype=np.uint32)
    avail = np.zeros((n, 3), dtype=np.int64)
    sched = np.zeros((n, 3), dtype=np.int64)
    avail[M] = avail_c
    sched[M] = sched_c
    return SetRef(M, inputs, avail_c, sched_c, D_c, X_c, avail, sched, to_cluster(D_c, M), to_cluster(X_c, M))


def to_cluster(nodes, M):
    """Member indices -> cluster indices; GF_NO_NODE stays."""
    nodes = np.asarray(nodes, dtype=np.uint32)
    out = nodes.copy()
    real = nodes != NO_NODE
    out[real] = M[nodes[real].astype(np.int64)].astype(np.uint32)
    return out


def results_to_cluster(results, M):
    """A batch's result records with driver_node in cluster indices."""
    out = results.copy()
    out["driver_node"] = to_cluster(results["driver_node"], M)
    return out


def rows_to_cluster(rows_c, M, n):
    """(m, 3) rows of the members -> (n, 3) rows of the cluster, zeros for every other node."""
    out = np.zeros((n, 3), dtype=np.int64)
    out[M] = rows_c
    return out


def known_answer():
    """nodesorting_test.go:98-152 (TestAZAwareNodeSorting): its four nodes are the members — zone 0 holds free memory 1 + 2 + 1,
    zone 1 holds 1, so zone 1's node comes first.  Two non-members sit in zone 1 with memory 10 each: counted, they would put
    zone 0 first.  Their names interleave with the members'."""
    c = dict(alloc=[[1, 1, 0], [1, 2, 0], [2, 1, 0], [1, 1, 0], [1, 10, 0], [1, 10, 0]], node_flags=[CAND] * 6,
             name_rank=[1, 2, 4, 5, 0, 3], overhead=None, res_node=None, res_req=None, zone=[0, 0, 0, 1, 1, 1], n_zones=2,
             driver_label_rank=None, exec_label_rank=None)
    return c, [0, 1, 2, 3], [3, 0, 2, 1]


# ---- what the GPU tests of the feature share: the cluster generator, the install and build calls, the applications
GIB = 1 << 30


def cluster(seed, n, n_rr, n_zones, with_overhead=True, labels=False):
    """The generator of tests/test_snapshot_build.py (same shapes).  Name ranks are distinct, so every order is determined."""
    rng = np.random.default_rng(seed)
    shape = rng.integers(0, 4, size=n)
    alloc = np.stack([np.array([16, 32, 64, 96])[shape] * 1000, np.array([64, 128, 256, 384])[shape] * GIB,
                      np.where(rng.random(n) < 0.1, 8, 0)], axis=1).astype(np.int64)
    overhead = None
    if with_overhead:
        overhead = np.stack([rng.integers(0, 8, size=n) * 250, rng.integers(0, 16, size=n) * (GIB // 4),
                             np.zeros(n, dtype=np.int64)], axis=1).astype(np.int64)
    ks = rng.integers(1, 25, size=n_rr)
    res_node = rng.integers(0, n + 3, size=int(ks.sum())).astype(np.uint32)  # a few entries point outside the cluster
    res_req = np.stack([rng.choice([1000, 2000, 4000], size=len(res_node)), rng.choice([4, 8, 16], size=len(res_node)) * GIB,
                        (rng.random(len(res_node)) < 0.02).astype(np.int64)], axis=1).astype(np.int64).reshape(-1, 3)
    flags = (np.where(rng.random(n) < 0.05, ps.UNSCHEDULABLE, 0) | np.where(rng.random(n) < 0.95, ps.READY, 0) |
             np.where(rng.random(n) < 0.8, ps.DRIVER_CANDIDATE, 0)).astype(np.uint32)
    dl = el = None
    if labels:
        dl = rng.choice([0, 1, ps.UNRANKED], size=n).astype(np.uint32)
        el = rng.choice([0, 1, 2, ps.UNRANKED], size=n).astype(np.uint32)
    return dict(alloc=alloc, node_flags=flags, name_rank=rng.permutation(n).astype(np.uint32), overhead=overhead, res_node=res_node,
                res_req=res_req, zone=rng.integers(0, n_zones, size=n).astype(np.uint32), n_zones=n_zones, driver_label_rank=dl,
                exec_label_rank=el)


def install(ctx, c, resident):
    """gf_cluster_set of the whole cluster; resident: its reservation entries as resident usage sums."""
    ctx.set_cluster(c["alloc"], c["node_flags"], c["name_rank"], overhead=c["overhead"], zone=c["zone"], n_zones=c["n_zones"])
    if resident and c["res_node"] is not None and len(c["res_node"]):
        ctx.usage_apply(c["res_node"], c["res_req"], +1)


def build_set(ctx, c, members, resident, **kw):
    labels = dict(driver_label_rank=c["driver_label_rank"], exec_label_rank=c["exec_label_rank"])
    if resident:
        return ctx.build_snapshot_resident_set(members, resident_usage=True, **labels, **kw)
    return ctx.build_snapshot_resident_set(members, res_node=c["res_node"], res_req=c["res_req"], **labels, **kw)


def apps_for(m, tiny=False):
    if tiny:  # the known answer's nodes hold one or two units
        drv, exe, k = [[1, 1, 0]] * 4, [[1, 1, 0]] * 4, [1, 1, 2, 5]
    else:
        from gangfit import workloads as wl

        w = wl.config(2, n_nodes=16, n_apps=min(64, 4 * max(m, 1)))
        drv, exe, k = w.drv, w.exe, w.k
    ones = np.ones(len(k), dtype=np.uint32)
    import gangfit
    from oracle import binding as ob

    return gangfit.make_apps(drv, exe, k, ones), ob.make_apps(drv, exe, k, ones)
