"""What tests/snapshot_sets.py promises (no GPU): the compaction of a cluster to the members of a node set and the mapping back
to cluster indices — the reference gf_snapshot_build_resident_set is compared with."""
import numpy as np

import snapshot_sets as ss
from oracle import pysnapshot as ps

GIB = 1 << 30


def _cluster(seed, n, n_zones):
    rng = np.random.default_rng(seed)
    alloc = np.stack([rng.integers(1, 64, size=n) * 1000, rng.integers(1, 256, size=n) * GIB, rng.integers(0, 2, size=n) * 8], axis=1)
    overhead = np.stack([rng.integers(0, 4, size=n) * 250, rng.integers(0, 4, size=n) * (GIB // 4), np.zeros(n, dtype=np.int64)], axis=1)
    res_node = rng.integers(0, n + 3, size=3 * n).astype(np.uint32)
    res_req = np.stack([rng.choice([1000, 2000], size=3 * n), rng.choice([4, 8], size=3 * n) * GIB, np.zeros(3 * n, dtype=np.int64)], axis=1)
    flags = (np.where(rng.random(n) < 0.9, ps.READY, 0) | np.where(rng.random(n) < 0.8, ps.DRIVER_CANDIDATE, 0)).astype(np.uint32)
    return dict(alloc=alloc.astype(np.int64), node_flags=flags, name_rank=rng.permutation(n).astype(np.uint32),
                overhead=overhead.astype(np.int64), res_node=res_node, res_req=res_req.astype(np.int64),
                zone=rng.integers(0, n_zones, size=n).astype(np.uint32), n_zones=n_zones,
                driver_label_rank=rng.choice([0, 1, ps.UNRANKED], size=n).astype(np.uint32), exec_label_rank=None)


def test_full_set_is_the_cluster():
    for seed, n, nz in ((1, 1, 1), (2, 65, 3), (3, 300, 4)):
        c = _cluster(seed, n, nz)
        avail, sched, D, X = ps.build(**c)
        for members in (np.arange(n), np.ones(n, dtype=bool)):
            r = ss.build(c, members)
            assert np.array_equal(r.M, np.arange(n))
            assert np.array_equal(r.avail, avail) and np.array_equal(r.sched, sched)
            assert np.array_equal(r.D, D) and np.array_equal(r.X, X)
            assert np.array_equal(r.D_c, D) and np.array_equal(r.X_c, X)
            assert np.array_equal(r.inputs["name_rank"], c["name_rank"])


def test_known_answer_foreign_nodes_do_not_flip_the_zone_order():
    c, members, expected = ss.known_answer()
    r = ss.build(c, members)
    assert r.D.tolist() == expected and r.X.tolist() == expected
    assert r.inputs["name_rank"].tolist() == [0, 1, 2, 3]
    assert r.avail[4:].tolist() == [[0, 0, 0], [0, 0, 0]] and r.sched[4:].tolist() == [[0, 0, 0], [0, 0, 0]]
    # the precondition of the case: over every node zone 0 comes first
    _, _, D, _ = ps.build(**c)
    assert D.tolist()[:3] == [0, 2, 1] and D.tolist()[3:] != [3]


def test_compaction_keeps_only_what_names_a_member():
    c = _cluster(9, 130, 3)
    mask = np.zeros(130, dtype=bool)
    mask[[0, 5, 63, 64, 65, 129]] = True
    r = ss.build(c, mask)
    assert r.M.tolist() == [0, 5, 63, 64, 65, 129]
    inp = r.inputs
    assert sorted(inp["name_rank"].tolist()) == list(range(6))
    assert np.array_equal(np.argsort(inp["name_rank"]), np.argsort(c["name_rank"][r.M]))  # the same name order
    rn = c["res_node"].astype(np.int64)
    named = np.isin(rn, r.M)
    assert len(inp["res_node"]) == int(named.sum())
    assert np.array_equal(r.M[inp["res_node"].astype(np.int64)], rn[named]) and np.array_equal(inp["res_req"], c["res_req"][named])
    # usage of a member: every entry that names it, nothing else
    usage = np.zeros((130, 3), dtype=np.int64)
    np.add.at(usage, rn[rn < 130], c["res_req"][rn < 130])
    assert np.array_equal(r.avail[r.M], (c["alloc"] - usage - c["overhead"])[r.M])
    assert not r.avail[~mask].any() and not r.sched[~mask].any()
    assert set(r.D.tolist()) <= set(r.M.tolist()) and set(r.X.tolist()) <= set(r.M.tolist())
    # the mapping helpers
    assert ss.to_cluster(np.array([0, ss.NO_NODE, 5], dtype=np.uint32), r.M).tolist() == [0, ss.NO_NODE, 129]
    assert ss.rows_to_cluster(r.avail_c, r.M, 130).tolist() == r.avail.tolist()


def test_empty_set():
    r = ss.build(_cluster(4, 65, 2), [])
    assert len(r.M) == 0 and len(r.D) == 0 and len(r.X) == 0 and r.avail.shape == (65, 3) and not r.avail.any()
