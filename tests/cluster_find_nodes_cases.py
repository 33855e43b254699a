"""What gf_cluster_find_nodes must answer, from the CPU oracle alone: oracle.binding.find_nodes per instance-group row, on
A = allocatable - (usage + overhead) computed in numpy and O_q = the row's ready, schedulable nodes in ascending create_rank.

A helper module, not a test file; tests/test_cluster_find_nodes_cpu.py checks what it promises.

Rows of a case with sets are disjoint (the chained call refuses rows that overlap without being equal): the last few nodes of a
cluster of eight or more are never ready and form a row of their own, the other rows share out the nodes before them; every case
with sets also carries an empty row.  The family "none" passes no sets at all: every node of the cluster.
"""
import numpy as np

from oracle import binding as ob
from oracle import pysnapshot as ps

GIB = 1 << 30
NO = 0xFFFFFFFF
MAX_K = 1 << 20
FAMILIES = ("none", "one", "three", "eight")
NODE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 300)  # a step's edge, the edge of four steps in flight, an odd size
RANKS = ("identity", "reversed", "random")
BIG = 4161  # 65 full steps and one node: run once


def available(c):
    """A: (n, 3) allocatable - (usage + overhead), what the resident columns hold."""
    alloc = np.asarray(c["alloc"], dtype=np.int64)
    n = len(alloc)
    usage = np.zeros_like(alloc)
    rn = np.asarray(c["res_node"], dtype=np.int64)
    rr = np.asarray(c["res_req"], dtype=np.int64).reshape(-1, 3)
    inside = rn < n
    np.add.at(usage, rn[inside], rr[inside])
    return alloc - (usage + np.asarray(c["overhead"], dtype=np.int64))


def row_members(c, q):
    n = len(c["alloc"])
    return np.ones(n, dtype=bool) if c["sets"] is None else np.asarray(c["sets"][int(c["req_set"][q])], dtype=bool)


def order_of(c, member):
    """O: the members that are ready and not unschedulable, in ascending create_rank."""
    flags = np.asarray(c["flags"], dtype=np.uint32)
    ok = member & ((flags & ps.READY) != 0) & ((flags & ps.UNSCHEDULABLE) == 0)
    idx = np.nonzero(ok)[0]
    return idx[np.argsort(np.asarray(c["create_rank"])[idx], kind="stable")].astype(np.uint32)


def groups(c):
    """[(member row, [q ...])]: the requests by the CONTENT of their row, ascending q inside a group, groups by first q."""
    out, at = [], {}
    for q in range(len(c["k"])):
        m = row_members(c, q)
        key = m.tobytes()
        if key not in at:
            at[key] = len(out)
            out.append((m, []))
        out[at[key]][1].append(q)
    return out


def expected(c, chained=True):
    """dict(placed, last, off, exec_nodes, adds, residual) — what Context.cluster_find_nodes(..., want_adds=True,
    want_residual=True) returns, from oracle.find_nodes on every group's own order."""
    A = available(c)
    n = len(A)
    exe = np.asarray(c["exe"], dtype=np.int64).reshape(-1, 3)
    k = np.asarray(c["k"], dtype=np.int32)
    R = len(k)
    off = np.zeros(R, dtype=np.uint64)
    off[1:] = np.cumsum(k[:-1].astype(np.int64)).astype(np.uint64)
    placed = np.zeros(R, dtype=np.uint32)
    last = np.full(R, NO, dtype=np.uint32)
    adds = np.zeros((R, n), dtype=np.uint32)
    nodes = np.zeros(int(k.astype(np.int64).sum()), dtype=np.uint32)
    work = A.copy()
    for member, qs in groups(c):
        O = order_of(c, member)
        if len(O) == 0:
            continue  # nothing to visit: no placement, no entry
        r = ob.find_nodes(work, exe[qs], k[qs], O, chained=chained)
        for i, q in enumerate(qs):
            placed[q] = r.placed[i]
            adds[q] = r.adds[i]
            p = r.placement(i)
            nodes[int(off[q]):int(off[q]) + len(p)] = p
            hit = O[r.adds[i][O] > 0]
            if len(hit):
                last[q] = hit[-1]  # every visited node is charged at least one add
        if chained:
            work = r.avail_after  # (the groups share no node: the order among them does not matter)
    return dict(placed=placed, last=last, off=off, exec_nodes=nodes, adds=adds, residual=work if chained else A)


def row_capacity(A, O, exe):
    """Executors of size exe the nodes of O hold on table A; None when the request is all zeros (every node holds any count)."""
    exe = np.asarray(exe, dtype=np.int64)
    if not exe.any():
        return None
    total = 0
    for node in O:
        a = A[node]
        if (a < 0).any():
            continue
        total += int(min(int(a[j]) // int(exe[j]) for j in range(3) if exe[j] > 0))
    return total


def cluster(seed, n):
    rng = np.random.default_rng(seed)
    alloc = np.stack([rng.choice([4000, 8000, 16000], size=n), rng.choice([8, 16, 32], size=n) * GIB,
                      rng.choice([0, 0, 1, 4], size=n)], axis=1).astype(np.int64)
    over = np.stack([rng.integers(0, 4, size=n) * 250, rng.integers(0, 5, size=n) * (GIB // 4), np.zeros(n, dtype=np.int64)],
                    axis=1).astype(np.int64)
    over[rng.random(n) < 0.2] = 0
    too_much = rng.random(n) < 0.06
    over[too_much, 0] = alloc[too_much, 0] + 1000  # negative available cpu: capacity 0, still visited and charged
    n_res = int(rng.integers(n, 2 * n + 2))
    res_node = rng.integers(0, n, size=n_res).astype(np.uint32)
    res_req = np.stack([rng.choice([0, 500, 1000], size=n_res), rng.choice([0, GIB // 2, GIB], size=n_res),
                        rng.choice([0, 0, 0, 1], size=n_res)], axis=1).astype(np.int64)
    flags = (np.where(rng.random(n) < 0.85, ps.READY, 0) | np.where(rng.random(n) < 0.5, ps.DRIVER_CANDIDATE, 0) |
             np.where(rng.random(n) < 0.08, ps.UNSCHEDULABLE, 0)).astype(np.uint32)
    flags[0] = ps.READY
    if n > 1:  # one ready node with a negative available value in every cluster
        flags[1] = ps.READY
        over[1, 0] = alloc[1, 0] + 1000
    return dict(alloc=alloc, overhead=over, flags=flags, name_rank=rng.permutation(n).astype(np.uint32), res_node=res_node,
                res_req=res_req)


def rows_of(family, n, flags):
    """(sets or None, the rows requests should name, index of the empty row, index of the row without a ready node)."""
    if family == "none":
        return None, [0], None, None
    dead = 3 if n >= 8 else 0
    live = n - dead
    flags[live:] &= ~np.uint32(ps.READY)
    idx = np.arange(live)
    if family == "one":
        parts = [idx]
    elif family == "three":
        parts = [idx[: live // 3], idx[live // 3: 2 * live // 3], idx[2 * live // 3:]]
    elif family == "eight":
        parts = [idx[idx % 8 == r] for r in range(8)]
    else:
        raise ValueError(family)
    sets = np.zeros((len(parts) + 2, n), dtype=bool)
    for r, p in enumerate(parts):
        sets[r, p] = True
    sets[len(parts) + 1, live:] = True  # no ready node (empty as well when n < 8)
    return sets, list(range(len(parts))), len(parts), len(parts) + 1


def create_rank(kind, n, seed):
    if kind == "identity":
        return np.arange(n, dtype=np.uint32)
    if kind == "reversed":
        return np.arange(n, dtype=np.uint32)[::-1].copy()
    return np.random.default_rng(seed + 5).permutation(n).astype(np.uint32)


KINDS = ("cap", "one", "cap1", "zero", "small", "one", "small", "cap", "small", "one", "cap1", "small")


def case(family, n, rank_kind, seed=None, max_per_row=12):
    """One cluster with its rows, create_rank and requests: 1-12 requests per row, interleaved across rows in q; k = 0, 1, the
    row's capacity, the capacity + 1 and small counts; zero dimensions and gpu-only requests."""
    seed = 100000 * FAMILIES.index(family) + 100 * n + RANKS.index(rank_kind) if seed is None else seed
    rng = np.random.default_rng(seed + 1)
    c = cluster(seed, n)
    sets, named, empty_row, dead_row = rows_of(family, n, c["flags"])
    c.update(sets=sets, create_rank=create_rank(rank_kind, n, seed))
    per_row = [int(rng.integers(1, max_per_row + 1)) for _ in named]
    per_row[0] = max(per_row[0], min(6, max_per_row))  # the first row holds at least one request of every kind
    req_set = np.concatenate([np.full(m, r, dtype=np.uint32) for r, m in zip(named, per_row)])
    if sets is not None:
        req_set = np.concatenate([req_set, np.array([empty_row, dead_row, empty_row], dtype=np.uint32)])
    req_set = req_set[rng.permutation(len(req_set))]
    R = len(req_set)
    exe = np.stack([rng.choice([0, 250, 1000, 3000], size=R), rng.choice([0, GIB, 6 * GIB], size=R),
                    rng.choice([0, 0, 1], size=R)], axis=1).astype(np.int64)
    seen, kinds = {}, []
    for q in range(R):  # the j-th request of a row: its kind of count, the rows out of step with each other
        row = 0 if sets is None else int(req_set[q])
        j = seen.get(row, 0)
        seen[row] = j + 1
        kinds.append(KINDS[(j + row) % len(KINDS)])
    special = {"one": [0, 0, 1],       # gpu only
               "cap": [1000, GIB, 0],
               "cap1": [250, 0, 0],    # a zero dimension
               "small": [0, 0, 0]}     # every dimension zero: a node that is not negative holds any count
    for kind, e in special.items():
        if kind in kinds:
            exe[kinds.index(kind)] = e
    c.update(req_set=None if sets is None else req_set, exe=exe, k=np.zeros(R, dtype=np.int32))
    A = available(c)
    k = np.zeros(R, dtype=np.int32)
    for q in range(R):
        kind = kinds[q]
        cap = row_capacity(A, order_of(c, row_members(c, q)), exe[q])
        small = int(rng.integers(2, 9))
        if kind == "zero":
            k[q] = 0
        elif kind == "one":
            k[q] = 1
        elif kind == "small" or cap is None:
            k[q] = small
        else:
            k[q] = min(cap + (1 if kind == "cap1" else 0), MAX_K)
    c["k"] = k
    return c


def case_k_max():
    """k = GF_MAX_K with an all-zero request: every capacity clamps at K, the first node of the order that is not negative takes
    them all; a second request of the row follows it."""
    c = case("one", 65, "random", seed=77, max_per_row=2)
    c["req_set"][0] = 0
    c["exe"][0] = [0, 0, 0]
    c["k"][0] = MAX_K
    return c


def case_big():
    return case("eight", BIG, "random", seed=4161, max_per_row=3)


def kinds_present(c):
    """Which kinds of request the case holds, from the oracle's answers alone."""
    A = available(c)
    plain, chain = expected(c, chained=False), expected(c, chained=True)
    k = np.asarray(c["k"])
    out = set()
    for q in range(len(k)):
        a = plain["adds"][q].astype(np.int64)
        mult = np.bincount(plain["exec_nodes"][int(plain["off"][q]):int(plain["off"][q]) + int(plain["placed"][q])],
                           minlength=len(A)).astype(np.int64)
        if k[q] > 0 and plain["placed"][q] == k[q]:
            out.add("filled")
        if plain["placed"][q] < k[q]:
            out.add("partial")
        if ((a > 0) & (a == mult + 1)).any():
            out.add("over-add")
        if ((a > 0) & (A < 0).any(axis=1)).any():
            out.add("negative")
        lo, hi = int(plain["off"][q]), int(plain["off"][q]) + int(k[q])
        if (plain["placed"][q] != chain["placed"][q] or not np.array_equal(plain["adds"][q], chain["adds"][q])
                or not np.array_equal(plain["exec_nodes"][lo:hi], chain["exec_nodes"][lo:hi])):
            out.add("chained differs")
    return out


ALL_KINDS = {"filled", "partial", "over-add", "negative", "chained differs"}
