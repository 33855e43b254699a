"""Problems whose decisions fall behind chunk group zero of the priority orders (a chunk is 64 slots, a group 64 chunks = 4 096
slots), in the shape of tests/magnitudes.py: (avail, sched, zone, D, X, drv, exe, k, flags) plus a dict that names
the boundary, the positions and the designated gangs.

A helper module, not a test file.  Every problem is a "hollow front": the first p positions of both orders decide nothing (or
only what the front's name says), so drivers and executors are found at position p and behind, with p on either side of a group
boundary: 4 095, 4 096, 4 097 and, at 8 400 nodes, 8 191, 8 192, 8 193.  "Position" is the position in the order; on the merged
and identical layouts that is the slot (positions() restates gangfit_slot_layout.h's merge: unknown names and a repeated driver
candidate take no slot).  tests/test_deep_orders_cpu.py checks that every front still reaches what it is named for.

  cleared          every front node below every request in cpu and memory, some negative: the chunk maxima rule out group 0.
  stale            the maxima admit every front chunk (cpu, memory and gpu each large on a different node of the chunk), no node fits.
  drivers-front    small drivers fit front nodes, executors do not: the driver in group 0, the pack behind p.
  executors-front  front slots are executor-only (merged layout): the driver's slot >= p, executors in group 0; the early front
                   chunks host small executors only, the last front chunk every shape.
  straddle         capacities of exactly 1, 1, 2 at p-3 .. p-1 and 3 at p for one request shape: gangs that reach K-1 at p-1 and K
                   at p, that end on p-1, that need the whole order, and one executor more (tightly-pack's run and
                   distribute-evenly's second pass).
  fallback         a gang of exactly the order's capacity: every driver on the 70 positions from p takes one executor's room of
                   its node, the first that does not sits in a later chunk; with a larger driver request none works.
  gpu-gangs        gpu executors, gpu nodes a minority: all in group 0 with drivers that only fit behind p, or all behind p.
  draining         (FIFO) a front of exactly the one-unit nodes the first 14 applications of a chain use up, the last at p-1.

Where more than 300 nodes lie behind p, only the first and the last 150 of them have room (LIVE): what the first ones cannot
hold is found in the last group, and the literal oracle's retry loops stay short.  Every batch has 40 applications; application
36 (LAST) fits nowhere and is the only one that is not skippable, so every FIFO chain ends there: behind its first deep
decision, behind skipped applications, and behind the checkpoint at 32 a second chain resumes from.
"""
import numpy as np

GROUP = 4096
LIVE = 150  # nodes with room right behind p and at the end of the order, when more than twice as many lie behind p
CPU, GIB = 1000, 1 << 30
UNKNOWN = (20000, 30000)  # names outside the metadata
FRONTS = ("cleared", "stale", "drivers-front", "executors-front", "straddle", "fallback", "gpu-gangs", "draining")
LAYOUTS = {"cleared": ("merged", "identical", "general"), "stale": ("merged", "identical"),
           "drivers-front": ("merged", "identical"), "executors-front": ("merged",),
           "straddle": ("merged", "identical", "general"), "fallback": ("merged", "identical"),
           "gpu-gangs": ("merged", "identical"), "draining": ("merged", "identical")}
ZONE_IDS = (3, 10, 17)  # wholly in the front, wholly behind p, mixed
# (n, p): 4 300 nodes are 68 chunks in two groups with a ragged last chunk, 8 400 nodes 132 chunks in three groups
BOUNDS = tuple((4300, p) for p in (4095, 4096, 4097)) + tuple((8400, p) for p in (4095, 4096, 4097, 8191, 8192, 8193))
# the one request shape of the straddle and fallback gangs
STRADDLE_DRV, STRADDLE_EXE = (500, GIB, 0), (3 * CPU, 8 * GIB, 0)
FALLBACK_DRV, FALLBACK_DRV_NONE, FALLBACK_EXE = (CPU, GIB, 0), (2 * CPU, 2 * GIB, 0), (2 * CPU, 8 * GIB, 0)
LAST = 36  # the application every FIFO chain ends at
UNIT = (CPU, GIB, 0)  # draining: drivers and executors alike


def positions(n, D, X, layout):
    """(dpos, xpos): per node its position in the driver / executor order as the kernels count them, -1 when absent.  Merged and
    identical: the slot of the merged order of the cleaned orders; general: the raw positions (first occurrence)."""
    dpos, xpos = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    if layout == "general":
        for i in range(len(D) - 1, -1, -1):
            if D[i] < n:
                dpos[D[i]] = i
        for i, v in enumerate(X):
            if v < n:
                xpos[v] = i
        return dpos, xpos
    xs = [int(v) for v in X if v < n]
    ds, seen = [], set()
    for v in D:
        if v < n and int(v) not in seen:
            seen.add(int(v))
            ds.append(int(v))
    in_x = set(xs)
    i = j = s = 0
    while i < len(ds) or j < len(xs):
        if i < len(ds) and j < len(xs) and ds[i] == xs[j]:
            dpos[ds[i]] = xpos[xs[j]] = s
            i, j = i + 1, j + 1
        elif i < len(ds) and ds[i] not in in_x:
            dpos[ds[i]] = s
            i += 1
        elif j < len(xs) and xs[j] not in seen:
            xpos[xs[j]] = s
            j += 1
        else:
            raise ValueError("the orders do not merge")
        s += 1
    return dpos, xpos


def _orders(rng, n, p, layout, keep, front_d=True, rear_single=True):
    """seq: node of position (the executor order's, and on the merged and identical layouts the slot's).  keep: positions that
    stay candidates of both orders.  front_d False: no front position is a driver candidate."""
    seq = rng.permutation(n).astype(np.int64)
    if layout == "identical":
        return seq, seq.astype(np.uint32), seq.astype(np.uint32)
    pos = np.arange(n)
    free = np.ones(n, dtype=bool)
    free[[q for q in keep if 0 <= q < n]] = False
    free[max(p - 2, 0):p + 2] = False  # a run of one-order slots must not carry a node across the boundary
    if layout == "merged":
        single = free & (rng.random(n) < 0.2) & (rear_single | (pos < p))
        d_only = single & (rng.random(n) < 0.5)
        is_d, is_x = ~(single & ~d_only), ~d_only
        if not front_d:
            is_d, is_x = is_d & (pos >= p), is_x | (pos < p)
        X, D = seq[is_x], seq[is_d]
        X = np.insert(X, int(rng.integers(0, len(X) + 1)), UNKNOWN[0])
        D = np.append(np.insert(D, int(rng.integers(0, len(D) + 1)), UNKNOWN[1]), D[0])  # a repeated driver candidate
        return seq, D.astype(np.uint32), X.astype(np.uint32)
    # general: the front is the same set of nodes in both orders, in another order; an unknown name holds one front position
    # of each, and three repeated candidates make the driver positions outnumber the slots
    fq = np.nonzero(free[:p])[0]
    u, v, w = (int(q) for q in rng.choice(fq, 3, replace=False))
    X = seq.copy()
    X[u] = UNKNOWN[0]  # node seq[u] is driver-only
    front = [int(seq[q]) for q in rng.permutation(p)]
    for q in sorted(keep):  # the designated front nodes keep their relative order, and come first
        if 0 <= q < p:
            front.remove(int(seq[q]))
    front = [int(seq[q]) for q in sorted(keep) if 0 <= q < p] + front
    front[front.index(int(seq[v]))] = UNKNOWN[1]  # node seq[v] is executor-only
    front[front.index(int(seq[w]))] = front[-1] if front[-1] != int(seq[w]) else front[-2]  # a repeat inside the front
    rear = [int(seq[p])] + [int(q) for q in rng.permutation(seq[p + 1:])]
    D = np.array(front + rear + [front[0], rear[0], rear[-1]], dtype=np.int64)
    return seq, D.astype(np.uint32), X.astype(np.uint32)


def _hollow(rng, m):
    """Nodes below every request: at most half a core, no memory; some negative."""
    return np.stack([rng.integers(-2, 1, size=m) * CPU + rng.choice([0, 250, 500], size=m), rng.integers(-4, 1, size=m) * GIB,
                     rng.integers(-1, 1, size=m)], axis=1).astype(np.int64)


def _rich(rng, m):
    return np.stack([rng.integers(4, 33, size=m) * CPU, rng.integers(16, 129, size=m) * GIB, np.zeros(m, dtype=np.int64)],
                    axis=1).astype(np.int64)


def _gangs(rng, a, drv_cpu=(1, 3), drv_mem=(1, 5), exe_cpu=(1, 5), exe_mem=(2, 17), kmax=60):
    """a applications, most of which fit a cluster of rich nodes; three cannot (an executor no node holds, a driver no node
    holds, both), wherever they are looked for."""
    drv = np.stack([rng.integers(*drv_cpu, size=a) * CPU, rng.integers(*drv_mem, size=a) * GIB, np.zeros(a, dtype=np.int64)],
                   axis=1).astype(np.int64)
    exe = np.stack([rng.integers(*exe_cpu, size=a) * CPU, rng.integers(*exe_mem, size=a) * GIB, np.zeros(a, dtype=np.int64)],
                   axis=1).astype(np.int64)
    k = rng.integers(0, kmax + 1, size=a).astype(np.int32)
    k[rng.integers(0, a)] = 0
    i, j, l = (int(q) for q in rng.choice(np.arange(2, 30), 3, replace=False))
    exe[i, 1], k[i] = 1024 * GIB, 3
    drv[j, 0] = 512 * CPU
    drv[l, 1], exe[l, 0], k[l] = 1024 * GIB, 512 * CPU, 2
    return drv, exe, k, [i, j, l]


def _cap(avail, e):
    """Executors of request e a node holds (capacity.go: a dimension the request leaves at 0 does not bound it)."""
    c = np.full(len(avail), 1 << 40, dtype=np.int64)
    for j in range(3):
        if e[j] > 0:
            c = np.minimum(c, np.where(avail[:, j] >= 0, avail[:, j] // e[j], 0))
        else:
            c = np.where(avail[:, j] < 0, 0, c)
    return c


def problem(front, n, p, layout="merged", n_zones=1, seed=0, variant=0, a=40, bytes_grained=False):
    """One hollow-front problem.  Returns ((avail, sched, zone, D, X, drv, exe, k, flags), info); info holds n, p, layout,
    dpos / xpos (positions per node), infeasible (gangs that fit nowhere), and the front's designated gangs."""
    assert front in FRONTS and layout in LAYOUTS[front] and 4 < p < n - 150 and a > LAST + 2
    rng = np.random.default_rng([seed, FRONTS.index(front), n, p, n_zones, variant, ("merged", "identical", "general").index(layout)])
    info = {"front": front, "n": n, "p": p, "layout": layout, "n_zones": n_zones, "variant": variant}
    keep = {p}
    if front == "straddle":
        keep |= {1, p - 3, p - 2, p - 1}
    if front == "fallback":
        keep |= set(range(p, p + 71))
    if front == "stale":
        keep |= set(range(1, p - 2, 64)) | set(range(2, p - 2, 64)) | set(range(3, p - 2, 64))
    if front == "draining":
        keep |= set(_drain_positions(p))
    seq, D, X = _orders(rng, n, p, layout, keep, front_d=front != "executors-front", rear_single=front != "fallback")
    at = np.zeros((n, 3), dtype=np.int64)  # availability by position
    at[:p], at[p:] = _hollow(rng, p), _rich(rng, n - p)
    if n - p > 2 * LIVE:  # a hollow middle: what the first nodes behind p cannot hold is found in the last group
        at[p + LIVE:n - LIVE] = _hollow(rng, n - p - 2 * LIVE)
    rear = np.concatenate([np.arange(p, min(p + LIVE, n)), np.arange(max(n - LIVE, p + LIVE), n)])
    at[p] = [64 * CPU, 256 * GIB, 0]  # the first node behind the front holds every shape
    flags = np.ones(a, dtype=np.uint32)
    if front == "cleared":
        drv, exe, k, bad = _gangs(rng, a)
    elif front == "stale":
        drv, exe, k, bad = _gangs(rng, a)
        for j, (col, big) in enumerate(((0, 64 * CPU), (1, 512 * GIB), (2, 8))):
            q = np.arange(1 + j, p - 2, 64)
            at[q] = 0
            at[q, col] = big
        exe[::5, 2] = 1  # gpu executors: that column's maxima decide too; twenty nodes right behind p have gpus, not the one at p
        at[p + 1:p + 60:3, 2] = 4
    elif front == "drivers-front":
        drv, exe, k, bad = _gangs(rng, a, drv_cpu=(1, 2), drv_mem=(1, 3), exe_cpu=(2, 5))
        at[:p:40] = [CPU + 250, 2 * GIB, 0]
        at[p - 1] = [CPU, 2 * GIB, 0]
        big = [q for q in range(3, a, 7) if q not in bad]
        drv[big, 0] = 2 * CPU  # these drivers fit no front node
        info["front_drivers"] = [q for q in range(a) if q not in bad and q not in big]
    elif front == "executors-front":
        drv, exe, k, bad = _gangs(rng, a)
        at[:p] = [2 * CPU, 4 * GIB, 0]  # the early chunks host the small shapes only
        at[:p:5] = _hollow(rng, len(at[:p:5]))
        last = (p - 1) // 64 * 64  # ... the last front chunk every shape
        at[last:p] = _rich(rng, p - last)
        small = [q for q in range(0, a, 2) if q not in bad]
        exe[small, 0], exe[small, 1] = rng.integers(1, 3, size=len(small)) * CPU, rng.integers(2, 5, size=len(small)) * GIB
        big = [q for q in range(1, a, 2) if q not in bad][0]  # the last front chunk, the node at p, and one executor more
        exe[big] = [4 * CPU, 16 * GIB, 0]
        k[big] = int(_cap(at[last:p + 1], exe[big]).sum()) + 1
        info["spill"] = big
        info["last_chunk_gangs"] = [q for q in range(a) if q not in bad and q not in small and k[q] > 0 and
                                    (exe[q, 0] > 2 * CPU or exe[q, 1] > 4 * GIB)]
    elif front == "straddle":
        drv, exe, k, bad = _gangs(rng, a)
        e = np.array(STRADDLE_EXE)
        at[rear[1:], 0] += rng.integers(0, 3, size=len(rear) - 1) * 250  # capacities that are no exact multiples, either
        at[1] = STRADDLE_DRV  # the designated gangs' driver node: it holds their driver and nothing else
        for q, c in ((p - 3, 1), (p - 2, 1), (p - 1, 2), (p, 3)):
            at[q] = e * c
        cap = _cap(at, e)
        cap[[int(q) for q in np.nonzero(~np.isin(seq, X))[0]]] = 0  # driver-only positions hold no executor
        total, holders = int(cap.sum()), int((cap > 0).sum())
        want = {"cross": 5, "end": 4, "whole": total, "over": total + 1, "even_cross": holders + 2, "even_end": holders + 1}
        free = [q for q in range(2, a) if q not in bad][:len(want)]
        info["designated"] = {}
        for (name, kk), q in zip(want.items(), free):
            drv[q], exe[q], k[q] = STRADDLE_DRV, STRADDLE_EXE, kk
            info["designated"][name] = q
        info["holders"], info["total"] = holders, total
    elif front == "fallback":
        drv, exe, k, bad = _gangs(rng, a)
        m = len(rear)
        c = rng.integers(1, 9, size=m)
        slack = rng.random(m) < 0.5
        slack[:70], slack[70] = False, True
        at[rear, 0] = c * 2 * CPU + slack * CPU  # exact nodes lose one executor's room to a driver of one core; slack ones to one of two
        at[rear, 1] = (c + 1 + rng.integers(0, 3, size=m)) * 8 * GIB + GIB
        cap = _cap(at, np.array(FALLBACK_EXE))
        assert int(cap[:p].sum()) == 0 and np.array_equal(cap[rear], c) and int(cap.sum()) == int(c.sum())
        total = int(cap.sum())
        g1, g2 = [q for q in range(2, a) if q not in bad][:2]
        drv[g1], exe[g1], k[g1] = FALLBACK_DRV, FALLBACK_EXE, total
        drv[g2], exe[g2], k[g2] = FALLBACK_DRV_NONE, FALLBACK_EXE, total
        info["designated"] = {"later_driver": g1, "no_driver": g2}
        info["total"] = total
    elif front == "gpu-gangs":
        drv, exe, k, bad = _gangs(rng, a, drv_mem=(40, 49), exe_cpu=(1, 3), exe_mem=(2, 5), kmax=40)
        gg = [q for q in range(a) if q % 3 != 2 and q not in bad]
        exe[gg, 2] = rng.integers(1, 3, size=len(gg))
        at[rear[1:], 1] = np.maximum(at[rear[1:], 1], rng.integers(40, 129, size=len(rear) - 1) * GIB)
        if variant == 0:  # the gpu nodes all in group 0, too small for any driver
            q = rng.choice(np.arange(2, min(p, GROUP) - 2), n // 12, replace=False)
            at[q] = np.stack([rng.integers(8, 33, size=len(q)) * CPU, rng.integers(16, 33, size=len(q)) * GIB,
                              rng.integers(1, 9, size=len(q))], axis=1)
        else:  # ... all behind p, the first of them at p
            q = np.concatenate([[p], rng.choice(rear[1:], 100, replace=False)])
            at[q, 2] = rng.integers(2, 9, size=len(q))
        at[p + 1] = [96 * CPU, 256 * GIB, at[p + 1, 2]]  # the only node of one gang's driver, whatever p is behind group 0
        drv[gg[0], 0] = 80 * CPU
        info["gpu_gangs"], info["gpu_positions"], info["second_driver"] = gg, np.sort(q), gg[0]
    elif front == "draining":
        drv, exe, k = np.tile(UNIT, (a, 1)).astype(np.int64), np.tile(UNIT, (a, 1)).astype(np.int64), rng.integers(3, 13, size=a).astype(np.int32)
        m = len(DRAIN_K)  # the first application that finds the front used up
        k[:m] = DRAIN_K
        # a chain charges a node one executor however many it placed there (sparkResourceUsage is a map by node name): the
        # front is exact only with nodes of one unit each, one per driver and executor of the first m applications
        units = int(sum(DRAIN_K) + m)
        at[_drain_positions(p)] = UNIT
        k[20] = units + 70  # alone, it needs the whole front and seventy places behind it: more than the node at p holds
        exe[25, 1], k[25] = 1024 * GIB, 2  # skippable, fits nowhere
        bad = [25]
        info["first_behind"], info["front_units"] = m, units
    # every chain ends at application 36, which is not skippable and fits nowhere: behind the first deep decision, and behind
    # the checkpoint a chain of forty leaves at 32
    exe[LAST, 1], k[LAST], flags[LAST] = 1024 * GIB, 2, 0
    info["failed_at"] = LAST
    info["infeasible"] = sorted(bad + [LAST])
    if bytes_grained:  # two front nodes one and two bytes of memory: the table's memory unit is the byte
        q = [s for s in range(5, p) if at[s, 1] <= 0 and s not in keep][:2]
        at[q[0], 1], at[q[1], 1] = 1, 2
    avail = np.zeros((n, 3), dtype=np.int64)
    avail[seq] = at
    sched = np.maximum(avail, 0) + np.stack([rng.integers(0, 9, size=n) * CPU, rng.integers(0, 65, size=n) * GIB,
                                             rng.integers(0, 2, size=n)], axis=1)
    sched[rng.random(n) < 0.02] = 0
    zone = np.full(n, ZONE_IDS[0], dtype=np.uint32)
    if n_zones == 3:
        zs = np.where(np.arange(n) < p, np.where(rng.random(n) < 0.5, ZONE_IDS[0], ZONE_IDS[2]),
                      np.where(rng.random(n) < 0.5, ZONE_IDS[1], ZONE_IDS[2]))
        zs[p] = ZONE_IDS[1]
        zone[seq] = zs
    info["dpos"], info["xpos"] = positions(n, D, X, layout)
    info["seq"] = seq
    return (avail, sched, zone, D, X, drv, exe, k, flags), info


DRAIN_K = tuple(3 + (5 * i) % 10 for i in range(14))


def _drain_positions(p):
    """One front position per driver and executor of the draining applications, the last one p-1."""
    return [int(q) for q in np.linspace(40, p - 1, sum(DRAIN_K) + len(DRAIN_K)).astype(np.int64)]


def cases(front, seed=0, sizes=(4300, 8400)):
    """Every boundary of every size once, the front's layouts and one / three zones taken in turn (gpu: its two placements
    too).  Returns [(name, problem tuple, info)]."""
    out = []
    for i, (n, p) in enumerate(b for b in BOUNDS if b[0] in sizes):
        layout = LAYOUTS[front][i % len(LAYOUTS[front])]
        nz = (1, 3)[(i // len(LAYOUTS[front]) + i % len(LAYOUTS[front])) % 2]
        variant = (i // 2) % 2 if front == "gpu-gangs" else 0
        prob, info = problem(front, n, p, layout, nz, seed, variant)
        out.append((f"{front}/n{n}/p{p}/{layout}/{nz}z" + (f"/v{variant}" if front == "gpu-gangs" else ""), prob, info))
    return out


# ------------------------------------------------------------------------------------- single executors and findNodes


def executor_cases(n, p, seed=0):
    """gf_executor_fit at boundary p of an identical order over n nodes: (avail, X, node_zone, requests, hosts, reserved, what).
    Requests 0..2 fit first at p-1, p, p+1.  Requests 3..5 are minimal-fragmentation questions, each over the capacities of a
    node family of its own (cpu-only, memory-only, gpu-only nodes and requests): the smallest capacity sits behind p; an
    equal-capacity twin in an earlier group must win; a node behind p hosts the application against smaller capacities in
    group 0.  what["answers"]: the position each request's answer sits at, plain / zoned / reserved.  Zone 1 is everything from
    p on: a zone filter that removes group 0.  `reserved` moves request 1 to p+1 and takes the twin in group 0 away."""
    rng = np.random.default_rng([seed, n, p])
    X = rng.permutation(n).astype(np.uint32)
    at = _hollow(rng, n)
    at[p - 1], at[p], at[p + 1] = [500, GIB, 0], [500, 2 * GIB, 0], [500, 3 * GIB, 0]
    shapes = np.array([[500, GIB, 0], [500, 2 * GIB, 0], [500, 3 * GIB, 0], [CPU, 0, 0], [0, 8 * GIB, 0], [0, 0, 1]], dtype=np.int64)
    for q, c in ((70, 3), (300, 4), (p + 5, 2), (p + 90, 5), (p + 130, 2)):  # the twin of p+5 lies behind it
        at[q] = [c * CPU, 0, 0]
    for q, c in ((71, 2), (p + 6, 2), (p + 91, 3)):
        at[q] = [0, c * 8 * GIB, 0]
    for q, c in ((72, 1), (301, 1), (p + 92, 3)):
        at[q] = [0, 0, c]
    hosts = np.zeros((len(shapes), n), dtype=bool)
    hosts[5, X[p + 92]] = True
    reserved = np.zeros((n, 3), dtype=np.int64)
    reserved[X[p]] = [0, GIB, 0]
    reserved[X[71]] = [0, 16 * GIB, 0]
    what = {"first_fit": {0: p - 1, 1: p, 2: p + 1}, "first_fit_reserved": {0: p - 1, 1: p + 1, 2: p + 1},
            "min_frag": {3: p + 5, 4: 71, 5: p + 92}, "min_frag_zoned": {3: p + 5, 4: p + 6, 5: p + 92},
            "min_frag_reserved": {3: p + 5, 4: p + 6, 5: p + 92}}
    avail = np.zeros((n, 3), dtype=np.int64)
    avail[X] = at
    node_zone = np.zeros(n, dtype=np.uint32)
    node_zone[X[p:]] = 1
    return avail, X, node_zone, shapes, hosts, reserved, what


def find_nodes_cases(n, p, seed=0):
    """gf_find_nodes on an identical order whose first p positions hold nothing (each is still visited and charged one add):
    (avail, X, exe, k, what).  Requests of one shape each reach K on position p-1 (a node put there for it), p and p+1; at
    n = 4 370 — 69 chunks, no multiple of the 4-chunk batches — the last request ends in the last, ragged chunk."""
    rng = np.random.default_rng([seed, n, p, 1])
    X = rng.permutation(n).astype(np.uint32)
    at = _hollow(rng, n)
    at[:, 2] = 0
    at[p - 1] = [2 * CPU, 64 * GIB, 0]
    at[p] = [6 * CPU, 64 * GIB, 0]
    at[p + 1] = [8 * CPU, 64 * GIB, 0]
    at[n - 3] = [4 * CPU, 64 * GIB, 0]
    exe = np.array([[2 * CPU, GIB, 0], [3 * CPU, GIB, 0], [4 * CPU, GIB, 0], [CPU, GIB, 0], [CPU, GIB, 0]], dtype=np.int64)
    # unchained, on the full table: shape 0 holds 1 at p-1, 3 at p, 4 at p+1, 2 at n-3; shape 1: 0, 2, 2, 1; shape 2: 0, 1, 2, 1
    k = np.array([1, 2, 2, 20, 21], dtype=np.int32)  # one core: 2 + 6 + 8 + 4 = 20 places, the 20th on n-3; 21 are one too many
    what = {"ends_at": {0: p - 1, 1: p, 2: p + 1, 3: n - 3}, "short": 4}
    avail = np.zeros((n, 3), dtype=np.int64)
    avail[X] = at
    return avail, X, exe, k, what


# ------------------------------------------------------------------------------------------------ the oracle's answers


def references(case_list, closed_form=False, algos=(0, 1, 2, 3, 4, 5), workers=8, modes=(False, True)):
    """{case name: {algo: (independent batch, FIFO chain)}} from the oracle, for cases() entries (None for a mode that was not
    asked for).  closed_form: a truth value, or a function of the case name.  The calls are independent and the library runs without the interpreter's lock: a few threads share them."""
    from concurrent.futures import ThreadPoolExecutor

    from oracle import binding as ob

    ob.lib()

    def one(task):
        name, (avail, sched, zone, D, X, drv, exe, k, flags), algo, fifo = task
        apps = ob.make_apps(drv, exe, k, flags)
        fn = ob.fit_fifo_chain if fifo else ob.fit_independent
        closed = closed_form(name) if callable(closed_form) else closed_form
        return name, algo, fifo, fn(algo, avail, apps, D, X, closed_form=closed, sched=sched, zone=zone)

    tasks = [(name, p, algo, fifo) for name, p, _ in case_list for algo in algos for fifo in modes]
    out = {name: {algo: [None, None] for algo in algos} for name, _, _ in case_list}
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for name, algo, fifo, ref in pool.map(one, tasks):
            out[name][algo][int(fifo)] = ref
    return {name: {algo: tuple(v) for algo, v in refs.items()} for name, refs in out.items()}


def tightly_pack_model(avail, D, X, drv, exe, k, d_visible=None, x_visible=None):
    """One tightly-pack decision (binpack.go:60-87 over pack_tightly.go:34-63) in closed form, numpy only: capacities, their
    sum under every driver candidate that fits, the first candidate under which it reaches k.  d_visible / x_visible: truth
    values per raw order entry; an entry that is not visible is passed over — the two wrong models of test_deep_orders_cpu.py."""
    n = len(avail)
    D, X = np.asarray(D, dtype=np.int64), np.asarray(X, dtype=np.int64)
    xs = X[(X < n) & (np.ones(len(X), dtype=bool) if x_visible is None else x_visible)]
    ds = D[(D < n) & (np.ones(len(D), dtype=bool) if d_visible is None else d_visible)]
    drv, exe = np.asarray(drv, dtype=np.int64), np.asarray(exe, dtype=np.int64)
    ds = ds[(avail[ds] >= drv).all(axis=1)]
    c0 = np.minimum(_cap(avail[xs], exe), k + 1)
    at = np.full(n, -1, dtype=np.int64)
    at[xs] = np.arange(len(xs))
    mine = np.where(at[ds] >= 0, np.minimum(_cap(avail[ds] - drv, exe), k + 1), 0)
    total = int(c0.sum()) - np.where(at[ds] >= 0, c0[at[ds]], 0) + mine
    works = np.nonzero(total >= k)[0]
    if len(works) == 0:
        return False, 0xFFFFFFFF, np.zeros(0, dtype=np.uint32)
    d = int(ds[works[0]])
    if at[d] >= 0:
        c0 = c0.copy()
        c0[at[d]] = mine[works[0]]
    return True, d, np.repeat(xs, c0)[:k].astype(np.uint32)


# ------------------------------------------------------------------------------------- where a chain's LDS front ends


def n_eval_zones(problem_tuple):
    """Zones of the evaluation list (single_az.go:23-72, plan_layout): those of the driver order that own an executor candidate."""
    avail, _, zone, D, X = problem_tuple[:5]
    n = len(avail)
    return len(set(zone[D[D < n]].tolist()) & set(zone[X[X < n]].tolist()))


def chain_lds_slots(algo, budget, n_slots, n_zones, target=None):
    """Slots of the table an LDS chain kernel of packer `algo` keeps in LDS under option lds_budget = budget, or None where the
    packer's tables do not fit and the generic chain serves: route_of's rules (solo_lds_slots, zoned_lds_geometry,
    minfrag_lds_geometry of gangfit_api_fit.cpp) over the library's own byte counts, gangfit::fifo_*_lds_bytes.  With
    target (a multiple of 64 below n_slots) and budget None: the budget that keeps exactly `target` slots in LDS."""
    import ctypes as C

    from gangfit import _native

    L = _native.load()

    def fn(name, n_args):
        f = getattr(L, name)
        f.restype, f.argtypes = C.c_size_t, [C.c_uint32] * n_args
        return f

    n_chunks = (n_slots + 63) // 64
    if algo in (0, 1):
        solo = fn("_ZN7gangfit19fifo_solo_lds_bytesEjj", 2)
        if budget is None:
            return solo(target, n_chunks)
        fixed = solo(0, n_chunks)
        fit = (budget - fixed) // (solo(64, n_chunks) - fixed) if budget > fixed else 0
        return min(fit, n_chunks) * 64
    if algo in (3, 4):
        zoned = fn("_ZN7gangfit20fifo_zoned_lds_bytesEjjjjj", 5)
        n_cand = n_zones + (1 if algo == 3 else 0)
        size = lambda slots, rows: zoned(slots, n_chunks, n_zones, n_cand, rows)  # noqa: E731
        rows, floor = 64, 4
    else:
        minfrag = fn("_ZN7gangfit22fifo_minfrag_lds_bytesEjjjj", 4)
        size = lambda slots, rows: minfrag(slots, n_chunks, n_zones if algo == 5 else 0, rows)  # noqa: E731
        rows, floor = 64, 0
    if budget is None:
        return size(target, 64)
    while rows > floor and size(64, rows) > budget:
        rows //= 2
    fixed = size(0, rows)
    if budget <= fixed + 12 * 64:
        return None
    slots = (budget - fixed) // 12
    return n_slots if slots >= n_slots else slots // 64 * 64


def tail_target(p):
    """An LDS front that ends behind p: position p and the two chunks after its chunk in LDS, the rest a global tail."""
    return (p // 64 + 3) * 64
