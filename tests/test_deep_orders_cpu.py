"""The oracle and the generator behind chunk group zero (tests/deep_orders.py): what tests/test_gpu_deep_orders.py trusts.
(a) The oracle's restatements agree on every problem: literal and closed form, all six packers, both modes; the pure-Python
restatement too on the problems of 4 300 nodes (its cost is the reference's: the designated gangs — those of the whole order's
capacity for tightly-pack, and for distribute-evenly at p = 4 096, only — and the first feasible ones).
(b) Every front still reaches what it is named for, read from the oracle's answers: a later edit cannot make the generator tame
without failing here.  (c) The battery discriminates: a model that ignores every position from 4 096 on and one that passes
over position p alone each differ from the oracle on every problem.  CPU only."""
import numpy as np
import pytest

import deep_orders as do
from oracle import binding as ob
from oracle import pyoracle as po

ALGOS = (0, 1, 2, 3, 4, 5)
NO = ob.NO_NODE
_CACHE = {}


def _cases(front):
    """[(name, problem, info, literal answers, closed-form answers)], once per front and run."""
    if front not in _CACHE:
        cs = do.cases(front)
        both = do.references([(form + name, p, info) for name, p, info in cs for form in "lc"], closed_form=lambda nm: nm[0] == "c")
        _CACHE[front] = [(name, p, info, both["l" + name], both["c" + name]) for name, p, info in cs]
    return _CACHE[front]


def _where(info, out, a):
    """(feasible, driver position, executor positions) of gang a."""
    ok, d, ex = out.placement(a)
    if not ok:
        return False, -1, np.zeros(0, dtype=np.int64)
    return True, int(info["dpos"][d]), info["xpos"][ex]


def _same(a, b, fifo, where):
    assert np.array_equal(a.results, b.results), where
    for i in np.nonzero(a.results["has_capacity"])[0]:
        assert np.array_equal(a.placement(int(i))[2], b.placement(int(i))[2]), (where, int(i))
    if fifo:
        assert a.failed_at == b.failed_at, where
        assert np.array_equal(a.avail_after, b.avail_after), where
    else:
        assert np.array_equal(a.avg_eff.view(np.uint64), b.avg_eff.view(np.uint64)), where


# ------------------------------------------------------------------------------------------- (a) the restatements agree


@pytest.mark.parametrize("front", do.FRONTS)
def test_literal_and_closed_form_agree(front):
    for name, p, info, lit, clo in _cases(front):
        for algo in ALGOS:
            _same(lit[algo][0], clo[algo][0], False, (name, algo))
            _same(lit[algo][1], clo[algo][1], True, (name, algo))


def _py_tables(avail, sched, zone, D, X):
    """The problem as the reference holds it: maps by node name, orders of names (the packers leave them unchanged)."""
    names = lambda ids: [f"n{i}" for i in ids]  # noqa: E731
    return (names(D.tolist()), names(X.tolist()), {f"n{i}": r for i, r in enumerate(avail.tolist())},
            {f"n{i}": r for i, r in enumerate(sched.tolist())}, {f"n{i}": z for i, z in enumerate(zone.tolist())})


def _py(algo, tables, drv, exe, k):
    D, X, av, sc, zn = tables
    drv, exe, k = [int(v) for v in drv], [int(v) for v in exe], int(k)
    plain = {0: po.tightly_pack, 1: po.distribute_evenly, 2: po.minimal_fragmentation_pack}
    if algo in plain:
        r = plain[algo](drv, exe, k, D, X, av)
    else:
        fn = {3: po.az_aware_tightly_pack, 4: po.single_az_tightly_pack, 5: po.single_az_minimal_fragmentation}[algo]
        r = fn(drv, exe, k, D, X, av, sc, zn)
    return r.has_capacity, r.driver_node, r.executor_nodes


@pytest.mark.parametrize("front", do.FRONTS)
def test_pure_python_restatement_agrees_at_4300(front):
    checked = 0
    for name, p, info, lit, _ in _cases(front):
        if info["n"] != 4300:
            continue
        avail, sched, zone, D, X, drv, exe, k, flags = p
        designated = list(info.get("designated", {}).values())
        tables = _py_tables(avail, sched, zone, D, X)
        for algo in ALGOS:
            ind = lit[algo][0]
            # (the gangs of the whole order's capacity cost the restatement seconds each: tightly-pack on every problem,
            #  distribute-evenly at p = 4 096)
            gangs = [g for g in designated if k[g] < 400 or algo == 0 or (algo == 1 and info["p"] == do.GROUP)]
            gangs += [int(g) for g in np.nonzero(ind.results["has_capacity"])[0] if k[g] < 400][:2]
            if algo == 0:
                gangs += [g for g in info["infeasible"] if drv[g, 0] > 256 * do.CPU][:1]  # no candidate: no retry loop
            for g in gangs:
                ok, d, ex = ind.placement(g)
                pok, pd, pex = _py(algo, tables, drv[g], exe[g], k[g])
                assert ok == pok, (name, algo, g)
                if ok:
                    assert pd == f"n{d}" and pex == [f"n{i}" for i in ex], (name, algo, g)
                checked += 1
    assert checked >= 30


# --------------------------------------------------------------------------------------- (b) the generator's edges


def test_the_sizes_are_the_chunk_counts_they_stand_for():
    """4 300 nodes: 68 chunks, two groups, a ragged last chunk; 4 370: 69, no multiple of the four-chunk batches; 8 400: 132,
    three groups — counted with the sentinel slot, as plan_layout does; and the boundaries lie around the group edges."""
    for n, chunks in ((4300, 68), (4370, 69), (8400, 132)):
        assert (n + 1 + 63) // 64 == chunks and (n + 1) % 64 != 0
    assert 69 % 4 != 0 and (68 + 63) // 64 == 2 and (132 + 63) // 64 == 3
    assert {p for _, p in do.BOUNDS} == {g * do.GROUP + d for g in (1, 2) for d in (-1, 0, 1)}
    assert {p for n, p in do.BOUNDS if n == 4300} == {4095, 4096, 4097}


@pytest.mark.parametrize("front", do.FRONTS)
def test_positions_and_layouts(front):
    """Position p is where the front ends in both orders; every layout of the front and both zone counts occur; the merged
    orders carry unknown names, one-order slots and a repeated driver candidate, the general ones more driver positions than
    slots; with three zones one lies wholly in the front, one wholly behind p, one on both sides."""
    layouts, zones = set(), set()
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), info, _, _ in _cases(front):
        n, p, layout = info["n"], info["p"], info["layout"]
        layouts.add(layout)
        zones.add(info["n_zones"])
        seq, dpos, xpos = info["seq"], info["dpos"], info["xpos"]
        for pos in (dpos, xpos):  # the node of position p, and the same set of nodes in front of it
            assert pos[seq[p]] == p, name
            assert ((pos[seq[:p]] < p)).all() and ((pos[seq[p:]] >= p) | (pos[seq[p:]] < 0)).all(), name
        if layout == "merged":
            assert (D >= n).sum() == 1 and (X >= n).sum() == 1 and len(set(D.tolist())) < len(D), name
            assert ((dpos < 0) & (xpos >= 0)).any(), name
            if front != "executors-front":
                assert ((xpos < 0) & (dpos >= 0)).any(), name
        if layout == "general":
            n_slots = len(X) + int(((dpos >= 0) & (xpos < 0)).sum()) + 1
            assert len(D) > n_slots and (D >= n).any() and (X >= n).any(), name
            assert (dpos[seq[:p]] != xpos[seq[:p]]).any(), name  # positions are not slots
        if info["n_zones"] == 3:
            a, b, c = do.ZONE_IDS
            zpos = np.where(xpos >= 0, xpos, dpos)
            assert (zpos[zone == a] < p).all() and (zpos[zone == b] >= p).all(), name
            assert (zpos[zone == c] < p).any() and (zpos[zone == c] >= p).any(), name
            assert set(zone.tolist()) == {a, b, c}
    assert layouts == set(do.LAYOUTS[front]) and zones == {1, 3}


# feasible gangs of tightly-pack's independent batch over the front's nine problems: (all, driver at a position >= p, some
# executor at a position >= p) — the figures DESIGN.md quotes
BEHIND = {"cleared": (324, 324, 311), "stale": (323, 323, 308), "drivers-front": (324, 48, 314),
          "executors-front": (324, 324, 52), "straddle": (315, 0, 287), "fallback": (315, 315, 303),
          "gpu-gangs": (324, 324, 138), "draining": (342, 0, 9)}


@pytest.mark.parametrize("front", do.FRONTS)
def test_decisions_fall_behind_p(front):
    got = [0, 0, 0]
    for name, p, info, lit, _ in _cases(front):
        ind = lit[0][0]
        for g in np.nonzero(ind.results["has_capacity"])[0]:
            _, dp, xp = _where(info, ind, int(g))
            got[0] += 1
            got[1] += dp >= info["p"]
            got[2] += bool(len(xp)) and bool((xp >= info["p"]).any())
    print(f"{front}: feasible {got[0]}, driver behind p {got[1]}, an executor behind p {got[2]}")
    assert tuple(got) == BEHIND[front]


@pytest.mark.parametrize("front", ("cleared", "stale"))
def test_hollow_fronts_decide_nothing(front):
    """Every packer, both modes: every feasible gang has its driver and every executor at a position >= p; at least half the
    gangs are feasible and at least three are not.  cleared: every front node is below every request in cpu and in memory, some
    are negative (the maxima rule out every front chunk).  stale: the maxima of every whole front chunk admit every request
    in every dimension, and no front node fits any driver or executor."""
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), info, lit, _ in _cases(front):
        p, a = info["p"], len(k)
        for algo in ALGOS:
            for out in lit[algo]:
                ok = out.results["has_capacity"] != 0
                if out.failed_at < 0:
                    assert ok.sum() * 2 >= a and (~ok).sum() >= 3, (name, algo)
                for g in np.nonzero(ok)[0]:
                    _, dp, xp = _where(info, out, int(g))
                    assert dp >= p and (xp >= p).all(), (name, algo, int(g))
        pos = np.where(info["xpos"] >= 0, info["xpos"], info["dpos"])
        front_nodes = avail[pos < p]
        reqs = np.concatenate([drv, exe[k > 0]])
        if front == "cleared":
            assert (front_nodes[:, 0].max() < reqs[:, 0].min()) and (front_nodes[:, 1].max() < reqs[:, 1].min()), name
            assert (front_nodes < 0).any(axis=0).all(), name
        else:
            by_pos = np.full((info["n"] + 2, 3), -(1 << 62), dtype=np.int64)
            by_pos[pos[pos >= 0]] = avail[pos >= 0]
            whole = (p - 2) // 64
            maxima = by_pos[:whole * 64].reshape(whole, 64, 3).max(axis=1)
            feasible_reqs = reqs[(reqs <= avail.max(axis=0)).all(axis=1)]
            assert (maxima >= feasible_reqs.max(axis=0)).all(), name
            assert not (front_nodes[:, None, :] >= reqs[None, :, :]).all(axis=2).any(), name


def test_drivers_front():
    """The small drivers sit in the front (in group 0 or, at the far boundaries, in the groups before p) with every executor
    behind p; the larger ones behind p."""
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), info, lit, _ in _cases("drivers-front"):
        p, ind = info["p"], lit[0][0]
        n_front = n_rear = 0
        for g in np.nonzero(ind.results["has_capacity"])[0]:
            _, dp, xp = _where(info, ind, int(g))
            assert (xp >= p).all(), (name, int(g))
            assert (dp < p) == (int(g) in info["front_drivers"]), (name, int(g))
            n_front += dp < p
            n_rear += dp >= p
            if dp < p and p < 5000:
                assert dp < do.GROUP
        assert n_front >= 20 and n_rear >= 3, name


def test_executors_front():
    """No driver candidate in front of p: every driver's slot is >= p.  Most gangs have executors in group 0; the gangs of the
    larger shapes find their first executor in the last front chunk, and at p = 4 095 and 4 097 that is the driver's chunk."""
    same_chunk = 0
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), info, lit, _ in _cases("executors-front"):
        p, ind = info["p"], lit[0][0]
        assert (info["dpos"][info["seq"][:p]] < 0).all(), name
        in_front = 0
        for g in np.nonzero(ind.results["has_capacity"])[0]:
            _, dp, xp = _where(info, ind, int(g))
            assert dp >= p, (name, int(g))
            in_front += bool(len(xp)) and bool((xp < min(p, do.GROUP)).any())
            if int(g) in info["last_chunk_gangs"]:
                assert xp[0] // 64 == (p - 1) // 64, (name, int(g))
                same_chunk += xp[0] // 64 == dp // 64
        assert in_front >= 10 and len(info["last_chunk_gangs"]) >= 5, name
        ok, dp, xp = _where(info, ind, info["spill"])  # the last front chunk, the node at p and one executor more
        assert ok and xp[0] // 64 == (p - 1) // 64 and (xp == p).any() and xp[-1] > p, name
    assert same_chunk >= 10


def test_straddle():
    """tightly-pack: the designated gangs place K-1 executors in front of p and the K-th on p; end on p-1; fill the order to its
    last holder; and fail with one executor more.  distribute-evenly: the second pass gives p-1 and p the last two places, or
    ends on p-1.  Their driver sits on the front node put there for it."""
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), info, lit, _ in _cases("straddle"):
        p, g, xpos = info["p"], info["designated"], info["xpos"]
        tight, even = lit[0][0], lit[1][0]
        ok, dp, xp = _where(info, tight, g["cross"])
        assert ok and k[g["cross"]] == 5 and (xp[:4] < p).all() and xp[3] == p - 1 and xp[4] == p, name
        assert info["dpos"][tight.placement(g["cross"])[1]] < p - 3, name
        ok, dp, xp = _where(info, tight, g["end"])
        assert ok and xp.tolist() == [p - 3, p - 2, p - 1, p - 1], name
        ok, dp, xp = _where(info, tight, g["whole"])
        holders = xpos[(xpos >= 0) & (do._cap(avail, np.array(do.STRADDLE_EXE)) > 0)]
        assert ok and len(xp) == info["total"] and xp[-1] == holders.max() and xp[-1] > p + do.LIVE, name
        assert not _where(info, tight, g["over"])[0] and k[g["over"]] == info["total"] + 1, name
        assert not _where(info, even, g["over"])[0], name
        ok, dp, xp = _where(info, even, g["even_cross"])
        assert ok and len(xp) == info["holders"] + 2 and xp[-2] == p - 1 and xp[-1] == p, name
        assert (np.sort(xp[:-2]) == np.sort(holders)).all(), name  # the first pass: one on every holder
        ok, dp, xp = _where(info, even, g["even_end"])
        assert ok and xp[-1] == p - 1 and len(xp) == info["holders"] + 1, name


def test_fallback():
    """The chosen driver is not the first fitting one: that one sits on p, every driver on the 70 positions from p costs its
    node one executor of the K = capacity the gang needs, and the driver that works sits in a later chunk.  With the larger
    driver request the same capacity is there and no driver works."""
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), info, lit, _ in _cases("fallback"):
        p, g = info["p"], info["designated"]
        for algo in (0, 1):
            ind = lit[algo][0]
            ok, dp, xp = _where(info, ind, g["later_driver"])
            fits = (avail >= drv[g["later_driver"]]).all(axis=1) & (info["dpos"] >= 0)
            first = int(info["dpos"][fits].min())
            assert first == p and ok and dp == p + 70 and dp // 64 > first // 64, (name, algo)
            assert len(xp) == info["total"] and xp.max() >= info["n"] - do.LIVE, (name, algo)
            assert not _where(info, ind, g["no_driver"])[0], (name, algo)
        in_x = info["xpos"] >= 0
        assert int(do._cap(avail[in_x], np.array(do.FALLBACK_EXE)).sum()) == k[g["no_driver"]] == info["total"], name


def test_gpu():
    """The gpu nodes are at most a quarter of the slots (the compact view exists); the gangs of gpu executors are mostly
    feasible; with the gpu nodes in group 0 every one of their executors sits there and the driver behind p (the generic
    search); with the gpu nodes behind p, everything does."""
    variants = set()
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), info, lit, _ in _cases("gpu-gangs"):
        p, ind = info["p"], lit[0][0]
        variants.add(info["variant"])
        has = (avail[:, 2] > 0) & (info["xpos"] >= 0)
        assert 0 < has.sum() * 4 <= info["n"], name
        gpos = info["xpos"][has]
        assert (gpos < do.GROUP).all() if info["variant"] == 0 else (gpos >= p).all() and gpos.min() == p, name
        fits = 0
        for g in info["gpu_gangs"]:
            ok, dp, xp = _where(info, ind, g)
            if ok and k[g] > 0:
                fits += 1
                assert dp >= p and ((xp < do.GROUP).all() if info["variant"] == 0 else (xp >= p).all()), (name, g)
        assert fits >= 15 and _where(info, ind, info["second_driver"])[1] == p + 1, name
    assert variants == {0, 1}


def test_draining():
    """tightly-pack's chain uses the front up with its first 14 applications, the last of them ending on p-1; the 15th —
    index in [8, a - 8] — is the first with anything at a position >= p, and everything after it lies there; the chain ends at
    the application that is not skippable, behind one that was skipped.  Nothing usable is left in the front."""
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), info, lit, _ in _cases("draining"):
        p, a, m = info["p"], len(k), info["first_behind"]
        fifo = lit[0][1]
        assert 8 <= m <= a - 8 and 25 > m, name
        assert not fifo.results["has_capacity"][25] and flags[25] == 1, name
        for g in range(fifo.failed_at):
            ok, dp, xp = _where(info, fifo, g)
            if g == 25:
                continue
            assert ok, (name, g)
            if g < m:
                assert dp < p and (xp < p).all(), (name, g)
            else:
                assert dp >= p and (xp >= p).all(), (name, g)
        assert _where(info, fifo, m - 1)[2][-1] == p - 1 and _where(info, fifo, m)[1] == p, name
        pos = np.where(info["xpos"] >= 0, info["xpos"], info["dpos"])
        left = fifo.avail_after[pos < p]
        assert not ((left[:, 0] >= do.CPU) & (left[:, 1] >= do.GIB) & (left[:, 2] >= 0)).any(), name
        ok, dp, xp = _where(info, lit[0][0], 20)  # alone, application 20 needs the whole front and seventy places behind it
        assert ok and (xp >= p).sum() == 71 and xp.max() > p and dp < p, name


def test_single_executor_and_find_nodes_cases():
    """The crafted gf_executor_fit and gf_find_nodes inputs give the answers they were built for."""
    for n, p in do.BOUNDS + tuple((4370, q) for q in (4095, 4096, 4097)):
        avail, X, node_zone, shapes, hosts, reserved, what = do.executor_cases(n, p)
        xpos = np.argsort(X)
        for key, mf, r, zoned in (("first_fit", False, None, False), ("first_fit_reserved", False, reserved, False),
                                  ("min_frag", True, None, False), ("min_frag_zoned", True, None, True),
                                  ("min_frag_reserved", True, reserved, False)):
            order = X[node_zone[X] == 1] if zoned else X
            for q, want in what[key].items():
                got = ob.executor_fit(avail, shapes[q], order, reserved=r, minimal_fragmentation=mf, hosts=hosts[q] if mf else None)
                assert got != NO and xpos[got] == want, (n, p, key, q)
        avail, X, exe, k, what = do.find_nodes_cases(n, p)
        xpos = np.argsort(X)
        ref = ob.find_nodes(avail, exe, k, X, chained=False)
        for q, want in what["ends_at"].items():
            assert ref.placed[q] == k[q] and xpos[ref.placement(q)[-1]] == want, (n, p, q)
            assert (ref.adds[q][X[:p - 1]] == 1).all(), (n, p, q)  # every front node visited and charged one add
        assert ref.placed[what["short"]] == k[what["short"]] - 1
        assert xpos[X[n - 3]] // 64 == n // 64 and (n + 1) % 64 != 0  # the last, ragged chunk


@pytest.mark.parametrize("front", do.FRONTS)
def test_every_chain_ends_behind_its_first_deep_decision(front):
    """Every packer's chain stops at the one application that is not skippable, index 36: behind the first application with
    anything at a position >= p, behind a skipped one, and behind the checkpoint at 32 that a second chain resumes from."""
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), info, lit, _ in _cases(front):
        assert (flags == 0).sum() == 1 and flags[do.LAST] == 0 and len(k) - 1 > do.LAST > 32, name
        for algo in ALGOS:
            fifo = lit[algo][1]
            assert fifo.failed_at == do.LAST, (name, algo)
            ok = fifo.results["has_capacity"][:do.LAST] != 0
            deep = [g for g in np.nonzero(ok)[0] if _where(info, fifo, int(g))[1] >= info["p"] or
                    (_where(info, fifo, int(g))[2] >= info["p"]).any()]
            assert deep and deep[0] < 32 and (~ok).any(), (name, algo)


def test_lds_budgets_place_the_chain_boundary():
    """Where the FIFO chains' LDS front ends (do.chain_lds_slots: route_of's geometry over the library's byte counts), for
    every packer, size and zone count of the battery: 24 000 and 50 000 bytes end it inside the hollow front, or leave the
    zone-aware and minimal-fragmentation packers to the generic chain; the derived budget ends it at do.tail_target(p), behind
    p and short of the table's end, within the 160 KiB of a compute unit; that much holds every whole table."""
    generic = 0
    for n, p in do.BOUNDS:
        for nz in (1, 3):
            for algo in ALGOS:
                for budget in (24000, 50000):
                    slots = do.chain_lds_slots(algo, budget, n + 1, nz)
                    generic += slots is None
                    assert slots is None or slots <= 4032 < p, (n, p, nz, algo, budget)
                    assert slots is not None or algo > 2 or (algo == 2 and budget < 50000), (n, p, nz, algo, budget)
                target = do.tail_target(p)
                budget = do.chain_lds_slots(algo, None, n + 1, nz, target=target)
                assert budget <= 160 * 1024 and p < target < n, (n, p, nz, algo)
                assert do.chain_lds_slots(algo, budget, n + 1, nz) == target, (n, p, nz, algo)
                assert do.chain_lds_slots(algo, budget - 12 * 64, n + 1, nz) == target - 64, (n, p, nz, algo)
                assert do.chain_lds_slots(algo, 160 * 1024, n + 1, nz) >= n + 1, (n, p, nz, algo)
    assert generic > 0


# ------------------------------------------------------------------------------------ (c) the battery discriminates


@pytest.mark.parametrize("front", do.FRONTS)
def test_two_wrong_models_differ_on_every_problem(front):
    """tightly_pack_model with every position visible is the oracle's tightly-pack, gang for gang; blind from position 4 096
    on, or to position p alone, it differs from the oracle on at least one gang of every problem."""
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), info, lit, _ in _cases(front):
        n, p, ind = info["n"], info["p"], lit[0][0]
        known_d, known_x = np.minimum(D, n - 1), np.minimum(X, n - 1)  # (unknown names are passed over whatever their mask says)
        dp, xp = info["dpos"][known_d], info["xpos"][known_x]
        masks = {"right": (None, None), "group 0 only": (dp < do.GROUP, xp < do.GROUP), "without p": (dp != p, xp != p)}
        for model, (dv, xv) in masks.items():
            differs = 0
            for g in range(len(k)):
                ok, d, ex = ind.placement(g)
                mok, md, mex = do.tightly_pack_model(avail, D, X, drv[g], exe[g], int(k[g]), dv, xv)
                same = ok == mok and (not ok or (d == md and np.array_equal(ex, mex)))
                if model == "right":
                    assert same, (name, g)
                differs += not same
            assert model == "right" or differs >= 1, (name, model)
