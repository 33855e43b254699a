"""What tests/test_gpu_worker_rows_edges.py trusts about the cases of tests/worker_rows_cases.py, recomputed on the CPU: the layout of
the deep cluster (chunks, groups, one-order slots), the rows by definition, and for every record of its tickets the oracle's answer
(oracle.binding.fit_independent, tightly-pack, literal and closed form) next to the row model's (tests/worker_rows_shim.cpp over
csrc/gangfit_worker_rows.h): the declared feasibility and driver node, SERVED / NOT SERVED, that a served placement is the oracle's,
and the two counts the GPU test bounds the row statistics with.  CPU only."""
import numpy as np
import pytest

import deep_orders as do
import worker_rows_cases as wc
from oracle import binding as ob

NO = ob.NO_NODE
_CACHE = {}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return wc.compile_shim(tmp_path_factory.mktemp("worker_rows_cases"))


def _deep(shim, variant):
    """(case, literal oracle, closed-form oracle, row model, dslot, xslot) once per variant."""
    if variant not in _CACHE:
        c = wc.deep_case(variant)
        oapps = ob.make_apps(c.drv, c.exe, c.k, np.zeros(len(c.k), dtype=np.uint32))
        lit = ob.fit_independent(0, c.avail, oapps, c.D, c.X)
        clo = ob.fit_independent(0, c.avail, oapps, c.D, c.X, closed_form=True)
        model = wc.row_model(shim, c.avail, c.D, c.X, c.drv, c.exe, c.k)
        dslot, xslot = do.positions(wc.N_DEEP, c.D, c.X, "merged")  # (raises when the orders do not merge)
        _CACHE[variant] = (c, lit, clo, model, dslot, xslot)
    return _CACHE[variant]


def _whole_units(c):
    """Per record: every request is a multiple of its column's unit (the gcd of the snapshot's column) — only such a record has a
    scaled form and looks a row up."""
    unit = [int(np.gcd.reduce(c.avail[:, j][c.avail[:, j] != 0])) for j in range(3)]
    assert unit == [500, wc.GIB, 1]  # (node 1 is there for this: 32 GiB and 2 gpus would be the units without it)
    assert [int(np.gcd.reduce(np.delete(c.avail[:, j], 1)[np.delete(c.avail[:, j], 1) != 0])) for j in range(3)] == [500, 32 * wc.GIB, 2]
    return np.array([all(int(v) % u == 0 for v, u in zip(np.concatenate([c.drv[a], c.exe[a]]), unit * 2)) for a in range(len(c.k))])


@pytest.mark.parametrize("variant", wc.DEEP_VARIANTS)
def test_layout_of_the_deep_cluster(shim, variant):
    c, _, _, _, dslot, xslot = _deep(shim, variant)
    slot = np.where(xslot >= 0, xslot, dslot)
    n_slots = int(slot.max()) + 1
    assert (n_slots + 1 + 63) // 64 == 67 and (n_slots + 1) % 64 in (6, 7)  # with the sentinel: 67 chunks, the last one ragged
    assert ((dslot < 0) | (xslot < 0) | (dslot == xslot)).all()
    gpu_x = int(((c.avail[:, 2] > 0) & (xslot >= 0)).sum())
    assert 0 < gpu_x and gpu_x * 4 <= n_slots  # the compact gpu table exists
    if variant == "all":
        assert np.array_equal(slot, np.arange(wc.N_DEEP)) and np.array_equal(dslot, xslot)
    else:
        assert dslot[4066] < 0 and xslot[4066] < 0 and int((slot < 0).sum()) == 1  # one node in neither order: it takes no slot
        assert np.array_equal(slot[:4066], np.arange(4066)) and np.array_equal(np.sort(slot[4067:]), np.arange(4066, wc.N_DEEP - 1))
        assert np.array_equal(slot[4067:4200], np.arange(4066, 4199))  # slot ids are not node ids behind the node that takes none
        assert dslot[4064] < 0 and xslot[4064] == 4064 and dslot[4200] < 0 and xslot[4200] == 4200  # executor-only slots
        # a driver-only slot behind group 0 (where a driver-only and an executor-only node meet, the merge takes the driver's first)
        assert xslot[4201] < 0 and dslot[4201] == 4199
        assert dslot[4065] == xslot[4065] == 4065
        d_only, x_only = (xslot < 0) & (dslot >= 0), (dslot < 0) & (xslot >= 0)
        assert d_only.sum() == 54 and x_only.sum() == 2 and ((dslot >= 0) & (xslot >= 0)).any()  # flags 2, 1 and 3
        assert (slot[d_only] >= 4064).all() and d_only[4069] and slot[4069] == 4068 < wc.GROUP < slot[d_only].max()  # on both sides of group 0
    # DBIG fits no slot of group 0: every maximum of its chunks is below the request (wave_row_driver finds no candidate chunk)
    in_g0 = (dslot >= 0) & (dslot < wc.GROUP)
    assert in_g0.sum() > 4000 and int(c.avail[in_g0, 0].max()) < wc.REQUESTS["DBIG"][0]


@pytest.mark.parametrize("variant", wc.DEEP_VARIANTS)
def test_rows_of_the_deep_cluster(shim, variant):
    """The rows by definition, in slots: where they start and end, and that A's is cut inside a chunk of 64 qualifying slots."""
    c, _, _, _, _, xslot = _deep(shim, variant)
    row_len = wc.consts(shim)[0]
    rows = {}
    for name in ("A", "B", "G"):
        _, node, cap, hdr = wc.row_of(shim, c.avail, c.X, np.array(wc.REQUESTS[name], dtype=np.int64))
        rows[name] = (xslot[node[:hdr]], node[:hdr], cap[:hdr])
    slots, nodes, cap = rows["A"]
    assert len(slots) == row_len == 64 and (cap == 4).all() and int(cap.sum()) == 256
    assert slots[0] == 4064 and slots[0] // 64 == 63 and slots[-1] // 64 >= 64 and slots[-1] % 64 != 63  # across groups 0 and 1, cut mid-chunk
    assert (slots < wc.GROUP).any() and (slots >= wc.GROUP).any()
    a_caps = wc._caps(c.avail[c.X], np.array(wc.REQUESTS["A"]), 1 << 20)
    assert int((a_caps >= 1).sum()) > 64  # a 65th qualifying slot exists
    if variant == "all":
        assert np.array_equal(slots, np.arange(4064, 4128)) and np.array_equal(nodes, slots)
        assert int(a_caps.sum()) == 784  # the whole cluster's capacity for A
        # chunk 64 holds 64 qualifying slots and the row has room for 32 of them
        assert (a_caps[4096:4160] >= 1).all() and int((slots >= 4096).sum()) == 32
        assert np.array_equal(rows["B"][0], np.arange(4200, 4230)) and (rows["B"][2] == 1).all()
        assert np.array_equal(rows["G"][0], np.arange(4210, 4214)) and (rows["G"][2] == 2).all()
    else:
        assert nodes[:4].tolist() == [4064, 4065, 4067, 4068] and slots[:4].tolist() == [4064, 4065, 4066, 4067]
        assert not np.array_equal(nodes, slots)
        assert len(rows["B"][0]) == 20 and rows["B"][1][0] == 4200 and rows["B"][0][0] == 4200 and (rows["B"][2] == 1).all()
        assert rows["G"][1].tolist() == [4211, 4212] and (rows["G"][2] == 2).all()
    assert rows["B"][0][-1] // 64 == 66  # ... ends in the last, ragged chunk


@pytest.mark.parametrize("variant", wc.DEEP_VARIANTS)
def test_declared_answers_of_the_deep_ticket(shim, variant):
    c, lit, clo, model, dslot, _ = _deep(shim, variant)
    assert np.array_equal(lit.results, clo.results)
    for a in np.nonzero(lit.results["has_capacity"])[0]:
        assert np.array_equal(lit.placement(int(a))[2], clo.placement(int(a))[2]), (variant, int(a))
    whole = _whole_units(c)
    # twenty records of K = 1 per shape; the first round of sixteen wavefronts holds ONE record that looks a row up, A's
    assert {s: sum(n for t, kk, n in wc.WARM_UP if t == s and kk == 1) for s in "ABG"} == {"A": 20, "B": 20, "G": 20}
    assert c.first_edge == 75 and (c.k[:c.first_edge] > 0).sum() == 60 and (c.drv[:c.first_edge] == wc.REQUESTS["D0"]).all()
    assert c.k[0] == 1 and (c.k[1:16] == 0).all() and (c.exe[:16] == wc.REQUESTS["A"]).all()
    assert [s for s, _, _ in wc.WARM_UP[2:]] == ["B", "G", "A"]  # A's row is built behind B's and G's
    s = f = 0
    for a in range(len(c.k)):
        d_name, e_name, kk = c.names[a]
        feasible, driver, served = (1, 0, kk > 0) if a < c.first_edge else c.edges[a - c.first_edge][3:]
        ok, dn, nodes = lit.placement(a)
        m_dn, m_ok, m_nodes = model[a]
        where = (variant, a, d_name, e_name, kk)
        assert ok == bool(feasible), where
        assert m_dn == driver and (not ok or dn == driver), where
        assert m_ok == served, where
        if m_ok:  # wherever the row model says SERVED, its placement is the oracle's
            assert ok and dn == m_dn and np.array_equal(nodes, m_nodes), where
        behind = dslot[m_dn] >= wc.GROUP
        assert behind == (d_name == "DBIG") and whole[a] == (e_name != "A+1"), where
        if behind:
            assert dslot[m_dn] // 64 == 65, where
        s += bool(m_ok and not behind and whole[a])
        f += bool(kk > 0 and whole[a] and (behind or not m_ok))
    print(f"{variant}: S = {s}, F = {f}, records {len(c.k)}, executors per ticket {int(c.k.sum())}")
    assert s == c.s == wc.DEEP_S[variant] and f == c.f == wc.DEEP_F[variant]
    # "served by the model, driver in group 0" alone counts one record more: the kernel never looks that one up
    assert sum(1 for a in range(len(c.k)) if model[a][1] and dslot[model[a][0]] < wc.GROUP) == s + 1  # (the request off its unit)
    # the edges the ticket is there for
    kinds = {(d, e, ok) for (d, e, _, _, _, ok) in c.edges}
    assert {("D0", "A", True), ("D0", "A", False), ("D1", "A", True), ("D1", "A", False), ("DALL", "A", True), ("DALL", "A", False),
            ("DBIG", "A", True), ("DBIG", "B", True), ("D0", "B", True), ("D0", "B", False), ("D0", "G", True), ("D0", "G", False)} <= kinds


@pytest.mark.parametrize("variant", wc.DEEP_VARIANTS)
def test_the_driver_sits_where_the_case_says(shim, variant):
    """D1 and DALL on the row's first entry (all) or its second, behind an executor-only slot (subsequences); DALL leaves its node
    no room (c_ds == 0), D1 room for three; DBIG's node is the first entry of B's row (all) or no executor candidate at all."""
    c, _, _, _, dslot, xslot = _deep(shim, variant)
    A, B = np.array(wc.REQUESTS["A"]), np.array(wc.REQUESTS["B"])
    _, a_nodes, _, _ = wc.row_of(shim, c.avail, c.X, A)
    _, b_nodes, _, _ = wc.row_of(shim, c.avail, c.X, B)
    d1 = wc.first_fitting_driver(c.avail, c.D, np.array(wc.REQUESTS["D1"]))
    assert d1 == wc.first_fitting_driver(c.avail, c.D, np.array(wc.REQUESTS["DALL"])) == int(a_nodes[0 if variant == "all" else 1])
    assert int(wc._caps((c.avail[d1] - wc.REQUESTS["D1"])[None, :], A, 1 << 20)[0]) == 3
    assert int(wc._caps((c.avail[d1] - wc.REQUESTS["DALL"])[None, :], A, 1 << 20)[0]) == 0
    dbig = wc.first_fitting_driver(c.avail, c.D, np.array(wc.REQUESTS["DBIG"]))
    if variant == "all":
        assert dbig == int(b_nodes[0]) == 4200
    else:
        assert dbig == 4201 and xslot[dbig] < 0 and dbig not in b_nodes.tolist() and xslot[int(a_nodes[0])] == 4064 and dslot[int(a_nodes[0])] < 0
    assert wc.first_fitting_driver(c.avail, c.D, np.array(wc.REQUESTS["D0"])) == 0


def test_unique_shape_tickets_and_the_small_cluster(shim):
    """Six tickets of 48 records, 288 executor requests that never repeat, whole units of the 130-node cluster, every one with room
    on a big node: more shapes than the directory has entries before any of them is seen kRowSightings times."""
    _, k_rows, sightings, _ = wc.consts(shim)
    avail, sched, order = wc.edge_cluster()
    tickets = wc.unique_shape_tickets()
    exe = np.concatenate([t[1] for t in tickets])
    assert len(tickets) == 6 and all(len(t[2]) == 48 for t in tickets) and len({tuple(e) for e in exe.tolist()}) == 288
    assert 48 > k_rows and sightings > 1
    unit = [int(np.gcd.reduce(avail[:, j][avail[:, j] != 0])) for j in range(2)]
    assert unit == [1000, wc.GIB] and (exe[:, 0] % unit[0] == 0).all() and (exe[:, 1] % unit[1] == 0).all() and (exe[:, 2] == 0).all()
    assert (exe <= avail[129]).all()
    for drv, e, k in tickets:
        oapps = ob.make_apps(drv, e, k, np.zeros(len(k), dtype=np.uint32))
        ref = ob.fit_independent(0, avail, oapps, order, order)
        assert (k >= 1).all() and ref.results["has_capacity"].all()
