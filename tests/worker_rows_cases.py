"""Cases for the shape rows of the resident worker (csrc/gangfit_worker_rows.h; SHAPE ROWS in csrc/gangfit_worker.inc): the numpy
row model, the hand-made clusters with their tickets and declared expectations, and the stream helpers of the GPU tests.

A helper module, not a test file.  tests/test_worker_rows_cases_cpu.py recomputes every declared figure from the CPU oracle and the
row model; tests/test_gpu_worker_rows_edges.py and tests/test_gpu_worker_rows.py run the streams.

THE ROW MODEL.  Per executor shape the row is cut from the capacities of the executor order WITHOUT a driver (numpy, from the
definition: min over the dimensions of floor(avail / request), 0 on a node that is short anywhere, a zero request never limits,
clamped at GF_MAX_K): the first kRowLen positions of capacity >= 1 (tests/worker_rows_shim.cpp, by the definition, NOT the kernel's
build).  The driver is the first node of the driver order that holds the driver request, c_ds its node's capacity with the driver
reserved; the header's decide() says SERVED or NOT SERVED.  A "slot" of the model is the position in the executor order: only its
equality with the driver's matters.

THE DEEP CLUSTER.  4 230 nodes; with the sentinel slot 67 chunks of 64 slots, so chunks 64 .. 66 lie behind group 0 of the chunk
index and the last chunk is ragged.  Nodes 0 .. 4063 hold half a core (a driver of 500 m and nothing else), 4064 .. 4199 8 cpu /
32 GiB, 4200 .. 4229 16 cpu / 64 GiB, and 4210 .. 4213 two gpus each: four gpu nodes, far fewer than a quarter of the slots, so the
compact gpu table exists.  THE UNITS: a record is looked up in the rows only when every request is a whole multiple of its
column's unit, the gcd of the availability column (fill_narrow, gangfit_slot_layout.h; scale_record).  With the nodes above alone the
units would be 500 m, 32 GiB and 2 gpus, no request of 1 or 8 GiB or of 1 gpu would have a scaled form, and no row would ever be
built.  So ONE node differs: node 1 has 500 m / 33 GiB / 1 gpu, which makes the units 500 m, 1 GiB and 1 gpu and changes no answer —
half a core holds no executor, and the 500 m driver takes node 0.  Two pairs of orders:
  all           both orders are arange(4230): slot = node.  Row of A = slots 4064 .. 4127, each of capacity 4 (total 256): it starts in
                the middle of chunk 63 and ends in the middle of chunk 64, across the boundary between groups 0 and 1, and chunk 64
                holds 64 qualifying slots of which the row takes 32 (the `pos < kRowLen` clip).  Row of B = the 30 slots 4200 .. 4229,
                incomplete, ending in the ragged chunk.  Row of G = four entries of capacity 2.
  subsequences  the executor order leaves out every node n >= 4064 with n % 3 == 1, the driver order 4064, 4066 and 4200: 4064 and 4200
                are executor-only slots, 4201, 4204, ... driver-only slots, and node 4066 (4066 % 3 == 1) is in neither order and takes
                no slot, so slot = node up to 4065 and node - 1 from 4067 on — a row's node ids are not its slot ids there.  The 1 cpu
                and the 8 cpu driver land on node 4065, the SECOND entry of A's row behind the executor-only slot 4064; the 9 cpu
                driver on node 4201 (slot 4199: the merge puts a driver-only node in front of the executor-only node it meets, 4200
                on slot 4200), a driver-only slot in chunk 65.
The 9 cpu driver (DBIG) fits no slot of group 0 — its maxima say so — and wave_row_driver looks at group 0 only: every DBIG record
must be decided by wave_decide, whatever the row would say.

The ticket opens with the warm-up, twenty records of K = 1 with the 500 m driver for each of A, B and G, in an order that decides
which row is built next to which.  A row's entries written past its 64th would land in the row of the NEXT directory entry, and
are wiped when that row is built later — so A's row, the one whose last chunk holds more qualifying slots than the row has room for,
has to own an entry in front of B's and be built after it.  Record 0 is A's; the other fifteen wavefronts of the first round get
records of A with K = 0, which look nothing up, so one wavefront sees A, claims entry 0 and leaves it at one sighting while the others
are still deciding; then twenty of B (entry 1, built while they pass), twenty of G (entry 2), and A's other nineteen, whose third
builds A's row LAST.  (On a tree that dropped the `pos < kRowLen` clip, an order in which A's row was built first passed; this
one failed on the answers of its first ticket.  None of this is needed for the test to pass: it is what makes it able to fail.)  Then the edge records.
"""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32 = ctypes.c_uint32, ctypes.c_int32
NO_SLOT = 0xFFFFFFFF
CPU, GIB = 1000, 1 << 30
GROUP = 4096  # slots of one group of the chunk index


# ------------------------------------------------------------------------------------------------------- the row model


def compile_shim(directory):
    """tests/worker_rows_shim.cpp with g++ into `directory`; the loaded library."""
    so = os.path.join(str(directory), "worker_rows_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", os.path.join(REPO, "k8s-spark-scheduler_amd", "csrc"),
                           os.path.join(REPO, "tests", "worker_rows_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.wrow_consts.restype = None
    lib.wrow_build.restype = U32
    lib.wrow_decide.restype = ctypes.c_int
    lib.wrow_directory_walk.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def consts(shim):
    """(kRowLen, kRows, kRowSightings, kCapClamp)"""
    c = np.zeros(4, dtype=np.uint32)
    shim.wrow_consts(_p(c))
    return [int(x) for x in c]


def _caps(avail_rows, exe, clamp):
    a = avail_rows.astype(np.int64)
    q = np.full(a.shape, np.iinfo(np.int64).max, dtype=np.int64)
    for d in range(3):
        if exe[d] > 0:
            q[:, d] = np.floor_divide(a[:, d], int(exe[d]))
    c = np.minimum(q.min(axis=1), clamp)
    c[(a < 0).any(axis=1)] = 0
    return np.maximum(c, 0).astype(np.int32)


def row_of(shim, avail, x_order, exe):
    """The row of one shape by the definition: (positions in the executor order, node ids, capacities, count)."""
    row_len, _, _, clamp = consts(shim)
    caps = _caps(avail[x_order], exe, clamp)
    slot_node = np.ascontiguousarray(x_order, dtype=np.uint32)
    slot, node, cap = np.zeros(row_len, np.uint32), np.zeros(row_len, np.uint32), np.zeros(row_len, np.int32)
    hdr = shim.wrow_build(U32(len(x_order)), _p(caps), _p(slot_node), _p(slot), _p(node), _p(cap))
    assert hdr == min(row_len, int((caps >= 1).sum()))
    return slot, node, cap, hdr


def first_fitting_driver(avail, d_order, drv):
    """The first node of the driver order that holds the driver request, or None."""
    fits = (avail[d_order] >= drv).all(axis=1)
    return int(d_order[int(np.argmax(fits))]) if fits.any() else None


def row_model(shim, avail, d_order, x_order, drv, exe, k):
    """Per record (first fitting driver node or None, SERVED, the row's placement or None).  No driver: the kernel's driver step
    finds none and the old path answers — NOT SERVED."""
    clamp = consts(shim)[3]
    pos_of = {int(n): j for j, n in enumerate(x_order)}
    rows, out = {}, []
    for a in range(len(k)):
        key = tuple(int(x) for x in exe[a])
        if key not in rows:
            rows[key] = row_of(shim, avail, x_order, exe[a])
        slot, node, cap, hdr = rows[key]
        dn = first_fitting_driver(avail, d_order, drv[a])
        if dn is None:
            out.append((None, False, None))
            continue
        ds = pos_of.get(dn, NO_SLOT)
        c_ds = int(_caps((avail[dn] - drv[a])[None, :], exe[a], clamp)[0])
        nodes = np.full(max(int(k[a]), 1), NO_SLOT, dtype=np.uint32)
        ok = bool(shim.wrow_decide(_p(slot), _p(node), _p(cap), U32(hdr), U32(ds), I32(c_ds), I32(int(k[a])), _p(nodes)))
        out.append((dn, ok, nodes[:int(k[a])] if ok else None))
    return out


# --------------------------------------------------------------------------------------------------- the small cluster


def edge_cluster():
    """130 nodes in priority order (memory, then cpu, then index): two overcommitted nodes, 118 nodes of 8 cpu / 32 GiB, ten of
    16 cpu / 64 GiB at the end.  Slots = positions: 0, 1 negative; 2 .. 119 small; 120 .. 129 big."""
    from gangfit import workloads as wl

    avail = np.zeros((130, 3), dtype=np.int64)
    avail[:2] = [-1000, -GIB, 0]
    avail[2:120] = [8000, 32 * GIB, 0]
    avail[120:] = [16000, 64 * GIB, 0]
    sched = np.abs(avail) + np.array([1000, GIB, 0])
    order = wl.reference_node_order(avail)
    assert np.array_equal(order, np.arange(130))
    return avail, sched, order


def unique_shape_tickets(n_tickets=6, n_records=48):
    """Tickets in which no executor request occurs twice, in whole units, each of which fits a big node of edge_cluster():
    cpu 1 .. 8 cores x memory 1 .. 36 GiB = 288 shapes.  [(drv, exe, k)]"""
    shapes = [[CPU * c, m * GIB, 0] for m in range(1, 37) for c in range(1, 9)]
    assert len(shapes) == n_tickets * n_records == len({tuple(s) for s in shapes})
    out = []
    for t in range(n_tickets):
        exe = np.array(shapes[t * n_records:(t + 1) * n_records], dtype=np.int64)
        drv = np.tile(np.array([CPU, GIB, 0], dtype=np.int64), (n_records, 1))
        out.append((drv, exe, (1 + (np.arange(n_records) * 7 + t) % 5).astype(np.int32)))  # (ten big nodes hold one of the largest each)
    return out


# ----------------------------------------------------------------------------------------------------- the deep cluster

N_DEEP = 4230
DEEP_VARIANTS = ("all", "subsequences")
REQUESTS = {"D0": (500, GIB, 0), "D1": (CPU, GIB, 0), "DALL": (8 * CPU, 32 * GIB, 0), "DBIG": (9 * CPU, GIB, 0),
            "A": (2 * CPU, 8 * GIB, 0), "B": (16 * CPU, 64 * GIB, 0), "G": (2 * CPU, 8 * GIB, 1),
            "A+1": (2 * CPU, 8 * GIB + 1, 0)}  # one byte off its unit: no scaled form, the int64 path, no lookup
WARM_UP = (("A", 1, 1), ("A", 0, 15), ("B", 1, 20), ("G", 1, 20), ("A", 1, 19))  # (shape, K, records)
# (driver, shape, K, feasible, first fitting driver node, the row model says SERVED)
_ALL = (("D0", "A", 256, 1, 0, True), ("D0", "A", 257, 1, 0, False),       # the row's total; a 65th qualifying slot exists
        ("D1", "A", 255, 1, 4064, True), ("D1", "A", 256, 1, 4064, False),  # the driver on the row's first entry: it keeps 3 of 4
        ("DALL", "A", 252, 1, 4064, True), ("DALL", "A", 253, 1, 4064, False),  # ... keeps none (c_ds == 0)
        ("DBIG", "A", 256, 1, 4200, True), ("DBIG", "A", 200, 1, 4200, True),  # the driver in chunk 65: the kernel falls back
        ("D0", "B", 30, 1, 0, True), ("D0", "B", 31, 0, 0, False),          # an incomplete row that ends in the ragged chunk
        ("DBIG", "B", 29, 1, 4200, True), ("DBIG", "B", 30, 0, 4200, False),  # the driver on the row's first entry, behind group 0
        ("D0", "G", 8, 1, 0, True), ("D0", "G", 9, 0, 0, False),
        ("D0", "A", 784, 1, 0, False), ("D0", "A", 785, 0, 0, False),       # the whole cluster's capacity for A, and one more
        ("D0", "A", 0, 1, 0, False), ("D0", "A", 9, 1, 0, True), ("D0", "A+1", 7, 1, 0, True), ("D0", "A", 7, 1, 0, True))
_SUB = (("D0", "A", 256, 1, 0, True), ("D0", "A", 257, 1, 0, False),
        ("D1", "A", 255, 1, 4065, True), ("D1", "A", 256, 1, 4065, False),  # the driver on the row's SECOND entry
        ("DALL", "A", 252, 1, 4065, True), ("DALL", "A", 253, 1, 4065, False),
        ("DBIG", "A", 256, 1, 4201, True), ("DBIG", "A", 200, 1, 4201, True),  # a driver-only slot in chunk 65
        ("D0", "B", 20, 1, 0, True), ("D0", "B", 21, 0, 0, False),
        ("DBIG", "B", 20, 1, 4201, True), ("DBIG", "B", 21, 0, 4201, False),  # (node 4201 is no executor candidate: nothing to correct)
        ("D0", "G", 4, 1, 0, True), ("D0", "G", 5, 0, 0, False),
        ("D0", "A", 0, 1, 0, False), ("D0", "A", 9, 1, 0, True), ("D0", "A+1", 7, 1, 0, True), ("D0", "A", 7, 1, 0, True))
EDGES = {"all": _ALL, "subsequences": _SUB}
# S: records of one ticket that the row model serves, whose driver's slot is below 4 096 and whose requests are whole units (a
# request off its unit is never looked up).  The sixty warm-up records of K = 1 and the served edges without DBIG and A+1.
DEEP_S = {"all": 67, "subsequences": 67}
# F: records of one ticket with K > 0 in whole units that look a row up and must fall back: DBIG's and the NOT SERVED ones.
DEEP_F = {"all": 11, "subsequences": 9}


def deep_case(variant):
    """The deep cluster with the orders of `variant` and its ticket: avail, sched, D, X, drv, exe, k, edges (the declared rows of
    EDGES[variant]), first_edge (index of the first edge record), s, f."""
    assert variant in DEEP_VARIANTS
    n = N_DEEP
    avail = np.zeros((n, 3), dtype=np.int64)
    avail[:4064] = [500, 32 * GIB, 0]
    avail[4064:4200] = [8 * CPU, 32 * GIB, 0]
    avail[4200:] = [16 * CPU, 64 * GIB, 0]
    avail[4210:4214, 2] = 2
    avail[1] = [500, 33 * GIB, 1]  # THE UNITS (see the module's text): without this node no request here would have a scaled form
    nodes = np.arange(n, dtype=np.uint32)
    if variant == "all":
        D, X = nodes.copy(), nodes.copy()
    else:
        X = nodes[~((nodes >= 4064) & (nodes % 3 == 1))]
        D = nodes[~np.isin(nodes, (4064, 4066, 4200))]
    recs = [("D0", shape, kk) for shape, kk, count in WARM_UP for _ in range(count)]
    first_edge = len(recs)
    recs += [(d, e, kk) for d, e, kk, _, _, _ in EDGES[variant]]
    drv = np.array([REQUESTS[d] for d, _, _ in recs], dtype=np.int64)
    exe = np.array([REQUESTS[e] for _, e, _ in recs], dtype=np.int64)
    k = np.array([kk for _, _, kk in recs], dtype=np.int32)
    return SimpleNamespace(variant=variant, avail=avail, sched=avail.copy(), D=D, X=X, drv=drv, exe=exe, k=k, names=recs,
                           edges=EDGES[variant], first_edge=first_edge, s=DEEP_S[variant], f=DEEP_F[variant])


# ------------------------------------------------------------------------------------------- streams through the worker


def apps_of(drv, exe, k):
    import gangfit

    apps, _ = gangfit.with_offsets(gangfit.make_apps(np.asarray(drv, dtype=np.int64), np.asarray(exe, dtype=np.int64),
                                                     np.asarray(k, dtype=np.int32)))
    return apps


def launch_answers(ctx, apps):
    """(d_apps, results, placements, mask of the placement words of feasible records) of one launch on `apps` (with offsets)."""
    import gangfit
    import torch
    from gangfit import _native as N

    dev = torch.device("cuda:0")
    total_k = int(apps["k"].sum())
    d_apps = torch.from_numpy(apps.view(np.uint8).copy()).to(dev)
    res = torch.zeros(len(apps) * 16, dtype=torch.uint8, device=dev)
    exe = torch.zeros(total_k + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.fit_batch_dev(gangfit.GF_MODE_INDEPENDENT, gangfit.GF_ALGO_TIGHTLY_PACK, len(apps), d_apps.data_ptr(), res.data_ptr(),
                      exe.data_ptr(), total_k)
    torch.cuda.synchronize()
    feas = res.cpu().numpy().view(N.RESULT_DTYPE)["has_capacity"] != 0
    mask = np.zeros(total_k + 1, dtype=bool)
    for a in np.nonzero(feas)[0]:
        mask[int(apps["exec_off"][a]): int(apps["exec_off"][a]) + int(apps["k"][a])] = True
    return d_apps, res, exe, torch.from_numpy(mask).to(dev), feas


def stream(ctx, tickets, host_outputs=False, stop=True, leave_after=False, answers=None):
    """Posts the tickets (a list of record arrays; identical objects share one upload and one launch) as ONE stream, waits, stops
    the worker, compares every ticket with the launch on its records.  Returns the feasibility vectors per distinct array.
    stop False: the tickets are waited for and the worker is left resident. leave_after: a bounded stream (GF_WORKER_LEAVE_AFTER on the last
    ticket).  answers: {id(array): launch_answers(ctx, array)} made earlier on the installed snapshot — no launch happens here then."""
    import gangfit
    import torch
    from gangfit import _native as N

    dev = torch.device("cuda:0")
    known = dict(answers or {})
    for t in tickets:
        if id(t) not in known:
            known[id(t)] = launch_answers(ctx, t)
    res, exe, batches = [], [], []
    for t in tickets:
        d_apps, _, w_exe, _, _ = known[id(t)]
        if host_outputs:
            res.append(torch.zeros(len(t) * 16, dtype=torch.uint8).pin_memory())
            exe.append(torch.zeros(len(w_exe), dtype=torch.int32).pin_memory())
        else:
            res.append(torch.zeros(len(t) * 16, dtype=torch.uint8, device=dev))
            exe.append(torch.zeros(len(w_exe), dtype=torch.int32, device=dev))
        batches.append((len(t), d_apps.data_ptr(), res[-1].data_ptr(), exe[-1].data_ptr(), len(w_exe) - 1,
                        N.GF_WORKER_HOST_OUTPUTS if host_outputs else 0))
    torch.cuda.synchronize()
    if leave_after:
        first = ctx.worker_submit_prepared(gangfit.GF_ALGO_TIGHTLY_PACK, ctx.worker_batches(batches, leave_after=True))
    else:
        first = ctx.worker_submit_dev(gangfit.GF_ALGO_TIGHTLY_PACK, batches)
    ctx.worker_wait(first, len(tickets))
    if stop:
        ctx.worker_stop()
        torch.cuda.synchronize()
    # (stop False: no device-wide wait, which would last until the worker idles out; every ticket was waited for, its answers
    #  were stored through to memory, and the comparisons below run on another stream than the worker's)
    bad = []
    for i, t in enumerate(tickets):
        _, w_res, w_exe, mask, _ = known[id(t)]
        if not torch.equal(res[i].to(dev), w_res):
            bad.append((i, "results"))
        if not torch.equal(exe[i].to(dev)[mask], w_exe[mask]):
            bad.append((i, "placements"))
    assert not bad, bad[:8]
    return {k: v[4] for k, v in known.items()}
