"""FIFO chains on the FLOORED narrow form (csrc/gangfit_floor_units.h): tables whose values share no unit — every node carries
a remainder, memory reaches 512 GiB, so the column gcds are 1 and the table has no exact int32 form — against queues whose
requests do share one.  The LDS chain kernels must serve them (gf_chain_cache_stats, gf_chain_units) and give what the literal
oracle's full replay gives, bit for bit: results, placements, failed_at and gf_residual_get.

Node values are planted where floor(value / unit) decides: A = rho u + (u - 1) against a request of (rho + 1) u, which must not fit;
A = rho u against rho u, which fits; -1, 0 and u - 1; a negative value with a remainder.

`python -m pytest tests/test_gpu_floor_units.py -m gpu`."""
from math import gcd

import numpy as np
import pytest

import deep_orders as do
import gangfit
import snapshot_inputs as si
import stress_lib
from oracle import binding as ob
from oracle import pysnapshot as ps

pytestmark = pytest.mark.gpu

FIFO = gangfit.GF_MODE_FIFO_CHAIN
ALGOS = (0, 1, 2, 3, 4, 5)
CPU_GRID, MIB, GIB = 250, 1 << 20, 1 << 30
UC, UM = 250, 256 * MIB  # the units the queues' requests share: a quarter core, 256 MiB (and one gpu)
B = 1 << 30
N_APPS, ENDS_AT = 48, 44
TOP = 2047  # the largest node holds TOP * UM + UM - 1 bytes: a request of (TOP + 1) * UM = 512 GiB fits nowhere


@pytest.fixture(scope="module")
def ctx():
    with gangfit.Context(0) as c:
        yield c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _col_gcd(col):
    g = 0
    for v in col.tolist():
        g = gcd(g, abs(int(v)))
    return g


def _cluster(n, nz, remainders=True):
    """Columns that are multiples of (250 milli-cores, 1 MiB, 1) plus a remainder per node (none with remainders=False: the exact
    twin), memory up to 512 GiB, and the planted nodes 0 .. 9.  Every node in both orders: the merged layout."""
    rng = np.random.default_rng([0xF100, n, nz])
    cpu = rng.integers(8, 257, size=n) * CPU_GRID
    mem = rng.integers(16 * 1024, 500 * 1024, size=n) * MIB
    gpu = rng.integers(0, 5, size=n)
    if remainders:
        cpu = cpu + rng.integers(0, CPU_GRID, size=n)
        mem = mem + rng.integers(0, MIB, size=n)
        # rho u + (u - 1) and rho u, the two largest: a driver of (TOP + 1) UM fits nowhere, one of 2040 UM fits exactly these two
        mem[0], mem[1] = TOP * UM + UM - 1, 2040 * UM
        mem[2], mem[3], mem[4] = -1, 0, UM - 1  # floors -1, 0, 0
        mem[5] = -3 * UM + 12345  # a negative value with a remainder: floor -3
        cpu[6], cpu[7], cpu[8] = -1, 0, UC - 1
        cpu[9] = 40 * UC + UC - 1  # ... and in cpu: 41 quarter cores do not fit, 40 do
        mem[9] = 300 * GIB + 1
        mem[10], mem[11] = 17 * GIB + 1, 17 * GIB + 2  # consecutive values: the memory gcd is 1 whatever else is drawn
        cpu[10], cpu[11] = 9001, 9002
    else:
        mem[0], mem[1] = TOP * UM, 2040 * UM
    avail = np.stack([cpu, mem, gpu], axis=1).astype(np.int64)
    sched = np.maximum(avail, 0) + np.stack([rng.integers(0, 9, size=n) * 1000 + 7, rng.integers(0, 65, size=n) * GIB + 5,
                                             np.zeros(n, dtype=np.int64)], axis=1)
    zone = (rng.permutation(n) % nz).astype(np.uint32)
    order = rng.permutation(n).astype(np.uint32)
    return avail, sched.astype(np.int64), zone, order


def _queue(n_apps=N_APPS, ends_at=ENDS_AT, um=UM):
    """Requests on the grid (UC, um, 1), the grid itself among them (the units are exactly these); a gang of gpu executors, executors
    that ask for no memory and for no cpu, the two planted drivers, gangs too large for the cluster, and — ends_at — one application
    that is not skippable and fits nowhere: the chain ends there."""
    i = np.arange(n_apps)
    exe = np.stack([(1 + i % 7) * UC, (1 + (i * 5) % 24) * 16 * um, np.zeros(n_apps, dtype=np.int64)], axis=1).astype(np.int64)
    drv = np.stack([(1 + i % 5) * UC, (1 + (i * 3) % 40) * um, (i % 11 == 0).astype(np.int64)], axis=1).astype(np.int64)
    k = (1 + (3 * i) % 6).astype(np.int32)
    flags = np.ones(n_apps, dtype=np.uint32)
    exe[0], drv[0] = [UC, um, 0], [UC, um, 0]
    exe[3, 2], k[3] = 1, 3  # a gpu gang
    exe[5, 1] = 0  # a zero-request dimension: memory, then cpu
    exe[6, 0] = 0
    drv[7, 1] = (TOP + 1) * um * (UM // um)  # 512 GiB: no node, not even rho u + (u - 1)
    drv[8, 1] = 2040 * um * (UM // um)  # rho u: nodes 0 and 1 alone
    drv[9, 0] = 41 * UC  # cpu: 40 u + (u - 1) does not hold 41 u
    k[10] = 30000  # a gang the cluster cannot host (skippable)
    if n_apps > 20:
        exe[20, 1], k[20] = 400 * um * (UM // um), 12
    if ends_at is not None:  # (its driver asks for the 512 GiB no node has: it ends the chain on a cluster of any size)
        k[ends_at], flags[ends_at], drv[ends_at, 1] = 100000, 0, (TOP + 1) * um * (UM // um)
    return drv, exe, k, flags


def _install(c, cl):
    avail, sched, zone, order = cl
    c.set_snapshot(avail, sched)
    c.set_zones(zone)
    c.set_orders(order, order)


def _ref(algo, cl, cols):
    avail, sched, zone, order = cl
    return ob.fit_fifo_chain(algo, avail, ob.make_apps(*cols), order, order, sched=sched, zone=zone)


def _check(c, algo, cols, ref, where):
    gpu = c.fit_batch(FIFO, algo, gangfit.make_apps(*cols))
    assert stress_lib.same(gpu, ref, True) is None, (where, stress_lib.same(gpu, ref, True))
    assert gpu.failed_at == ref.failed_at, where
    assert np.array_equal(c.residual(), ref.avail_after), where
    return gpu


_REFS = {}


def _case(n, nz):
    """The cluster of (n, nz) and the oracle's full replay of the 48 applications for every packer, computed once per module run."""
    if (n, nz) not in _REFS:
        cl = _cluster(n, nz)
        cols = _queue()
        _REFS[n, nz] = (cl, cols, {algo: _ref(algo, cl, cols) for algo in ALGOS})
    return _REFS[n, nz]


@pytest.mark.parametrize("nz", [1, 3])
@pytest.mark.parametrize("n", [65, 130, 4100])
def test_parity_on_the_floored_form(ctx, n, nz):
    cl, cols, refs = _case(n, nz)
    avail = cl[0]
    assert all(_col_gcd(avail[:, j]) == 1 for j in (0, 1)) and int(avail[:, 1].max()) >= B  # gcd 1, no exact int32 form (narrow_ok = 0)
    assert do.n_eval_zones((avail, cl[1], cl[2], cl[3], cl[3])) == nz
    _install(ctx, cl)
    for algo in ALGOS:
        where = f"n={n} zones={nz} algo={algo}"
        ref = refs[algo]
        ev = ref.results["evaluated"] != 0
        assert ref.failed_at == ENDS_AT and (ref.results["has_capacity"][ev] != 0).any() and (ref.results["has_capacity"][ev] == 0).any(), where
        ctx.chain_cache_stats(reset=True)
        _check(ctx, algo, cols, ref, where)
        assert ctx.chain_cache_stats()[0] == 1, where  # an LDS chain kernel served
        assert ctx.chain_units() == (UC, UM, 1, 1), where


def test_route_witness_and_the_switch(ctx):
    """The floored form is what puts these chains on the LDS kernels: with narrow_floor = 0 the same batch takes the wide / generic
    kernels (no chain counted, no units) and answers the same — results, placements, residuals and the Filter's packing efficiency
    against the residual table, bit for bit."""
    cl, cols, refs = _case(130, 3)
    _install(ctx, cl)
    apps = gangfit.make_apps(*cols)
    last = ENDS_AT - 1  # the last application the chain committed nothing behind... of those evaluated: any feasible one serves
    try:
        for algo in ALGOS:
            where = f"algo={algo}"
            got = {}
            for floor in (1, 0):
                ctx.set_option("narrow_floor", floor)
                ctx.chain_cache_stats(reset=True)
                gpu = _check(ctx, algo, cols, refs[algo], (where, floor))
                assert ctx.chain_cache_stats()[0] == floor, (where, floor)
                assert ctx.chain_units() == ((UC, UM, 1, 1) if floor else (0, 0, 0, 0)), (where, floor)
                a = max(int(x) for x in np.nonzero(gpu.results["has_capacity"][:last + 1])[0])
                avg, counts = ctx.filter_efficiency(algo, apps[a], gpu.results[a], gpu.placement(a)[2], against="residual")
                got[floor] = (_bits(avg).tolist(), counts, ctx.residual().tobytes())
            assert got[1] == got[0], where
    finally:
        ctx.set_option("narrow_floor", 1)


def test_resume_and_new_units(ctx):
    """The queue plus one application resumes from the cached floored chain.  A new application that is no multiple of the cached
    units replays in the new ones; one with an odd byte has no unit to share and goes back to the wide kernels."""
    cl, _, _ = _case(130, 3)
    _install(ctx, cl)
    drv, exe, k, flags = _queue(ends_at=None)
    for algo in ALGOS:
        where = f"algo={algo}"
        head = tuple(c[:-1] for c in (drv, exe, k, flags))
        ctx.chain_cache_stats(reset=True)
        _check(ctx, algo, head, _ref(algo, cl, head), where)
        _check(ctx, algo, (drv, exe, k, flags), _ref(algo, cl, (drv, exe, k, flags)), where)
        chains, resumed, _, skipped = ctx.chain_cache_stats()
        assert (chains, resumed) == (2, 1) and skipped > 0 and ctx.chain_units() == (UC, UM, 1, 1), (where, chains, resumed, skipped)
        half = (drv.copy(), exe.copy(), k, flags)
        half[1][-1, 1] = UM // 2  # 128 MiB: the units halve, the checkpoints of the cached chain are of no use
        _check(ctx, algo, half, _ref(algo, cl, half), where)
        assert ctx.chain_cache_stats()[:2] == (3, 1) and ctx.chain_units() == (UC, UM // 2, 1, 1), where
        odd = (drv.copy(), exe.copy(), k, flags)
        odd[0][-1, 1] = 3 * UM + 1  # gcd 1 against 512 GiB: no narrow form of either kind
        _check(ctx, algo, odd, _ref(algo, cl, odd), where)
        assert ctx.chain_cache_stats()[:2] == (3, 1), where  # the wide kernels count no chain


EDGE_U = 1024
EDGES = (("table-at-bound", (B - 1) * EDGE_U + EDGE_U - 1, None, True), ("table-past-bound", B * EDGE_U, None, False),
         ("negative-at-bound", -(B - 1) * EDGE_U, None, True), ("negative-past-bound", -(B - 1) * EDGE_U - 1, None, False),
         ("request-at-bound", None, (B - 1) * EDGE_U, True), ("request-past-bound", None, B * EDGE_U, False))


@pytest.mark.parametrize("name,planted,asked,floored", EDGES, ids=[e[0] for e in EDGES])
def test_magnitude_edges(ctx, name, planted, asked, floored):
    """floor(value / unit) of exactly 2^30 - 1 is on the floored form and 2^30 off it; on the negative side -(2^30 - 1) u is on and
    one byte less — it floors to -2^30 — is off.  A request of 2^30 - 1 units is on, one of 2^30 off.  Unit 1024 bytes."""
    n = 65
    rng = np.random.default_rng(len(name))
    avail, sched, zone, order = _cluster(n, 3)
    avail = avail.copy()
    avail[:, 1] = rng.integers(1, 1 << 39, size=n) | 1  # below 2^29 units, odd bytes
    avail[12, 1] = (B - 2) * EDGE_U + 5  # (the driver of 2^30 - 1 units fits nowhere, or only the planted node)
    if planted is not None:
        avail[13, 1] = planted
    sched = np.maximum(avail, 0) + 3
    cl = (avail, sched, zone, order)
    drv, exe, k, flags = _queue(n_apps=24, ends_at=20, um=EDGE_U)
    drv[2, 1] = asked if asked is not None else (B - 1) * EDGE_U
    assert _col_gcd(avail[:, 1]) == 1 and int(avail[:, 1].max()) >= B
    _install(ctx, cl)
    for algo in ALGOS:
        where = f"{name} algo={algo}"
        ctx.chain_cache_stats(reset=True)
        _check(ctx, algo, (drv, exe, k, flags), _ref(algo, cl, (drv, exe, k, flags)), where)
        assert ctx.chain_cache_stats()[0] == (1 if floored else 0), where
        assert ctx.chain_units() == ((UC, EDGE_U, 1, 1) if floored else (0, 0, 0, 0)), where


def test_unit_of_2_32(ctx):
    """Requests of 4 GiB multiples only: the memory unit is 2^32 — the remainders do not fit an int32 — against arbitrary bytes up
    to 2^50."""
    g4 = 1 << 32
    avail, sched, zone, order = _cluster(130, 3)
    rng = np.random.default_rng(32)
    avail = avail.copy()
    avail[:, 1] = rng.integers(-(1 << 33), 1 << 50, size=len(avail)) | 1
    avail[0, 1], avail[1, 1], avail[2, 1] = 7 * g4 + g4 - 1, 7 * g4, -1
    sched = np.maximum(avail, 0) + 11
    cl = (avail, sched, zone, order)
    drv, exe, k, flags = _queue(um=UM)
    drv[:, 1], exe[:, 1] = drv[:, 1] // UM * g4, exe[:, 1] // UM * g4
    _install(ctx, cl)
    for algo in ALGOS:
        ctx.chain_cache_stats(reset=True)
        _check(ctx, algo, (drv, exe, k, flags), _ref(algo, cl, (drv, exe, k, flags)), f"algo={algo}")
        assert ctx.chain_cache_stats()[0] == 1 and ctx.chain_units() == (UC, g4, 1, 1), algo


def test_dimension_nobody_asks_for(ctx):
    """No gpu request in the queue and a gpu column that holds 2^40: the column takes the unit 2^11, the smallest power of two that
    brings it inside (-2^30, 2^30), and the residuals still come back to the byte."""
    avail, sched, zone, order = _cluster(130, 3)
    avail = avail.copy()
    avail[20, 2], avail[21, 2], avail[22, 2] = 1 << 40, (1 << 40) - 1, -5
    sched = np.maximum(avail, 0) + 2
    cl = (avail, sched, zone, order)
    drv, exe, k, flags = _queue()
    drv[:, 2], exe[:, 2] = 0, 0
    _install(ctx, cl)
    for algo in ALGOS:
        ctx.chain_cache_stats(reset=True)
        _check(ctx, algo, (drv, exe, k, flags), _ref(algo, cl, (drv, exe, k, flags)), f"algo={algo}")
        assert ctx.chain_cache_stats()[0] == 1 and ctx.chain_units() == (UC, UM, 1 << 11, 1), algo


_LONG = {}


def _long_case():
    """4 100 nodes, three zones, 140 applications without one that ends the chain: past the 128 applications between two checkpoints
    of the zone-aware chain on a table with a global tail."""
    if not _LONG:
        cl = _cluster(4100, 3)
        drv, exe, k, flags = _queue(n_apps=140, ends_at=None)
        k = np.minimum(k, 4).astype(np.int32)
        k[10] = 30000
        _LONG.update(cl=cl, cols=(drv, exe, k, flags))
    return _LONG


@pytest.mark.parametrize("algo,target", [(0, 64), (1, 64), (3, 128), (5, 128)])
def test_global_tail_and_resume_across_a_checkpoint(ctx, algo, target):
    """lds_budget as in test_gpu_chain_lds_edges.py: exactly one chunk (the solo kernel: delta checkpoints every 32 applications) or
    two (the zone-aware and single-az minimal-fragmentation chains: whole-table checkpoints every 128) of the 65 in LDS, the rest a
    global tail that starts from the floored snapshot.  The queue without its last application, then the queue: the second chain
    restores a checkpoint and evaluates the applications behind it."""
    w = _long_case()
    cl, cols = w["cl"], w["cols"]
    n_slots = len(cl[0]) + 1
    default = ctx.device_info()["lds_bytes_per_cu"]
    _install(ctx, cl)
    try:
        budget = do.chain_lds_slots(algo, None, n_slots, 3, target=target)
        ctx.set_option("lds_budget", budget)
        assert do.chain_lds_slots(algo, budget, n_slots, 3) == target < n_slots
        head = tuple(c[:-1] for c in cols)
        ctx.chain_cache_stats(reset=True)
        _check(ctx, algo, head, _ref(algo, cl, head), f"algo={algo} head")
        _check(ctx, algo, cols, _ref(algo, cl, cols), f"algo={algo} whole")
        chains, resumed, _, skipped = ctx.chain_cache_stats()
        assert (chains, resumed) == (2, 1) and skipped == 128 and ctx.chain_units() == (UC, UM, 1, 1), (chains, resumed, skipped)
    finally:
        ctx.set_option("lds_budget", default)


@pytest.mark.parametrize("setting,setting_name", [(0, "device"), (1, "host")])
def test_device_built_snapshot(ctx, setting, setting_name):
    """gf_snapshot_build with both finalize settings: a table built on the device reads back magnitudes only, the range the floored
    form is decided from is fetched when the first chain asks.  The floored form serves on both."""
    avail, sched, zone, _ = _cluster(130, 3)
    c = si.as_build_inputs((avail, sched, zone), np.random.default_rng(5), "all")
    ravail, rsched, D, X = ps.build(**c)
    assert np.array_equal(ravail, avail)
    cols = _queue()
    apps = ob.make_apps(*cols)
    ctx.set_option("snapshot_finalize_host", setting)
    try:
        ctx.build_snapshot(**c)
        assert ctx.build_info()[0] == (1 if setting == 0 else 2)
        for algo in ALGOS:
            where = f"finalize={setting_name} algo={algo}"
            ref = ob.fit_fifo_chain(algo, ravail, apps, D, X, sched=rsched, zone=c["zone"])
            ctx.chain_cache_stats(reset=True)
            _check(ctx, algo, cols, ref, where)
            assert ctx.chain_cache_stats()[0] == 1 and ctx.chain_units() == (UC, UM, 1, 1), where
    finally:
        ctx.set_option("snapshot_finalize_host", 0)


def test_a_view_builds_its_own(ctx):
    """A view aliases the parent's wide table and floors it for itself."""
    cl, cols, refs = _case(130, 3)
    _install(ctx, cl)
    view = ctx.view()
    try:
        for algo in (3, 0):
            view.chain_cache_stats(reset=True)
            _check(view, algo, cols, refs[algo], f"view algo={algo}")
            assert view.chain_cache_stats()[0] == 1 and view.chain_units() == (UC, UM, 1, 1), algo
        _check(ctx, 3, cols, refs[3], "parent")  # ... next to the parent's
    finally:
        view.close()


def test_an_exact_table_stays_exact(ctx):
    """The same cluster without the remainders has the exact form: the floored one is not tried (gf_chain_units out[3] = 0)."""
    cl = _cluster(130, 3, remainders=False)
    cols = _queue()
    _install(ctx, cl)
    for algo in ALGOS:
        ctx.chain_cache_stats(reset=True)
        _check(ctx, algo, cols, _ref(algo, cl, cols), f"exact algo={algo}")
        units = ctx.chain_units()
        assert ctx.chain_cache_stats()[0] == 1 and units[3] == 0 and all(u > 0 for u in units[:3]), (algo, units)
