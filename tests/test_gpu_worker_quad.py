"""The resident worker's tightly-pack decisions read the snapshot's int32 twin as one 16-byte record per slot, {cpu, mem, gpu, node}
(NodeTable::nquad; NarrowView, gangfit_kernels.hip), and take every node id they write from that record.  Two producers write it
— the host layout (gangfit_slot_layout.h) and finalize_narrow_zones_kernel — in the pass that writes the columns.  What can go
wrong: a record that is not its slot's columns and node (at the sentinel, in a ragged last chunk, behind group 0 of the chunk
index, on a slot the executor order leaves out), and a STALE record after an install that changes the values, the node order or
whether the twin exists at all.  Every answer of a bounded worker stream, longer than the ticket ring, is compared bit for bit
with gf_fit_batch_dev on the same inputs: that launch decides in int64 and never reads the records.
`python -m pytest tests -m gpu`."""
import numpy as np
import pytest

import gangfit
from test_gpu_worker_operands import A_FALLBACK, A_INFEASIBLE, A_K0, A_ODD, A_RUN, GIB, TIGHT, _batch, _Stream

pytestmark = pytest.mark.gpu

STREAM = 70  # tickets: more than the ring of 64
READY_DRIVER = 2 | 4  # GF_NODE_READY | GF_NODE_DRIVER_CANDIDATE


def _cluster(n_nodes, seed=0x0A9):
    """cpu in whole cores, memory in whole GiB (the units are the columns' gcds), a gpu on every thirteenth node; node 0 and the last
    node hold two of the fallback gang's executors and nothing to spare (tests/test_gpu_worker_operands.py), at any size."""
    rng = np.random.default_rng(seed)
    avail = np.zeros((n_nodes, 3), dtype=np.int64)
    avail[:, 0] = 1000 * rng.choice([64, 67, 72], size=n_nodes)
    avail[:, 1] = GIB * rng.choice([64, 97, 128], size=n_nodes)
    avail[::13, 2] = rng.choice([1, 2, 4, 8], size=len(avail[::13]))
    avail[0] = (60000, 64 * GIB, 0)
    avail[n_nodes - 1] = (60000, 64 * GIB, 0)
    if n_nodes > 3:
        avail[1, :2] = (67000, 97 * GIB)
        avail[n_nodes - 2, :2] = (67000, 97 * GIB)
    return avail


def _orders(n, layout):
    order = np.arange(n, dtype=np.uint32)
    if layout == "merged":
        return order, order
    if layout == "general":   # the two orders disagree: driver positions go through dslot
        return order[::-1].copy(), order
    assert layout == "left_out"  # every third node is no executor candidate (still a driver candidate: the layout stays merged)
    return order, order[order % 3 != 1].copy()


def _install(ctx, avail, layout="merged", perm=None):
    d, x = _orders(len(avail), layout)
    if perm is not None:
        d, x = perm[d], perm[x]
    ctx.set_snapshot(avail, avail.copy())
    ctx.set_orders(d, x)


def _serve(ctx, avail, n_tickets=STREAM):
    """The forty-application batch of test_gpu_worker_operands on the installed snapshot: the launch path's answers, then a stream."""
    drv, exe, k = _batch(avail)
    s = _Stream(ctx, TIGHT, drv, exe, k)
    ok = s.res["has_capacity"] != 0
    assert ok.sum() >= 10 and ok[A_K0] and not ok[A_INFEASIBLE] and ok[A_ODD]  # narrow and int64 decisions, K = 0, an infeasible gang
    s.run(n_tickets)
    return s


@pytest.mark.parametrize("layout", ["merged", "general"])
@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 130])
def test_sizes_around_a_chunk(n_nodes, layout):
    """1 node; 63: the sentinel closes the only chunk; 64: it is alone in chunk 1; 65 and 130: ragged last chunks."""
    avail = _cluster(n_nodes)
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail, layout)
        s = _serve(ctx, avail)
        if n_nodes >= 63:
            assert s.res["has_capacity"][A_RUN] and np.max(np.bincount(s.placement(A_RUN))) > 16  # forty on one node
            # the fallback gang took the fallback (wave_fallback on the record view): its first fitting driver candidate loses an
            # executor to the driver, the next candidate is taken (tests/test_gpu_worker_operands.py, _assert_categories)
            assert s.res["has_capacity"][A_FALLBACK]
            assert s.res["driver_node"][A_FALLBACK] == (1 if layout == "merged" else n_nodes - 2)
    finally:
        ctx.close()


def test_an_order_that_leaves_nodes_out():
    avail = _cluster(130)
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail, "left_out")
        s = _serve(ctx, avail)
        placed = np.concatenate([s.placement(a) for a in np.nonzero(s.res["has_capacity"])[0]])
        assert len(placed) > 100 and (placed % 3 != 1).all()
    finally:
        ctx.close()


def test_chunk_64_behind_group_zero():
    """4 160 nodes are 65 chunks of slots: chunk 64 is the one chunk behind group 0 of the chunk index.  Nodes 0 .. 4 095 are too small
    for any executor and for the larger drivers, so gangs have their driver, and all have their last executor, in chunk 64."""
    n_nodes, small = 4160, 4096
    avail = _cluster(n_nodes)
    avail[:small, 0] = 500
    avail[:small, 2] = 0
    avail[small + 13, 2] = 3
    drv, exe, k = _batch(avail)
    drv[::2, 0] = 500  # every other driver fits node 0
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail)
        s = _Stream(ctx, TIGHT, drv, exe, k)
        ok = np.nonzero(s.res["has_capacity"])[0]
        assert len(ok) >= 25
        assert (s.res["driver_node"][ok] >= small).any() and (s.res["driver_node"][ok] < 64).any()
        assert all(s.placement(a)[-1] >= small for a in ok if s.apps["k"][a] > 0)
        s.run(STREAM)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- the two producers

def _built_cluster(n_nodes, seed=0xB17):
    """Allocatable, reservation entries and the available they leave; memory differs from node to node, so the build's order (least
    memory first) is no order the test could have installed by accident."""
    rng = np.random.default_rng(seed)
    avail = _cluster(n_nodes, seed)
    avail[:, 1] = GIB * rng.permutation(np.arange(40, 40 + n_nodes))
    res_node = rng.integers(0, n_nodes, size=3 * n_nodes).astype(np.uint32)
    res_req = np.stack([1000 * rng.integers(0, 3, size=len(res_node)), GIB * rng.integers(0, 3, size=len(res_node)),
                        np.zeros(len(res_node), dtype=np.int64)], axis=1).astype(np.int64)
    alloc = avail.copy()
    np.add.at(alloc, res_node, res_req)
    flags = np.full(n_nodes, READY_DRIVER, dtype=np.uint32)
    return alloc, avail, res_node, res_req, flags, np.arange(n_nodes, dtype=np.uint32)


def _answers(s):
    return s.res.copy(), s.exec_nodes.copy()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_host_built_and_device_built_snapshots_of_one_cluster():
    """gf_snapshot_build, the resident build with usage applied, and set_snapshot + set_orders with the build's own orders."""
    n_nodes = 130
    alloc, avail, res_node, res_req, flags, ranks = _built_cluster(n_nodes)
    got = []
    ctx = gangfit.Context(0)
    try:
        d, x = ctx.build_snapshot(alloc, flags, ranks, res_node=res_node, res_req=res_req)
        assert np.array_equal(d, np.lexsort((ranks, avail[:, 0], avail[:, 1])))
        got.append(_answers(_serve(ctx, avail)))
    finally:
        ctx.close()
    ctx = gangfit.Context(0)
    try:
        ctx.set_cluster(alloc, flags, ranks)
        ctx.usage_apply(res_node, res_req)
        ctx.build_snapshot_resident(resident_usage=True, want_orders=False)
        got.append(_answers(_serve(ctx, avail)))
    finally:
        ctx.close()
    ctx = gangfit.Context(0)
    try:
        ctx.set_snapshot(avail, alloc)
        ctx.set_orders(d, x)
        got.append(_answers(_serve(ctx, avail)))
    finally:
        ctx.close()
    assert _same(got[0], got[1]) and _same(got[0], got[2])


def test_both_producers_write_the_same_records():
    """Nothing reads the records back, so a batch names every slot: memory and cpu grow with the node's place in the order, the
    driver of every gang lands on the first node and gang i's ONE executor — as large as node i, gpus included — on node i, the
    first it fits.
    Device-built and host-built, the worker's answers (node ids from the records, fits decided on the records' values) agree."""
    n_nodes = 130
    rng = np.random.default_rng(0x51D)
    place = rng.permutation(n_nodes)                  # node -> its place in the priority order
    avail = np.zeros((n_nodes, 3), dtype=np.int64)
    avail[:, 0] = 1000 * (8 + place)
    avail[:, 1] = GIB * (9 + place)
    order = np.argsort(place).astype(np.uint32)       # place -> node
    # every third place has gpus, more of them the later its place (more than a quarter of the order: no sparse gpu view, so the
    # host-built snapshot's gangs of gpu executors are decided on the records too)
    gpu_places = np.arange(2, n_nodes, 3)
    avail[order[gpu_places], 2] = 1 + np.arange(len(gpu_places))
    alloc = avail + np.array([1000, GIB, 0])
    res_node = np.arange(n_nodes, dtype=np.uint32)
    res_req = np.tile(np.array([1000, GIB, 0], dtype=np.int64), (n_nodes, 1))
    flags = np.full(n_nodes, READY_DRIVER, dtype=np.uint32)
    ranks = np.arange(n_nodes, dtype=np.uint32)
    gangs = np.arange(1, n_nodes)                     # gang for place 1 .. n - 1 (the driver names place 0)
    # ... and one more gang per gpu node whose executor is small but for its gpus: only the third word of the records decides that the
    # first node it fits is its own
    small = np.tile(np.array([1000, GIB, 0], dtype=np.int64), (len(gpu_places), 1))
    small[:, 2] = avail[order[gpu_places], 2]
    exe = np.concatenate([avail[order[gangs]], small])
    want_nodes = np.concatenate([order[gangs], order[gpu_places]])
    drv = np.tile(np.array([1000, GIB, 0], dtype=np.int64), (len(exe), 1))
    k = np.ones(len(exe), dtype=np.int32)
    got = []
    for built in (True, False):
        ctx = gangfit.Context(0)
        try:
            if built:
                d, x = ctx.build_snapshot(alloc, flags, ranks, res_node=res_node, res_req=res_req)
                assert np.array_equal(d, order) and np.array_equal(x, order)
            else:
                ctx.set_snapshot(avail, alloc)
                ctx.set_orders(order, order)
            s = _Stream(ctx, TIGHT, drv, exe, k)
            assert (s.res["has_capacity"] != 0).all() and (s.res["driver_node"] == order[0]).all()
            assert np.array_equal(s.exec_nodes[:len(exe)], want_nodes)  # every slot named, each gang on its own node
            s.run(STREAM)
            got.append(_answers(s))
        finally:
            ctx.close()
    assert _same(got[0], got[1])


# ---------------------------------------------------------------------------------------------- staleness: ONE context each

def test_a_second_set_orders_permutes_the_nodes():
    """Same values, another order: stale records would answer with the old node ids."""
    avail = _cluster(130)
    perm = np.random.default_rng(7).permutation(130).astype(np.uint32)
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail)
        first = _answers(_serve(ctx, avail))
        d, x = _orders(130, "merged")
        ctx.set_orders(perm[d], perm[x])
        second = _answers(_serve(ctx, avail))
        assert not np.array_equal(first[1], second[1])
    finally:
        ctx.close()


def test_a_usage_delta_and_a_resident_rebuild():
    """Same cluster, more usage: stale records would answer from the old values (and the old order)."""
    n_nodes = 130
    alloc, avail, res_node, res_req, flags, ranks = _built_cluster(n_nodes)
    ctx = gangfit.Context(0)
    try:
        ctx.set_cluster(alloc, flags, ranks)
        ctx.usage_apply(res_node, res_req)
        ctx.build_snapshot_resident(resident_usage=True, want_orders=False)
        first = _answers(_serve(ctx, avail))
        more_node = np.arange(0, n_nodes, 2, dtype=np.uint32)  # every other node loses most of what it has
        more_req = np.stack([avail[more_node, 0] - 3000, avail[more_node, 1] - 3 * GIB, np.zeros(len(more_node), dtype=np.int64)], axis=1)
        ctx.usage_apply(more_node, more_req)
        ctx.build_snapshot_resident(resident_usage=True, want_orders=False)
        avail2 = avail.copy()
        avail2[more_node] -= more_req
        second = _answers(_serve(ctx, avail2))
        assert not np.array_equal(first[1], second[1])
    finally:
        ctx.close()


def test_a_second_snapshot_with_other_units():
    avail = _cluster(130)
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail)
        first = _answers(_serve(ctx, avail))
        avail2 = avail.copy()
        avail2[:, 0] += 500 * (np.arange(130) % 2)   # half cores: the cpu unit is 500
        avail2[:, 1] += (GIB // 4) * (np.arange(130) % 4)
        avail2[0, :2] = (2500, 2 * GIB + GIB // 4)   # ... and the first node is nearly full: the placements move
        assert int(np.gcd.reduce(avail2[:, 0])) == 500 and int(np.gcd.reduce(avail2[:, 1])) == GIB // 4
        _install(ctx, avail2)
        second = _answers(_serve(ctx, avail2))
        _install(ctx, avail)
        third = _answers(_serve(ctx, avail))
        assert _same(first, third) and not np.array_equal(first[1], second[1])
    finally:
        ctx.close()


def test_a_snapshot_without_the_twin_and_one_with_it_again():
    """One odd byte: the memory unit is 1 and 64 GiB is not below 2^30 units — no narrow form (fill_narrow's criterion), the records of
    the install before must not be read; then a snapshot that has the form again, in another node order."""
    avail = _cluster(130)
    odd = avail.copy()
    odd[5, 1] += 1
    assert int(np.gcd.reduce(odd[:, 1])) == 1 and int(odd[:, 1].max()) >= 1 << 30
    perm = np.random.default_rng(11).permutation(130).astype(np.uint32)
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail)
        first = _answers(_serve(ctx, avail))
        _install(ctx, odd, perm=perm)
        second = _answers(_serve(ctx, odd))
        assert not np.array_equal(first[1], second[1])
        _install(ctx, avail, perm=perm[::-1].copy())
        third = _answers(_serve(ctx, avail))
        assert not np.array_equal(second[1], third[1])
    finally:
        ctx.close()
