"""FIFO chains of all six packers where the regions of the chain kernels' LDS layouts (for the wide and the zoned kernel:
csrc/gangfit_chain_lds.h) abut and their alignment pads appear — geometries the suite's round shapes skip —, bit for bit
against the oracle: failed_at, results, placements and gf_residual_get.

  nodes 65, 130, 4 100      2, 3 and 65 chunks: one and two words per shape-index row, the solo kernel's row stride at its floor of
                            four; odd chunk counts leave the regions behind the chunk maxima at 4 and 12 modulo 16
  zones 1, 3, 16 (15 for    odd n_views x n_shapes x words products, sixteen candidate views: every entry of ZonedShared / MfShared
  az-aware: 16 candidates)
  budgets                   the default (whole table in LDS), and the budget that keeps exactly one chunk in LDS and the rest in a
                            global tail (do.chain_lds_slots with target=64).  The zone-aware and minimal-fragmentation routes want
                            more than one chunk next to their fixed tables — at that budget the generic chain serves them —, so
                            where the table has more than two chunks they also run with exactly two in LDS (target=128).
  70 applications           70 distinct executor requests and 70 distinct driver requests: the staging refills of 16, 32 and 64
                            are crossed, shape ids 0 .. 63 are all handed out (the last row of every shape table is written) and six
                            requests stay unindexed.  Application 68 is not skippable and fits nowhere: 69 is not evaluated.
  packers 0 and 1 once more with one request that is no multiple of the table's memory unit: the wide LDS chain serves.

`python -m pytest tests/test_gpu_chain_lds_edges.py -m gpu`."""
import numpy as np
import pytest

import deep_orders as do
import gangfit
import stress_lib
from oracle import binding as ob

pytestmark = pytest.mark.gpu

FIFO = gangfit.GF_MODE_FIFO_CHAIN
CPU, GIB = 1000, 1 << 30
N_APPS, ENDS_AT = 70, 68


@pytest.fixture(scope="module")
def ctx():
    with gangfit.Context(0) as c:
        yield c


def _cluster(n, nz):
    rng = np.random.default_rng([0xC1D5, n, nz])
    avail = np.stack([rng.integers(8, 65, size=n) * CPU, rng.integers(16, 257, size=n) * GIB, rng.integers(0, 5, size=n)], axis=1)
    avail = avail.astype(np.int64)
    avail[0], avail[1] = [9 * CPU, 17 * GIB, 1], [10 * CPU, 18 * GIB, 2]  # the table's units: one core, one GiB, one gpu
    sched = avail + np.stack([rng.integers(0, 9, size=n) * CPU, rng.integers(0, 65, size=n) * GIB, np.zeros(n, dtype=np.int64)], axis=1)
    zone = (rng.permutation(n) % nz).astype(np.uint32)
    order = rng.permutation(n).astype(np.uint32)
    return avail, sched, zone, order


def _queue(wide):
    i = np.arange(N_APPS)
    exe = np.stack([(1 + i % 7) * CPU, (1 + i // 7) * GIB, np.zeros(N_APPS, dtype=np.int64)], axis=1).astype(np.int64)
    drv = np.stack([(1 + i % 5) * CPU, (1 + i // 5) * GIB, (i % 11 == 0).astype(np.int64)], axis=1).astype(np.int64)
    assert len({tuple(r) for r in exe}) == N_APPS and len({tuple(r) for r in drv}) == N_APPS
    k = (1 + (3 * i) % 5).astype(np.int32)
    flags = np.ones(N_APPS, dtype=np.uint32)
    k[ENDS_AT], flags[ENDS_AT] = 100000, 0
    if wide:
        exe[5, 1] += 1  # no multiple of the memory unit: no scaled form, the wide chain kernel serves the batch
    return drv, exe, k, flags


@pytest.mark.parametrize("nz", [1, 3, 15, 16])
@pytest.mark.parametrize("n", [65, 130, 4100])
def test_chains_at_the_layouts_edges(ctx, n, nz):
    avail, sched, zone, order = _cluster(n, nz)
    n_slots = n + 1  # every node in both orders: the merged layout, one slot per node and the sentinel
    ctx.set_snapshot(avail, sched)
    ctx.set_zones(zone)
    ctx.set_orders(order, order)
    assert do.n_eval_zones((avail, sched, zone, order, order)) == nz
    default = ctx.device_info()["lds_bytes_per_cu"]
    algos = (3,) if nz == 15 else (0, 1, 2, 3, 4, 5)
    runs = [(algo, False, target) for algo in algos for target in (None, 64) + ((128,) if algo >= 2 and n_slots > 128 else ())]
    if nz != 15:
        runs += [(algo, True, target) for algo in (0, 1) for target in (None, 64)]
    refs = {}
    try:
        for algo, wide, target in runs:
            where = f"n={n} zones={nz} algo={algo} wide={wide} front={target}"
            cols = _queue(wide)
            if (algo, wide) not in refs:
                refs[algo, wide] = ob.fit_fifo_chain(algo, avail, ob.make_apps(*cols), order, order, sched=sched, zone=zone)
            ref = refs[algo, wide]
            budget = default if target is None else do.chain_lds_slots(algo, None, n_slots, nz, target=target)
            ctx.set_option("lds_budget", budget)
            slots = do.chain_lds_slots(algo, budget, n_slots, nz)
            if target is None:
                assert slots is None or slots >= n_slots, where
            elif algo < 2 or target == 128:
                # (for the wide runs this is the narrow solo route's front at this budget: the wide kernel sizes its own front
                #  from fifo_v2_lds_bytes, a few slots at most here, and its size is not pinned by this test)
                assert slots == target < n_slots, where
            else:
                assert slots is None, where  # one chunk next to the fixed tables: the generic chain serves
            print(f"{where}: budget {budget}, LDS slots {slots} of {n_slots}")
            gpu = ctx.fit_batch(FIFO, algo, gangfit.make_apps(*cols))
            assert gpu.failed_at == ref.failed_at == ENDS_AT, where
            assert stress_lib.same(gpu, ref, True) is None, where
            assert np.array_equal(ctx.residual(), ref.avail_after), where
    finally:
        ctx.set_option("lds_budget", default)
