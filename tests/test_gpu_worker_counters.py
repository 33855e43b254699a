"""The tightly-pack worker has two instances: fit_worker_kernel<tightly-pack>, with nothing of the scan counters compiled in, and the
counting one the host launches while gf_scan_stats is on (gangfit_worker.inc, launch_fit_worker).  What can go wrong: the wrong
instance launched — counters that stay zero while they are on (bench.py --full reads them through a short worker stream), or that
move while they are off — and a counting instance that decides or counts differently.  With the counters on, every ticket of a
worker stream adds exactly what ONE launch of gf_fit_batch_dev adds for the same batch (the launch path's formula: both run
wave_decide); with them off, they stay zero.  Answers are compared bit for bit either way.  `python -m pytest tests -m gpu`."""
import numpy as np
import pytest

import gangfit
from test_gpu_worker_operands import A_FALLBACK, TIGHT, _batch, _cluster, _install, _Stream

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_nodes, layout", [(130, "merged"), (130, "general"), (4300, "merged")])
def test_counters_on_are_the_launch_paths_and_off_stay_zero(n_nodes, layout):
    """130 nodes: group 0 only, both layouts; 4 300: chunks behind group 0 (the per-group and per-chunk updates of both counters)."""
    avail, sched, zone = _cluster(n_nodes)
    if n_nodes > 4096:  # (tests/test_gpu_worker_operands.py, test_chunks_behind_group_zero: no executor fits the first 4 200 nodes)
        avail[:4200, 0] = 500
        avail[:4200, 2] = 0
        sched = avail.copy()
    drv, exe, k = _batch(avail)
    if n_nodes > 4096:
        drv[:, 0] = 500
    ctx = gangfit.Context(0)
    try:
        _install(ctx, avail, sched, zone, layout=layout)
        ctx.scan_stats(enable=True, reset=True)
        s = _Stream(ctx, TIGHT, drv, exe, k)  # one launch, counted
        want = ctx.scan_stats(enable=True, reset=True)
        assert want[0] > 0 and want[1] > 0 and (n_nodes > 4096 or s.res["has_capacity"][A_FALLBACK])
        for n_tickets in (1, 3):
            s.run(n_tickets)
            assert ctx.scan_stats(enable=True, reset=True) == (n_tickets * want[0], n_tickets * want[1])
        # off: neither the worker nor a launch moves them
        assert ctx.scan_stats(enable=False, reset=True) == (0, 0)
        s.run(3)
        assert ctx.scan_stats(enable=False, reset=False) == (0, 0)
        # ... and on again, on the same context: the counting instance is launched again
        ctx.scan_stats(enable=True, reset=True)
        s.run(2)
        assert ctx.scan_stats(enable=False, reset=True) == (2 * want[0], 2 * want[1])
    finally:
        ctx.close()
