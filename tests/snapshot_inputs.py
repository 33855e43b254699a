"""The problems of tests/magnitudes.py as inputs of gf_snapshot_build (Context.build_snapshot / oracle.pysnapshot.build), so that
the tables a decision reads are the ones the DEVICE built (gangfit_snapshot.hip: finalize_slots_kernel, finalize_reduce_kernel,
finalize_narrow_zones_kernel) from values at the edges of the quantity contract.

A helper module, not a test file; tests/test_snapshot_inputs_cpu.py checks what it promises.

The build can only express available = allocatable - (usage + overhead) with usage >= 0, every reservation entry below 2^61 and
every node's entries summing below 2^62 (check_reservations, gangfit_api_snapshot.cpp).  So, per node and dimension:

  avail  = max(p.avail, -(QMAX - 1))      -QMAX itself would need three entries; nothing else of magnitudes.py is touched
  sched' = max(p.sched, avail, 0)         the build has no used < 0 (available above schedulable)
  alloc  = sched', no overhead
  usage  = sched' - avail, as at most two entries of at most 2^61 - 1 each; where that would pass 2 (2^61 - 1), sched' is first
           lowered to max(avail, 0)

The problem's own orders are dropped (the build decides the order); its zones travel as they are — the sparse ids 3, 10, 17
with n_zones = max + 1, the empty ids in between included.
"""
import numpy as np

from magnitudes import QMAX
from oracle import pysnapshot as ps

ENTRY_MAX = (1 << 61) - 1  # the largest reservation entry gf_snapshot_build admits
EDGE_NODES = 5             # magnitudes.narrow_edge puts its edge values on nodes 0 .. 4
CANDIDATES = ("all", "drawn")


def tables(p):
    """(avail, sched') the build must reproduce for problem p: the clamps of the module docstring."""
    avail = np.maximum(np.asarray(p[0], dtype=np.int64), -(QMAX - 1))
    sched = np.maximum(np.maximum(np.asarray(p[1], dtype=np.int64), avail), 0)
    # (sched' <= 2^62 - 1 and avail >= -(2^62 - 2): the difference stays below 2^63)
    sched = np.where(sched - avail > 2 * ENTRY_MAX, np.maximum(avail, 0), sched)
    return avail, sched


def as_build_inputs(p, rng, candidates):
    """Keyword arguments of Context.build_snapshot / oracle.pysnapshot.build for problem p of magnitudes.cases(regime).
    candidates: "all" = every node READY | DRIVER_CANDIDATE; "drawn" = 85 % READY, 75 % DRIVER_CANDIDATE, 5 % UNSCHEDULABLE,
    nodes 0 .. 4 kept as full candidates."""
    avail, sched = tables(p)
    n = len(avail)
    usage = sched - avail
    first = np.minimum(usage, ENTRY_MAX)
    second = usage - first
    assert usage.min() >= 0 and second.max(initial=0) <= ENTRY_MAX
    has1, has2 = first.any(axis=1), second.any(axis=1)
    res_node = np.concatenate([np.nonzero(has1)[0], np.nonzero(has2)[0]]).astype(np.uint32)
    res_req = np.concatenate([first[has1], second[has2]]).astype(np.int64).reshape(-1, 3)
    mix = rng.permutation(len(res_node))  # the replay adds in any order
    res_node, res_req = res_node[mix], res_req[mix]
    name_rank = rng.permutation(n).astype(np.uint32)
    if candidates == "all":
        flags = np.full(n, ps.READY | ps.DRIVER_CANDIDATE, dtype=np.uint32)
    elif candidates == "drawn":
        flags = (np.where(rng.random(n) < 0.85, ps.READY, 0) | np.where(rng.random(n) < 0.75, ps.DRIVER_CANDIDATE, 0) |
                 np.where(rng.random(n) < 0.05, ps.UNSCHEDULABLE, 0)).astype(np.uint32)
        flags[:EDGE_NODES] = ps.READY | ps.DRIVER_CANDIDATE
    else:
        raise ValueError(candidates)
    zone = np.asarray(p[2], dtype=np.uint32)
    return dict(alloc=sched, node_flags=flags, name_rank=name_rank, overhead=None, res_node=res_node, res_req=res_req,
                zone=zone, n_zones=int(zone.max()) + 1)
