"""gf_filter_efficiency's contract, restated in numpy float64 and shared by test_filter_efficiency_cpu.py and
test_gpu_filter_efficiency.py.

The reference (computeAvgPackingEfficiencyForResult, internal/extender/resource.go:372-381) sums one PackingEfficiency per metadata
key in Go map-range order, which is unspecified.  The device sums in a FIXED tree (include/gangfit.h, gangfit_filter_eff.inc):

  1. nodes 64c .. 64c + 63 form chunk c; a node that is no key (not a member, or past n_nodes) contributes +0.0; the chunk's
     partial is the balanced binary tree over its 64 positions (2i with 2i + 1, then pairs of pairs, ... six levels);
  2. the partials are padded with +0.0 to a multiple of 64 and added per position l = c mod 64, in ascending c, onto +0.0;
  3. the 64 sums are added by the same balanced tree.

cpu, memory, gpu (over the keys with a schedulable gpu) and max share the tree; len and nodesWithGPU are integers.  The per-node
efficiencies come from the oracle (held to bit identity with the device by tests/test_gpu_zones.py)."""
import numpy as np

from oracle import binding as ob

GIB = 1 << 30
MIB = 1 << 20
RESERVES_EXECUTORS = {ob.ALGO_TIGHTLY_PACK: True, ob.ALGO_DISTRIBUTE_EVENLY: True, ob.ALGO_MINIMAL_FRAGMENTATION: False,
                      ob.ALGO_AZ_AWARE_TIGHTLY_PACK: True, ob.ALGO_SINGLE_AZ_TIGHTLY_PACK: True,
                      ob.ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION: False}
ZONE_AWARE = (ob.ALGO_AZ_AWARE_TIGHTLY_PACK, ob.ALGO_SINGLE_AZ_TIGHTLY_PACK, ob.ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION)
ALL_ALGOS = tuple(sorted(RESERVES_EXECUTORS))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def tree64(v):
    """The balanced binary tree over the last axis (64 positions): 2i with 2i + 1, then pairs of pairs, ..."""
    v = np.asarray(v, dtype=np.float64)
    assert v.shape[-1] == 64
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def node_efficiencies(algo, avail, sched, drv, exe, driver_node, exec_nodes):
    """(n, 3) PackingResult.PackingEfficiencies from the oracle; the minimal-fragmentation packers leave the driver only in
    `reserved` (minimal_fragmentation.go:59-91)."""
    ex = exec_nodes if RESERVES_EXECUTORS[algo] else []
    return ob.packing_efficiency(avail, sched, drv, exe, driver_node, ex)[0]


def addends(eff, sched, members=None):
    """(4, n) the addends of cpu | memory | gpu | max per node, +0.0 where the node is no key; (n,) key, (n,) key with gpu."""
    eff = np.asarray(eff, dtype=np.float64).reshape(-1, 3)
    sched = np.asarray(sched, dtype=np.int64).reshape(-1, 3)
    key = np.ones(len(eff), dtype=bool) if members is None else np.asarray(members, dtype=bool)
    has_gpu = key & (sched[:, 2] != 0)
    add = np.zeros((4, len(eff)), dtype=np.float64)
    add[0, key] = eff[key, 0]
    add[1, key] = eff[key, 1]
    add[2, has_gpu] = eff[has_gpu, 2]
    add[3, key] = np.maximum(eff[key, 2], np.maximum(eff[key, 0], eff[key, 1]))
    return add, key, has_gpu


def finish(sums, n_len, n_gpu):
    if n_len == 0:
        return np.zeros(4, dtype=np.float64)  # WorstAvgPackingEfficiency
    length = np.float64(n_len)
    return np.array([sums[0] / length, sums[1] / length, np.float64(1.0) if n_gpu == 0 else sums[2] / np.float64(n_gpu),
                     sums[3] / length], dtype=np.float64)


def restate(eff, sched, members=None):
    """The device's summation tree -> (avg (4,), (len, nodesWithGPU))."""
    add, key, has_gpu = addends(eff, sched, members)
    n = add.shape[1]
    n_chunks = (n + 63) // 64
    n_pad = ((n_chunks + 63) // 64) * 64
    padded = np.zeros((4, n_pad * 64), dtype=np.float64)
    padded[:, :n] = add
    part = tree64(padded.reshape(4, n_pad, 64))  # levels 1 and 2: (4, n_pad)
    rows = part.reshape(4, n_pad // 64, 64)
    acc = np.zeros((4, 64), dtype=np.float64)
    for g in range(rows.shape[1]):  # ascending chunk order per position
        acc = acc + rows[:, g, :]
    sums = tree64(acc)  # level 3
    n_len, n_gpu = int(key.sum()), int(has_gpu.sum())
    return finish(sums, n_len, n_gpu), (n_len, n_gpu)


def sequential(eff, sched, members=None, order=None):
    """ComputeAvgPackingEfficiency's own loop over the keys in `order` (default: node-index order, the oracle's)."""
    add, key, has_gpu = addends(eff, sched, members)
    order = np.arange(add.shape[1]) if order is None else np.asarray(order)
    sums = [0.0, 0.0, 0.0, 0.0]
    for n in order:
        if key[n]:
            sums[0] += float(add[0, n])
            sums[1] += float(add[1, n])
            if has_gpu[n]:
                sums[2] += float(add[2, n])
            sums[3] += float(add[3, n])
    return finish(np.array(sums), int(key.sum()), int(has_gpu.sum()))


def reorder_bound(eff, sched, members=None):
    """(4,) 2 (n - 1) 2^-53 sum|e_i| / len per field: two sums of the same n addends in any two orders differ by no more
    (each is within (n - 1) 2^-53 sum|e_i| of the exact sum, to first order)."""
    add, key, _ = addends(eff, sched, members)
    n = int(key.sum())
    if n == 0:
        return np.zeros(4)
    return 2.0 * (n - 1) * 2.0 ** -53 * np.abs(add).sum(axis=1) / n


def oracle_sum(algo, avail, sched, drv, exe, driver_node, exec_nodes, members=None):
    """The oracle's sequential sum (go_packing_efficiency's average) over the keys: with a member row, over the members' rows
    alone — placements on non-members fall out with their keys."""
    avail = np.asarray(avail, dtype=np.int64).reshape(-1, 3)
    sched = np.asarray(sched, dtype=np.int64).reshape(-1, 3)
    ex = [int(v) for v in exec_nodes] if RESERVES_EXECUTORS[algo] else []
    if members is None:
        return ob.packing_efficiency(avail, sched, drv, exe, int(driver_node), ex)[1]
    m = np.asarray(members, dtype=bool)
    if not m.any():
        return np.zeros(4)
    compact = np.cumsum(m) - 1
    gone = int(m.sum())  # an index past the compact table: the oracle ignores it
    d = int(compact[driver_node]) if m[driver_node] else gone
    return ob.packing_efficiency(avail[m], sched[m], drv, exe, d, [int(compact[v]) for v in ex if m[v]])[1]


class Problem:
    pass


def problem(seed, n, dyadic, n_apps=6, n_zones=1, gpus=True, cpu_request=None, mem_unit=1, merged=False):
    """A cluster of n nodes, a queue of n_apps skippable applications that fits it, and both priority orders.
    dyadic: schedulable quantities are powers of two (cpu in whole cores, memory in bytes) and every used or requested quantity
    is a multiple of whole cores / MiB, so that every per-node efficiency is a dyadic rational with few bits and any order of
    addition gives the same bits.  Otherwise quantities are arbitrary (quarter cores, odd bytes; cpu_request in milli, e.g. 1500:
    the Value() rounding).  Either way the cluster holds a node with available above schedulable (a negative efficiency), an
    overcommitted node (above 1), a node with nothing schedulable (normalizeResource) and, from 3 nodes on, a node in neither
    order.  mem_unit: every memory quantity is a multiple of it (4096: the table has a scaled int32 form); merged: both orders are
    subsequences of one priority order (with mem_unit, what the LDS chain kernels and with them the chain cache serve)."""
    rng = np.random.default_rng(seed)
    p = Problem()
    sched = np.zeros((n, 3), dtype=np.int64)
    if dyadic:
        sched[:, 0] = 1000 * (1 << rng.integers(3, 7, size=n))
        sched[:, 1] = np.int64(1) << rng.integers(33, 36, size=n)
        used_cpu = 1000 * rng.integers(0, 5, size=n)
        used_mem = MIB * rng.integers(0, 4096, size=n)
    else:
        sched[:, 0] = 250 * rng.integers(16, 256, size=n)
        sched[:, 1] = mem_unit * rng.integers(8 * GIB // mem_unit, 256 * GIB // mem_unit, size=n)
        used_cpu = rng.integers(0, 3000, size=n)
        used_mem = mem_unit * rng.integers(0, 6 * GIB // mem_unit, size=n)
    if gpus:
        sched[:, 2] = rng.choice([0, 0, 1, 2, 4, 8], size=n)
    avail = sched.copy()
    avail[:, 0] -= used_cpu
    avail[:, 1] -= used_mem
    avail[:, 2] -= np.minimum(sched[:, 2], rng.integers(0, 3, size=n))
    special = rng.permutation(n)
    if n >= 2:
        avail[special[0]] = sched[special[0]] + [2000, 3 * GIB, 0]  # available above schedulable
    if n >= 4:
        avail[special[1]] = [-1000, -GIB, 0]  # overcommitted
        sched[special[2]] = 0  # nothing schedulable
        avail[special[2]] = 0
    in_d = rng.random(n) < 0.8
    in_x = rng.random(n) < 0.8
    if n >= 3:
        in_d[special[-1]] = in_x[special[-1]] = False  # a key that owns no slot
    in_d[special[n // 2]] = in_x[special[n // 2]] = True
    p.D = rng.permutation(np.nonzero(in_d)[0]).astype(np.uint32)
    p.X = rng.permutation(np.nonzero(in_x)[0]).astype(np.uint32)
    if merged:
        priority = rng.permutation(n)
        p.D = priority[in_d[priority]].astype(np.uint32)
        p.X = priority[in_x[priority]].astype(np.uint32)
    p.neither = np.nonzero(~in_d & ~in_x)[0]
    cpu = 1000 if cpu_request is None else cpu_request
    p.drv = np.tile(np.array([cpu, GIB, 0], dtype=np.int64), (n_apps, 1))
    p.exe = np.tile(np.array([cpu, 2 * GIB, 0], dtype=np.int64), (n_apps, 1))
    if gpus:
        p.exe[::3, 2] = 1
    p.k = rng.integers(0, 4, size=n_apps).astype(np.int32)
    p.k[-1] = 3  # the driver being filtered
    p.flags = np.ones(n_apps, dtype=np.uint32)  # skippable: an earlier driver that does not fit is passed over
    p.avail, p.sched = avail, sched
    p.zone = (rng.integers(0, n_zones, size=n).astype(np.uint32) * 7 + 3) if n_zones > 1 else None
    p.n = n
    return p


def member_rows(n, seed=0):
    """Member rows for a cluster of n nodes: empty words, a single bit, a full word and a ragged last word among them."""
    rng = np.random.default_rng(1000 + seed)
    rows = []
    one = np.zeros(n, dtype=bool)
    one[n // 2] = True
    rows.append(one)  # a single bit (every other word empty)
    if n > 64:
        full = np.zeros(n, dtype=bool)
        full[64:128] = True  # a full word (ragged when it is the last) between empty ones
        rows.append(full)
        tail = np.zeros(n, dtype=bool)
        tail[(n - 1) // 64 * 64:] = True  # the last word alone
        rows.append(tail)
    rows.append(rng.random(n) < 0.5)
    rows.append(np.zeros(n, dtype=bool))  # no key at all
    return rows
