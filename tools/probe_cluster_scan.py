"""The UnschedulablePodMarker's minute at the headline size (10 000 nodes, 1 000 applications): the capacity scan followed by the
next Filter, on two routes.
   resident   gf_cluster_fit_feasible (nothing installed), then the Filter: a chain-cache resume
   install    today's route: the empty-cluster snapshot installed (gf_snapshot_set + gf_zones_set + gf_orders_set, the arrays
              prepared beforehand: the host's O(n_nodes) flatten is NOT in the figure), gf_fit_feasible, then what the next
              Filter pays: gf_snapshot_build_resident and a cold chain
   python tools/probe_cluster_scan.py [n_nodes] [n_apps] [rounds]      (run on the MI355X box)"""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "k8s-spark-scheduler_amd")]
import gangfit
from gangfit import workloads as wl
from oracle import pysnapshot as ps
n_nodes = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
n_apps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 20
FIFO = gangfit.GF_MODE_FIFO_CHAIN
rng = np.random.default_rng(n_nodes)
shape = rng.integers(0, 4, size=n_nodes)
alloc = np.stack([np.array([16, 32, 64, 96])[shape] * 1000, np.array([64, 128, 256, 384])[shape] * wl.GIB, np.where(rng.random(n_nodes) < 0.1, 8, 0)], axis=1).astype(np.int64)
over = np.stack([rng.integers(0, 8, size=n_nodes) * 250, rng.integers(0, 16, size=n_nodes) * (wl.GIB // 4), np.zeros(n_nodes, dtype=np.int64)], axis=1).astype(np.int64)
ks = rng.integers(2, 26, size=n_nodes // 5)
rnode = rng.integers(0, n_nodes, size=int(ks.sum())).astype(np.uint32)
rreq = np.stack([rng.choice([1000, 2000, 4000], size=len(rnode)), rng.choice([4, 8, 16], size=len(rnode)) * wl.GIB, np.zeros(len(rnode), dtype=np.int64)], axis=1).astype(np.int64)
flags = np.full(n_nodes, ps.READY | ps.DRIVER_CANDIDATE, dtype=np.uint32)
ranks = rng.permutation(n_nodes).astype(np.uint32)
zone = rng.integers(0, 3, size=n_nodes).astype(np.uint32)
select = rng.random(n_nodes) < 0.9                       # the nodes the drivers' affinity matches
non_schedulable = over // 2                              # the part of the overhead the marker subtracts
w = wl.config(2, n_nodes=n_nodes, n_apps=n_apps)
apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
sel_flags = np.where(select, ps.READY | ps.DRIVER_CANDIDATE, 0).astype(np.uint32)
e_avail, e_sched, e_D, e_X = ps.build(alloc, sel_flags, ranks, overhead=non_schedulable, zone=zone, n_zones=3)
p50 = lambda v: sorted(v)[len(v) // 2]
ms = lambda a, b: (b - a) * 1e3
print(f"# {n_nodes} nodes, {n_apps} applications, {rounds} rounds, p50 in ms; the Filter = gf_fit_batch(GF_MODE_FIFO_CHAIN) of the {n_apps} applications")
for name, algo in (("tightly-pack", gangfit.GF_ALGO_TIGHTLY_PACK), ("single-az-tightly-pack", gangfit.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK)):
    with gangfit.Context(0) as ctx:
        ctx.set_cluster(alloc, flags, ranks, overhead=over, zone=zone, n_zones=3)
        ctx.usage_apply(rnode, res_cols=[np.ascontiguousarray(rreq[:, j]) for j in range(3)], sign=+1)
        build = lambda: ctx.build_snapshot_resident(resident_usage=True, want_orders=False)
        chain = lambda: ctx.fit_batch(FIFO, algo, apps)

        def warm():
            build()
            first = chain()
            chain()
            return first

        def install_scan():
            ctx.set_snapshot(e_avail, e_sched)
            ctx.set_zones(zone)
            ctx.set_orders(e_D, e_X)
            return ctx.fit_feasible(algo, apps)

        want = warm()
        t_scan, t_filter, t_iscan, t_build, t_cold, resumed = [], [], [], [], [], 0
        for r in range(rounds + 3):
            warm()
            ctx.chain_cache_stats(reset=True)
            t0 = time.perf_counter()
            a_res = ctx.cluster_fit_feasible(algo, apps, overhead=non_schedulable, node_select=select)
            t1 = time.perf_counter()
            got = chain()
            t2 = time.perf_counter()
            st = ctx.chain_cache_stats()
            assert got.results.tobytes() == want.results.tobytes() and got.exec_nodes.tobytes() == want.exec_nodes.tobytes()
            warm()
            t3 = time.perf_counter()
            a_ins = install_scan()
            t4 = time.perf_counter()
            build()
            t5 = time.perf_counter()
            got = chain()
            t6 = time.perf_counter()
            assert got.results.tobytes() == want.results.tobytes() and np.array_equal(a_res, a_ins)
            if r >= 3:  # (the first rounds grow buffers)
                resumed += int(st[0] == 1 and st[1] == 1)
                t_scan.append(ms(t0, t1)); t_filter.append(ms(t1, t2)); t_iscan.append(ms(t3, t4)); t_build.append(ms(t4, t5)); t_cold.append(ms(t5, t6))
        print(f"{name}: {int(a_res.sum())} of {n_apps} fit the empty cluster; the Filter after the resident scan was a chain-cache resume in {resumed} of {rounds} rounds")
        print(f"  resident  scan {p50(t_scan):.3f} + next Filter {p50(t_filter):.3f} = {p50(t_scan) + p50(t_filter):.3f}")
        print(f"  install   scan {p50(t_iscan):.3f} (install + gf_fit_feasible) + rebuild {p50(t_build):.3f} + cold chain {p50(t_cold):.3f} = {p50(t_iscan) + p50(t_build) + p50(t_cold):.3f}")
