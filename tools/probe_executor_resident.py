"""One executor Filter (rescheduleExecutor, every node offered) between two driver Filters, on two routes, at 10 000 and 100 000
nodes, three zones, overhead on every node; p50 over interleaved rounds.
   resident   gf_cluster_executor_fit (nothing installed), then the driver Filter: a chain-cache resume
   install    the route a resident host had before: gf_snapshot_build_resident(GF_RESIDENT_USAGE) + gf_executor_fit with the dense
              n_nodes x 3 `reserved` array uploaded (prepared beforehand: the host's O(n_nodes) walk is NOT in the figure), then the
              driver Filter, cold: the install dropped its chain cache
   python tools/probe_executor_resident.py [rounds] [n_apps]      (run on the MI355X box)"""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "k8s-spark-scheduler_amd")]
import gangfit
from gangfit import workloads as wl
from oracle import pysnapshot as ps
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n_apps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
FIFO, ALGO = gangfit.GF_MODE_FIFO_CHAIN, gangfit.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK
p50 = lambda v: sorted(v)[len(v) // 2]
ms = lambda a, b: (b - a) * 1e3
print(f"# {rounds} interleaved rounds, p50 in ms; one request per executor Filter; the driver Filter = gf_fit_batch(GF_MODE_FIFO_CHAIN, single-az-tightly-pack) of {n_apps} applications")
for n_nodes in (10000, 100000):
    rng = np.random.default_rng(n_nodes)
    shape = rng.integers(0, 4, size=n_nodes)
    alloc = np.stack([np.array([16, 32, 64, 96])[shape] * 1000, np.array([64, 128, 256, 384])[shape] * wl.GIB, np.where(rng.random(n_nodes) < 0.1, 8, 0)], axis=1).astype(np.int64)
    over = np.stack([rng.integers(1, 8, size=n_nodes) * 250, rng.integers(1, 16, size=n_nodes) * (wl.GIB // 4), np.zeros(n_nodes, dtype=np.int64)], axis=1).astype(np.int64)
    ks = rng.integers(2, 26, size=n_nodes // 5)
    rnode = rng.integers(0, n_nodes, size=int(ks.sum())).astype(np.uint32)
    rreq = np.stack([rng.choice([1000, 2000, 4000], size=len(rnode)), rng.choice([4, 8, 16], size=len(rnode)) * wl.GIB, np.zeros(len(rnode), dtype=np.int64)], axis=1).astype(np.int64)
    flags = np.full(n_nodes, ps.READY | ps.DRIVER_CANDIDATE, dtype=np.uint32)
    ranks = rng.permutation(n_nodes).astype(np.uint32)
    zone = rng.integers(0, 3, size=n_nodes).astype(np.uint32)
    w = wl.config(2, n_nodes=n_nodes, n_apps=n_apps)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    exe = np.array([[2000, 8 * wl.GIB, 0]], dtype=np.int64)
    for minfrag in (False, True):
        # what the installing route subtracts: the overhead of the nodes that carry a reservation / of every node
        reserved = over if minfrag else over * (np.bincount(rnode, minlength=n_nodes) > 0)[:, None]
        with gangfit.Context(0) as ctx:
            ctx.set_cluster(alloc, flags, ranks, overhead=over, zone=zone, n_zones=3)
            ctx.usage_apply(rnode, res_cols=[np.ascontiguousarray(rreq[:, j]) for j in range(3)], sign=+1)
            build = lambda: ctx.build_snapshot_resident(resident_usage=True, want_orders=False)
            chain = lambda: ctx.fit_batch(FIFO, ALGO, apps)

            def warm():
                build()
                first = chain()
                chain()
                return first

            want = warm()
            t_res, t_next, t_ins, t_cold, resumed, cold = [], [], [], [], 0, 0
            for r in range(rounds + 3):
                warm()
                ctx.chain_cache_stats(reset=True)
                t0 = time.perf_counter()
                a_res = ctx.cluster_executor_fit(exe, minimal_fragmentation=minfrag)
                t1 = time.perf_counter()
                got = chain()
                t2 = time.perf_counter()
                st = ctx.chain_cache_stats()
                assert got.results.tobytes() == want.results.tobytes() and got.exec_nodes.tobytes() == want.exec_nodes.tobytes()
                warm()
                ctx.chain_cache_stats(reset=True)
                t3 = time.perf_counter()
                build()
                a_ins = ctx.executor_fit(exe, reserved=reserved, minimal_fragmentation=minfrag)
                t4 = time.perf_counter()
                got = chain()
                t5 = time.perf_counter()
                st2 = ctx.chain_cache_stats()
                assert got.results.tobytes() == want.results.tobytes() and np.array_equal(a_res, a_ins) and a_res[0] != 0xFFFFFFFF
                if r >= 3:  # (the first rounds grow buffers)
                    resumed += int(st[0] == 1 and st[1] == 1)
                    cold += int(st2[1] == 0)
                    t_res.append(ms(t0, t1)); t_next.append(ms(t1, t2)); t_ins.append(ms(t3, t4)); t_cold.append(ms(t4, t5))
            print(f"{n_nodes} nodes, {'minimal fragmentation' if minfrag else 'first fit'}: node {int(a_res[0])} on both routes; the driver Filter "
                  f"resumed in {resumed} of {rounds} rounds after the resident call, replayed in {cold} of {rounds} after the install")
            print(f"  resident  executor Filter {p50(t_res):.3f} + next driver Filter {p50(t_next):.3f} = {p50(t_res) + p50(t_next):.3f}")
            print(f"  install   executor Filter {p50(t_ins):.3f} (build + gf_executor_fit) + next driver Filter {p50(t_cold):.3f} = {p50(t_ins) + p50(t_cold):.3f}")
