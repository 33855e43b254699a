"""What the cluster-wide average packing efficiency of a driver Filter costs (gf_filter_efficiency), on one context, at
   10 000 and 100 000 nodes:
  new     gf_filter_efficiency against the chain's residual: one 40-byte answer
  rows    the route before it: gf_packing_efficiencies (3 x n_nodes float64 come back, against the SNAPSHOT — for a Filter with an
          earlier driver not even the right number) + the numpy sums
  filter  the warm Filter — the same FIFO chain again on an unchanged snapshot — alone, and followed by the new call
The arms are interleaved round by round; a figure is the median over the rounds of the mean of `calls` back-to-back blocking calls
(each call ends in a device synchronise), in microseconds.  Every array is prepared beforehand: the figures are the C entry
points', not the binding's packing.
   python tools/probe_filter_efficiency.py [rounds >= 7] [calls] [out]      (run on the MI355X box; out: profiles/filter_efficiency.txt)"""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "k8s-spark-scheduler_amd")]
import gangfit
from gangfit import _native as N
from gangfit import workloads as wl
rounds = max(7, int(sys.argv[1])) if len(sys.argv) > 1 else 9
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 100
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "filter_efficiency.txt")
FIFO, ALGO = gangfit.GF_MODE_FIFO_CHAIN, gangfit.GF_ALGO_TIGHTLY_PACK
median = lambda v: sorted(v)[len(v) // 2]
lines = [f"# gf_filter_efficiency: {rounds} interleaved rounds, median of the mean of {calls} blocking calls, microseconds per call",
         "# new = gf_filter_efficiency (residual); rows = gf_packing_efficiencies + numpy sums (snapshot); filter = the warm FIFO Filter",
         "# (a queue of 24 applications, tip resume) alone and followed by the new call"]
for n_nodes in (10000, 100000):
    w = wl.headline(n_nodes, 24)
    s = w.snapshot
    apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    apps_off, total_k = gangfit.with_offsets(apps)
    with gangfit.Context(0) as ctx:
        ctx.set_snapshot(s.avail, s.sched)
        ctx.set_orders(s.driver_order, s.exec_order)
        L, h = ctx._lib, ctx._h
        res = np.zeros(len(apps), dtype=N.RESULT_DTYPE)
        exec_nodes = np.zeros(total_k + 1, dtype=np.uint32)
        failed = np.zeros(1, dtype=np.int32)

        def chain():
            rc = L.gf_fit_batch(h, FIFO, ALGO, len(apps), N.ptr(apps), N.ptr(res), N.ptr(exec_nodes), total_k, N.ptr(failed))
            assert rc == N.GF_OK, ctx.last_error()

        chain()
        assert res[-1]["has_capacity"] == 1, "the probe's last application must fit"
        last_app = np.ascontiguousarray(apps_off[-1:])
        last_app["exec_off"] = 0
        last_res = np.ascontiguousarray(res[-1:])
        last_exec = np.ascontiguousarray(exec_nodes[int(apps_off[-1]["exec_off"]):total_k])
        avg, counts = np.zeros(4), np.zeros(2, dtype=np.uint32)
        eff = np.zeros((n_nodes, 3), dtype=np.float64)
        has_gpu = s.sched[:, 2] != 0
        host = np.zeros(4)

        def new():
            rc = L.gf_filter_efficiency(h, ALGO, N.GF_EFF_AGAINST_RESIDUAL, N.ptr(last_app), N.ptr(last_res), N.ptr(last_exec), None,
                                        N.ptr(avg), N.ptr(counts))
            assert rc == N.GF_OK, ctx.last_error()

        def rows():
            rc = L.gf_packing_efficiencies(h, ALGO, N.ptr(last_app), N.ptr(last_res), N.ptr(last_exec), N.ptr(eff))
            assert rc == N.GF_OK, ctx.last_error()
            host[0], host[1] = eff[:, 0].sum() / n_nodes, eff[:, 1].sum() / n_nodes
            g = int(has_gpu.sum())
            host[2] = eff[has_gpu, 2].sum() / g if g else 1.0
            host[3] = eff.max(axis=1).sum() / n_nodes

        def filter_alone():
            chain()

        def filter_and_new():
            chain()
            new()

        arms = (("new", new), ("rows", rows), ("filter", filter_alone), ("filter+new", filter_and_new))
        t = {name: [] for name, _ in arms}
        for r in range(rounds + 2):
            for name, fn in arms:
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                if r >= 2:  # (the first rounds grow buffers and load code objects)
                    t[name].append((time.perf_counter() - t0) * 1e6 / calls)
        m = {name: median(v) for name, v in t.items()}
        spread = {name: (min(v), max(v)) for name, v in t.items()}
        lines.append(f"{n_nodes} nodes: new {m['new']:.1f} [{spread['new'][0]:.1f}, {spread['new'][1]:.1f}]  rows {m['rows']:.1f} "
                     f"[{spread['rows'][0]:.1f}, {spread['rows'][1]:.1f}]  (x{m['rows'] / m['new']:.1f})  filter {m['filter']:.1f} "
                     f"[{spread['filter'][0]:.1f}, {spread['filter'][1]:.1f}]  filter+new {m['filter+new']:.1f} "
                     f"[{spread['filter+new'][0]:.1f}, {spread['filter+new'][1]:.1f}]  "
                     f"(len {int(counts[0])}, nodesWithGPU {int(counts[1])}, Max {avg[3]:.6f}; rows' Max over the snapshot {host[3]:.6f})")
        print(lines[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
