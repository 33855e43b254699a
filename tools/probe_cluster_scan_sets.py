"""The UnschedulablePodMarker's minute on a cluster of G instance groups: G blocking gf_cluster_fit_feasible calls (one per group,
its applications, its node selection) against ONE gf_cluster_fit_feasible_sets call, in one session, on
   10 000 nodes x 1 000 applications in  8 instance groups
  100 000 nodes x 1 000 applications in 32 instance groups
with the groups contiguous (node ranges) and scattered (node index mod G).  The per-group calls go through an entry point the
sets call did not change: they are the cost before it.  For information: one one-set call over ALL nodes with the same
applications (what the row walk costs when nothing can be skipped).  Every array is prepared beforehand: the figures are the C
entry points', not the binding's packing.
   python tools/probe_cluster_scan_sets.py [rounds] > profiles/cluster_scan_sets.txt      (run on the MI355X box)"""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "k8s-spark-scheduler_amd")]
import gangfit
from gangfit import _native as N
from gangfit import workloads as wl
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n_apps = 1000
p50 = lambda v: sorted(v)[len(v) // 2]
print(f"# {n_apps} applications, {rounds} rounds, p50 in ms; per group = the sum of G gf_cluster_fit_feasible calls, sets = one gf_cluster_fit_feasible_sets call,")
print("# full = one gf_cluster_fit_feasible call over every node with the same applications (for information)")
for n_nodes, G in ((10000, 8), (100000, 32)):
    rng = np.random.default_rng(n_nodes)
    shape = rng.integers(0, 4, size=n_nodes)
    alloc = np.stack([np.array([16, 32, 64, 96])[shape] * 1000, np.array([64, 128, 256, 384])[shape] * wl.GIB, np.where(rng.random(n_nodes) < 0.1, 8, 0)], axis=1).astype(np.int64)
    over = np.stack([rng.integers(0, 4, size=n_nodes) * 250, rng.integers(0, 8, size=n_nodes) * (wl.GIB // 4), np.zeros(n_nodes, dtype=np.int64)], axis=1).astype(np.int64)
    ocols = [np.ascontiguousarray(over[:, j]) for j in range(3)]
    flags = np.full(n_nodes, 3, dtype=np.uint32)
    ranks = rng.permutation(n_nodes).astype(np.uint32)
    zone = rng.integers(0, 3, size=n_nodes).astype(np.uint32)
    w = wl.config(2, n_nodes=n_nodes, n_apps=n_apps)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    app_set = np.ascontiguousarray(rng.integers(0, G, size=n_apps).astype(np.uint32))  # the listing interleaves the groups
    idx = [np.nonzero(app_set == g)[0] for g in range(G)]
    group_apps = [np.ascontiguousarray(apps[i]) for i in idx]
    node = np.arange(n_nodes)
    for layout, group_of in (("contiguous", node * G // n_nodes), ("scattered", node % G)):
        sets = np.stack([group_of == g for g in range(G)])
        selects = [np.ascontiguousarray(sets[g], dtype=np.uint8) for g in range(G)]
        words = gangfit.pack_node_sets(sets, n_nodes)
        for name, algo in (("tightly-pack", gangfit.GF_ALGO_TIGHTLY_PACK), ("single-az-tightly-pack", gangfit.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK)):
            with gangfit.Context(0) as ctx:
                ctx.set_cluster(alloc, flags, ranks, overhead=None, zone=zone, n_zones=3)
                L, h = ctx._lib, ctx._h
                out_g = [np.zeros(len(i), dtype=np.uint8) for i in idx]
                out_s, out_f = np.zeros(n_apps, dtype=np.uint8), np.zeros(n_apps, dtype=np.uint8)

                def per_group():
                    for g in range(G):
                        rc = L.gf_cluster_fit_feasible(h, algo, N.ptr(ocols[0]), N.ptr(ocols[1]), N.ptr(ocols[2]), N.ptr(selects[g]), len(idx[g]), N.ptr(group_apps[g]), N.ptr(out_g[g]))
                        assert rc == N.GF_OK, ctx.last_error()

                def one_sets():
                    rc = L.gf_cluster_fit_feasible_sets(h, algo, N.ptr(ocols[0]), N.ptr(ocols[1]), N.ptr(ocols[2]), G, N.ptr(words), N.ptr(app_set), n_apps, N.ptr(apps), N.ptr(out_s))
                    assert rc == N.GF_OK, ctx.last_error()

                def full():
                    rc = L.gf_cluster_fit_feasible(h, algo, N.ptr(ocols[0]), N.ptr(ocols[1]), N.ptr(ocols[2]), None, n_apps, N.ptr(apps), N.ptr(out_f))
                    assert rc == N.GF_OK, ctx.last_error()

                t = {"per group": [], "sets": [], "full": []}
                for r in range(rounds + 3):
                    for key, fn in (("per group", per_group), ("sets", one_sets), ("full", full)):
                        t0 = time.perf_counter()
                        fn()
                        if r >= 3:  # (the first rounds grow buffers)
                            t[key].append((time.perf_counter() - t0) * 1e3)
                merged = np.zeros(n_apps, dtype=np.uint8)
                for g in range(G):
                    merged[idx[g]] = out_g[g]
                assert merged.tobytes() == out_s.tobytes(), "the sets call differs from the per-group calls"
                print(f"{n_nodes} nodes, {G} groups {layout}, {name}: per group {p50(t['per group']):.3f}  sets {p50(t['sets']):.3f}  "
                      f"(x{p50(t['per group']) / p50(t['sets']):.1f})  full {p50(t['full']):.3f}  [{int(out_s.sum())} of {n_apps} fit their group]", flush=True)
