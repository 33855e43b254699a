"""The failover reconciler's findNodes for the stale applications of every instance group, in front of a driver Filter, on two
routes: 10 000 nodes in 8 groups and 100 000 in 32, 64 stale applications per group with k = 8, overhead on every node and
resident usage; p50 over interleaved rounds through the Python binding.
   resident   one gf_cluster_find_nodes (nothing installed), then the driver Filter: a chain-cache resume
   install    today's route, per group: gf_snapshot_set + gf_orders_set + gf_find_nodes on the group's available columns (derived
              beforehand: the host's walk is NOT in the figure), then the rebuild the Filter needs (gf_snapshot_build_resident) and
              the driver Filter, cold: the installs dropped its chain cache
   python tools/probe_cluster_find_nodes.py [rounds] [n_apps]      (run on the MI355X box)"""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "k8s-spark-scheduler_amd")]
import gangfit
from gangfit import workloads as wl
from oracle import pysnapshot as ps
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n_apps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
PER_GROUP, K = 64, 8
FIFO, ALGO = gangfit.GF_MODE_FIFO_CHAIN, gangfit.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK
p50 = lambda v: sorted(v)[len(v) // 2]
ms = lambda a, b: (b - a) * 1e3
print(f"# {rounds} interleaved rounds, p50 in ms; {PER_GROUP} stale applications per group, k = {K}; the driver Filter = gf_fit_batch(GF_MODE_FIFO_CHAIN, single-az-tightly-pack) of {n_apps} applications")
for n_nodes, n_groups in ((10000, 8), (100000, 32)):
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
    group = rng.integers(0, n_groups, size=n_nodes)
    sets = np.stack([group == g for g in range(n_groups)])
    create_rank = rng.permutation(n_nodes).astype(np.uint32)
    w = wl.config(2, n_nodes=n_nodes, n_apps=n_apps)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    R = PER_GROUP * n_groups
    req_set = (np.arange(R) % n_groups).astype(np.uint32)  # the groups interleaved
    exe = np.stack([rng.choice([1000, 2000, 4000], size=R), rng.choice([4, 8, 16], size=R) * wl.GIB, np.zeros(R, dtype=np.int64)], axis=1).astype(np.int64)
    k = np.full(R, K, dtype=np.int32)
    # what today's route uploads per group: the available columns of the group's nodes in visiting order (the host's walk)
    usage = np.zeros_like(alloc)
    np.add.at(usage, rnode, rreq)
    avail = alloc - (usage + over)
    order = [np.nonzero(sets[g])[0][np.argsort(create_rank[sets[g]], kind="stable")] for g in range(n_groups)]
    cols = [np.ascontiguousarray(avail[o]) for o in order]
    ident = [np.arange(len(o), dtype=np.uint32) for o in order]
    mine = [np.nonzero(req_set == g)[0] for g in range(n_groups)]
    gexe, gk = [np.ascontiguousarray(exe[m]) for m in mine], [np.ascontiguousarray(k[m]) for m in mine]
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

        def per_group():
            raw = []
            for g in range(n_groups):
                ctx.set_snapshot(cols[g])
                ctx.set_orders(ident[g], ident[g])
                raw.append(ctx.find_nodes(gexe[g], gk[g], chained=True, want_adds=False))
            return raw

        def cluster_names(raw):  # (not timed: the group's positions back to cluster indices)
            names = [None] * R
            for g, (placed, _, off, nodes, _) in enumerate(raw):
                for i, q in enumerate(mine[g]):
                    names[q] = order[g][nodes[int(off[i]):int(off[i]) + int(placed[i])]]
            return names

        want = warm()
        t_res, t_next, t_ins, t_build, t_cold, resumed, cold = [], [], [], [], [], 0, 0
        for r in range(rounds + 3):
            warm()
            ctx.chain_cache_stats(reset=True)
            t0 = time.perf_counter()
            placed, _, off, nodes, _, _ = ctx.cluster_find_nodes(exe, k, create_rank, sets=sets, req_set=req_set, chained=True)
            t1 = time.perf_counter()
            got = chain()
            t2 = time.perf_counter()
            st = ctx.chain_cache_stats()
            assert got.results.tobytes() == want.results.tobytes() and got.exec_nodes.tobytes() == want.exec_nodes.tobytes()
            warm()
            ctx.chain_cache_stats(reset=True)
            t3 = time.perf_counter()
            raw = per_group()
            t4 = time.perf_counter()
            names = cluster_names(raw)
            t4b = time.perf_counter()
            build()
            t5 = time.perf_counter()
            got = chain()
            t6 = time.perf_counter()
            st2 = ctx.chain_cache_stats()
            assert got.results.tobytes() == want.results.tobytes()
            assert all(np.array_equal(names[q], nodes[int(off[q]):int(off[q]) + int(placed[q])]) for q in range(R)), "the two routes name different nodes"
            if r >= 3:  # (the first rounds grow buffers)
                resumed += int(st[0] == 1 and st[1] == 1)
                cold += int(st2[1] == 0)
                t_res.append(ms(t0, t1)); t_next.append(ms(t1, t2)); t_ins.append(ms(t3, t4)); t_build.append(ms(t4b, t5)); t_cold.append(ms(t5, t6))
        assert resumed == rounds, f"the driver Filter resumed in {resumed} of {rounds} rounds after the resident call"
        print(f"{n_nodes} nodes, {n_groups} groups, {R} requests ({int(placed.sum())} executors placed): the same nodes on both routes; the driver Filter "
              f"resumed in {resumed} of {rounds} rounds after the resident call, replayed in {cold} of {rounds} after the installs")
        print(f"  resident  reconcile {p50(t_res):.3f} (one gf_cluster_find_nodes) + next driver Filter {p50(t_next):.3f} = {p50(t_res) + p50(t_next):.3f}")
        print(f"  install   reconcile {p50(t_ins):.3f} ({n_groups} x gf_snapshot_set + gf_orders_set + gf_find_nodes) + rebuild {p50(t_build):.3f} "
              f"+ next driver Filter {p50(t_cold):.3f} = {p50(t_ins) + p50(t_build) + p50(t_cold):.3f}")
