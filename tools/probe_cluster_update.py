"""A node event on a resident host, on two routes: 10 000 and 100 000 nodes, a reservation list of config 5's size (20 000
reservations, ~270 k entries) resident as usage sums, overhead on every node; interleaved arms, p50 and the spread (min .. max) in ms
through the Python binding.
   set       the route without gf_cluster_update: gf_cluster_set of the whole node side + gf_usage_reset + gf_usage_apply of the
             whole entry list
   update    gf_cluster_update of 1 row and of 1 % of the rows, with and without the rank array; usage and overhead stay
Behind each route the FIRST driver Filter: gf_snapshot_build_resident_set (every node) + a 999 + 1 chain.  The update does not
make that Filter warm — the rebuild and the cold chain are still paid — and the figures say what they cost.
   python tools/probe_cluster_update.py [rounds] [n_apps]      (run on the MI355X box)"""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "k8s-spark-scheduler_amd")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import gangfit
from gangfit import workloads as wl
from oracle import pysnapshot as ps
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n_apps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
FIFO, ALGO = gangfit.GF_MODE_FIFO_CHAIN, gangfit.GF_ALGO_TIGHTLY_PACK
ms = lambda a, b: (b - a) * 1e3
stat = lambda v: f"{sorted(v)[len(v) // 2]:.3f} ({min(v):.3f} .. {max(v):.3f})"
print(f"# {rounds} interleaved rounds after 3 unrecorded ones; p50 (min .. max) in ms; the first driver Filter = gf_snapshot_build_resident_set "
      f"(GF_RESIDENT_USAGE, request flags) + gf_fit_batch(GF_MODE_FIFO_CHAIN, tightly-pack) of {n_apps - 1} + 1 applications")
for n in (10000, 100000):
    rng = np.random.default_rng(n)
    shape = rng.integers(0, 4, size=n)
    alloc = np.stack([np.array([16, 32, 64, 96])[shape] * 1000, np.array([64, 128, 256, 384])[shape] * wl.GIB, np.where(rng.random(n) < 0.1, 8, 0)], axis=1).astype(np.int64)
    over = np.stack([rng.integers(1, 8, size=n) * 250, rng.integers(1, 16, size=n) * (wl.GIB // 4), np.zeros(n, dtype=np.int64)], axis=1).astype(np.int64)
    ks = rng.integers(2, 26, size=20000)
    rnode = rng.integers(0, n, size=int(ks.sum())).astype(np.uint32)
    rcols = [np.ascontiguousarray(c) for c in (rng.choice([1000, 2000, 4000], size=len(rnode)).astype(np.int64),
                                               rng.choice([4, 8, 16], size=len(rnode)).astype(np.int64) * wl.GIB, np.zeros(len(rnode), dtype=np.int64))]
    base = np.full(n, ps.READY, dtype=np.uint32)
    req_flags = base | np.uint32(ps.DRIVER_CANDIDATE)
    ranks = [rng.permutation(n).astype(np.uint32), rng.permutation(n).astype(np.uint32)]  # the order before / after a name joined
    zone = rng.integers(0, 3, size=n).astype(np.uint32)
    everyone = np.ones(n, dtype=bool)
    w = wl.config(2, n_nodes=n, n_apps=n_apps)
    apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
    rows = {"1 row": rng.permutation(n)[:1].astype(np.uint32), "1 % of the rows": np.sort(rng.permutation(n)[: n // 100]).astype(np.uint32)}
    with gangfit.Context(0) as ctx:
        state = {"alloc": alloc.copy(), "rank": 0}

        def full_set():
            ctx.set_cluster(state["alloc"], base, ranks[state["rank"]], overhead=over, zone=zone, n_zones=3)
            ctx.usage_reset()
            ctx.usage_apply(rnode, res_cols=rcols, sign=+1)

        def first_filter():
            t0 = time.perf_counter()
            ctx.build_snapshot_resident_set(everyone, resident_usage=True, node_flags=req_flags, want_orders=False)
            t1 = time.perf_counter()
            out = ctx.fit_batch(FIFO, ALGO, apps)
            return ms(t0, t1), ms(t1, time.perf_counter()), out

        def change(which, with_ranks):  # the event: the named rows resized (toggled between two sizes), the name order moved
            r = rows[which]
            state["alloc"][r, 0] = np.where(state["alloc"][r, 0] == 48000, 32000, 48000)
            if with_ranks:
                state["rank"] ^= 1
            return r

        full_set()
        arms = [("set", w, False) for w in rows] + [("update", w, rk) for w in rows for rk in (False, True)]
        t = {arm: {"sync": [], "build": [], "chain": []} for arm in arms}
        for r in range(rounds + 3):
            for arm in arms:
                route, which, with_ranks = arm
                first_filter()  # the Filter before the event: the route starts from a warm host
                moved = change(which, with_ranks or route == "set")
                t0 = time.perf_counter()
                if route == "set":
                    full_set()
                else:
                    ctx.cluster_update(moved, state["alloc"][moved], base[moved], zone=zone[moved], name_rank=ranks[state["rank"]] if with_ranks else None)
                t1 = time.perf_counter()
                build, chain, got = first_filter()
                if r >= 3:  # (the first rounds grow buffers)
                    t[arm]["sync"].append(ms(t0, t1)); t[arm]["build"].append(build); t[arm]["chain"].append(chain)
            # both routes leave the same state behind: the Filter on it answers the same after a set from scratch
            want = first_filter()[2]
            full_set()
            again = first_filter()[2]
            assert again.results.tobytes() == want.results.tobytes() and again.exec_nodes.tobytes() == want.exec_nodes.tobytes(), "the routes disagree"
        print(f"{n} nodes, {len(rnode)} reservation entries resident, overhead on every node")
        for arm in arms:
            route, which, with_ranks = arm
            what = (f"gf_cluster_set + gf_usage_reset + gf_usage_apply ({which} changed)" if route == "set" else
                    f"gf_cluster_update, {which}, {'with' if with_ranks else 'without'} the rank array")
            print(f"  {what:78s} {stat(t[arm]['sync'])}   then rebuild {stat(t[arm]['build'])} + cold chain {stat(t[arm]['chain'])}")
