"""gf_snapshot_build_resident on a resident cluster + resident usage (what a Filter pays when the snapshot changed), N builds.
   python tools/probe_snapshot_resident.py <n_nodes> [builds]      (run on the MI355X box; under rocprofv3 for the per-kernel split)
   ... --labels          the builds carry label ranks: one prioritized label for drivers and executors (both lists re-sorted by it)
   ... --tree DIR        import gangfit from DIR (a checkout of another commit with its library built) instead of this tree
   python tools/probe_snapshot_resident.py --compare DIR [--reps 5] [--out FILE]
                         this tree against DIR (the parent commit, `git worktree add DIR HEAD~` + its build), unlabelled and
                         labelled, at 10 000 and 100 000 nodes: one fresh process per measurement, the two trees interleaved;
                         minimum and median of the runs' p50, and the run-to-run spread (max - min), as a table"""
import argparse, os, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("n_nodes", nargs="?", type=int, default=10000)
ap.add_argument("builds", nargs="?", type=int, default=200)
ap.add_argument("--labels", action="store_true")
ap.add_argument("--tree", default=REPO)
ap.add_argument("--compare", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

if args.compare:
    trees = (("this", REPO), ("parent", os.path.abspath(args.compare)))
    runs = {}
    for rep in range(args.reps):
        for n in (10000, 100000):
            for labels in (False, True):
                for name, tree in trees:  # interleaved: a drift of the machine hits both trees alike
                    cmd = [sys.executable, os.path.abspath(__file__), str(n), str(args.builds), "--tree", tree] + (["--labels"] if labels else [])
                    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
                    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                    if p.returncode != 0 or not line:
                        sys.exit("a measurement failed (nothing more is started):\n" + p.stdout[-2000:])
                    f = line[-1].split()
                    runs.setdefault((n, labels, name), []).append((float(f[1]), float(f[2]), f[3]))
                    print(rep, n, "labels" if labels else "plain", name, line[-1], flush=True)
    rows = ["gf_snapshot_build_resident, resident cluster + resident usage, want_orders = False; p50 of %d builds per run, %d runs per cell,"
            % (args.builds, args.reps),
            "one process per run, the two trees interleaved.  ms.  route = gf_snapshot_build_info (1 device, 2 host; - = the parent has no such call)",
            "%8s %-7s %-7s %6s %9s %9s %9s" % ("nodes", "labels", "tree", "route", "min", "median", "spread")]
    for n in (10000, 100000):
        for labels in (False, True):
            for name, _ in trees:
                r = sorted(v[0] for v in runs[(n, labels, name)])
                rows.append("%8d %-7s %-7s %6s %9.3f %9.3f %9.3f" % (n, "yes" if labels else "no", name, runs[(n, labels, name)][0][2],
                                                                     r[0], r[len(r) // 2], r[-1] - r[0]))
    text = "\n".join(rows) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    sys.exit(0)

sys.path[:0] = [args.tree, os.path.join(args.tree, "k8s-spark-scheduler_amd")]
import numpy as np
import gangfit
from gangfit import workloads as wl
assert os.path.abspath(gangfit.__file__).startswith(os.path.abspath(args.tree)), gangfit.__file__
n_nodes, builds = args.n_nodes, args.builds
n_rr = n_nodes // 5
ctx = gangfit.Context(0, options={"chain_cache": 0})
rng = np.random.default_rng(n_nodes)
shape = rng.integers(0, 4, size=n_nodes)
alloc = np.stack([np.array([16, 32, 64, 96])[shape] * 1000, np.array([64, 128, 256, 384])[shape] * wl.GIB, np.zeros(n_nodes, dtype=np.int64)], axis=1).astype(np.int64)
ks = rng.integers(2, 26, size=n_rr)
rnode = rng.integers(0, n_nodes, size=int(ks.sum())).astype(np.uint32)
rreq = np.stack([rng.choice([1000, 2000, 4000], size=len(rnode)), rng.choice([4, 8, 16], size=len(rnode)) * wl.GIB, np.zeros(len(rnode), dtype=np.int64)], axis=1).astype(np.int64)
flags = np.full(n_nodes, 6, dtype=np.uint32)
ranks = rng.permutation(n_nodes).astype(np.uint32)
zone = rng.integers(0, 3, size=n_nodes).astype(np.uint32)
label = rng.choice([0, 1, 2, 0xFFFFFFFF], size=n_nodes).astype(np.uint32) if args.labels else None
ctx.set_cluster(alloc, flags, ranks, zone=zone, n_zones=3)
ctx.usage_reset()
ctx.usage_apply(rnode, res_cols=[np.ascontiguousarray(rreq[:, j]) for j in range(3)], sign=+1)
h = lambda: ctx.build_snapshot_resident(resident_usage=True, want_orders=False, driver_label_rank=label, exec_label_rank=label)
for _ in range(5):
    h()
ts = []
for _ in range(builds):
    t0 = time.perf_counter(); h(); ts.append((time.perf_counter() - t0) * 1e3)
ts.sort()
p50, p99 = ts[len(ts) // 2], ts[int(len(ts) * 0.99) - 1]
route = str(ctx.build_info()[0]) if hasattr(ctx, "build_info") else "-"
print(n_nodes, "nodes%s: resident cluster + resident usage p50 %.3f ms p99 %.3f ms" % (" with label ranks" if args.labels else "", p50, p99))
print("RESULT %.4f %.4f %s" % (p50, p99, route))
