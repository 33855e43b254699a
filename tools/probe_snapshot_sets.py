"""Switching the driver Filter's instance group on ONE resident cluster (gf_snapshot_build_resident_set) against today's route
(gf_cluster_set of the group's rows + gf_usage_apply of its entries + gf_snapshot_build_resident), and the cold FIFO chain on a
group built as a set against the same nodes as a cluster of their own.
   python tools/probe_snapshot_sets.py [--reps 5] [--out FILE]          (run on the MI355X box)
Sizes: 10 000 nodes in 8 groups and 100 000 nodes in 32 groups, contiguous and scattered, resident usage with overhead.
The arms are interleaved inside every repetition (a drift of the machine hits both alike); a cell is the median over the
repetitions of the repetition's p50, with the range of those p50s.  Host-side preparation of arm B (compacting the group's rows
and renaming its entries) is done once, outside the timed region: arm B is timed at its best."""
import argparse, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "k8s-spark-scheduler_amd")]
import numpy as np
import gangfit
from gangfit import workloads as wl

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
FIFO = gangfit.GF_MODE_FIFO_CHAIN


def cluster(n, seed):
    rng = np.random.default_rng(seed)
    shape = rng.integers(0, 4, size=n)
    alloc = np.stack([np.array([16, 32, 64, 96])[shape] * 1000, np.array([64, 128, 256, 384])[shape] * wl.GIB, np.zeros(n, dtype=np.int64)], axis=1).astype(np.int64)
    over = np.stack([rng.integers(1, 8, size=n) * 250, rng.integers(1, 16, size=n) * (wl.GIB // 4), np.zeros(n, dtype=np.int64)], axis=1).astype(np.int64)
    ks = rng.integers(2, 26, size=n // 5)
    rnode = rng.integers(0, n, size=int(ks.sum())).astype(np.uint32)
    rreq = np.stack([rng.choice([1000, 2000, 4000], size=len(rnode)), rng.choice([4, 8, 16], size=len(rnode)) * wl.GIB, np.zeros(len(rnode), dtype=np.int64)], axis=1).astype(np.int64)
    return dict(alloc=alloc, over=over, rnode=rnode, rreq=rreq, flags=np.full(n, 6, dtype=np.uint32), ranks=rng.permutation(n).astype(np.uint32),
                zone=rng.integers(0, 3, size=n).astype(np.uint32))


def alone(c, members):
    """The group as a cluster of its own: what today's route sends on every switch."""
    M = np.nonzero(members)[0]
    where = np.full(len(members), -1, dtype=np.int64)
    where[M] = np.arange(len(M))
    rank = np.empty(len(M), dtype=np.int64)
    rank[np.argsort(c["ranks"][M], kind="stable")] = np.arange(len(M))
    keep = where[c["rnode"].astype(np.int64)] >= 0
    return dict(alloc=c["alloc"][M], over=c["over"][M], flags=c["flags"][M], ranks=rank.astype(np.uint32), zone=c["zone"][M],
                rnode=where[c["rnode"][keep].astype(np.int64)].astype(np.uint32), rcols=[np.ascontiguousarray(c["rreq"][keep][:, j]) for j in range(3)])


def p50(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def cell(values):
    v = sorted(values)
    return "%8.3f [%7.3f .. %7.3f]" % (v[len(v) // 2], v[0], v[-1])


rows = ["gf_snapshot_build_resident_set: switching the Filter's instance group.  ms per switch, want_orders = False, resident usage with overhead;",
        "median over %d repetitions of the repetition's p50 [range of those p50s]; arms interleaved inside a repetition." % args.reps,
        "A = gf_snapshot_build_resident_set on one resident cluster;  B = gf_cluster_set(group) + gf_usage_apply(group) + gf_snapshot_build_resident",
        "%8s %6s %-10s %8s  %-30s %-30s %s" % ("nodes", "groups", "layout", "members", "A", "B", "route A/B")]
w = wl.config(2, n_nodes=16, n_apps=1000)  # the chain: 999 earlier drivers + 1
apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(len(w.k), dtype=np.uint32))
chain_rows = ["", "cold FIFO chain (999 + 1, tightly-pack, chain cache off) on group 0: built as a set | the same nodes as a cluster of their own.  ms;",
              "same statistics.  layout = (built from a set, members, slots, chunks) of gf_snapshot_set_info",
              "%8s %6s %-10s  %-30s %-30s %s" % ("nodes", "groups", "layout", "set", "alone", "layouts set | alone")]
with gangfit.Context(0, options={"chain_cache": 0}) as one, gangfit.Context(0, options={"chain_cache": 0}) as other:
    for n, G in ((10000, 8), (100000, 32)):
        c = cluster(n, n)
        switches = 40 if n <= 10000 else 16
        for layout in ("contiguous", "scattered"):
            group = (np.arange(n) * G // n) if layout == "contiguous" else np.random.default_rng(G).integers(0, G, size=n)
            sets = [group == g for g in range(G)]
            solo = [alone(c, s) for s in sets]
            one.set_cluster(c["alloc"], c["flags"], c["ranks"], overhead=c["over"], zone=c["zone"], n_zones=3)
            one.usage_apply(c["rnode"], res_cols=[np.ascontiguousarray(c["rreq"][:, j]) for j in range(3)], sign=+1)

            def arm_a(g):
                one.build_snapshot_resident_set(sets[g], resident_usage=True, want_orders=False)

            def arm_b(g):
                s = solo[g]
                other.set_cluster(s["alloc"], s["flags"], s["ranks"], overhead=s["over"], zone=s["zone"], n_zones=3)
                other.usage_apply(s["rnode"], res_cols=s["rcols"], sign=+1)
                other.build_snapshot_resident(resident_usage=True, want_orders=False)

            for g in range(min(G, 4)):  # warm: buffers grown, code loaded
                arm_a(g), arm_b(g)
            pa, pb, ca, cb = [], [], [], []
            for rep in range(args.reps):
                for arm, out in ((arm_a, pa), (arm_b, pb)):
                    ts = []
                    for i in range(switches):
                        t0 = time.perf_counter(); arm((i + 1) % G); ts.append((time.perf_counter() - t0) * 1e3)
                    out.append(p50(ts))
                route = "%d/%d" % (one.build_info()[0], other.build_info()[0])
                # the cold chain on group 0, same process: the two layouts are the same, the times are expected equal
                arm_a(0), arm_b(0)
                info = (one.snapshot_set_info(), other.snapshot_set_info())
                for ctx, out in ((one, ca), (other, cb)):
                    ts = []
                    for _ in range(7):
                        t0 = time.perf_counter(); r = ctx.fit_batch(FIFO, 0, apps); ts.append((time.perf_counter() - t0) * 1e3)
                    out.append(p50(ts))
                print(n, layout, rep, "A %.3f B %.3f chain set %.3f alone %.3f" % (pa[-1], pb[-1], ca[-1], cb[-1]), flush=True)
            rows.append("%8d %6d %-10s %8d  %-30s %-30s %s" % (n, G, layout, int(sets[0].sum()), cell(pa), cell(pb), route))
            chain_rows.append("%8d %6d %-10s  %-30s %-30s %s | %s" % (n, G, layout, cell(ca), cell(cb), info[0], info[1]))
text = "\n".join(rows + chain_rows) + "\n"
print(text)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(text)
