"""Resident worker on the zone-aware tightly-pack packers against the one-launch kernel (fit_zoned_fused_kernel), one process,
arms interleaved.  Headline workload: 10 000 nodes x 1 000 applications, three zones, AZ-major order.
  (a) a stream of K = 2 000 and K = 20 device-resident tickets through the worker, both packers: us per ticket
  (b) the same batches as K gf_fit_batch_dev launches on one stream: us per batch
  (c) blocking gf_worker_fit against gf_fit_batch, 1 and 1 000 applications
  (d) (a) with 1 / 2 / 3 applications per wavefront (worker_blocks_per_set 63 / 32 / 21)
  (e) a blocking gf_fit_batch of single-az-tightly-pack issued while a worker is resident (does the launch wait for it?)
      python tools/probe_worker_zoned.py [repetitions]  > profiles/worker_zoned.txt        (run on the MI355X)"""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "k8s-spark-scheduler_amd")]
import torch
import gangfit
from gangfit import workloads as wl

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
IND = gangfit.GF_MODE_INDEPENDENT
PACKERS = (("single-az-tightly-pack", gangfit.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK), ("az-aware-tightly-pack", gangfit.GF_ALGO_AZ_AWARE_TIGHTLY_PACK))
dev = torch.device("cuda:0")
w = wl.headline(10000, 1000, seed=0x5EED0010)
s = w.snapshot
zone = (wl.splitmix64(0xA2, len(s.avail), 9) % np.uint64(3)).astype(np.uint32)
D = np.asarray(s.driver_order)[np.argsort(zone[s.driver_order], kind="stable")]  # AZ-major
X = np.asarray(s.exec_order)[np.argsort(zone[s.exec_order], kind="stable")]
apps, total_k = gangfit.with_offsets(gangfit.make_apps(w.drv, w.exe, w.k, w.flags))
n = len(apps)
d_apps = torch.from_numpy(apps.view(np.uint8).copy()).to(dev)
NOUT = 8
outs = [(torch.zeros(n * 16, dtype=torch.uint8, device=dev), torch.zeros(total_k + 1, dtype=torch.int32, device=dev)) for _ in range(NOUT)]
side = torch.cuda.Stream()


def make(opts):
    c = gangfit.Context(0, options=opts)
    c.set_snapshot(s.avail, s.sched)
    c.set_zones(zone)
    c.set_orders(D, X)
    return c


def stats(x):
    x = sorted(x)
    return f"median {x[len(x) // 2]:8.2f}  range {x[0]:8.2f} .. {x[-1]:8.2f}"


def stream(c, algo, K):  # (a): K tickets posted, worker launched, served, left, device synchronised — what bench.py times
    arr = c.worker_batches([(n, d_apps.data_ptr(), outs[i % NOUT][0].data_ptr(), outs[i % NOUT][1].data_ptr(), total_k) for i in range(K)], leave_after=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c.worker_submit_prepared(algo, arr)
    c.worker_stop()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e6


def launches(c, algo, K):  # (b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(K):
        c.fit_batch_dev(IND, algo, n, d_apps.data_ptr(), outs[i % NOUT][0].data_ptr(), outs[i % NOUT][1].data_ptr(), total_k, stream=side.cuda_stream)
    side.synchronize()
    return (time.perf_counter() - t0) / K * 1e6


def blocking(fn, algo, a, reps=200):  # (c)
    fn(algo, a)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn(algo, a)
    return (time.perf_counter() - t0) / reps * 1e6


print(f"# {n} applications x {len(s.avail)} nodes, 3 zones (AZ-major), {REPS} repetitions per arm, arms interleaved; us")
ctx = make({})
geo = {"1 per wavefront": make({"worker_blocks_per_set": 63}), "2 per wavefront": make({"worker_blocks_per_set": 32}),
       "3 per wavefront": make({"worker_blocks_per_set": 21})}
ok = True
for name, algo in PACKERS:  # answers first: the worker's == the launch's
    ref = ctx.fit_batch(IND, algo, apps)
    got = ctx.worker_fit(algo, apps)
    ctx.worker_stop()
    same = np.array_equal(ref.results, got.results) and all(
        np.array_equal(ref.placement(int(a))[2], got.placement(int(a))[2]) for a in np.nonzero(ref.results["has_capacity"])[0])
    ok = ok and same
    print(f"# {name}: worker == launch: {same}; feasible {int(ref.results['has_capacity'].sum())} of {n}")
res = {}
one = apps[:1].copy()
for rep in range(REPS + 1):  # (the first pass warms up and is dropped)
    for name, algo in PACKERS:
        for K in (2000, 20):
            v = {(name, f"(a) worker stream K={K}", "us/ticket"): stream(ctx, algo, K),
                 (name, f"(b) launches K={K}", "us/batch"): launches(ctx, algo, K)}
            for g, c in geo.items():
                v[(name, f"(d) worker stream K={K}, {g}", "us/ticket")] = stream(c, algo, K)
            for k2, x in v.items():
                res.setdefault(k2, []).append(x)
        for na, a in ((1, one), (n, apps)):
            res.setdefault((name, f"(c) blocking gf_worker_fit, {na} applications", "us/call"), []).append(blocking(ctx.worker_fit, algo, a))
            ctx.worker_stop()
            res.setdefault((name, f"(c) blocking gf_fit_batch,  {na} applications", "us/call"), []).append(
                blocking(lambda al, aa: ctx.fit_batch(IND, al, aa), algo, a))
for (name, arm, unit), x in sorted(res.items()):
    print(f"{name:24s} {arm:48s} {stats(x[1:])} {unit}")
# (e) a launch of the one-launch kernel (104 VGPRs a wavefront) issued while a worker is resident (idle period 200 ms)
cw = make({"worker_idle_us": 200000})
for wname, walgo in (("tightly-pack", gangfit.GF_ALGO_TIGHTLY_PACK),) + PACKERS[:1]:
    for rep in range(3):
        cw.worker_fit(walgo, apps)
        before = cw.worker_stats()["resident"]
        t0 = time.perf_counter()
        cw.fit_batch(IND, PACKERS[0][1], apps)
        dt = (time.perf_counter() - t0) * 1e6
        print(f"(e) gf_fit_batch(single-az-tightly-pack) next to a worker resident on {wname:24s}: {dt:10.1f} us/call; "
              f"worker resident before {before}, after {cw.worker_stats()['resident']}")
        cw.worker_stop()
cw.close()
print(f"# geometry of the default stream (sets, workgroups per set): {ctx.worker_geometry()}")
for c in list(geo.values()) + [ctx]:
    c.close()
sys.exit(0 if ok else 1)
