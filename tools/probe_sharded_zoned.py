"""Node-range sharding of the zone-aware tightly-pack packers, ms per independent batch: one device (gf_fit_batch,
fit_zoned_fused_kernel), 8 shards of one device through the in-library multi-device context (gf_init with a repeated id), and 8
shards as a thread group of HipShardEngines (gangfit/sharded.py).  Sizes: the headline (10 000 nodes x 1 000 applications) and
BASELINE config 4 congested (50 000 x 10 000); three zones in the reference's AZ-major order.  Every answer is compared with the
one-device answer.  Run on the MI355X box:  python tools/probe_sharded_zoned.py [out.json]"""
import json
import os
import sys
import threading
import time

import numpy as np

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "k8s-spark-scheduler_amd")]
import torch  # noqa: E402

import gangfit  # noqa: E402
from gangfit import sharded  # noqa: E402
from gangfit import workloads as wl  # noqa: E402

IND = gangfit.GF_MODE_INDEPENDENT
SHARDS = 8
ALGOS = [("single-az-tightly-pack", gangfit.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK), ("az-aware-tightly-pack", gangfit.GF_ALGO_AZ_AWARE_TIGHTLY_PACK),
         ("tightly-pack", gangfit.GF_ALGO_TIGHTLY_PACK)]


def _install(ctx, snap, zone, order):
    ctx.set_snapshot(snap.avail, snap.sched)
    ctx.set_zones(zone)
    ctx.set_orders(order, order)


def _ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _thread_group(snap, zone, order, algo, apps, steps, warmup):
    """ms per batch of SHARDS HipShardEngines on cuda:0 (rank 0's wall time, median) and rank 0's answer."""
    group = sharded.ThreadGroup(SHARDS)
    out, errs = {}, []

    def work(r):
        try:
            with gangfit.Context(0) as ctx:
                _install(ctx, snap, zone, order)
                eng = sharded.HipShardEngine(ctx, r, SHARDS, "cuda:0")
                sb = sharded.ShardedBatch(eng, group.comm(r), algo, apps)
                ts = []
                for i in range(warmup + steps):
                    group._barrier.wait()
                    t0 = time.perf_counter()
                    sb.step()
                    eng.stream.synchronize()
                    group._barrier.wait()
                    if i >= warmup:
                        ts.append((time.perf_counter() - t0) * 1e3)
                if r == 0:
                    out["ms"] = float(np.median(ts))
                    out["answer"] = sb.fetch()
        except Exception as e:
            errs.append(e)
            group._barrier.abort()

    ts = [threading.Thread(target=work, args=(r,)) for r in range(SHARDS)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    if errs:
        raise errs[0]
    return out["ms"], out["answer"]


def _same(a, b):
    return bool(np.array_equal(a.results, b.results) and np.array_equal(a.exec_nodes, b.exec_nodes))


def main():
    torch.cuda.init()
    sizes = [("headline 10000 x 1000", wl.headline(10000, 1000).snapshot, wl.headline(10000, 1000), 20, 5),
             ("config4 congested 50000 x 10000", wl.make_snapshot(50000, 0x5EED0004, 0.93, 1.0), wl.config(4), 5, 2)]
    rows = []
    for name, snap, w, steps, warmup in sizes:
        zone = (wl.splitmix64(0xA3, len(snap.avail), 9) % np.uint64(3)).astype(np.uint32)
        order = wl.reference_node_order(snap.avail, zone)
        apps = gangfit.make_apps(w.drv, w.exe, w.k)
        for aname, algo in ALGOS:
            with gangfit.Context(0) as one:
                _install(one, snap, zone, order)
                ref = one.fit_batch(IND, algo, apps)
                one_ms = _ms(lambda: one.fit_batch(IND, algo, apps), steps, warmup)
            with gangfit.Context(devices=[0] * SHARDS) as g:
                _install(g, snap, zone, order)
                g_ok = _same(g.fit_batch(IND, algo, apps), ref) and g.shard_count() == SHARDS
                g_ms = _ms(lambda: g.fit_batch(IND, algo, apps), steps, warmup)
            tg_ms, tg_out = _thread_group(snap, zone, order, algo, apps, steps, warmup)
            row = {"size": name, "packer": aname, "zones": 3, "order": "az-major (reference)", "shards": SHARDS,
                   "one_device_ms": round(one_ms, 3), "in_library_8_shards_ms": round(g_ms, 3),
                   "thread_group_8_shards_ms": round(tg_ms, 3), "in_library_same": g_ok, "thread_group_same": _same(tg_out, ref),
                   "feasible_fraction": float(ref.results["has_capacity"].mean())}
            print(json.dumps(row), flush=True)
            rows.append(row)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
