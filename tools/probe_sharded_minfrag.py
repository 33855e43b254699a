"""Node-range sharding of the minimal-fragmentation packers, ms per independent batch: one device (gf_fit_batch) against 8
in-process shards of the same device — a thread group of HipShardEngines (gangfit/sharded.py: ShardedMinfragBatch) and the in-library
multi-device context (gf_init with a repeated id).  Sizes: the headline (10 000 nodes x 1 000 applications) and BASELINE config 4
on the congested cluster (50 000 x 10 000); three zones in the reference's AZ-major order.  The three routes are timed in
INTERLEAVED rounds of one process (one device, in-library, thread group, one device, ...) and reported as medians (and minima);
then the three exchanges of a batch from step_timed, and the bytes a rank contributes to the first exchange per application.
Every answer is compared with the one-device answer.  Eight shards of ONE device share its compute units: this measures the
overhead of the decomposition, not what eight GPUs would gain.
Run on the MI355X box:  python tools/probe_sharded_minfrag.py [out.txt]"""
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
ALGOS = [("minimal-fragmentation", gangfit.GF_ALGO_MINIMAL_FRAGMENTATION),
         ("single-az-minimal-fragmentation", gangfit.GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION)]


def _install(ctx, snap, zone, order):
    ctx.set_snapshot(snap.avail, snap.sched)
    ctx.set_zones(zone)
    ctx.set_orders(order, order)


def _same(a, b):
    return bool(np.array_equal(a.results, b.results) and np.array_equal(a.exec_nodes, b.exec_nodes))


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _probe(snap, zone, order, algo, apps, rounds, warmup, timed_rounds):
    """Interleaved rounds; the shards' threads wait at `gate` while the main thread times the other two routes."""
    group = sharded.ThreadGroup(SHARDS)
    gate = threading.Barrier(SHARDS + 1)
    total = warmup + rounds + timed_rounds
    out, errs = {"tg_ms": [], "exchange_us": []}, []

    def work(r):
        try:
            with gangfit.Context(0) as ctx:
                _install(ctx, snap, zone, order)
                eng = sharded.HipShardEngine(ctx, r, SHARDS, "cuda:0")
                sb = sharded.ShardedMinfragBatch(eng, group.comm(r), algo, apps)
                for i in range(total):
                    gate.wait()
                    t0 = time.perf_counter()
                    if i < warmup + rounds:
                        sb.step()
                        eng.stream.synchronize()
                    else:
                        ex = sb.step_timed()
                    gate.wait()
                    if r == 0 and warmup <= i < warmup + rounds:
                        out["tg_ms"].append((time.perf_counter() - t0) * 1e3)
                    if r == 0 and i >= warmup + rounds:
                        out["exchange_us"].append(ex)
                if r == 0:
                    out["answer"] = sb.fetch()
                    out["first_exchange_bytes_per_app"] = sb.first_exchange_bytes_per_app()
        except Exception as e:
            errs.append(e)
            gate.abort()
            group._barrier.abort()

    ts = [threading.Thread(target=work, args=(r,)) for r in range(SHARDS)]
    [t.start() for t in ts]
    one_ms, lib_ms = [], []
    try:
        with gangfit.Context(0) as one, gangfit.Context(devices=[0] * SHARDS) as g:
            _install(one, snap, zone, order)
            _install(g, snap, zone, order)
            ref = one.fit_batch(IND, algo, apps)
            lib_ok = _same(g.fit_batch(IND, algo, apps), ref) and g.shard_count() == SHARDS
            for i in range(total):
                a = _timed(lambda: one.fit_batch(IND, algo, apps))
                b = _timed(lambda: g.fit_batch(IND, algo, apps))
                if warmup <= i < warmup + rounds:
                    one_ms.append(a)
                    lib_ms.append(b)
                gate.wait()  # the thread group's turn
                gate.wait()
            lib_ok = lib_ok and g.shard_count() == SHARDS
    except threading.BrokenBarrierError:
        pass
    except BaseException:  # the shards' threads must not wait for a main thread that is gone
        gate.abort()
        group._barrier.abort()
        [t.join() for t in ts]
        raise
    [t.join() for t in ts]
    if errs:
        raise errs[0]
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    return {"one_device_ms": med(one_ms), "one_device_min_ms": round(min(one_ms), 3),
            "in_library_8_shards_ms": med(lib_ms), "in_library_8_shards_min_ms": round(min(lib_ms), 3),
            "thread_group_8_shards_ms": med(out["tg_ms"]), "thread_group_8_shards_min_ms": round(min(out["tg_ms"]), 3),
            "exchange_us_counts_drivers_placements": [round(float(x), 1) for x in np.median(np.array(out["exchange_us"]), axis=0)],
            "first_exchange_bytes_per_app_and_rank": out["first_exchange_bytes_per_app"],
            "in_library_same": lib_ok, "thread_group_same": _same(out["answer"], ref),
            "feasible_fraction": float(ref.results["has_capacity"].mean()), "rounds": rounds}


def main():
    torch.cuda.init()
    sizes = [("headline 10000 x 1000", wl.headline(10000, 1000).snapshot, wl.headline(10000, 1000), 15, 3, 5),
             ("config4 congested 50000 x 10000", wl.make_snapshot(50000, 0x5EED0004, 0.93, 1.0), wl.config(4), 7, 2, 3)]
    lines = ["device: " + torch.cuda.get_device_name(0)]
    for name, snap, w, rounds, warmup, timed_rounds in sizes:
        zone = (wl.splitmix64(0xA3, len(snap.avail), 9) % np.uint64(3)).astype(np.uint32)
        order = wl.reference_node_order(snap.avail, zone)
        apps = gangfit.make_apps(w.drv, w.exe, w.k)
        for aname, algo in ALGOS:
            row = {"size": name, "packer": aname, "zones": 3, "order": "az-major (reference)", "shards": SHARDS}
            row.update(_probe(snap, zone, order, algo, apps, rounds, warmup, timed_rounds))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
