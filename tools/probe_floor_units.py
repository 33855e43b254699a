"""What the floored narrow form (csrc/gangfit_floor_units.h) buys a FIFO chain whose table shares no unit, for every packer, at
   10 000 nodes x 3 zones with a queue of 999 + 1 drivers (the headline workload's shapes; every node carries a remainder of up to
   99 milli-cores and 2^20 - 1 bytes, so the column gcds are 1 and memory has no exact int32 form):
  floored  option narrow_floor = 1 (the default): the LDS chain kernels on floor(value / unit) + remainders
  wide     option narrow_floor = 0 on the same table: the route the floored form replaces (fit_fifo_chain_kernel /
           fit_fifo_generic_kernel, no chain cache)
  exact    the same queue on the same table with the remainders removed: the exact LDS chain of the same tree — the difference to
           `floored` is what the remainder reads and the residual fix-up cost
Per arm: `first` = the first chain after an install (floored: includes building the floored snapshot), `cold` = a chain with the
cache dropped, `warm` = the same Filter again (resumed from the cached chain's tip where there is a cache).  One context per
arm, the arms interleaved round by round in one process; a figure is the median over the rounds [min, max], milliseconds per
blocking gf_fit_batch call (each ends in a device synchronise); warm is the mean of `calls` back-to-back calls per round.
The last figures: tightly-pack behind gf_snapshot_build finalized on the device, build and first chain, floored against wide.
   python tools/probe_floor_units.py [rounds >= 5] [calls] [out]      (run on the MI355X box; out: profiles/floor_units.txt)"""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "k8s-spark-scheduler_amd")]
import gangfit
from gangfit import _native as N
from gangfit import workloads as wl
rounds = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "floor_units.txt")
FIFO = gangfit.GF_MODE_FIFO_CHAIN
PACKERS = ((0, "tightly-pack"), (1, "distribute-evenly"), (2, "minimal-fragmentation"), (3, "az-aware-tightly-pack"),
           (4, "single-az-tightly-pack"), (5, "single-az-minimal-fragmentation"))
N_NODES, N_APPS, N_ZONES = 10000, 1000, 3
median = lambda v: sorted(v)[len(v) // 2]
fmt = lambda v: f"{median(v):8.3f} [{min(v):.3f}, {max(v):.3f}]"

w = wl.headline(N_NODES, N_APPS)
rng = np.random.default_rng(0xF100)
zone = rng.integers(0, N_ZONES, size=N_NODES).astype(np.uint32)
exact = w.snapshot.avail
rem = exact + np.stack([rng.integers(0, 100, size=N_NODES), rng.integers(0, 1 << 20, size=N_NODES), np.zeros(N_NODES, dtype=np.int64)], axis=1)
sched = np.maximum(w.snapshot.sched, rem)
order = wl.reference_node_order(exact, zone)  # one order for both tables: the arms decide the same queue over the same slots
apps = gangfit.make_apps(w.drv, w.exe, w.k, np.ones(N_APPS, dtype=np.uint32))
_, total_k = gangfit.with_offsets(apps)
ARMS = (("floored", rem, 1), ("wide", rem, 0), ("exact", exact, 1))

lines = [f"# FIFO chains of {N_APPS - 1} + 1 drivers, {N_NODES} nodes x {N_ZONES} zones: {rounds} interleaved rounds, median [min, max] in ms per blocking call",
         f"# floored / wide = narrow_floor 1 / 0 on a table with a remainder on every node; exact = the same table without them; warm = mean of {calls} calls"]
ctxs = {name: gangfit.Context(0, options={"narrow_floor": floor}) for name, _, floor in ARMS}
try:
    res = np.zeros(N_APPS, dtype=N.RESULT_DTYPE)
    exec_nodes = np.zeros(total_k + 1, dtype=np.uint32)
    failed = np.zeros(1, dtype=np.int32)

    def install(name, table):
        c = ctxs[name]
        c.set_snapshot(table, sched)
        c.set_zones(zone)
        c.set_orders(order, order)

    def chain(name, algo):
        c = ctxs[name]
        t0 = time.perf_counter()
        rc = c._lib.gf_fit_batch(c._h, FIFO, algo, N_APPS, N.ptr(apps), N.ptr(res), N.ptr(exec_nodes), total_k, N.ptr(failed))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == N.GF_OK, c.last_error()
        return dt

    for algo, pname in PACKERS:
        t = {(name, what): [] for name, _, _ in ARMS for what in ("first", "cold", "warm")}
        answers = {}
        for r in range(rounds + 1):
            for name, table, _ in ARMS:
                install(name, table)
                ctxs[name].chain_cache_stats(reset=True)
                first = chain(name, algo)
                answers[name] = (res.tobytes(), exec_nodes.tobytes(), int(failed[0]), ctxs[name].chain_units(), ctxs[name].chain_cache_stats()[0])
                ctxs[name].set_option("chain_cache", 1)  # drops the cache, keeps the floored snapshot
                cold = chain(name, algo)
                warm = sum(chain(name, algo) for _ in range(calls)) / calls
                if r >= 1:  # (the first round grows buffers and loads code objects)
                    t[name, "first"].append(first)
                    t[name, "cold"].append(cold)
                    t[name, "warm"].append(warm)
        assert answers["floored"][:3] == answers["wide"][:3], f"{pname}: the two routes disagree"
        routes = {name: answers[name][3:] for name, _, _ in ARMS}  # (units, floored) and the chains an LDS kernel served
        assert routes["floored"][0][3] == 1 and routes["floored"][1] == 1 and routes["wide"][1] == 0 and routes["exact"][0][3] == 0, routes
        lines.append(f"{pname} (units {answers['floored'][3][:3]}, exact {answers['exact'][3][:3]}; chain ends at {answers['floored'][2]}):")
        for name, _, _ in ARMS:
            lines.append(f"  {name:8s} first {fmt(t[name, 'first'])}  cold {fmt(t[name, 'cold'])}  warm {fmt(t[name, 'warm'])}")
        fl, wd, ex = (median(t[n, "cold"]) for n in ("floored", "wide", "exact"))
        lines.append(f"  cold: wide / floored x{wd / fl:.1f}, floored / exact x{fl / ex:.3f};  warm: wide / floored "
                     f"x{median(t['wide', 'warm']) / median(t['floored', 'warm']):.1f}, floored / exact x{median(t['floored', 'warm']) / median(t['exact', 'warm']):.3f}")
        print("\n".join(lines[-5:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    # A snapshot built on the device (gf_snapshot_build, finalized there) reads back no signs: the first floored chain behind it also
    # fetches the table's range (table_range_kernel + one blocking copy of six words).  `first` of tightly-pack behind such a build,
    # floored against wide, and the build itself.
    usage = sched - rem
    has = usage.any(axis=1)
    build = dict(alloc=sched, node_flags=np.full(N_NODES, 2 | 4, dtype=np.uint32), name_rank=np.arange(N_NODES, dtype=np.uint32),
                 res_node=np.nonzero(has)[0].astype(np.uint32), res_req=usage[has], zone=zone, n_zones=N_ZONES, want_orders=False)
    tb = {(name, what): [] for name in ("floored", "wide") for what in ("build", "first")}
    for r in range(rounds + 1):
        for name in ("floored", "wide"):
            t0 = time.perf_counter()
            ctxs[name].build_snapshot(**build)
            dt = (time.perf_counter() - t0) * 1e3
            first = chain(name, 0)
            if r >= 1:
                tb[name, "build"].append(dt)
                tb[name, "first"].append(first)
        assert ctxs["floored"].chain_units()[3] == 1 and ctxs["wide"].chain_units()[3] == 0
    lines.append("tightly-pack behind gf_snapshot_build finalized on the device (the floored arm's first chain fetches the table's range too):")
    for name in ("floored", "wide"):
        lines.append(f"  {name:8s} build {fmt(tb[name, 'build'])}  first {fmt(tb[name, 'first'])}")
    print("\n".join(lines[-3:]), flush=True)
finally:
    for c in ctxs.values():
        c.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
