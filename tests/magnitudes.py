"""Problems at the edges of the quantity contract (include/gangfit.h: available in (-2^62, 2^62), requests in [0, 2^62),
K in [0, GF_MAX_K]), in the shape of test_gpu_zones._zoned_problem: (avail, sched, zone, D, X, drv, exe, k, flags).

A helper module, not a test file.  Every regime puts its edges in on purpose; tests/test_oracle_magnitudes.py checks that it
still does.  What each drawn value reaches:

  bytes        memory in arbitrary bytes (gcd 1, magnitudes >= 2^30): the table has no narrow form, every chain of every
               packer takes the wide kernels (fit_fifo_chain_kernel, fit_fifo_generic_kernel).  Decimal requests (4G = 4e9),
               milli-cpus off the quarter-core grid: Quantity.Value()'s rounding away from zero in the efficiencies.
  narrow-edge  a scaled magnitude of exactly 2^30-1 (and -(2^30-1)) in the table, requests scaling to 2^30-1: the LDS chains.
               Twins one unit past (a table value or a request scaling to 2^30): the wide twins (prepare_app, narrow_ok).  Unit
               refinement (narrow_units) landing exactly on room = (2^30-1)/nmax, and one past it.
  huge         availabilities q*e-1, q*e, q*e+e-1 around every request e in 1 .. 2^62-1, q in {0, 1, K-1, K, K+1, 2^40-1,
               2^40, 2^40+1, (2^62-1)/e}: cap_dim's +-1 fix-up and its clamp at k+1, cap_dim_full's 64-bit division (q >= 2^40),
               the int64 -> float64 roundings of the efficiencies; requests with a zero dimension and all-zero requests
               (capacity math.MaxInt: minimal fragmentation's (K + maxCapacity) / 2 wraps).  +-(2^62-1) itself.
  max-k        K = GF_MAX_K and GF_MAX_K-1 with zero requests (unlimited capacity) and with capacity sums of exactly K-1, K, K+1.
  efficiency   schedulable / used quantities >= 2^53 with low bits float64 cannot hold; cpu around 2^32 milli-cores (the
               small_cpu shortcut of gangfit_fifo_zoned.inc, its >> 32 test); used < 0 and schedulable = 0; zones that are
               exact twins (equal averages) and twins one ulp apart: chooseBestResult's strict <.
"""
import numpy as np

GF_MAX_K = 1 << 20
QMAX = (1 << 62) - 1  # the largest quantity the contract admits
GIB = 1 << 30
NARROW = (1 << 30) - 1  # the largest scaled magnitude of the int32 chains
REGIMES = ("bytes", "narrow-edge", "huge", "max-k", "efficiency")
LAYOUTS = ("merged", "identical", "general")
# the literal oracle's driver retry loop is O(|D| N) per gang that does not fit: only max-k's infeasible gangs of 2^20
# executors make that matter
CLOSED_FORM = {"bytes": False, "narrow-edge": False, "huge": False, "max-k": True, "efficiency": False}


def orders(rng, n, layout):
    """Driver / executor orders as test_gpu_parity._random_problem draws them (unknown names and, merged, a repeated driver
    candidate included)."""
    unknown = np.array([n + 5, n + 1000], dtype=np.int64)
    if layout == "general":
        X = rng.permutation(np.concatenate([rng.permutation(n)[: int(rng.integers(max(1, n // 2), n + 1))], unknown[:1]]))
        D = rng.permutation(np.concatenate([rng.permutation(n)[: int(rng.integers(1, n + 1))], unknown]))
        return D.astype(np.uint32), X.astype(np.uint32)
    base = rng.permutation(n)
    if layout == "identical":
        return base.astype(np.uint32), base.astype(np.uint32)
    X = base[rng.random(n) < 0.85]
    D = base[rng.random(n) < 0.75]
    X = X if len(X) else base[:1]
    D = D if len(D) else base[-1:]
    X = np.insert(X, int(rng.integers(0, len(X) + 1)), unknown[0])
    D = np.append(np.insert(D, int(rng.integers(0, len(D) + 1)), unknown[1]), D[0])
    return D.astype(np.uint32), X.astype(np.uint32)


def _sched_over(rng, avail, spread):
    """Schedulable >= max(available, 0), below 2^62; some nodes at 0 (normalizeResource), some overcommitted."""
    sched = np.minimum(np.maximum(avail, 0) + rng.integers(0, spread, size=avail.shape), QMAX).astype(np.int64)
    sched[rng.random(len(avail)) < 0.05] = 0
    return sched


def _zones(rng, n, n_zones):
    return (rng.integers(0, n_zones, size=n).astype(np.uint32) * 7 + 3).astype(np.uint32)


def bytes_regime(rng, layout, n_zones, n=300, a=40):
    mem_s = rng.integers(16, 513, size=n) * GIB + rng.integers(-(1 << 29), 1 << 29, size=n)
    mem_a = mem_s - rng.integers(0, 1 << 36, size=n)
    over = rng.random(n) < 0.05
    mem_a[over] = mem_s[over] + rng.integers(1, 1 << 26, size=int(over.sum()))  # used < 0 (available above schedulable)
    mem_a[0], mem_a[1] = 17 * GIB + 1, 17 * GIB + 2  # consecutive values: the memory gcd is 1, whatever else is drawn
    cpu_s = rng.integers(4000, 96000, size=n) | 1  # odd milli-cores: never a multiple of 250
    cpu_a = cpu_s - rng.integers(-300, 40000, size=n)
    avail = np.stack([cpu_a, mem_a, rng.integers(-1, 9, size=n)], axis=1).astype(np.int64)
    sched = np.stack([cpu_s, mem_s, rng.integers(0, 9, size=n)], axis=1).astype(np.int64)
    sched[:, 2] = np.maximum(sched[:, 2], avail[:, 2])
    decimal = np.array([10 ** 9, 4 * 10 ** 9, 2 * 10 ** 9 + 500 * 10 ** 6, 8 * 10 ** 9], dtype=np.int64)
    binary = np.array([GIB, 4 * GIB, 7 * GIB + 13, 3 * GIB - 4096 + 1], dtype=np.int64)
    pick = lambda size: np.where(rng.random(size) < 0.5, rng.choice(decimal, size), rng.choice(binary, size))  # noqa: E731
    drv = np.stack([rng.integers(1, 8000, size=a), pick(a), np.zeros(a, dtype=np.int64)], axis=1).astype(np.int64)
    exe = np.stack([rng.choice([333, 1001, 1500, 2750, 3999], size=a), pick(a), (rng.random(a) < 0.2).astype(np.int64)],
                   axis=1).astype(np.int64)
    k = rng.integers(0, 160, size=a).astype(np.int32)
    D, X = orders(rng, n, layout)
    return avail, sched, _zones(rng, n, n_zones), D, X, drv, exe, k, (rng.random(a) < 0.9).astype(np.uint32)


# narrow-edge variants: (name, route the FIFO chains of a batch must take on the merged layout)
NARROW_VARIANTS = (("table-at-bound", "lds"), ("table-past-bound", "wide"), ("request-at-bound", "lds"),
                   ("request-past-bound", "wide"), ("refine-at-room", "lds"), ("refine-past-room", "wide"))
REFINE_UNIT = 1025 * 1024  # the refinement tables' memory unit; nmax = 2^20-1 gives room = (2^30-1) // (2^20-1) = 1024


def narrow_edge(rng, layout, n_zones, variant, n=160, a=24):
    """variant: an entry of NARROW_VARIANTS.  Cpu in quarter cores (unit 250), memory in MiB (unit 2^20) or, refine-*, in
    REFINE_UNIT; gpu in ones.  Every request of a batch is a multiple of the table's units, except the one refine-* request
    that moves them: the route is the variant's, not chance's."""
    unit = REFINE_UNIT if variant.startswith("refine") else 1 << 20
    top = (1 << 20) - 1 if variant.startswith("refine") else NARROW
    mem = rng.integers(1, 1 << 12, size=n) * 2 - 1  # odd scaled values: gcd(unit-multiples) stays the unit
    mem[0], mem[1] = top, -top  # the largest scaled magnitude, both signs
    mem[2] = 1
    if variant == "table-past-bound":
        mem[3] = NARROW + 1  # one unit past 2^30-1: the table has no narrow form
    cpu = rng.integers(-4, 400, size=n)
    cpu[4] = 1
    avail = np.stack([cpu * 250, mem * unit, rng.integers(-1, 9, size=n)], axis=1).astype(np.int64)
    sched = _sched_over(rng, avail, 1 << 30)
    sched[:, 0] = sched[:, 0] // 250 * 250
    drv = np.stack([rng.integers(0, 8, size=a) * 250, rng.integers(0, 64, size=a) * unit, np.zeros(a, dtype=np.int64)],
                   axis=1).astype(np.int64)
    exe = np.stack([rng.integers(1, 6, size=a) * 250, rng.integers(1, 512, size=a) * unit, (rng.random(a) < 0.3) * 1],
                   axis=1).astype(np.int64)
    drv[0, 1] = top * unit  # a driver that fits only node 0, exactly: q*e with q = 1
    if variant == "request-at-bound":
        exe[1, 1] = NARROW * unit  # scaled value 2^30-1: still narrow
        drv[2, 1] = NARROW * unit
    if variant == "request-past-bound":
        exe[1, 1] = (NARROW + 1) * unit  # scaled value 2^30: the wide twin
    if variant == "refine-at-room":
        exe[1, 1] = 1025  # units -> gcd(1025*1024, 1025) = 1025: factor 1024 = room
    if variant == "refine-past-room":
        exe[1, 1] = 1024  # units -> 1024: factor 1025 = room + 1, no refinement, and 1024 is not a multiple of the unit
    k = rng.integers(0, 40, size=a).astype(np.int32)
    D, X = orders(rng, n, layout)
    return avail, sched, _zones(rng, n, n_zones), D, X, drv, exe, k, np.ones(a, dtype=np.uint32)


HUGE_REQUESTS = (1, 3, 1000, (1 << 20) + 7, NARROW, 1 << 30, (1 << 33) + 5, 1 << 40, (1 << 40) + 9, (1 << 50) + 3,
                 (1 << 61) + 1, QMAX)


def huge_quotients(e, k):
    """The quotients whose neighbourhoods the availabilities around request e sit in."""
    qs = {0, 1, max(k - 1, 0), k, k + 1, (1 << 40) - 1, 1 << 40, (1 << 40) + 1, QMAX // e - 1, QMAX // e}
    return sorted(q for q in qs if 0 <= q and q * e + e - 1 <= QMAX)


def huge(rng, layout, n_zones, a=None):
    reqs = list(HUGE_REQUESTS)
    a = len(reqs) + 4 if a is None else a
    drv = np.zeros((a, 3), dtype=np.int64)
    exe = np.zeros((a, 3), dtype=np.int64)
    k = np.zeros(a, dtype=np.int32)
    rows = []
    for i in range(a):
        e = reqs[i % len(reqs)]
        j = (0, 1, 1)[i % 3]  # mostly memory, sometimes cpu
        k[i] = int(rng.choice([1, 2, 7, 1000]))
        if i >= len(reqs):  # every dimension 0 (capacity math.MaxInt), or cpu-only with memory 0
            e, j = (0, 1) if i % 2 else (reqs[int(rng.integers(0, len(reqs)))], 0)
        exe[i, j] = e
        if i % 4 == 1 and e:
            exe[i, 2 - j // 2] = int(rng.integers(1, 4))  # a second, small dimension
        drv[i, j] = int(rng.choice([0, 1, e]))
        for q in huge_quotients(max(e, 1), int(k[i])):
            for off in (-1, 0, max(e, 1) - 1):
                v = q * max(e, 1) + off
                if -QMAX <= v <= QMAX:
                    row = [int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 62)), int(rng.integers(0, 9))]
                    row[j] = v
                    rows.append(row)
    rows += [[QMAX, QMAX, QMAX], [-QMAX, -QMAX, -QMAX], [QMAX, -QMAX, 0], [0, 0, 0]]
    avail = np.array(rows, dtype=np.int64)
    avail = avail[rng.permutation(len(avail))]
    n = len(avail)
    sched = _sched_over(rng, avail, 1 << 62)
    D, X = orders(rng, n, layout)
    flags = (rng.random(a) < 0.9).astype(np.uint32)
    return avail, sched, _zones(rng, n, n_zones), D, X, drv, exe, k, flags


def max_k(rng, layout, n_zones, n=48):
    """Five gangs: zero requests at K = 2^20 and 2^20-1; memory executors against a memory column whose capacity sum is
    exactly K, then K+1 for K-1; gpu executors against a gpu column that holds K-1.  The driver asks for cpu only (its node
    keeps its executor capacity) and fits two nodes."""
    K = GF_MAX_K
    e_mem, e_gpu = 3 * GIB + 1, 5
    cmem = np.full(n, K // n, dtype=np.int64)
    cmem[: K - int(cmem.sum())] += 1  # sum exactly K
    cgpu = cmem.copy()
    cgpu[int(np.argmax(cgpu))] -= 1  # sum K-1
    avail = np.stack([np.full(n, 8000, dtype=np.int64), cmem * e_mem + rng.integers(0, e_mem, size=n),
                      cgpu * e_gpu + rng.integers(0, e_gpu, size=n)], axis=1).astype(np.int64)
    avail[[3, n - 5], 0] = 64000
    sched = np.maximum(avail, 0) + 1
    drv = np.tile(np.array([[64000, 0, 0]], dtype=np.int64), (5, 1))
    exe = np.array([[0, 0, 0], [0, 0, 0], [0, e_mem, 0], [0, 0, e_gpu], [0, e_mem, 0]], dtype=np.int64)
    k = np.array([K, K - 1, K, K, K - 1], dtype=np.int32)
    D, X = orders(rng, n, layout)
    return avail, sched, _zones(rng, n, n_zones), D, X, drv, exe, k, np.ones(5, dtype=np.uint32)


def node_eff(avail, sched):
    """computePackingEfficiency of one node with nothing reserved: [cpu, memory, gpu] (efficiency.go:79-103)."""
    def value(v, unit):
        q, r = abs(v) // unit, abs(v) % unit
        return (1 if v >= 0 else -1) * (q + (r > 0))
    e = [value(sched[j] - avail[j], u) / float(max(value(sched[j], u), 1) if sched[j] else 1) for j, u in
         enumerate((1000, 1, 1))]
    return e if sched[2] else e[:2] + [0.0]


def efficiency(rng, layout, n_zones, m=40, a=24):
    """A block of m nodes repeated once per zone (zone z holds node z*m + i, a copy of block node i); zone 1 is zone 0's exact
    twin, zone 2 its twin with every memory-bound node moved up by one ulp of its efficiency.  Orders are block orders with
    the copies of a node next to each other, so the twins pack alike."""
    cpu_s = rng.choice([(1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 32) - 1000], size=m).astype(np.int64)
    cpu_heavy = rng.random(m) < 0.4
    cpu_a = np.where(cpu_heavy, rng.integers(500, 6000, size=m), cpu_s - rng.integers(0, 1 << 20, size=m))  # used crosses 2^32
    mem_s = (np.int64(1) << rng.integers(53, 60, size=m)) + rng.integers(1, 1 << 20, size=m) * 2 + 1  # odd, >= 2^53
    mem_a = mem_s - (mem_s // 10 * rng.integers(2, 9, size=m)) - rng.integers(0, 1 << 10, size=m)
    over = rng.random(m) < 0.1
    mem_a[over] = mem_s[over] + rng.integers(1, 1 << 40, size=int(over.sum()))  # used < 0
    avail = np.stack([cpu_a, mem_a, rng.integers(0, 3, size=m)], axis=1).astype(np.int64)
    sched = np.stack([cpu_s, mem_s, rng.integers(0, 9, size=m)], axis=1).astype(np.int64)
    sched[:, 2] = np.maximum(sched[:, 2], avail[:, 2])
    sched[0] = 0  # schedulable 0 in every dimension: normalizeResource
    avail[0] = [8000, 1 << 54, 0]
    blocks_a, blocks_s = [avail], [sched]
    for z in range(1, n_zones):
        a2 = avail.copy()
        if z == 2:
            for i in range(1, m):
                a2[i, 1] = ulp_twin(avail[i], sched[i])
        blocks_a.append(a2)
        blocks_s.append(sched.copy())
    avail, sched = np.concatenate(blocks_a), np.concatenate(blocks_s)
    zone = (np.repeat(np.arange(n_zones), m) * 7 + 3).astype(np.uint32)
    bD, bX = orders(rng, m, layout)
    expand = lambda o: np.array([int(v) + z * m if v < m else int(v) + (n_zones - 1) * m for v in o for z in  # noqa: E731
                                 (range(n_zones) if v < m else range(1))], dtype=np.uint32)
    D, X = expand(bD), expand(bX)
    drv = np.stack([rng.choice([0, 999, 1000, 1001], size=a), rng.choice([0, 1, (1 << 50) + 1], size=a),
                    np.zeros(a, dtype=np.int64)], axis=1).astype(np.int64)
    exe = np.stack([rng.choice([1, 999, 1000, 2501], size=a), np.where(rng.random(a) < 0.5, 0, (1 << 51) + 7),
                    (rng.random(a) < 0.2) * 1], axis=1).astype(np.int64)  # memory 0: the twins' efficiencies stay apart
    k = rng.integers(0, 30, size=a).astype(np.int32)
    return avail, sched, zone, D, X, drv, exe, k, (rng.random(a) < 0.9).astype(np.uint32)


def ulp_twin(avail, sched):
    """An available memory whose node's memory efficiency is one ulp above this one's; the same value when no such value is
    near (the node is not memory-bound, or schedulable is 0)."""
    e = node_eff(avail, sched)
    if sched[1] == 0 or e[1] <= max(e[0], e[2]):
        return int(avail[1])
    want = np.nextafter(e[1], 2.0)
    for d in range(1, 1 << 12):
        v = int(avail[1]) - d
        if node_eff([avail[0], v, avail[2]], sched)[1] == want:
            return v
    return int(avail[1])


def problem(regime, rng, layout="merged", n_zones=1, variant=None):
    """(avail, sched, zone, D, X, drv, exe, k, flags) of one regime.  variant: a NARROW_VARIANTS name (narrow-edge only)."""
    if regime == "bytes":
        return bytes_regime(rng, layout, n_zones)
    if regime == "narrow-edge":
        return narrow_edge(rng, layout, n_zones, variant or NARROW_VARIANTS[int(rng.integers(0, len(NARROW_VARIANTS)))][0])
    if regime == "huge":
        return huge(rng, layout, n_zones)
    if regime == "max-k":
        return max_k(rng, layout, n_zones)
    if regime == "efficiency":
        return efficiency(rng, layout, n_zones)
    raise ValueError(regime)


def cases(regime, seed=0):
    """Every layout with 1 and 3 zones (narrow-edge: every variant on the merged layout, the others on one layout each).
    Returns [(name, problem tuple, expected FIFO route or None)]."""
    out = []
    rng = np.random.default_rng(seed + 1000 * REGIMES.index(regime))
    if regime == "narrow-edge":
        for v, route in NARROW_VARIANTS:
            for layout, nz in (("merged", 1), ("merged", 3), ("identical" if route == "lds" else "general", 3)):
                out.append((f"{v}/{layout}/{nz}z", narrow_edge(rng, layout, nz, v), route if layout == "merged" else None))
        return out
    for layout in LAYOUTS:
        for nz in (1, 3):
            out.append((f"{layout}/{nz}z", problem(regime, rng, layout, nz), None))
    return out
