"""The edges of the priority sort (csrc/gangfit_snapshot.hip, priority_sort_kernel): crafted build inputs, and a restatement in
plain Python integers of what the kernel plans for them — field widths, key groups, pass count, segment geometry, buffer walk.
No GPU and no gangfit import: tests/test_sort_edges_cpu.py proves here that every case reaches the arm it is built for, and
tests/test_gpu_sort_edges.py runs the same cases on the device against oracle/pysnapshot.py.

plan() and buffer_walk() are NEVER a reference for the order (that is oracle.pysnapshot.build, one np.lexsort); they exist so
that a test can show that a case is on its edge, and they fail that test when the generator drifts off it.

How the columns are made.  A column is lo + (f << tz): f is the field the kernel sorts (width w = bits of its largest value),
tz the trailing zeros every difference shares.  The free values are produced through the real inputs only: allocatable in
[0, 2^62), overhead in [0, 2^61), reservation entries in [0, 2^61).  A negative free value comes from overhead on most nodes
and from reservation entries (in part or in full) on others; the entries of a case sum to less than 2^60 per dimension, so that
the same entries are also accepted by gf_usage_apply (whose bound is on the sum of everything applied plus the largest
overhead).  Every field of width w > 0 holds 0, its largest value (2^w - 1, except the 63-bit memory column whose range ends
at 2^62 + 2^61 - 2) and an odd value; node 0 holds a third of the largest value — neither extreme, yet the reference point of
the trailing zeros — except in the case built for node 0 being the maximum, and where a field has only the values 0 and 1.
The zone field holds every rank 0 .. n_zones - 1 (the value n_zones stands for an unknown zone id, which the ABI refuses).

Wide random memory makes the per-zone sums wrap: the restatement (np.add.at on int64) and the device (64-bit atomic adds) both
add in wrapping 64-bit arithmetic and rank the zones by the wrapped sums, as test_priority_sort_key_groups[two-keys] relies on.

The trailing-zero case "all-even": values that are all even have even differences, so the differences cannot be free of a
common factor; the case takes the nearest edge — every value even, the fields odd and even: tz is exactly 1, the smallest
shift, and a kernel that took the trailing zeros of the VALUES' residues or none at all would build other fields.

Planted into every case of n >= 63 (one node has one order; two nodes cannot hold a tie next to a varying key, and their
only difference per column loses its trailing zeros: the case of two nodes lets the cpu field decide against the name order):
  - min(32, n // 4) groups of two or three nodes equal in (zone, memory, cpu) whose name ranks are j, n - 1 - j and n // 2 + j:
    far apart, and in different segments of the initial (name) order whenever there is more than one segment;
  - with wc > 0: min(32, n // 8) pairs equal in (zone, memory) that differ in cpu only, half of them with the smaller cpu on the
    larger name rank;
  - with wm > 0: one pair equal in (zone, cpu) with memory fields 2^(wm-1) - 1 and 2^(wm-1), the smaller on the larger name rank
    (a memory field one bit too narrow turns the pair round).
"""
import numpy as np

UNSCHEDULABLE, READY, DRIVER_CANDIDATE = 1, 2, 4
UNRANKED = 0xFFFFFFFF
SORT_WG = 64          # kSortWG
MIN_FREE = -((1 << 61) - 1)   # alloc 0, overhead 2^61 - 1
MAX_FREE = (1 << 62) - 1
RES_BUDGET = 1 << 60  # sum of a case's reservation entries per dimension (see the module docstring)
M64 = (1 << 64) - 1


def bits_of(v):
    return int(v).bit_length()


def _biased(v):
    return (int(v) + (1 << 63)) & M64


def plan(avail_cpu, avail_mem, n_zones, label_width=0):
    """Steps 1-2 of priority_sort_kernel (and metadata_kernel's range words) on Python integers."""
    c = [_biased(v) for v in avail_cpu]
    m = [_biased(v) for v in avail_mem]
    n = len(c)
    cor = mor = 0
    for v in c:
        cor |= (v - c[0]) & M64
    for v in m:
        mor |= (v - m[0]) & M64
    tzc = (cor & -cor).bit_length() - 1 if cor else 0
    tzm = (mor & -mor).bit_length() - 1 if mor else 0
    wc, wm, wz = bits_of((max(c) - min(c)) >> tzc), bits_of((max(m) - min(m)) >> tzm), bits_of(n_zones)
    n_groups = 1 if wc + wm + wz <= 64 else (2 if wm + wz <= 64 else 3)
    groups = []
    for g in range(n_groups):
        has_c, has_m, has_z = g == 0, n_groups == 1 or g == 1, g + 1 == n_groups
        groups.append((wc if has_c else 0) + (wm if has_m else 0) + (wz if has_z else 0))
    if label_width:
        groups.append(int(label_width))
    seg_log = 6
    while (SORT_WG << seg_log) < n:
        seg_log += 1
    seg = 1 << seg_log
    return dict(wc=wc, wm=wm, wz=wz, tzc=tzc, tzm=tzm, n_groups=n_groups, groups=groups,
                total_passes=sum((w + 7) // 8 for w in groups), seg=seg, n_seg=(n + seg - 1) >> seg_log)


def buffer_walk(group_widths):
    """The dst_buf rule of the pass loop: [(src, dst)] per pass, over all groups (a group of width 0 is skipped)."""
    total = sum((w + 7) // 8 for w in group_widths)
    walk, src, P = [], 0, 0
    for w in group_widths:
        for _shift in range(0, w, 8):
            remaining = total - P
            dst = 1 if remaining & 1 else (0 if src == 2 else 2)
            walk.append((src, dst))
            src = dst
            P += 1
    return walk


def key_build_sources(group_widths):
    """[(group index, buffer its key build reads and rewrites, passes done before it)] for every group that runs."""
    out, P = [], 0
    walk = buffer_walk(group_widths)
    for g, w in enumerate(group_widths):
        if w == 0:
            continue
        out.append((g, walk[P - 1][1] if P else 0, P))
        P += (w + 7) // 8
    return out


def label_width_of(rank):
    """plan_labels (gangfit_label_plan.h): bits of the largest ranked value + 1; 0 when the array re-sorts nothing."""
    if rank is None or len(np.unique(rank)) <= 1:
        return 0
    r = np.asarray(rank, dtype=np.uint64)
    ranked = r[r != UNRANKED]
    return bits_of((int(ranked.max()) if len(ranked) else 0) + 1)


# ------------------------------------------------------------------------------------------------------------- the generator
def _split_inputs(rng, n, free):
    """allocatable, overhead and reservation entries (one dimension) with allocatable - (usage + overhead) = free."""
    alloc, over = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    ent_node, ent_amt = [], []
    budget, by_res = RES_BUDGET - (1 << 30), 0
    for i in range(n):
        v = int(free[i])
        if v >= 0:
            o = int(rng.integers(0, min(1 << 16, MAX_FREE - v) + 1)) if rng.random() < 0.5 else 0
            alloc[i] = v + o
            if o and rng.random() < 0.25 and o <= budget:
                ent_node.append(i)
                ent_amt.append(o)
                budget -= o
            else:
                over[i] = o
            continue
        a = int(rng.integers(0, min(1 << 20, v - MIN_FREE) + 1))
        alloc[i] = a
        need = a - v  # usage + overhead
        r = 0
        if i % 3 != 1 and by_res < 192 and budget > 0:  # reservations carry it on these nodes, in full where the budget allows
            r = min(need, budget, 1 << 58)
            budget -= r
            by_res += 1
            first = r // 3 if (i % 2 and r >= 3) else 0  # some nodes: two entries
            for amt in ((first, r - first) if first else (r,)):
                ent_node.append(i)
                ent_amt.append(amt)
        over[i] = need - r
    return alloc, over, ent_node, ent_amt


def _inputs(rng, free_cpu, free_mem):
    n = len(free_cpu)
    ac, oc, cn, ca = _split_inputs(rng, n, free_cpu)
    am, om, mn, ma = _split_inputs(rng, n, free_mem)
    gpu = np.where(rng.random(n) < 0.1, 8, 0).astype(np.int64)
    alloc = np.stack([ac, am, gpu], axis=1)
    over = np.stack([oc, om, np.zeros(n, dtype=np.int64)], axis=1)
    res_node = np.array(cn + mn + [n + 1], dtype=np.uint32)  # the last entry names no listed node: ignored
    res_req = np.zeros((len(res_node), 3), dtype=np.int64)
    res_req[:len(cn), 0] = ca
    res_req[len(cn):len(cn) + len(mn), 1] = ma
    res_req[-1] = (1000, 1 << 30, 1)
    order = rng.permutation(len(res_node))
    return alloc, over, res_node[order], res_req[order]


def _fmax(w):
    return (1 << w) - 1


def _lo(fmax, tz):
    return max(MIN_FREE, -((fmax << tz) // 3))


def _case(seed, n, wc, wm, n_zones, tzc=0, tzm=0, loc=None, lom=None, node0_max=False, label_max=None):
    """One build input whose cpu / memory fields are wc / wm bits wide behind tzc / tzm shared trailing zeros."""
    rng = np.random.default_rng(seed)
    fmc, fmm = _fmax(wc), _fmax(wm)
    if wm == 63:  # the widest range the ABI admits: [-(2^61 - 1), 2^62 - 1]
        lom, fmm = MIN_FREE, MAX_FREE - MIN_FREE
    loc = (_lo(fmc, tzc) if wc else 777) if loc is None else loc
    lom = (_lo(fmm, tzm) if wm else 12345) if lom is None else lom
    assert MIN_FREE <= loc and loc + (fmc << tzc) <= MAX_FREE and MIN_FREE <= lom and lom + (fmm << tzm) <= MAX_FREE
    name_rank = rng.permutation(n).astype(np.uint32)
    at_name = np.argsort(name_rank)  # name position -> node
    zone = rng.integers(0, n_zones, size=n).astype(np.uint32)
    fc = rng.integers(0, fmc + 1, size=n, dtype=np.int64)
    fm = rng.integers(0, fmm + 1, size=n, dtype=np.int64)
    tie_groups = cpu_pairs = 0
    together = []  # planted nodes that must stay comparable under a label group: they get one label rank
    if n == 2:  # two nodes of one zone: the cpu field decides, against the name order
        fc[:], zone[1] = ((0, fmc) if name_rank[0] > name_rank[1] else (fmc, 0)), zone[0]
    elif n >= 63:
        G, Q = min(32, n // 4), (min(32, n // 8) if wc else 0)
        groups = []
        for j in range(G):
            pos = [j, n - 1 - j] + ([n // 2 + j] if (j % 2 == 0 and n >= 256) else [])
            groups.append([int(at_name[p]) for p in pos])
        tied = {i for g in groups for i in g}
        free = [int(i) for i in rng.permutation(np.arange(1, n)) if int(i) not in tied]
        take = iter(free)
        fc[0], fm[0] = (fmc, fmm) if node0_max else (fmc // 3, fmm // 3)
        for f, fmax, w in ((fc, fmc, wc), (fm, fmm, wm)):
            if w:
                f[next(take)], f[next(take)], f[next(take)] = 0, fmax, int(rng.integers(0, fmax + 1)) | 1
        if wm:
            a, b = next(take), next(take)
            if name_rank[a] < name_rank[b]:
                a, b = b, a
            zone[b], fc[b] = zone[a], fc[a]
            fm[a], fm[b] = (1 << (wm - 1)) - 1, 1 << (wm - 1)
            together.append([a, b])
        for q in range(Q):
            a, b = next(take), next(take)
            if (name_rank[a] < name_rank[b]) == (q % 2 == 0):
                a, b = b, a  # even q: a carries the larger name rank
            zone[b], fm[b] = zone[a], fm[a]
            fc[a] &= ~np.int64(1)  # ... and the smaller cpu
            fc[b] = fc[a] | 1
            cpu_pairs += 1
            together.append([a, b])
        for g in groups:
            src = 0 if 0 in g else g[0]
            for i in g:
                zone[i], fc[i], fm[i] = zone[src], fc[src], fm[src]
            tie_groups += 1
            together.append(g)
    free_cpu = loc + (fc << tzc)
    free_mem = lom + (fm << tzm)
    alloc, over, res_node, res_req = _inputs(rng, free_cpu, free_mem)
    flags = (np.where(rng.random(n) < 0.05, UNSCHEDULABLE, 0) | np.where(rng.random(n) < 0.95, READY, 0) |
             np.where(rng.random(n) < 0.8, DRIVER_CANDIDATE, 0)).astype(np.uint32)
    label = None
    if label_max is not None:  # one array for both lists: they merge, the build stays on the device
        label = rng.integers(0, label_max + 1, size=n).astype(np.uint32)
        label[rng.random(n) < 0.2] = UNRANKED
        for g in together:
            label[g] = label[g[0]]
        planted = {i for g in together for i in g}
        spots = [int(i) for i in rng.permutation(n) if int(i) not in planted][:3]
        label[spots[0]], label[spots[1]], label[spots[2]] = 0, label_max, UNRANKED
    inputs = dict(alloc=alloc, node_flags=flags, name_rank=name_rank, overhead=over, res_node=res_node, res_req=res_req, zone=zone,
                  n_zones=n_zones, driver_label_rank=label, exec_label_rank=None if label is None else label.copy())
    return inputs, dict(tie_groups=tie_groups, cpu_pairs=cpu_pairs, planted=[list(map(int, g)) for g in together])


def _geometry(n):
    seg = 64
    while SORT_WG * seg < n:
        seg *= 2
    return seg, -(-n // seg)


def _promise(n, groups, tz, planted, **more):
    seg, n_seg = _geometry(n)
    passes = sum(-(-w // 8) for w in groups)
    # the walk in closed form: buffer 0 only at the start, then 1 and 2 in turn so that the last pass writes buffer 1
    dsts = [1 if (passes - k) % 2 else 2 for k in range(passes)]
    return dict(n=n, groups=list(groups), passes=passes, seg=seg, n_seg=n_seg, tz=tuple(tz),
                walk=list(zip([0] + dsts[:-1], dsts)), **planted, **more)


def _groups(wc, wm, n_zones, label_width=0):
    """The expected grouping of the issue's table, written out by hand rather than through plan()'s rule."""
    wz = n_zones.bit_length()
    if wc + wm + wz <= 64:
        g = [wc + wm + wz]
    elif wm + wz <= 64:
        g = [wc, wm + wz]
    else:
        g = [wc, wm, wz]
    return g + ([label_width] if label_width else [])


GEOMETRY_N = (1, 2, 63, 64, 65, 2048, 2049, 4095, 4096, 4097, 8192, 8193, 32769, 65536, 65537)
GEOMETRY_SEG = {1: (64, 1), 2: (64, 1), 63: (64, 1), 64: (64, 1), 65: (64, 2), 2048: (64, 32), 2049: (64, 33), 4095: (64, 64),
                4096: (64, 64), 4097: (128, 33), 8192: (128, 64), 8193: (256, 33), 32769: (1024, 33), 65536: (1024, 64),
                65537: (2048, 33)}
# (wc, wm, n_zones): expected group widths, passes — the issue's table, then the fillers (field sums 17, 25, 33, 41, 49)
WIDTHS = (((22, 40, 3), [64], 8), ((23, 40, 3), [23, 42], 9), ((0, 62, 3), [64], 8), ((0, 62, 4), [0, 62, 3], 9),
          ((1, 62, 4), [1, 62, 3], 10), ((20, 62, 2), [20, 64], 11), ((20, 63, 1), [20, 64], 11), ((20, 63, 2), [20, 63, 2], 12),
          ((0, 0, 1), [1], 1), ((0, 0, 64), [7], 1), ((0, 0, 65), [7], 1), ((7, 0, 1), [8], 1), ((8, 0, 1), [9], 2),
          ((5, 10, 3), [17], 3), ((9, 14, 3), [25], 4), ((11, 20, 3), [33], 5), ((13, 26, 3), [41], 6), ((17, 30, 3), [49], 7))
N_EDGE = 4097  # seg = 128, n_seg = 33: one row past kSortRowBatch, a last segment of one element, 31 wavefronts without any
# labels on top: (wc, wm, n_zones) of three width cases x label_max 254 (width 8, one pass) | 255 (width 9, two passes)
LABELS = (((22, 40, 3), "one-group-even"), ((23, 40, 3), "two-groups-odd"), ((0, 62, 4), "first-skipped"))

_CACHE = None


def cases():
    """[(name, family, inputs, promise)] — inputs in the keyword shape of oracle.pysnapshot.build / Context.build_snapshot,
    promise = what the case reaches: groups (widths, a label group last), passes, seg, n_seg, tz = (cpu, memory), walk, and
    the planted tie_groups / cpu_pairs (planted = their nodes: the memory pair, the cpu pairs, then the tie groups).  Built
    once per process; nobody writes to the arrays."""
    global _CACHE
    if _CACHE is not None:
        return _CACHE
    out = []
    for n in GEOMETRY_N:
        # a 12-bit key: cpu 4 | memory 6 | three zones 2 — two passes.  One node: only the zone field is left.  Two nodes: a
        # column's only difference loses its trailing zeros and nothing can tie next to a varying key, so cpu 10 | zones 2
        # keeps the 12 bits and the memory column is constant.
        wc, wm = {1: (0, 0), 2: (10, 0)}.get(n, (4, 6))
        inputs, planted = _case(1000 + n, n, wc, wm, 3)
        p = _promise(n, [2] if n == 1 else [12], (0, 0), planted, wc=wc, wm=wm)
        assert (p["seg"], p["n_seg"]) == GEOMETRY_SEG[n]
        out.append((f"n{n}", "geometry", inputs, p))
    for k, ((wc, wm, nz), groups, passes) in enumerate(WIDTHS):
        inputs, planted = _case(2000 + k, N_EDGE, wc, wm, nz)
        p = _promise(N_EDGE, groups, (0, 0), planted, wc=wc, wm=wm)
        assert p["groups"] == _groups(wc, wm, nz) and p["passes"] == passes
        out.append((f"c{wc}-m{wm}-z{nz}", "widths", inputs, p))
    # trailing zeros: large tz with a residue on both sides of zero | node 0 the maximum | two values 2^61 apart | tz = 1
    tz_cases = (("residue", dict(wc=12, wm=14, tzc=20, tzm=28, loc=7 - (1 << 61), lom=(1 << 61) + 5)),
                ("node0-max", dict(wc=12, wm=14, tzc=20, tzm=28, loc=7 - (1 << 31), lom=5 - (1 << 41), node0_max=True)),
                ("two-values", dict(wc=9, wm=1, tzc=0, tzm=61, lom=-(1 << 60))),
                ("all-even", dict(wc=10, wm=11, tzc=1, tzm=1, loc=-300, lom=-(1 << 11))))
    for k, (name, kw) in enumerate(tz_cases):
        inputs, planted = _case(3000 + k, N_EDGE, n_zones=3, **kw)
        p = _promise(N_EDGE, _groups(kw["wc"], kw["wm"], 3), (kw["tzc"], kw["tzm"]), planted, wc=kw["wc"], wm=kw["wm"])
        out.append((f"tz-{name}", "trailing-zeros", inputs, p))
    for k, ((wc, wm, nz), name) in enumerate(LABELS):
        for label_max in (254, 255):
            lw = (label_max + 1).bit_length()
            inputs, planted = _case(4000 + 2 * k + (label_max & 1), N_EDGE, wc, wm, nz, label_max=label_max)
            p = _promise(N_EDGE, _groups(wc, wm, nz, lw), (0, 0), planted, wc=wc, wm=wm, label_width=lw)
            out.append((f"label-{name}-max{label_max}", "labels", inputs, p))
    for _, _, inputs, _ in out:
        for v in inputs.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    _CACHE = out
    return out


def case(name):
    return next(c for c in cases() if c[0] == name)


def all_ready(inputs):
    """The same build with every node ready and a driver candidate: both lists are the whole priority order."""
    return dict(inputs, node_flags=np.full(len(inputs["alloc"]), READY | DRIVER_CANDIDATE, dtype=np.uint32))


def free_columns(inputs):
    """(free cpu, free memory) as Python integers, from the inputs alone."""
    alloc = np.asarray(inputs["alloc"], dtype=np.int64)
    n = len(alloc)
    use = [[0, 0] for _ in range(n)]
    for node, req in zip(inputs["res_node"].tolist(), inputs["res_req"].tolist()):
        if node < n:
            use[node][0] += req[0]
            use[node][1] += req[1]
    a, o = alloc.tolist(), inputs["overhead"].tolist()
    return ([a[i][0] - (use[i][0] + o[i][0]) for i in range(n)], [a[i][1] - (use[i][1] + o[i][1]) for i in range(n)])
