"""The edge cases of the priority sort (tests/sort_edges.py) without a GPU: every case reaches the arm it promises, the buffer
walk is sound for every feasible list of key groups, a lane-level numpy model of the pass loop — segments, digit-major offsets
over (digit, segment), in-chunk peer ranks, next-digit counting into the destination segment's row, three rotating count tables
and buffers — gives np.lexsort's order, and three plausible mistakes give another order than oracle.pysnapshot.build on every case
they apply to (so the device comparison in tests/test_gpu_sort_edges.py can tell them apart).  The lane model follows the
precedent of tests/test_lane_algorithms.py: it restates the algorithm, it is not the kernel."""
import itertools

import numpy as np
import pytest

import sort_edges as se
from oracle import pysnapshot as ps

CASES = se.cases()
IDS = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
U64 = np.uint64


def _free(inputs):
    cpu, mem = se.free_columns(inputs)
    return np.array(cpu, dtype=np.int64), np.array(mem, dtype=np.int64)


def _fields(inputs):
    """What the kernel sorts by: (cpu field, memory field, zone rank by node, label key or None, plan)."""
    cpu, mem = _free(inputs)
    nz = inputs["n_zones"]
    label = inputs["driver_label_rank"]
    p = se.plan(cpu.tolist(), mem.tolist(), nz, se.label_width_of(label))
    bc, bm = cpu.view(U64) ^ U64(1 << 63), mem.view(U64) ^ U64(1 << 63)
    kc, km = (bc - bc.min()) >> U64(p["tzc"]), (bm - bm.min()) >> U64(p["tzm"])
    z = inputs["zone"].astype(np.int64)
    zm, zc = np.zeros(nz, dtype=np.int64), np.zeros(nz, dtype=np.int64)
    np.add.at(zm, z, mem)  # wrapping 64-bit sums, like the device's atomic adds
    np.add.at(zc, z, cpu)
    # the kernel's rule: rank = the zones that sort before mine (memory, cpu, zone id)
    zr = np.array([sum(1 for y in range(nz) if (zm[y], zc[y], y) < (zm[x], zc[x], x)) for x in range(nz)], dtype=np.int64)
    lab = None
    if p["groups"][p["n_groups"]:]:
        lmax = int(label[label != se.UNRANKED].max())
        lab = np.where(label > lmax, lmax + 1, label).astype(np.int64)
    return kc, km, zr[z], lab, p


def _order_of(name, kc, km, zrank, lab):
    order = np.lexsort((name, kc, km, zrank))
    return order if lab is None else order[np.argsort(lab[order], kind="stable")]


def _oracle_order(inputs):
    _, _, D, X = ps.build(**se.all_ready(inputs))
    assert np.array_equal(D, X)
    return D.astype(np.int64)


# ------------------------------------------------------------------------------------------------ every case keeps its promise
@pytest.mark.parametrize("name", IDS)
def test_case_reaches_its_edge(name):
    _, family, inputs, promise = BY_NAME[name]
    assert "gpu" not in name
    cpu, mem = se.free_columns(inputs)
    n = len(cpu)
    p = se.plan(cpu, mem, inputs["n_zones"], se.label_width_of(inputs["driver_label_rank"]))
    assert p["groups"] == promise["groups"] and p["total_passes"] == promise["passes"]
    assert (p["seg"], p["n_seg"]) == (promise["seg"], promise["n_seg"]) and n == promise["n"]
    assert (p["tzc"], p["tzm"]) == promise["tz"]
    assert (p["wc"], p["wm"]) == (promise["wc"], promise["wm"])
    assert se.buffer_walk(p["groups"]) == promise["walk"] and promise["walk"][-1][1] == 1
    if inputs["driver_label_rank"] is not None:
        assert np.array_equal(inputs["driver_label_rank"], inputs["exec_label_rank"])  # one array: the lists merge
        assert promise["label_width"] == p["groups"][-1] and (inputs["driver_label_rank"] == se.UNRANKED).any()
    if n < 63:
        return
    # the fields hold 0, their largest value and an odd value; node 0 is neither extreme
    for col, tz, w in ((cpu, p["tzc"], p["wc"]), (mem, p["tzm"], p["wm"])):
        low = min(col)
        f = [(v - low) >> tz for v in col]
        if w == 0:
            assert max(f) == 0
            continue
        assert min(f) == 0 and any(v & 1 for v in f)
        assert max(f) == ((1 << w) - 1 if w < 63 else se.MAX_FREE - se.MIN_FREE)
        if name == "tz-node0-max":
            assert f[0] == max(f)
        elif w > 1:
            assert 0 < f[0] < max(f)
    if p["wm"] >= 62 or (family == "trailing-zeros" and name != "tz-residue"):
        assert min(mem) < 0 < max(mem)  # values on both sides of zero
    if name == "tz-residue":
        assert all(v % (1 << 20) == 7 for v in cpu) and all(v % (1 << 28) == 5 for v in mem) and max(cpu) < 0 < min(mem)
    if name == "tz-two-values":
        assert sorted(set(mem)) == [-(1 << 60), 1 << 60]
    if name == "tz-all-even":
        assert not any(v & 1 for v in cpu + mem)
    if p["wm"] == 63:
        assert min(mem) == se.MIN_FREE and max(mem) == se.MAX_FREE
    # the planted ties: equal (zone, memory, cpu) with name ranks far apart and in different segments of the name order
    rank, zone = inputs["name_rank"].tolist(), inputs["zone"].tolist()
    assert promise["tie_groups"] == min(32, n // 4) and promise["cpu_pairs"] == (min(32, n // 8) if p["wc"] else 0)
    ties = promise["planted"][len(promise["planted"]) - promise["tie_groups"]:]
    pairs = promise["planted"][(1 if p["wm"] else 0):][:promise["cpu_pairs"]]
    assert len({i for g in promise["planted"] for i in g}) == sum(len(g) for g in promise["planted"])  # nobody planted twice
    crossing = 0
    for g in ties:
        assert len(g) >= 2 and len({(zone[i], mem[i], cpu[i]) for i in g}) == 1
        r = [rank[i] for i in g]
        assert max(r) - min(r) >= n // 2 - 1
        crossing += min(r) // p["seg"] != max(r) // p["seg"]
    assert crossing == (0 if p["n_seg"] == 1 else (len(ties) if n >= 256 else 1))
    for a, b in pairs:
        assert (zone[a], mem[a]) == (zone[b], mem[b]) and cpu[a] < cpu[b]
    assert any(rank[a] > rank[b] for a, b in pairs) == bool(pairs) and any(rank[a] < rank[b] for a, b in pairs) == bool(pairs)
    if p["wm"]:
        a, b = promise["planted"][0]
        assert (zone[a], cpu[a]) == (zone[b], cpu[b]) and mem[a] < mem[b] and rank[a] > rank[b]


def test_families_cover_what_the_issue_lists():
    fam = {}
    for name, family, _, promise in CASES:
        fam.setdefault(family, []).append(promise)
    assert {f: len(v) for f, v in fam.items()} == {"geometry": 15, "widths": 18, "trailing-zeros": 4, "labels": 6}
    assert {p["passes"] for p in fam["widths"]} == set(range(1, 13))  # every total from 1 to 12
    assert [p["n"] for p in fam["geometry"]] == list(se.GEOMETRY_N)
    assert any(p["groups"][0] == 0 and len(p["groups"]) == 3 for p in fam["widths"])        # a group of width 0 in front
    assert any(p["groups"] == [64] for p in fam["widths"]) and any(p["groups"] == [20, 64] for p in fam["widths"])
    assert {(len(p["groups"]) - 1, p["passes"] % 2, p["label_width"]) for p in fam["labels"]} == \
        {(1, 1, 8), (1, 0, 9), (2, 0, 8), (2, 1, 9), (3, 0, 8), (3, 1, 9)}
    assert any(p["groups"][0] == 0 for p in fam["labels"])  # three groups, the first skipped, a label on top


# ---------------------------------------------------------------------------------------------------------- the buffer walk
def test_buffer_walk_for_every_feasible_group_list():
    """Every (wc, wm, wz, label width) the ABI can produce, up to the pass counts: 1 .. 22 passes in all."""
    steps = sorted({0, 63} | {8 * k + d for k in range(8) for d in (-1, 0, 1) if 0 <= 8 * k + d <= 63})
    totals = set()
    for wc, wm, wz, lw in itertools.product(steps, steps, range(1, 14), (0, 1, 8, 9, 16, 17, 24, 25, 32)):
        n_groups = 1 if wc + wm + wz <= 64 else (2 if wm + wz <= 64 else 3)
        groups = [[wc + wm + wz], [wc, wm + wz], [wc, wm, wz]][n_groups - 1] + ([lw] if lw else [])
        walk = se.buffer_walk(groups)
        total = sum((w + 7) // 8 for w in groups)
        totals.add(total)
        assert len(walk) == total
        assert all(s != d for s, d in walk), groups
        assert walk[0][0] == 0 and walk[-1][1] == 1, groups
        assert all(walk[k][0] == walk[k - 1][1] for k in range(1, total)), groups
        for g, src, done in se.key_build_sources(groups):
            # a key build reads the order where the pass before it left it — the name order in buffer 0 when there was none
            assert src == (walk[done - 1][1] if done else 0), groups
            if lw and g == len(groups) - 1:
                assert done > 0 and src == walk[done - 1][1], groups  # wz >= 1: something always ran before a label group
    assert totals == set(range(1, 23))


# ------------------------------------------------------------------------------------------------------------ the lane model
def _lane_model(inputs):
    """The pass loop of priority_sort_kernel at lane level.  Returns the content of buffer 1 after the last pass."""
    kc, km, zrank, lab, p = _fields(inputs)
    n, seg, n_seg = len(kc), p["seg"], p["n_seg"]
    seg_log = seg.bit_length() - 1
    wc, wm = p["wc"], p["wm"]
    total = p["total_passes"]
    keys = [None, None, None]
    perm = [np.argsort(inputs["name_rank"]).astype(np.int64), np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)]
    hist = np.zeros((3, se.SORT_WG, 256), dtype=np.int64)  # zero at launch
    lower = np.tril(np.ones((64, 64), dtype=bool), -1)
    src = P = 0
    for g, width in enumerate(p["groups"]):
        if width == 0:
            continue
        is_l = g == p["n_groups"]
        has_c, has_m, has_z = not is_l and g == 0, not is_l and (p["n_groups"] == 1 or g == 1), not is_l and g + 1 == p["n_groups"]
        node = perm[src]
        assert (node >= 0).all()  # the key build reads a buffer that holds an order
        key, sft = np.zeros(n, dtype=U64), 0
        if has_c:
            key, sft = kc[node].copy(), wc
        if has_m:
            if sft < 64:
                key |= km[node] << U64(sft)
            sft += wm
        if has_z and sft < 64:
            key |= zrank[node].astype(U64) << U64(sft)
        if is_l:
            key = lab[node].astype(U64)
        keys[src] = key
        for wave in range(se.SORT_WG):  # every wavefront STORES its row of first-digit counts (the empty ones zeros)
            lo, hi = min(wave << seg_log, n), min((wave + 1) << seg_log, n)
            hist[P % 3, wave] = np.bincount((key[lo:hi] & U64(255)).astype(np.int64), minlength=256)
        for shift in range(0, width, 8):
            nxt, feeds = shift + 8, shift + 8 < width
            remaining = total - P
            dst = 1 if remaining & 1 else (0 if src == 2 else 2)
            kin, pin = keys[src], perm[src]
            kout, pout = np.zeros(n, dtype=U64), np.full(n, -1, dtype=np.int64)
            cur, nx = hist[P % 3], hist[(P + 1) % 3]
            hist[(P + 2) % 3] = 0
            flat = cur[:n_seg].T.reshape(-1)  # digit-major over (digit, segment)
            excl = (np.cumsum(flat) - flat).reshape(256, n_seg)
            for wave in range(n_seg):
                off = excl[:, wave].copy()
                lo, hi = wave << seg_log, min((wave + 1) << seg_log, n)
                for base in range(lo, hi, 64):
                    k, v = kin[base:min(base + 64, hi)], pin[base:min(base + 64, hi)]
                    d = ((k >> U64(shift)) & U64(255)).astype(np.int64)
                    m = len(d)
                    rank = ((d[:, None] == d[None, :]) & lower[:m, :m]).sum(axis=1)  # peers on lower lanes
                    pos = off[d] + rank
                    np.add.at(off, d, 1)
                    kout[pos], pout[pos] = k, v
                    if feeds:
                        np.add.at(nx, (pos >> seg_log, ((k >> U64(nxt)) & U64(255)).astype(np.int64)), 1)
            keys[dst], perm[dst] = kout, pout
            src, P = dst, P + 1
    assert P == total and src == 1
    return perm[1], (kc, km, zrank, lab)


@pytest.mark.parametrize("name", [c[0] for c in CASES if c[3]["n"] <= 8193])
def test_lane_model_gives_the_lexsort_order(name):
    inputs = BY_NAME[name][2]
    got, (kc, km, zrank, lab) = _lane_model(inputs)
    cpu, mem = _free(inputs)
    nz = inputs["n_zones"]
    z = inputs["zone"].astype(np.int64)
    zm, zc = np.zeros(nz, dtype=np.int64), np.zeros(nz, dtype=np.int64)
    np.add.at(zm, z, mem)
    np.add.at(zc, z, cpu)
    zorder = np.lexsort((np.arange(nz), zc, zm))
    zr = np.empty(nz, dtype=np.int64)
    zr[zorder] = np.arange(nz)
    want = np.lexsort((inputs["name_rank"].astype(np.int64), cpu, mem, zr[z]))
    if lab is not None:
        want = want[np.argsort(lab[want], kind="stable")]
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------- the wrong models
@pytest.mark.parametrize("name", IDS)
def test_wrong_models_differ_from_the_restatement(name):
    """A case on which an applicable wrong model agrees with oracle.pysnapshot.build could not catch that mistake on the device:
    a generator bug.  (n = 1 has one order; n = 2 holds no tie next to its varying key: see tests/sort_edges.py.)"""
    _, _, inputs, promise = BY_NAME[name]
    kc, km, zrank, lab, p = _fields(inputs)
    nm = inputs["name_rank"].astype(np.int64)
    want = _oracle_order(inputs)
    assert np.array_equal(_order_of(nm, kc, km, zrank, lab), want)  # the fields, shifts and zone ranks themselves are right
    applied = 0
    if p["wm"] > 0:  # a memory field one bit too narrow
        applied += 1
        assert not np.array_equal(_order_of(nm, kc, km & U64((1 << (p["wm"] - 1)) - 1), zrank, lab), want)
    if promise["tie_groups"] > 0:  # ties broken by descending name rank
        applied += 1
        assert not np.array_equal(_order_of(-nm, kc, km, zrank, lab), want)
    if p["wc"] > 0:  # group 0 (the cpu field) dropped
        applied += 1
        assert not np.array_equal(_order_of(nm, np.zeros_like(kc), km, zrank, lab), want)
    assert applied == (p["wm"] > 0) + (promise["n"] >= 63) + (p["wc"] > 0)


# ------------------------------------------------------------------------------------------------------ the ABI's range checks
@pytest.mark.parametrize("name", IDS)
def test_inputs_pass_the_range_checks_of_the_abi(name):
    inputs = BY_NAME[name][2]
    alloc, over, rn, rr = inputs["alloc"], inputs["overhead"], inputs["res_node"], inputs["res_req"]
    n = len(alloc)
    assert alloc.dtype == np.int64 and (alloc >= 0).all() and (alloc < 1 << 62).all()
    assert (over >= 0).all() and (over < 1 << 61).all()
    assert (rr >= 0).all() and (rr < 1 << 61).all() and (rn >= n).sum() == 1
    listed = rn < n
    for j in range(3):
        entries = [int(v) for v in rr[listed, j]]
        # gf_usage_apply: everything applied plus the largest overhead stays below 2^62 (implies the per-node bound)
        assert sum(entries) + int(over[:, j].max()) < 1 << 62
        # gf_snapshot_build: the most entries one node carries, times the largest entry, plus the largest overhead
        most = int(np.bincount(rn[listed].astype(np.int64), minlength=n).max()) if listed.any() else 0
        assert most * int(rr[:, j].max()) + int(over[:, j].max()) < 1 << 62
    assert 1 <= inputs["n_zones"] <= 4096 and (inputs["zone"] < inputs["n_zones"]).all()
    assert np.array_equal(np.sort(inputs["name_rank"]), np.arange(n))
    cpu, mem = se.free_columns(inputs)
    avail = ps.build(**inputs)[0]
    assert avail[:, 0].tolist() == cpu and avail[:, 1].tolist() == mem
    if n >= 63:  # negative values come from overhead on some nodes and from reservation entries on others
        neg = np.nonzero((avail[:, :2] < 0).any(axis=1))[0]
        if len(neg):
            has_res = np.isin(neg, rn)
            assert has_res.any() and (~has_res).any()
