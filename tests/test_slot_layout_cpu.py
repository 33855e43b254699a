"""The slot layout (csrc/gangfit_slot_layout.h: plan_layout + fill_layout) against a plain-Python restatement, on the CPU: the header
is pure host code, so a small extern "C" shim (tests/slot_layout_shim.cpp) compiled with g++ is all it takes — no HIP, no
libgangfit.so.  Every table and fact gf_orders_set uploads or keeps is compared exactly."""
import ctypes
import os
import subprocess
from math import gcd

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = 0xFFFFFFFF  # GF_NO_NODE
GF_ERR_INVALID = -3
SENTINEL = -(1 << 62)
NARROW_NEVER = -(1 << 31) // 2
TABLES = ("table", "index", "masks", "cmax", "ntable", "gtab", "gidx", "gmask", "sched", "zmasks", "zspan")
DTYPES = dict(table=np.int64, index=np.uint32, masks=np.uint64, cmax=np.int64, ntable=np.int32, gtab=np.int64, gidx=np.uint32,
              gmask=np.uint64, sched=np.int64, zmasks=np.uint64, zspan=np.uint32)
GUARD = 8  # elements behind every buffer that fill_layout must leave alone


class Facts(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in
                ("n_slots", "n_x", "n_d", "n_chunks", "merged", "identity", "narrow_ok", "n_g", "n_gpad", "n_zones", "zstride",
                 "zd_row0", "zspan_ok", "host_stale", "n_node_slot", "n_g_prefix")] + \
               [("unit", ctypes.c_int64 * 3), ("nmax", ctypes.c_int64 * 3)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("slot_layout") / "slot_layout_shim.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", os.path.join(REPO, "include"),
                           "-I", os.path.join(REPO, "k8s-spark-scheduler_amd", "csrc"),
                           os.path.join(REPO, "tests", "slot_layout_shim.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.sl_plan.restype = ctypes.c_int
    lib.sl_fill.restype = lib.sl_vectors.restype = lib.sl_free.restype = None
    return lib


def run_shim(lib, avail, sched, zone, D, X, force_general=False, sparse_gpu=True):
    """-> (code, message, facts dict, tables dict) through the two steps of the header."""
    avail = np.ascontiguousarray(np.asarray(avail, dtype=np.int64).reshape(-1, 3).T)  # [3][n]
    n = avail.shape[1]
    cols = [avail[j] for j in range(3)]
    if sched is not None:
        sched = np.ascontiguousarray(np.asarray(sched, dtype=np.int64).reshape(-1, 3).T)
        cols += [sched[j] for j in range(3)]
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
    col_ptrs = (ctypes.c_void_p * 6)(*[ptr(c) for c in cols] + [None] * (6 - len(cols)))
    zone = None if zone is None else np.asarray(zone, dtype=np.uint32)
    D, X = np.asarray(D, dtype=np.uint32), np.asarray(X, dtype=np.uint32)
    handle, err, sizes = ctypes.c_void_p(), ctypes.create_string_buffer(256), (ctypes.c_uint64 * 11)()
    code = lib.sl_plan(ctypes.c_uint32(n), col_ptrs, ptr(zone), ptr(D), ctypes.c_uint32(len(D)), ptr(X), ctypes.c_uint32(len(X)),
                       int(force_general), int(sparse_gpu), ctypes.byref(handle), err, ctypes.c_size_t(256), sizes)
    if code != 0:
        assert handle.value is None and not any(sizes)
        return code, err.value.decode(), None, None
    bufs = {}
    for name, size in zip(TABLES, sizes):
        info = np.iinfo(DTYPES[name])
        bufs[name] = np.full(size + GUARD, info.max - 5, dtype=DTYPES[name])
    facts = Facts()
    lib.sl_fill(handle, (ctypes.c_void_p * 11)(*[bufs[k].ctypes.data for k in TABLES]), ctypes.byref(facts))
    node_slot, g_prefix = np.zeros(facts.n_node_slot, np.uint32), np.zeros(facts.n_g_prefix, np.uint32)
    lib.sl_vectors(handle, ptr(node_slot), ptr(g_prefix))
    lib.sl_free(handle)
    tables = {}
    for name, size in zip(TABLES, sizes):
        assert (bufs[name][size:] == np.iinfo(DTYPES[name]).max - 5).all(), f"{name}: written past its size"
        tables[name] = bufs[name][:size]
    f = {k: getattr(facts, k) for k, _ in Facts._fields_[:14]}
    f.update(unit=list(facts.unit), nmax=list(facts.nmax), node_slot=node_slot.tolist(), g_prefix=g_prefix.tolist())
    return 0, "", f, tables


def _words(bits, n_words):
    w = [0] * n_words
    for b in bits:
        w[b >> 6] |= 1 << (b & 63)
    return w


def _chunk_max(col):
    return [max(col[c:c + 64]) for c in range(0, len(col), 64)]


def _span(*rows):
    hit = [c for c in range(len(rows[0])) if any(r[c] for r in rows)]
    return [hit[0], hit[-1] + 1] if hit else [0, 0]


def restate(avail, sched, zone, D, X, force_general=False, sparse_gpu=True):
    """The layout from its rules (DESIGN.md §3 "Slot space"; the reference's binpack.go / single_az.go), written as sets and lists.

    Orders: a name >= n_nodes is unknown and hosts nothing; a repeated driver candidate counts once (its first position); a
    repeated executor candidate is refused.  If the known nodes common to both orders come in the same relative order, the
    MERGED layout: walk the common nodes in order, and before each one (and after the last) come the driver-only nodes that
    precede it in the driver order, then the executor-only nodes that precede it in the executor order; slot s = position s,
    dslot is the identity, n_x = n_d = the length.  Otherwise (or when forced) the GENERAL layout: slot i = raw position i of
    the executor order (unknown names stay empty slots), then the driver-only nodes in driver order; n_x and n_d are the raw
    lengths and dslot maps each raw driver position to its node's slot, unknown names to the sentinel; the driver mask is all
    ones (positions go through dslot) and the zones' driver rows are indexed by raw driver position.
    Values the layout itself defines: one sentinel slot closes the slot space (n_slots = slots + 1); it and every empty slot
    hold -2^62 in all three dimensions ("not in the metadata": below every legal quantity, whose magnitudes stay under 2^62),
    node id GF_NO_NODE, schedulable 0.  Chunks are 64 slots; cmax is the maximum per chunk and dimension.  unit[j] is the gcd of
    the magnitudes of dimension j over the real slots (1 when all are zero); the int32 twin holds value / unit (the sign
    survives), INT32_MIN / 2 on empty and sentinel slots (never fits a request, and two of them still add without wrapping), its
    chunk maxima behind it; it exists (narrow_ok) only when every |value / unit| < 2^30, and nmax is the largest such magnitude.
    Zones: the evaluation list is the zones in order of first appearance in the cleaned driver order, without those that own no
    executor candidate; zstride = max(n_chunks, words of n_d); executor rows first, then driver rows from row n_zones (zd_row0);
    in the merged layout each zone also gets the chunk span [lo, hi) of its candidates ([0, 0) when it has none).
    Sparse gpu view (merged only, option on): the executor candidates with gpu > 0, when there is one and at most a quarter of
    the order: compact SoA table padded to 64 with -2^62, its chunk maxima, node of sub-slot (GF_NO_NODE on the padding),
    sub-slot of slot (GF_NO_NODE elsewhere), slot of sub-slot (the sentinel slot on the padding); g_prefix[c] = sub-slots before
    chunk c of the full order, n_g from the first chunk past the order on (n_slots / 64 + 2 entries); candidate words: row 0
    every sub-slot, row 1 + i the sub-slots of evaluation zone i, whose chunk spans on the compact table fill the zone spans'
    last two words."""
    avail = np.asarray(avail, dtype=np.int64).reshape(-1, 3)
    n = len(avail)
    zone_of = (lambda v: 0) if zone is None else (lambda v: int(zone[v]))
    D, X = [int(v) for v in D], [int(v) for v in X]
    xs = [v for v in X if v < n]
    if len(set(xs)) != len(xs):
        return None
    ds = list(dict.fromkeys(v for v in D if v < n))
    xset, dset = set(xs), set(ds)
    common = [v for v in ds if v in xset]
    merged = not force_general and common == [v for v in xs if v in dset]
    if merged:
        order, d_rest, x_rest = [], list(ds), list(xs)
        for c in common + [None]:
            while d_rest and d_rest[0] != c:
                order.append(d_rest.pop(0))
            while x_rest and x_rest[0] != c:
                order.append(x_rest.pop(0))
            if c is not None:
                order.append(c)
                d_rest.pop(0), x_rest.pop(0)
        slot_node = order + [NO]
        n_x = n_d = len(order)
        x_bits = [s for s, v in enumerate(order) if v in xset]
        d_bits = [s for s, v in enumerate(order) if v in dset]
    else:
        slot_node = [v if v < n else NO for v in X] + [v for v in ds if v not in xset] + [NO]
        n_x, n_d = len(X), len(D)
        x_bits = [i for i, v in enumerate(X) if v < n]
    S = len(slot_node)
    C = (S + 63) // 64
    node_slot = [NO] * n
    for s, v in enumerate(slot_node):
        if v != NO:
            node_slot[v] = s
    dslot = list(range(n_d)) if merged else [node_slot[v] if v < n else S - 1 for v in D]
    real = [s for s in range(S) if slot_node[s] != NO]
    cols = [[int(avail[v][j]) if v != NO else SENTINEL for v in slot_node] for j in range(3)]
    out = dict(n_slots=S, n_x=n_x, n_d=n_d, n_chunks=C, merged=int(merged), identity=int(merged), node_slot=node_slot, host_stale=0)
    out["table"] = cols[0] + cols[1] + cols[2]
    out["index"] = slot_node + dslot + node_slot
    out["masks"] = _words(x_bits, C) + (_words(d_bits, C) if merged else [(1 << 64) - 1] * C)
    out["cmax"] = sum((_chunk_max(c) for c in cols), [])
    unit = [gcd(*[abs(cols[j][s]) for s in real]) or 1 for j in range(3)]
    scaled = [[cols[j][s] // unit[j] if slot_node[s] != NO else NARROW_NEVER for s in range(S)] for j in range(3)]
    assert all(scaled[j][s] * unit[j] == cols[j][s] for j in range(3) for s in real)
    out["unit"] = unit
    out["narrow_ok"] = int(all(abs(scaled[j][s]) < (1 << 30) for j in range(3) for s in real))
    if out["narrow_ok"]:
        out["nmax"] = [max([abs(scaled[j][s]) for s in real], default=0) for j in range(3)]
        out["ntable"] = scaled[0] + scaled[1] + scaled[2] + sum((_chunk_max(c) for c in scaled), [])
    out["sched"] = None if sched is None else [int(np.asarray(sched).reshape(-1, 3)[v][j]) if v != NO else 0
                                               for j in range(3) for v in slot_node]
    # ---- zones
    ev = [z for z in dict.fromkeys(zone_of(v) for v in ds) if any(zone_of(v) == z for v in xs)]
    Z = (n_d + 63) // 64
    stride = max(C, Z)
    out.update(n_zones=len(ev), zd_row0=len(ev), zstride=stride, eval=ev)
    if merged:
        zx = [_words([s for s in x_bits if zone_of(order[s]) == z], stride) for z in ev]
        zd = [_words([s for s in d_bits if zone_of(order[s]) == z], stride) for z in ev]
    else:
        zx = [_words([i for i in x_bits if zone_of(X[i]) == z], stride) for z in ev]
        zd = [_words([i for i, v in enumerate(D) if v < n and zone_of(v) == z], stride) for z in ev]
    out["zmasks"] = sum(zx + zd, [])
    # ---- sparse gpu view and the spans
    g_slots = [s for s in x_bits if cols[2][s] > 0] if merged and sparse_gpu else []
    if not g_slots or 4 * len(g_slots) > n_x:
        g_slots = []
    G = len(g_slots)
    P = (G + 63) // 64 * 64
    out.update(n_g=G, n_gpad=P, g_prefix=[], gtab=[], gidx=[], gmask=[])
    gz = []
    if G:
        pad = lambda vals, fill: vals + [fill] * (P - G)
        gcols = [pad([cols[j][s] for s in g_slots], SENTINEL) for j in range(3)]
        out["gtab"] = gcols[0] + gcols[1] + gcols[2] + sum((_chunk_max(c) for c in gcols), [])
        sub_of_slot = [NO] * S
        for k, s in enumerate(g_slots):
            sub_of_slot[s] = k
        out["gidx"] = pad([slot_node[s] for s in g_slots], NO) + sub_of_slot + pad(g_slots, S - 1)
        out["g_prefix"] = [sum(1 for s in g_slots if s < 64 * c) for c in range(S // 64 + 2)]
        gz = [_words([k for k, s in enumerate(g_slots) if zone_of(slot_node[s]) == z], P // 64) for z in ev]
        out["gmask"] = sum([_words(range(G), P // 64)] + gz, [])
    out["zspan_ok"] = int(merged and len(ev) > 0)
    out["zspan"] = []
    if out["zspan_ok"]:
        for i in range(len(ev)):
            out["zspan"] += _span(zx[i][:C], zd[i][:C]) + (_span(gz[i]) if G else [0, 0])
        out["zspan"] += [0, 0, 0, 0]
    return out


def check(lib, avail, sched, zone, D, X, **opts):
    want = restate(avail, sched, zone, D, X, **opts)
    code, msg, facts, tables = run_shim(lib, avail, sched, zone, D, X, **opts)
    assert code == 0 and want is not None, msg
    for k in ("n_slots", "n_x", "n_d", "n_chunks", "merged", "identity", "narrow_ok", "n_g", "n_gpad", "n_zones", "zstride",
              "zd_row0", "zspan_ok", "host_stale", "unit", "node_slot", "g_prefix"):
        assert facts[k] == want[k], k
    for name in TABLES:
        got = [int(v) for v in tables[name]]
        if name == "ntable":
            assert len(got) == 3 * want["n_slots"] + 3 * want["n_chunks"]
            if not want["narrow_ok"]:
                continue  # no narrow form: the region is scratch and is not uploaded
        if name == "sched" and want["sched"] is None:
            assert got == []
            continue
        exp = [v & 0xFFFFFFFFFFFFFFFF for v in want[name]] if DTYPES[name] == np.uint64 else want[name]
        assert got == exp, name
    if want["narrow_ok"]:
        assert facts["nmax"] == want["nmax"]
    return want, facts, tables


def _identity_case(n, seed):
    rng = np.random.default_rng(seed)
    avail = rng.integers(-3, 4000, size=(n, 3))
    avail[:, 2] = rng.integers(0, 3, size=n)
    return avail, (avail + 5 if n else None), list(range(n)), list(range(n))


@pytest.mark.parametrize("n, n_chunks", [(0, 1), (63, 1), (64, 2)])
def test_sentinel_and_chunk_edges(shim, n, n_chunks):
    """0 nodes; 63 nodes: the sentinel closes the only chunk; 64 nodes: the sentinel is alone in chunk 1."""
    avail, sched, D, X = _identity_case(n, 7)
    want, facts, tables = check(shim, avail, sched, None, D, X)
    assert facts["n_slots"] == n + 1 and facts["n_chunks"] == n_chunks and facts["merged"] and facts["identity"]
    assert int(tables["index"][n]) == NO and [int(tables["table"][j * (n + 1) + n]) for j in range(3)] == [SENTINEL] * 3
    assert int(tables["cmax"][n_chunks - 1]) == (SENTINEL if n in (0, 64) else max(avail[:, 0]))
    assert facts["n_zones"] == (1 if n else 0)


def _case130(n_gpu=6):
    """130 nodes, three zones: base order = a fixed permutation; roles by position; zone 1 owns driver-only nodes only, zone 2
    lives in the first 50 positions and is the first zone of the driver order."""
    rng = np.random.default_rng(130)
    n = 130
    base = rng.permutation(n)
    role = np.array([("both", "both", "driver", "exec", "both", "none", "both")[i % 7] for i in range(n)])
    zone_at = np.zeros(n, dtype=np.uint32)
    zone_at[[i for i in range(50) if i % 7 in (0, 3)]] = 2
    zone_at[[i for i in range(n) if role[i] == "driver" and i % 2 == 0]] = 1
    zone = np.zeros(n, dtype=np.uint32)
    zone[base] = zone_at
    avail = rng.integers(-3, 4000, size=(n, 3))
    avail[:, 2] = 0
    x_pos = [i for i in range(n) if role[i] in ("both", "exec")]
    for i in x_pos[3::max(1, len(x_pos) // n_gpu)][:n_gpu]:
        avail[base[i], 2] = 1 + i % 4
    d_only = [i for i in range(n) if role[i] == "driver"]
    avail[base[d_only[0]], 2] = 8   # a free gpu on a node that is no executor candidate: not in the view
    avail[base[x_pos[0]], 2] = -1   # and a negative one on a candidate
    sched = np.abs(avail) + 11
    D = [int(base[i]) for i in range(n) if role[i] in ("both", "driver")]
    X = [int(base[i]) for i in range(n) if role[i] in ("both", "exec")]
    D = D[:9] + [n + 5] + D[9:40] + [D[1]] + D[40:] + [n + 1000]  # unknown names and a repeated candidate
    X = X[:20] + [n + 1] + X[20:]
    return avail, sched, zone, D, X


def test_merged_130_nodes_three_zones_sparse_view(shim):
    avail, sched, zone, D, X = _case130()
    want, facts, tables = check(shim, avail, sched, zone, D, X)
    assert facts["merged"] and facts["identity"] and facts["n_chunks"] == 2
    assert facts["n_g"] == 6 and facts["n_gpad"] == 64 and 4 * facts["n_g"] <= facts["n_x"]
    assert len(tables["gmask"]) == 1 + facts["n_zones"] and int(tables["gmask"][0]) == 0b111111
    assert facts["g_prefix"][0] == 0 and facts["g_prefix"][-1] == 6 and len(facts["g_prefix"]) == facts["n_slots"] // 64 + 2
    # zone 1 is in the driver order but owns no executor candidate; the list goes by first appearance in the driver order
    assert zone[D[0]] == 2 and 1 in [int(zone[v]) for v in D if v < 130]
    assert want["eval"] == [2, 0] and facts["n_zones"] == 2 and facts["zspan_ok"]
    assert [int(v) for v in tables["zspan"][:2]] == [0, 1] and [int(v) for v in tables["zspan"][4:6]] == [0, 2]


def test_merged_130_more_than_a_quarter_with_gpu_has_no_view(shim):
    avail, sched, zone, D, X = _case130(n_gpu=40)
    want, facts, tables = check(shim, avail, sched, zone, D, X)
    assert facts["merged"] and facts["n_g"] == 0 and facts["g_prefix"] == [] and len(tables["gtab"]) == 0
    assert sum(1 for v in set(X) if v < 130 and avail[v, 2] > 0) * 4 > facts["n_x"]


def test_merged_130_sparse_gpu_off(shim):
    avail, sched, zone, D, X = _case130()
    want, facts, tables = check(shim, avail, sched, zone, D, X, sparse_gpu=False)
    assert facts["merged"] and facts["n_g"] == 0 and len(tables["gmask"]) == 0 and facts["zspan_ok"]
    assert [int(v) for v in tables["zspan"][2:4]] == [0, 0]


def test_general_layout_when_two_nodes_disagree(shim):
    avail, sched, zone, D, X = _case130()
    common = [v for v in X if v in D]
    i, j = X.index(common[4]), X.index(common[9])
    X[i], X[j] = X[j], X[i]  # two nodes in opposite relative order in the two orders
    want, facts, tables = check(shim, avail, sched, zone, D, X)
    S = facts["n_slots"]
    assert not facts["merged"] and not facts["identity"] and facts["n_x"] == len(X) and facts["n_d"] == len(D)
    assert int(tables["index"][X.index(131)]) == NO  # the executor order's unknown name stays an empty slot
    dslot = [int(v) for v in tables["index"][S:S + len(D)]]
    assert [dslot[k] for k, v in enumerate(D) if v >= 130] == [S - 1, S - 1]  # unknown drivers: the sentinel
    assert all(int(v) == (1 << 64) - 1 for v in tables["masks"][facts["n_chunks"]:])  # dmask
    assert facts["n_g"] == 0 and not facts["zspan_ok"] and len(tables["zspan"]) == 0
    zd = tables["zmasks"][facts["n_zones"] * facts["zstride"]:]
    k = D.index(D[41], 10)  # the repeated candidate's second POSITION carries its zone's driver bit too
    row = want["eval"].index(int(zone[D[k]]))
    assert (int(zd[row * facts["zstride"] + (k >> 6)]) >> (k & 63)) & 1


def test_force_general_layout_on_mergeable_orders(shim):
    avail, sched, zone, D, X = _case130()
    want, facts, tables = check(shim, avail, sched, zone, D, X, force_general=True)
    assert not facts["merged"] and not facts["identity"] and facts["n_g"] == 0 and facts["n_x"] == len(X)


def test_units_and_the_narrow_twin(shim):
    # 2^30 units in one dimension: no narrow form, everything else as usual
    avail = [[1, 6, 0], [1 << 30, 9, 0], [5, 12, 0]]
    want, facts, _ = check(shim, avail, None, None, [0, 1, 2], [0, 1, 2])
    assert not facts["narrow_ok"] and facts["unit"] == [1, 3, 1]  # the gpu dimension is all zero: unit 1
    # one below: narrow; negative values: the gcd works on magnitudes and the signs survive in the twin
    avail = [[-6, (1 << 30) - 1, 0], [9, 1, 0], [-12, 2, 0]]
    want, facts, tables = check(shim, avail, None, None, [0, 1, 2], [0, 1, 2])
    assert facts["narrow_ok"] and facts["unit"] == [3, 1, 1] and facts["nmax"] == [4, (1 << 30) - 1, 0]
    assert [int(v) for v in tables["ntable"][:4]] == [-2, 3, -4, NARROW_NEVER]


def test_executor_named_twice_is_refused(shim):
    avail, sched, zone, D, X = _case130()
    assert restate(avail, sched, zone, D, X + [X[3]]) is None
    code, msg, facts, tables = run_shim(shim, avail, sched, zone, D, X + [X[3]])
    assert code == GF_ERR_INVALID and f"node {X[3]} appears twice" in msg and facts is None and tables is None
