"""The label merge check of gf_snapshot_build (gangfit_snapshot.hip: label_merge_check_kernel, label_merge_carry_kernel and their
d_summary rows) on inputs with ONE inversion, placed where only one mechanism of the check can see it: the lane before in a
chunk, the carry from the chunk before inside a wavefront's run, the summary rows of two neighbouring runs, the carry kernel's
second step of 64 runs — and the same with a stretch of nodes that are candidates of neither role in between, so that the
comparison has to reach back over a chunk (or a whole run) that contributes nothing.

P is the unlabelled priority order (every node a candidate), t a position in it, G the length of the gap (0, one chunk, or a
run of two chunks) and g0 = t - G.  One rank array over the nodes — 0 on P[0 .. g0-2] and P[t], 1 on the gap P[g0 .. t-1], the
largest value elsewhere — makes the label group's order C = P[0 .. g0-2], P[t], gap, P[g0-1], P[t+1 ..]: P[t] and P[g0-1]
change places, at C positions g0-1 and t.  The list the label sorts follows C by construction; the OTHER list keeps P's order,
so it is a subsequence of C unless both swapped nodes are its candidates.  Then the build must fall back to the host route —
build_info (2, 1, 1) — and with the twin that takes P[g0-1] out of that list it must stay on the device — (1, 1, 0).  Either
way snapshot, lists and decisions equal oracle/pysnapshot.build and the oracle.
`python -m pytest tests/test_gpu_label_merge_edges.py -m gpu`."""
import numpy as np
import pytest

from oracle import pysnapshot as ps
from test_gpu_snapshot_labels import _check_decisions, _check_snapshot, _cluster, _same_relative_order

FULL = ps.READY | ps.DRIVER_CANDIDATE
DECISIONS_UP_TO = 4097
# (n, t, G).  Chunks of 64 positions; the check runs min(chunks, 1024) wavefronts over ceil(chunks / wavefronts) chunks each.
PLACEMENTS = [
    # 130 nodes: 3 chunks, one per wavefront
    (130, 1, 0), (130, 64, 0), (130, 128, 0), (130, 129, 0),
    (130, 128, 64),                       # C positions 63 | 128: run 0 against run 2 over a run without candidates
    # 4 097 nodes: 65 chunks, one per wavefront; run 63 | 64 is the carry kernel's second step
    (4097, 64, 0), (4097, 4032, 0), (4097, 4096, 0),
    (4097, 4032, 64), (4097, 4096, 64),   # the second step's first run against the carry of the first step, over an empty run 63
    # 65 601 nodes: 1 026 chunks, two per wavefront
    (65601, 64, 0),                       # the chunk carry inside run 0
    (65601, 128, 0),                      # run 0 | 1
    (65601, 8192, 0),                     # run 63 | 64
    (65601, 65600, 0),                    # the last chunk holds one position
    (65601, 128, 64),                     # C positions 63 | 128: an empty second chunk of run 0, then the run boundary
    (65601, 8192, 128),                   # all of run 63 empty: 8 063 | 8 192
    (65601, 65600, 64),                   # run 511's last position against run 512's second chunk, its first chunk empty
]
# (a gap needs a candidate before it — t = 1 and t = 64 have none — and t on a chunk edge, else more than one pair inverts)


def _pid(p):
    return f"n{p[0]}-t{p[1]}-gap{p[2]}"


_BASE = {}


def _base(n):
    """(build inputs with every node a candidate and no labels, P)"""
    if n not in _BASE:
        c = _cluster(5000 + n, n, min(n, 300), 3)
        c["node_flags"] = np.full(n, FULL, dtype=np.uint32)
        _BASE[n] = (c, ps.build(**c)[2])
    return _BASE[n]


def _case(n, t, gap, role, twin):
    """role "exec": an executor label only, the driver list is the one that can break; "driver": the mirror."""
    base, P = _base(n)
    g0 = t - gap
    assert 1 <= g0 <= t < n and len(P) == n
    r = np.full(n, 2 if gap else 1, dtype=np.uint32)
    r[P[:g0 - 1]] = 0
    r[P[t]] = 0
    r[P[g0:t]] = 1
    flags = base["node_flags"].copy()
    flags[P[g0:t]] = 0
    other = ps.DRIVER_CANDIDATE if role == "exec" else ps.READY  # the role of the list the label does NOT sort
    if twin:
        flags[P[g0 - 1]] &= ~np.uint32(other)
    c = dict(base, node_flags=flags, exec_label_rank=r if role == "exec" else None,
             driver_label_rank=r if role == "driver" else None)
    return c, P, r, g0, other


def _descents(c, P, r, other):
    """C positions i where the next candidate of the unsorted list along C has a smaller position in P."""
    n = len(P)
    C = P[np.argsort(r[P], kind="stable")]
    ppos = np.empty(n, dtype=np.int64)
    ppos[P] = np.arange(n)
    fl = c["node_flags"][C]
    if other == ps.DRIVER_CANDIDATE:
        cand = (fl & ps.DRIVER_CANDIDATE) != 0
    else:
        cand = ((fl & ps.READY) != 0) & ((fl & ps.UNSCHEDULABLE) == 0)
    at = np.nonzero(cand)[0]
    down = np.nonzero(np.diff(ppos[C[at]]) < 0)[0]
    return [(int(at[i]), int(at[i + 1])) for i in down]


@pytest.mark.parametrize("role", ["exec", "driver"])
@pytest.mark.parametrize("place", PLACEMENTS, ids=_pid)
def test_one_inversion_is_what_the_inputs_hold(place, role):
    """No GPU: exactly one inverted pair, at C positions g0-1 | t, and none in the twin; the restated lists conflict exactly
    when it is there."""
    n, t, gap = place
    for twin in (False, True):
        c, P, r, g0, other = _case(n, t, gap, role, twin)
        assert _descents(c, P, r, other) == ([] if twin else [(g0 - 1, t)])
        _, _, D, X = ps.build(**c)
        assert _same_relative_order(D, X) == twin


@pytest.mark.gpu
@pytest.mark.parametrize("twin", [False, True], ids=["inversion", "twin"])
@pytest.mark.parametrize("role", ["exec", "driver"])
@pytest.mark.parametrize("place", PLACEMENTS, ids=_pid)
def test_one_placed_inversion(gf_ctx, place, role, twin):
    n, t, gap = place
    c, P, r, g0, other = _case(n, t, gap, role, twin)
    D, X = gf_ctx.build_snapshot(**c)
    info = gf_ctx.build_info()
    print("build_info", _pid(place), role, "twin" if twin else "inversion", info)
    assert info[:3] == ((1, 1, 0) if twin else (2, 1, 1)), info
    avail, sched, rD, rX = _check_snapshot(gf_ctx, c, D, X)
    if n <= DECISIONS_UP_TO:
        _check_decisions(gf_ctx, c, avail, sched, rD, rX)


def _two_labels(n, t, twin):
    """Both labels active: the executor ranks are 2 x driver rank + 3 — the same order — except on w = P[t], whose driver rank
    is the lowest and whose executor rank is the highest.  The label group sorts by the driver label, so w sits in C's first
    group while the executor list wants it in its last one; the twin takes w out of the executor list."""
    base, P = _base(n)
    rng = np.random.default_rng(n + t)
    dl = rng.choice([0, 1, 2], size=n).astype(np.uint32)
    w = P[t]
    dl[w] = 0
    el = (dl * 2 + 3).astype(np.uint32)
    el[w] = 7
    flags = base["node_flags"].copy()
    if twin:
        flags[w] &= ~np.uint32(ps.READY)
    return dict(base, node_flags=flags, driver_label_rank=dl, exec_label_rank=el)


@pytest.mark.parametrize("n,t", [(130, 64), (4097, 4096)])
def test_two_labels_conflict_on_one_node_only(n, t):
    """No GPU: the restated lists conflict with w in the executor list and merge without it."""
    for twin in (False, True):
        _, _, D, X = ps.build(**_two_labels(n, t, twin))
        assert _same_relative_order(D, X) == twin


@pytest.mark.gpu
@pytest.mark.parametrize("twin", [False, True], ids=["conflict", "twin"])
@pytest.mark.parametrize("n,t", [(130, 64), (4097, 4096)])
def test_two_labels_monotone_but_for_one_node(gf_ctx, n, t, twin):
    c = _two_labels(n, t, twin)
    D, X = gf_ctx.build_snapshot(**c)
    info = gf_ctx.build_info()
    print("build_info two labels", n, t, "twin" if twin else "conflict", info)
    assert info[:3] == ((1, 1, 0) if twin else (2, 1, 1)), info
    avail, sched, rD, rX = _check_snapshot(gf_ctx, c, D, X)
    _check_decisions(gf_ctx, c, avail, sched, rD, rX)
