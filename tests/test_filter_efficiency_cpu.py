"""gf_filter_efficiency's summation tree (tests/filter_efficiency.py) against the oracle, without a GPU: exact where the per-node
efficiencies are dyadic rationals, inside the reordering bound otherwise — and the condition that keeps the exact part honest:
on the dyadic inputs the oracle's own sequential sum does not depend on the node order."""
import numpy as np
import pytest

import filter_efficiency as fe
from oracle import binding as ob

SIZES = [1, 63, 64, 65, 130, 4096, 4097]


def _filter(p, algo):
    """The oracle's Filter: the FIFO replay of the queue, the last application's placement, the residual table before it."""
    apps = ob.make_apps(p.drv, p.exe, p.k, p.flags)
    ref = ob.fit_fifo_chain(algo, p.avail, apps, p.D, p.X, sched=p.sched, zone=p.zone)
    ok, d, ex = ref.placement(len(apps) - 1)
    return ok, d, ex, ref.avail_after


@pytest.mark.parametrize("n", SIZES)
def test_restatement_is_the_oracles_sum_on_dyadic_inputs(n):
    p = fe.problem(n, n, dyadic=True)
    ok, d, ex, residual = _filter(p, ob.ALGO_TIGHTLY_PACK)
    assert ok or n < 4
    if not ok:
        d, ex = 0, []
    eff = fe.node_efficiencies(0, residual, p.sched, p.drv[-1], p.exe[-1], d, ex)
    want = fe.oracle_sum(0, residual, p.sched, p.drv[-1], p.exe[-1], d, ex)
    got, counts = fe.restate(eff, p.sched)
    assert np.array_equal(fe.bits(got), fe.bits(want))
    assert counts == (n, int((p.sched[:, 2] != 0).sum()))
    for members in fe.member_rows(n, n):
        want = fe.oracle_sum(0, residual, p.sched, p.drv[-1], p.exe[-1], d, ex, members)
        got, counts = fe.restate(eff, p.sched, members)
        assert np.array_equal(fe.bits(got), fe.bits(want))
        assert counts == (int(members.sum()), int((members & (p.sched[:, 2] != 0)).sum()))


@pytest.mark.parametrize("n", [65, 4097])
def test_dyadic_inputs_are_exact_for_the_oracle_alone(n):
    """Three permutations of the node order: the oracle's sequential sum keeps its bits, so bit identity with it says something
    about the values and nothing about the order."""
    p = fe.problem(n, n, dyadic=True)
    ok, d, ex, residual = _filter(p, ob.ALGO_TIGHTLY_PACK)
    assert ok
    base = fe.oracle_sum(0, residual, p.sched, p.drv[-1], p.exe[-1], d, ex)
    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(n)  # new index i holds old node perm[i]
        inv = np.argsort(perm)
        again = fe.oracle_sum(0, residual[perm], p.sched[perm], p.drv[-1], p.exe[-1], int(inv[d]), [int(inv[v]) for v in ex])
        assert np.array_equal(fe.bits(again), fe.bits(base))
    assert base[3] > 0.0


@pytest.mark.parametrize("n", SIZES)
def test_restatement_within_the_reordering_bound(n):
    p = fe.problem(100 + n, n, dyadic=False, cpu_request=1500)
    ok, d, ex, residual = _filter(p, ob.ALGO_DISTRIBUTE_EVENLY)
    assert ok or n < 4
    if not ok:
        d, ex = 0, []
    eff = fe.node_efficiencies(1, residual, p.sched, p.drv[-1], p.exe[-1], d, ex)
    for members in [None] + fe.member_rows(n, n):
        want = fe.oracle_sum(1, residual, p.sched, p.drv[-1], p.exe[-1], d, ex, members)
        got, _ = fe.restate(eff, p.sched, members)
        bound = fe.reorder_bound(eff, p.sched, members)
        assert np.all(np.abs(got - want) <= bound), (got, want, bound)
        seq = fe.sequential(eff, p.sched, members)  # the module's own loop IS the oracle's
        assert np.array_equal(fe.bits(seq), fe.bits(want))


def test_exact_parts():
    sched = np.array([[8000, 8 * fe.GIB, 0]] * 5, dtype=np.int64)
    eff = np.full((5, 3), 0.25)
    eff[:, 2] = 0.0
    got, counts = fe.restate(eff, sched)
    assert got.tolist() == [0.25, 0.25, 1.0, 0.25] and counts == (5, 0)  # no key with a schedulable gpu: GPU == 1.0
    got, counts = fe.restate(eff, sched, np.zeros(5, dtype=bool))
    assert got.tolist() == [0.0, 0.0, 0.0, 0.0] and counts == (0, 0)  # no key: WorstAvgPackingEfficiency


def test_tree_shape():
    """The tree is the one the header spells out: position pairs first, chunk partials per position in ascending order."""
    v = np.zeros(64)
    v[0], v[1], v[2] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert fe.tree64(v) == 1.0  # (v0 + v1) + (v2 + v3): 1 + 2^-53 rounds to 1, and so does 1 + 2^-53 once more ...
    v[1], v[2], v[3] = 0.0, 2.0 ** -53, 2.0 ** -53
    assert fe.tree64(v) == 1.0 + 2.0 ** -52  # ... while v2 + v3 = 2^-52 survives
    n = 64 * 64 * 2  # a power of two: the division by len is exact
    sched = np.zeros((n, 3), dtype=np.int64)
    eff = np.zeros((n, 3))
    eff[0, 0] = 1.0
    eff[64 * 64, 0] = eff[64 * 64 + 1, 0] = 2.0 ** -53  # one pair of chunk 64: 2^-52 reaches chunk 0's partial at position 0
    assert fe.restate(eff, sched)[0][0] * n == 1.0 + 2.0 ** -52
    eff[64 * 64 + 1, 0] = 0.0
    eff[64 * 65, 0] = 2.0 ** -53  # chunks 64 and 65: positions 0 and 1 of the second group, each 2^-53 is lost on its way
    assert fe.restate(eff, sched)[0][0] * n == 1.0
