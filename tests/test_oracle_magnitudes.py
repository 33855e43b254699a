"""The oracle at the edges of the quantity contract (tests/magnitudes.py): the GPU magnitude tests trust it, and its
restatements had only been cross-checked on small values.  Literal and closed form, every packer, both modes, must agree on
results, placements, residuals and efficiencies; the string-keyed map restatement (fit_maps) too, for the packers it has.
And the generator must still hit its edges: a later edit cannot make it tame without failing here.  CPU only."""
import math

import numpy as np
import pytest

import magnitudes as mg
from oracle import binding as ob

ALGOS = (0, 1, 2, 3, 4, 5)


def _small(regime):
    """The regime's cases, with max-k's gangs cut to a few thousand executors (the literal loops are O(K) per driver)."""
    out = []
    for name, p, route in mg.cases(regime, seed=7):
        if regime == "max-k":
            avail, sched, zone, D, X, drv, exe, k, flags = p
            p = (avail, sched, zone, D, X, drv, exe, np.minimum(k, 3000).astype(np.int32), flags)
        out.append((name, p))
    return out


def _same(a: ob.BatchOut, b: ob.BatchOut, fifo: bool):
    assert np.array_equal(a.results, b.results)
    for i in np.nonzero(a.results["has_capacity"])[0]:
        assert np.array_equal(a.placement(int(i))[2], b.placement(int(i))[2]), f"app {i}"
    if fifo:
        assert a.failed_at == b.failed_at
        assert np.array_equal(a.avail_after, b.avail_after)


@pytest.mark.parametrize("regime", mg.REGIMES)
def test_literal_and_closed_form_agree(regime):
    for name, (avail, sched, zone, D, X, drv, exe, k, flags) in _small(regime):
        apps = ob.make_apps(drv, exe, k, flags)
        for algo in ALGOS:
            lit = ob.fit_independent(algo, avail, apps, D, X, sched=sched, zone=zone)
            clo = ob.fit_independent(algo, avail, apps, D, X, closed_form=True, sched=sched, zone=zone)
            _same(lit, clo, False)
            assert np.array_equal(lit.avg_eff.view(np.uint64), clo.avg_eff.view(np.uint64)), (name, algo)
            lit = ob.fit_fifo_chain(algo, avail, apps, D, X, sched=sched, zone=zone)
            clo = ob.fit_fifo_chain(algo, avail, apps, D, X, closed_form=True, sched=sched, zone=zone)
            _same(lit, clo, True)
            if regime != "max-k":  # (the map of every successful pack: the reference's cost shape, O(K N) per gang)
                eff = ob.fit_fifo_chain(algo, avail, apps, D, X, sched=sched, zone=zone, with_efficiencies=True)
                _same(lit, eff, True)


@pytest.mark.parametrize("regime", mg.REGIMES)
def test_string_keyed_maps_agree(regime):
    for name, (avail, sched, zone, D, X, drv, exe, k, flags) in _small(regime):
        apps = ob.make_apps(drv, exe, k, flags)
        for algo in (0, 1):
            _same(ob.fit_independent(algo, avail, apps, D, X), ob.fit_maps(algo, avail, apps, D, X, False, sched=sched), False)
            _same(ob.fit_fifo_chain(algo, avail, apps, D, X), ob.fit_maps(algo, avail, apps, D, X, True, sched=sched), True)


@pytest.mark.parametrize("regime", mg.REGIMES)
def test_efficiencies_agree(regime):
    """The average a packer reports against the list average (efficiency.go:114-156) over its placement, and the per-node
    map (go_packing_efficiency) of the nodes the placement leaves alone against magnitudes.node_eff, the restatement the
    generator builds its one-ulp twins with."""
    checked = 0
    for name, (avail, sched, zone, D, X, drv, exe, k, flags) in _small(regime)[:2]:
        ref = ob.fit_independent(0, avail, ob.make_apps(drv, exe, k, flags), D, X, sched=sched)
        for a in np.nonzero(ref.results["has_capacity"])[0][:3]:
            _, d, ex = ref.placement(int(a))
            want = ob.avg_packing_efficiency_list(avail, sched, drv[a], exe[a], d, ex)
            assert np.array_equal(ref.avg_eff[a].view(np.uint64), want.view(np.uint64))
            eff, _ = ob.packing_efficiency(avail, sched, drv[a], exe[a], d, ex)
            untouched = np.setdiff1d(np.arange(len(avail)), np.append(ex, d))[:64]
            for n in untouched:
                assert eff[n].tolist() == mg.node_eff(avail[n], sched[n]), (name, n)
            checked += 1
    assert checked > 0


# ---------------------------------------------------------------------------------------------- the generator's edges


def test_bytes_has_no_narrow_form():
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), _ in mg.cases("bytes"):
        mem = [int(v) for v in avail[:, 1]]
        assert math.gcd(*mem) == 1 and max(abs(v) for v in mem) >= 1 << 30, name  # every chain takes the wide kernels
        assert (avail[:, 0] % 250 != 0).any() and (exe[:, 0] % 250 != 0).any()
        assert (exe[:, 1] % 10 ** 9 == 0).any() and (exe[:, 1] % (1 << 30) != 0).any()  # decimal sizes
        assert (avail[:, 1] > sched[:, 1]).any()  # used < 0


def _units(col):
    return math.gcd(*[abs(int(v)) for v in col])


def test_narrow_edge_sits_on_the_bound():
    seen = set()
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), route in mg.cases("narrow-edge"):
        v = name.split("/")[0]
        u = _units(avail[:, 1])
        scaled = avail[:, 1] // u
        if v == "table-at-bound":
            assert scaled.max() == mg.NARROW and scaled.min() == -mg.NARROW
        if v == "table-past-bound":
            assert scaled.max() == mg.NARROW + 1
        if v == "request-at-bound":
            assert (exe[:, 1] // u).max() == mg.NARROW and (exe[:, 1] % u == 0).all()
        if v == "request-past-bound":
            assert (exe[:, 1] // u).max() == mg.NARROW + 1 and (exe[:, 1] % u == 0).all()
        if v.startswith("refine"):  # narrow_units (gangfit_api_fit.cpp): gcd with every request, factor against room
            eff = math.gcd(u, *[int(x) for x in np.concatenate([drv[:, 1], exe[:, 1]]) if x > 0])
            room = mg.NARROW // int(np.abs(scaled).max())
            assert u // eff == (room if v == "refine-at-room" else room + 1)
        if route == "lds":  # every other column and request is a multiple of the table's units
            for j in (0, 2):
                uj = _units(avail[:, j])
                assert (drv[:, j] % uj == 0).all() and (exe[:, j] % uj == 0).all()
        seen.add((v, route))
    assert {(v, r) for v, r in mg.NARROW_VARIANTS} <= seen


def test_huge_reaches_both_sides_of_2_40_and_exact_multiples():
    below = above = exact = clamp = False
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), _ in mg.cases("huge"):
        assert np.abs(avail).max() == mg.QMAX and exe.max() == mg.QMAX and (avail < 1 << 62).all()
        assert (~exe.any(axis=1)).any() and ((exe == 0).any(axis=1) & exe.any(axis=1)).any()
        for a in range(len(k)):
            for j in range(3):
                e = int(exe[a, j])
                if e == 0:
                    continue
                q = [int(v) // e for v in avail[:, j] if v >= 0]
                below |= any(x == (1 << 40) - 1 for x in q)
                above |= any(x == 1 << 40 for x in q) and any(x == (1 << 40) + 1 for x in q)
                exact |= any(int(v) % e == 0 and int(v) // e >= 2 for v in avail[:, j] if v > 0)
                clamp |= all(any(x == int(k[a]) + d for x in q) for d in (-1, 0, 1)) and k[a] > 1
    assert below and above and exact and clamp


def test_max_k_capacity_sums():
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), _ in mg.cases("max-k"):
        assert set(k.tolist()) == {mg.GF_MAX_K, mg.GF_MAX_K - 1}
        assert (~exe.any(axis=1)).sum() == 2
        assert int((avail[:, 1] // exe[2, 1]).sum()) == k[2] == k[4] + 1
        assert int((avail[:, 2] // exe[3, 2]).sum()) == k[3] - 1


def test_efficiency_edges():
    twins = ulp = 0
    for name, (avail, sched, zone, D, X, drv, exe, k, flags), _ in mg.cases("efficiency"):
        big = sched[:, 1] >= 1 << 53
        assert big.any() and any(int(float(v)) != int(v) for v in sched[big, 1])  # low bits float64 cannot hold
        assert {(1 << 32) - 1, 1 << 32} <= set(sched[:, 0].tolist())
        used = sched[:, 0] - avail[:, 0]
        assert ((used < 1 << 32) & (used + exe[:, 0].max() * 2 >= 1 << 32)).any()  # two executors cross 2^32
        assert (avail[:, 1] > sched[:, 1]).any() and (~sched.any(axis=1)).any()
        zs = sorted(set(zone.tolist()))
        if len(zs) >= 3:
            m = len(avail) // len(zs)
            for i in range(m):
                e0 = mg.node_eff(avail[i], sched[i])
                assert mg.node_eff(avail[m + i], sched[m + i]) == e0  # the exact twin
                e2 = mg.node_eff(avail[2 * m + i], sched[2 * m + i])
                if e2 != e0:
                    assert e2[1] == np.nextafter(e0[1], 2.0)
                    ulp += 1
            twins += 1
    assert twins and ulp >= 5
