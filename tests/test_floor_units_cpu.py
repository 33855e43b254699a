"""The narrow units of a FIFO chain (csrc/gangfit_floor_units.h: refine_units, floor_units, chain_units, exact_fails_at) against a
plain-Python restatement, on the CPU: the header is pure host code, so a small extern "C" shim (tests/floor_units_shim.cpp) compiled
with g++ is all it takes — no HIP, no libgangfit.so.  Also here: the five equivalences the floored form rests on, by brute force
over small integers, and the queues whose routes tests/magnitudes.py pins — they must stay off the floored form."""
import ctypes
import os
import subprocess
from math import gcd

import numpy as np
import pytest

import magnitudes as mg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 1 << 30  # scaled values lie strictly inside (-2^30, 2^30)
GF_MAX_K = 1 << 20
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
NO_RANGE = ([I64_MAX] * 3, [I64_MIN] * 3)  # tmin > tmax: no real slot


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("floor_units") / "floor_units_shim.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", os.path.join(REPO, "include"),
                           "-I", os.path.join(REPO, "k8s-spark-scheduler_amd", "csrc"),
                           os.path.join(REPO, "tests", "floor_units_shim.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.fu_floor_div.restype = ctypes.c_int64
    lib.fu_floor_div.argtypes = [ctypes.c_int64, ctypes.c_int64]
    lib.fu_chain_units.restype = None
    lib.fu_floor_units.restype = ctypes.c_int
    lib.fu_exact_fails_at.restype = ctypes.c_uint32
    return lib


# ---------------------------------------------------------------------------------------------------- the restatement
def py_refine(unit, nmax, apps):
    """-> (eff, factor, proven): gcd(table unit, requests) while every scaled magnitude stays below 2^30, else the table's units."""
    eff = list(unit)
    for drv, exe, _ in apps:
        for j in range(3):
            for v in (drv[j], exe[j]):
                if v > 0:
                    eff[j] = gcd(eff[j], v)
    factor, ok = [1, 1, 1], True
    for j in range(3):
        room = (B - 1) // nmax[j] if nmax[j] > 0 else B - 1
        ok = ok and unit[j] // eff[j] <= room
        factor[j] = unit[j] // eff[j] if ok else 1
    if not ok:
        eff, factor = list(unit), [1, 1, 1]
    proven = all(v >= 0 and v % eff[j] == 0 and v // eff[j] < B for drv, exe, _ in apps for j in range(3) for v in (drv[j], exe[j]))
    return eff, factor, proven


def py_range_ok(tmin, tmax, u):
    return tmin > tmax or (tmax // u < B and tmin // u > -B)  # Python's // floors


def py_floor_units(tmin, tmax, apps):
    """-> units, or None.  gcd of the positive requests; nobody asks: the smallest power of two that brings the column inside."""
    if any(k < 0 or k > GF_MAX_K for _, _, k in apps) or any(v < 0 for drv, exe, _ in apps for v in list(drv) + list(exe)):
        return None
    unit = []
    for j in range(3):
        reqs = [v for drv, exe, _ in apps for v in (drv[j], exe[j]) if v > 0]
        if not reqs:
            u = 1
            while not py_range_ok(tmin[j], tmax[j], u):
                u *= 2
        else:
            u = 0
            for v in reqs:
                u = gcd(u, v)
            if max(reqs) // u >= B or not py_range_ok(tmin[j], tmax[j], u):
                return None
        unit.append(u)
    return unit


def py_chain_units(narrow_ok, unit, nmax, tmin, tmax, apps, allow_floor=True):
    """-> (unit, factor, proven, floored)"""
    eff, factor, proven = [1, 1, 1], [1, 1, 1], False
    if narrow_ok:
        eff, factor, proven = py_refine(unit, nmax, apps)
    if proven or not allow_floor:
        return eff, factor, proven, False
    fu = py_floor_units(tmin, tmax, apps)
    return (fu, [1, 1, 1], True, True) if fu is not None else (eff, factor, False, False)


def _arrays(apps):
    drv = np.array([a[0] for a in apps], dtype=np.int64).reshape(-1, 3)
    exe = np.array([a[1] for a in apps], dtype=np.int64).reshape(-1, 3)
    k = np.array([a[2] for a in apps], dtype=np.int32)
    return drv, exe, k


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def c_chain_units(lib, narrow_ok, unit, nmax, tmin, tmax, apps, allow_floor=True):
    drv, exe, k = _arrays(apps)
    facts = np.array(list(unit) + list(nmax) + list(tmin) + list(tmax), dtype=np.int64)
    out = np.zeros(8, dtype=np.int64)
    lib.fu_chain_units(int(narrow_ok), _ptr(facts), ctypes.c_uint32(len(apps)), _ptr(drv), _ptr(exe), _ptr(k), int(allow_floor), _ptr(out))
    return [int(v) for v in out[:3]], [int(v) for v in out[3:6]], bool(out[6]), bool(out[7])


def c_floor_units(lib, tmin, tmax, apps):
    drv, exe, k = _arrays(apps)
    rng_ = np.array(list(tmin) + list(tmax), dtype=np.int64)
    unit = np.zeros(3, dtype=np.int64)
    ok = lib.fu_floor_units(_ptr(rng_), ctypes.c_uint32(len(apps)), _ptr(drv), _ptr(exe), _ptr(k), _ptr(unit))
    return [int(v) for v in unit] if ok else None


def c_exact_fails_at(lib, unit, nmax, apps):
    drv, exe, k = _arrays(apps)
    facts = np.array(list(unit) + list(nmax), dtype=np.int64)
    return int(lib.fu_exact_fails_at(_ptr(facts), ctypes.c_uint32(len(apps)), _ptr(drv), _ptr(exe), _ptr(k)))


def app(drv, exe, k=1):
    return (list(drv), list(exe), k)


# ---------------------------------------------------------------------------------------------------- the arithmetic
def test_floor_div_rounds_toward_minus_infinity(shim):
    rng = np.random.default_rng(1)
    cases = [(a, u) for a in (-9, -8, -1, 0, 1, 7, 8, 9) for u in (1, 2, 8)]
    cases += [(-(B - 1) * 1024 - 1, 1024), ((1 << 62) - 1, 1 << 32), (-(1 << 62) + 1, 1 << 32), (-(1 << 62) + 1, (1 << 62) - 1)]
    cases += [(int(rng.integers(-(1 << 62) + 1, 1 << 62)), int(rng.integers(1, 1 << int(rng.integers(1, 62))))) for _ in range(2000)]
    for a, u in cases:
        assert shim.fu_floor_div(a, u) == a // u, (a, u)


def test_the_five_equivalences_on_small_integers():
    """A = q u + r, q = floor(A / u), 0 <= r < u; a chain leaves A' = q' u + r.  For a request rho u, a reserved base beta u and an
    executor request eps u: the driver check, the negative test, the capacity, a chunk maximum and a commit are the same on q'
    as on A' — every u, every A' (negatives included), exhaustively over a small box."""
    for u in range(1, 8):
        values = range(-5 * u - 3, 6 * u + 4)
        for A in values:
            q, r = A // u, A % u
            assert A == q * u + r and 0 <= r < u
            for rho in range(0, 8):
                assert (rho * u > A) == (rho > q)  # the driver does not fit
                assert (A - rho * u) // u == q - rho and (A - rho * u) % u == r  # a commit subtracts rho from q and leaves r alone
                for beta in range(0, 4):
                    assert (A - beta * u < 0) == (q - beta < 0)  # the negative test
                    if q - beta >= 0:
                        for eps in range(1, 6):
                            assert (A - beta * u) // (eps * u) == (q - beta) // eps  # the capacity
        # a chunk maximum over q rules a chunk out exactly when the maximum over A would
        rng = np.random.default_rng(u)
        for _ in range(200):
            chunk = rng.integers(-5 * u, 6 * u, size=8)
            for rho in range(0, 8):
                assert (int(chunk.max()) < rho * u) == (int((chunk // u).max()) < rho)


# ---------------------------------------------------------------------------------------------------- the units
def _random_queue(rng, units, n):
    apps = []
    for _ in range(n):
        drv = [int(rng.integers(0, 50)) * units[0], int(rng.integers(0, 64)) * units[1], 0]
        exe = [int(rng.integers(0, 9)) * units[0], int(rng.integers(0, 600)) * units[1], int(rng.random() < 0.3) * units[2]]
        apps.append(app(drv, exe, int(rng.integers(0, 100))))
    return apps


def test_units_are_the_gcds_of_the_requests(shim):
    rng = np.random.default_rng(2)
    for it in range(300):
        units = [int(rng.choice([1, 5, 250, 1000])), int(rng.choice([1, 256, 1 << 20, 10 ** 6, 1 << 32, 3 * (1 << 30) + 1])), 1]
        apps = _random_queue(rng, units, int(rng.integers(1, 20)))
        hi = [int(rng.integers(0, 1 << 20)), int(rng.integers(0, 1 << int(rng.integers(20, 62)))), int(rng.integers(0, 1 << 41))]
        lo = [-int(rng.integers(0, 1 << 12)), -int(rng.integers(0, 1 << int(rng.integers(1, 62)))), -int(rng.integers(0, 3))]
        want = py_floor_units(lo, hi, apps)
        assert c_floor_units(shim, lo, hi, apps) == want, (it, units, lo, hi)
        if want is not None:
            for j in range(3):
                reqs = [v for d, e, _ in apps for v in (d[j], e[j]) if v > 0]
                assert all(v % want[j] == 0 and v // want[j] < B for v in reqs)
                assert want[j] % units[j] == 0 or not reqs  # (the drawn grid divides the gcd)
                assert -B < lo[j] // want[j] and hi[j] // want[j] < B
        # ... and as chain_units sees it on a table without an exact form
        assert c_chain_units(shim, False, [1, 1, 1], [0, 0, 0], lo, hi, apps) == \
            py_chain_units(False, [1, 1, 1], [0, 0, 0], lo, hi, apps)


def test_asymmetric_bound_at_2_30(shim):
    """floor(A / u) in (-2^30, 2^30): +(2^30 - 1) u + (u - 1) is in and 2^30 u is out; -(2^30 - 1) u is in and one byte less floors to
    -2^30 and is out.  A request of 2^30 - 1 units is in, one of 2^30 is out."""
    u = 1024
    queue = [app([250, u, 0], [250, 3 * u, 0], 4)]
    ranges = {  # (tmin[1], tmax[1]) -> floored?
        (0, (B - 1) * u): True, (0, (B - 1) * u + u - 1): True, (0, B * u): False,
        (-(B - 1) * u, 0): True, (-(B - 1) * u - 1, 0): False, (-B * u, 0): False,
        (-(B - 1) * u, (B - 1) * u + u - 1): True,
    }
    for (lo, hi), want in ranges.items():
        tmin, tmax = [0, lo, 0], [64000, hi, 8]
        got = c_floor_units(shim, tmin, tmax, queue)
        assert (got is not None) == want, (lo, hi, got)
        assert got == py_floor_units(tmin, tmax, queue)
        if want:
            assert got == [250, u, 1]
    tmin, tmax = [0, 0, 0], [64000, 1 << 39, 8]
    at = queue + [app([0, (B - 1) * u, 0], [0, u, 0], 1)]
    past = queue + [app([0, B * u, 0], [0, u, 0], 1)]
    assert c_floor_units(shim, tmin, tmax, at) == [250, u, 1] == py_floor_units(tmin, tmax, at)
    assert c_floor_units(shim, tmin, tmax, past) is None and py_floor_units(tmin, tmax, past) is None
    for bad_k in (-1, GF_MAX_K + 1):
        assert c_floor_units(shim, tmin, tmax, queue + [app([0, u, 0], [0, u, 0], bad_k)]) is None
    assert c_floor_units(shim, tmin, tmax, queue + [app([0, u, 0], [0, u, 0], GF_MAX_K)]) == [250, u, 1]


def test_unit_of_2_32(shim):
    """Requests of 4 GiB multiples only: the unit is 2^32 (no int32 holds a remainder), tables of arbitrary bytes up to 2^61."""
    g4 = 1 << 32
    queue = [app([1000, g4, 0], [500, 3 * g4, 0], 7), app([250, 5 * g4, 0], [250, g4, 1], 2)]
    tmin, tmax = [-3, -(1 << 40) - 12345, -1], [96001, (1 << 61) + 987654321, 8]
    assert c_floor_units(shim, tmin, tmax, queue) == [250, g4, 1] == py_floor_units(tmin, tmax, queue)
    assert c_floor_units(shim, tmin, [96001, (B << 32), 8], queue) is None  # floor = 2^30
    assert c_floor_units(shim, tmin, [96001, (B << 32) - 1, 8], queue) == [250, g4, 1]


def test_dimension_nobody_asks_for(shim):
    """No gpu request in the queue: the gpu column takes the smallest power of two that brings it inside the range — 2^11 for 2^40
    (2^40 / 2^10 is 2^30, one too many), 1 for a column that is inside already, 1 for a column without a real slot."""
    queue = [app([1000, 1 << 20, 0], [500, 1 << 21, 0], 3)]
    for top, want in ((8, 1), (B - 1, 1), (B, 2), (1 << 40, 1 << 11), ((1 << 40) - 1, 1 << 10), ((1 << 62) - 1, 1 << 32)):
        tmin, tmax = [0, 0, -1], [64000, 1 << 39, top]
        assert c_floor_units(shim, tmin, tmax, queue) == [500, 1 << 20, want] == py_floor_units(tmin, tmax, queue), top
    tmin, tmax = [0, 0, -(1 << 40)], [64000, 1 << 39, 0]
    assert c_floor_units(shim, tmin, tmax, queue) == [500, 1 << 20, 1 << 11]  # floor(-2^40 / 2^10) = -2^30 is out too
    assert c_floor_units(shim, NO_RANGE[0], NO_RANGE[1], queue) == [500, 1 << 20, 1]
    assert c_floor_units(shim, [0, 0, 0], [1, 1, 1], [app([0, 0, 0], [0, 0, 0], 5)]) == [1, 1, 1]  # nobody asks for anything


def test_a_batch_the_exact_form_proves_is_untouched(shim):
    """narrow_ok and every request a multiple of the (refined) units: chain_units returns refine_units' answer, floored = 0 —
    although the floored form exists too, with other units.  One request off the grid, and the floored form takes over."""
    unit, nmax = [250, 1 << 20, 1], [400, 1 << 18, 8]
    tmin, tmax = [-1000, -(1 << 38), -1], [100000, 1 << 38, 8]
    queue = [app([500, 4 << 20, 0], [1000, 8 << 20, 0], 3), app([250, 2 << 20, 0], [750, 6 << 20, 1], 9)]
    got = c_chain_units(shim, True, unit, nmax, tmin, tmax, queue)
    assert got == py_chain_units(True, unit, nmax, tmin, tmax, queue) == (unit, [1, 1, 1], True, False)
    assert py_floor_units(tmin, tmax, queue) == [250, 2 << 20, 1]  # (it would have been coarser)
    finer = queue + [app([250, 1 << 19, 0], [250, 1 << 19, 0], 1)]  # refinement by 2: room = (2^30 - 1) // 2^18 = 4095
    assert c_chain_units(shim, True, unit, nmax, tmin, tmax, finer) == ([250, 1 << 19, 1], [1, 2, 1], True, False)
    # decimal requests: gcd(MiB, 100M) = 2^8 refines by 4096, one past the room; the requests alone share 10^8
    odd = [app([250, 10 ** 8, 0], [500, 2 * 10 ** 8, 0], 5), app([250, 3 * 10 ** 8, 0], [250, 10 ** 8, 0], 1)]
    assert gcd(1 << 20, 10 ** 8) == 256 and py_refine(unit, nmax, odd) == (unit, [1, 1, 1], False)
    got = c_chain_units(shim, True, unit, nmax, tmin, tmax, odd)
    assert got == py_chain_units(True, unit, nmax, tmin, tmax, odd) == ([250, 10 ** 8, 1], [1, 1, 1], True, True)
    assert c_chain_units(shim, True, unit, nmax, tmin, tmax, odd, allow_floor=False) == (unit, [1, 1, 1], False, False)
    # without any narrow form: proven = floored = 0, whatever the units say
    wide = queue + [app([1, 7 * (1 << 30) + 13, 0], [1, 1 << 20, 0], 1)]
    got = c_chain_units(shim, True, unit, nmax, tmin, [100000, 1 << 45, 8], wide)
    assert got[2:] == (False, False) and got == py_chain_units(True, unit, nmax, tmin, [100000, 1 << 45, 8], wide)


def test_chain_units_random(shim):
    rng = np.random.default_rng(3)
    seen = set()
    for it in range(400):
        unit = [250, int(rng.choice([1 << 20, 1 << 10, 1025 * 1024])), 1]
        nmax = [int(rng.integers(1, 400)), int(rng.integers(1, 1 << int(rng.integers(10, 31)))), 8]
        narrow_ok = bool(rng.random() < 0.7)
        tmax = [nmax[0] * 250, nmax[1] * unit[1] + (0 if narrow_ok else int(rng.integers(0, unit[1]))), 8]
        tmin = [-250, -int(rng.integers(0, nmax[1] + 1)) * unit[1], -1]
        grid = [250, int(rng.choice([unit[1], 1 << 8, 1000, 1 << 20, 1025])), 1]
        apps = _random_queue(rng, grid, int(rng.integers(1, 12)))
        got = c_chain_units(shim, narrow_ok, unit, nmax, tmin, tmax, apps)
        assert got == py_chain_units(narrow_ok, unit, nmax, tmin, tmax, apps), (it, narrow_ok, unit, nmax, grid)
        seen.add(got[2:])
    assert seen == {(True, False), (True, True), (False, False)}


def test_exact_fails_at_is_the_shortest_unproven_prefix(shim):
    """exact_fails_at = the length of the shortest prefix refine_units does not prove (0: none), and every longer prefix is
    unproven too — what lets a queue that begins with the cached floored chain's prefix skip the scan of the exact form."""
    rng = np.random.default_rng(4)
    hit = 0
    for it in range(300):
        unit = [250, int(rng.choice([1 << 20, 1025 * 1024])), 1]
        nmax = [int(rng.integers(1, 400)), int(rng.integers(1, 1 << int(rng.integers(10, 31)))), 8]
        grid = [250, int(rng.choice([unit[1], unit[1], 1 << 8, 1 << 19, 1025, 1024])), 1]
        apps = _random_queue(rng, [250, unit[1], 1], int(rng.integers(1, 8))) + _random_queue(rng, grid, int(rng.integers(1, 6))) + \
            _random_queue(rng, [250, unit[1], 1], 2)
        if rng.random() < 0.2:
            apps[int(rng.integers(0, len(apps)))][1][1] = int(rng.choice([B - 1, B])) * unit[1]
        proven = [py_refine(unit, nmax, apps[:n])[2] for n in range(1, len(apps) + 1)]
        want = next((n + 1 for n, p in enumerate(proven) if not p), 0)
        assert c_exact_fails_at(shim, unit, nmax, apps) == want, (it, proven)
        if want:
            assert not any(proven[want - 1:]), (it, proven)  # monotone
            hit += 1
    assert 50 < hit < 290


# ---------------------------------------------------------------------------------------------------- the routes tests pin
def _facts(avail, D, X):
    """unit, nmax, narrow_ok, tmin, tmax of the slots a merged layout gives the known nodes of the two orders (fill_narrow, fill_range)."""
    n = len(avail)
    real = sorted({int(v) for v in list(D) + list(X) if v < n})
    unit, nmax, tmin, tmax, ok = [], [], [], [], True
    for j in range(3):
        col = [int(avail[i, j]) for i in real]
        g = 0
        for v in col:
            g = gcd(g, abs(v))
        g = g or 1
        unit.append(g)
        nmax.append(max(abs(v) // g for v in col))
        ok = ok and all(abs(v) // g < B for v in col)
        tmin.append(min(col))
        tmax.append(max(col))
    return ok, unit, nmax, tmin, tmax


def _queue(drv, exe, k):
    return [app([int(v) for v in drv[i]], [int(v) for v in exe[i]], int(k[i])) for i in range(len(k))]


def test_pinned_routes_stay_where_they_are(shim):
    """tests/magnitudes.py names the route of every narrow-edge variant on the merged layout and puts the "bytes" regime on the wide
    kernels; test_gpu_snapshot_magnitudes.test_wide_gcd_branch_with_decisions pins its queue there too.  With the floored form
    allowed every "lds" case is still proven exact (floored = 0, the same units) and no "wide" case has a floored form."""
    routes = set()
    for name, p, route in mg.cases("narrow-edge"):
        if route is None:
            continue
        ok, unit, nmax, tmin, tmax = _facts(p[0], p[3], p[4])
        apps = _queue(*p[5:8])
        got = c_chain_units(shim, ok, unit, nmax, tmin, tmax, apps)
        assert got == py_chain_units(ok, unit, nmax, tmin, tmax, apps), name
        assert got == c_chain_units(shim, ok, unit, nmax, tmin, tmax, apps, allow_floor=False), name  # nothing moves
        assert got[2:] == ((True, False) if route == "lds" else (False, False)), (name, got)
        routes.add(route)
    assert routes == {"lds", "wide"}
    for name, p, _ in mg.cases("bytes"):
        ok, unit, nmax, tmin, tmax = _facts(p[0], p[3], p[4])
        assert not ok and unit[1] == 1, name
        got = c_chain_units(shim, ok, unit, nmax, tmin, tmax, _queue(*p[5:8]))
        assert got[2:] == (False, False), (name, got)
    # the wide-gcd queue: bytes_regime's request shapes against odd 61-bit memory (any such column: the memory unit decides)
    drv, exe, k, _ = mg.bytes_regime(np.random.default_rng(61), "merged", 3, n=8, a=64)[5:9]
    tmin, tmax = [0, 1, 0], [(1 << 20) - 1, (1 << 61) - 1, 8]
    got = c_chain_units(shim, False, [1, 1, 1], [0, 0, 0], tmin, tmax, _queue(drv, exe, k))
    assert got[2:] == (False, False), got
