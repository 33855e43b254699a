"""The row decision of the resident worker (csrc/gangfit_worker_rows.h) against the literal oracle's tightly-pack on the CPU: the
header is pure code, so a small extern "C" shim (tests/worker_rows_shim.cpp) compiled with g++ is all it takes — no HIP, no
libgangfit.so.

What is proven here is the row DECISION (entry_cap, served, run_of).  The rows themselves are cut by the definition in the shim, not
by the kernel's build — its chunk skips and its `fill + rank` placement are covered by tests/test_gpu_worker_rows.py and
tests/test_gpu_worker_rows_edges.py only.

Per application: the row of its executor shape is cut from the capacities of the executor order WITHOUT a driver (numpy, from the
definition: min over the dimensions of floor(avail / request), 0 on a node that is short anywhere, a zero request never limits,
clamped at GF_MAX_K), the driver is the first node of the driver order that holds the driver request, c_ds its node's capacity
with the driver reserved.  Whenever the row says SERVED, driver and placements are the oracle's; when it says NOT SERVED nothing is
claimed — and that happens for at most a quarter of the cases."""
import ctypes

import numpy as np
import pytest

import worker_rows_cases as wc
from gangfit import workloads as wl
from oracle import binding as ob
from worker_rows_cases import U32, I32, _p

# (the numpy row model — _caps, the row by definition, the first fitting driver, c_ds — lives in tests/worker_rows_cases.py: one copy
#  for this file and for tests/test_worker_rows_cases_cpu.py)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return wc.compile_shim(tmp_path_factory.mktemp("worker_rows"))


def _consts(shim):
    return wc.consts(shim)


def _rows_against_oracle(shim, avail, d_order, x_order, drv, exe, k):
    oapps = ob.make_apps(drv, exe, k, np.zeros(len(k), dtype=np.uint32))
    ref = ob.fit_independent(0, avail, oapps, d_order, x_order)
    served = 0
    for a, (dn, ok, nodes) in enumerate(wc.row_model(shim, avail, d_order, x_order, drv, exe, k)):
        if ok:
            served += 1
            feasible, r_dn, r_nodes = ref.placement(a)
            assert feasible and r_dn == dn, (a, dn, r_dn)
            assert np.array_equal(r_nodes, nodes), a
    return served


@pytest.mark.parametrize("n_nodes,seed", [(40, 1), (100, 2), (130, 3), (257, 4), (400, 5)])
def test_served_rows_are_the_oracles_tightly_pack(shim, n_nodes, seed):
    avail = wl.make_snapshot(n_nodes, 0xC0FFEE + seed).avail.copy()
    avail[3], avail[n_nodes // 2, 0] = [-500, -(1 << 30), 0], -100  # overcommitted nodes, whatever the seed drew
    order = wl.reference_node_order(avail)
    drop = wl.splitmix64(0xD0 + seed, n_nodes, 3) % np.uint64(10) == 0  # the executor order: a subset of the nodes
    x_order = order[~drop[order]]
    assert len(x_order) % 64 != 0 and len(x_order) < n_nodes
    drv, exe, k, _, _ = wl.make_apps(200, 0xA99 + seed, k_cap=48)
    k = k.copy()
    k[:4] = [0, 1, 2, 48]
    served = _rows_against_oracle(shim, avail, order, x_order, drv, exe, k)
    assert served * 4 >= 3 * len(k), (served, len(k))


def test_the_small_problem_is_served_entirely(shim):
    w = wl.config(2, n_nodes=300, n_apps=165)
    s = w.snapshot
    assert _rows_against_oracle(shim, s.avail, s.driver_order, s.exec_order, w.drv, w.exe, w.k) == 165


def test_directory_word(shim):
    _, _, sightings, _ = _consts(shim)
    word, builders, ready_at = U32(0), U32(0), I32(0)

    def walk(ev):
        e = np.asarray(ev, dtype=np.uint8)
        shim.wrow_directory_walk(U32(len(e)), _p(e), ctypes.byref(word), ctypes.byref(builders), ctypes.byref(ready_at))
        return word.value, builders.value, ready_at.value

    assert walk([1, 1, 2]) == (0, 0, -1)                                 # EMPTY: sightings and a publish change nothing
    assert walk([0] + [1] * (sightings - 2)) == (sightings, 0, -1)       # COUNTING: claim = first sighting
    assert walk([0] + [1] * (sightings - 2) + [2]) == (sightings, 0, -1)  # nothing to publish before the build
    w, b, r = walk([0] + [1] * (sightings + 5) + [2, 1, 1, 2])
    assert b == 1 and r == sightings + 6 and w == (0x80000000 | (sightings + 1))  # one builder; BUILDING and READY count no more
