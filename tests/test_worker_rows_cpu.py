"""The row decision of the resident worker (csrc/gangfit_worker_rows.h) against the literal oracle's tightly-pack on the CPU: the
header is pure code, so a small extern "C" shim (tests/worker_rows_shim.cpp) compiled with g++ is all it takes — no HIP, no
libgangfit.so.

What is proven here is the row DECISION (entry_cap, served, run_of).  The rows themselves are cut by the definition in the shim, not
by the kernel's build — its chunk skips and its `fill + rank` placement are covered by tests/test_gpu_worker_rows.py only.

Per application: the row of its executor shape is cut from the capacities of the executor order WITHOUT a driver (numpy, from the
definition: min over the dimensions of floor(avail / request), 0 on a node that is short anywhere, a zero request never limits,
clamped at GF_MAX_K), the driver is the first node of the driver order that holds the driver request, c_ds its node's capacity
with the driver reserved.  Whenever the row says SERVED, driver and placements are the oracle's; when it says NOT SERVED nothing is
claimed — and that happens for at most a quarter of the cases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from gangfit import workloads as wl
from oracle import binding as ob

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32 = ctypes.c_uint32, ctypes.c_int32
NO_SLOT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("worker_rows") / "worker_rows_shim.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", os.path.join(REPO, "k8s-spark-scheduler_amd", "csrc"),
                           os.path.join(REPO, "tests", "worker_rows_shim.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.wrow_consts.restype = None
    lib.wrow_build.restype = U32
    lib.wrow_decide.restype = ctypes.c_int
    lib.wrow_directory_walk.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _consts(shim):
    c = np.zeros(4, dtype=np.uint32)
    shim.wrow_consts(_p(c))
    return [int(x) for x in c]


def _caps(avail_rows, exe, clamp):
    a = avail_rows.astype(np.int64)
    q = np.full(a.shape, np.iinfo(np.int64).max, dtype=np.int64)
    for d in range(3):
        if exe[d] > 0:
            q[:, d] = np.floor_divide(a[:, d], int(exe[d]))
    c = np.minimum(q.min(axis=1), clamp)
    c[(a < 0).any(axis=1)] = 0
    return np.maximum(c, 0).astype(np.int32)


def _rows_against_oracle(shim, avail, d_order, x_order, drv, exe, k):
    row_len, _, _, clamp = _consts(shim)
    oapps = ob.make_apps(drv, exe, k, np.zeros(len(k), dtype=np.uint32))
    ref = ob.fit_independent(0, avail, oapps, d_order, x_order)
    slot_node = np.ascontiguousarray(x_order, dtype=np.uint32)
    pos_of = {int(n): j for j, n in enumerate(x_order)}
    served = 0
    rows = {}
    for a in range(len(k)):
        key = tuple(int(x) for x in exe[a])
        if key not in rows:
            caps = _caps(avail[x_order], exe[a], clamp)
            slot, node, cap = np.zeros(row_len, np.uint32), np.zeros(row_len, np.uint32), np.zeros(row_len, np.int32)
            hdr = shim.wrow_build(U32(len(x_order)), _p(caps), _p(slot_node), _p(slot), _p(node), _p(cap))
            assert hdr == min(row_len, int((caps >= 1).sum()))
            rows[key] = (slot, node, cap, hdr)
        slot, node, cap, hdr = rows[key]
        fits = (avail[d_order] >= drv[a]).all(axis=1)
        if not fits.any():
            continue  # (no driver: the kernel's driver step finds none and the old path answers)
        dn = int(d_order[int(np.argmax(fits))])
        ds = pos_of.get(dn, NO_SLOT)
        c_ds = int(_caps((avail[dn] - drv[a])[None, :], exe[a], clamp)[0])
        out = np.full(max(int(k[a]), 1), NO_SLOT, dtype=np.uint32)
        if shim.wrow_decide(_p(slot), _p(node), _p(cap), U32(hdr), U32(ds), I32(c_ds), I32(int(k[a])), _p(out)):
            served += 1
            feasible, r_dn, r_nodes = ref.placement(a)
            assert feasible and r_dn == dn, (a, dn, r_dn)
            assert np.array_equal(r_nodes, out[:int(k[a])]), a
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
