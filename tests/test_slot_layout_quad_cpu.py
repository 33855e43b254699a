"""The record form of the snapshot's int32 twin (csrc/gangfit_slot_layout.h: LayoutTables::nquad, written by fill_narrow in the pass
that writes the columns) on the CPU, through a shim of its own (tests/slot_layout_quad_shim.cpp, g++ only): for EVERY slot — the
sentinel that closes the slot space and the empty slots an unknown name leaves in the general layout included — the record is
(ncpu[s], nmem[s], ngpu[s], slot_node[s]); its size is four words per slot and nothing is written behind it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = 0xFFFFFFFF  # GF_NO_NODE
NARROW_NEVER = -(1 << 31) // 2
GUARD, GUARD_VALUE = 8, 0x5A5A5A5


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("slot_layout_quad") / "slot_layout_quad_shim.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", os.path.join(REPO, "include"),
                           "-I", os.path.join(REPO, "k8s-spark-scheduler_amd", "csrc"),
                           os.path.join(REPO, "tests", "slot_layout_quad_shim.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.slq_fill.restype = ctypes.c_int
    return lib


def _fill(lib, avail, D, X, force_general):
    avail = np.ascontiguousarray(np.asarray(avail, dtype=np.int64).reshape(-1, 3).T)
    n = avail.shape[1]
    cols = (ctypes.c_void_p * 3)(*[avail[j].ctypes.data for j in range(3)])
    D, X = np.asarray(D, dtype=np.uint32), np.asarray(X, dtype=np.uint32)
    cap = len(X) + len(D) + 2
    ntable = np.zeros(3 * cap, dtype=np.int32)
    index = np.zeros(cap, dtype=np.uint32)
    nquad = np.zeros(4 * cap + GUARD, dtype=np.int32)
    ok, size = ctypes.c_int(0), ctypes.c_uint64(0)
    S = lib.slq_fill(ctypes.c_uint32(n), cols, D.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(D)),
                     X.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(X)), int(force_general), ctypes.c_uint32(cap),
                     ntable.ctypes.data_as(ctypes.c_void_p), index.ctypes.data_as(ctypes.c_void_p),
                     nquad.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(GUARD), ctypes.c_int32(GUARD_VALUE), ctypes.byref(ok),
                     ctypes.byref(size))
    assert S > 0
    return S, bool(ok.value), int(size.value), ntable[:3 * S].reshape(3, S), index[:S], nquad[:4 * S + GUARD]


def _cluster(n, seed):
    rng = np.random.default_rng(seed)
    avail = np.zeros((n, 3), dtype=np.int64)
    avail[:, 0] = 500 * rng.integers(-2, 200, size=n)   # a negative value or two: the sign survives in the twin
    avail[:, 1] = (1 << 20) * rng.integers(1, 4000, size=n)
    avail[:, 2] = rng.integers(0, 5, size=n)
    return avail


@pytest.mark.parametrize("layout", ["merged", "general"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_every_record_is_its_slots_columns_and_node(shim, n, layout):
    avail = _cluster(n, 0x9A0 + n)
    order = np.random.default_rng(n).permutation(n).astype(np.uint32)
    X = [int(v) for v in order if n < 4 or v % 7 != 3]  # some nodes are no executor candidates
    if n >= 4:
        X = X[:2] + [n + 9] + X[2:]                     # an unknown name: an empty slot in the general layout
    D = [int(v) for v in order] if layout == "merged" else [int(v) for v in order[::-1]]
    S, narrow_ok, size, cols, slot_node, quad = _fill(shim, avail, D, X, force_general=(layout == "general"))
    assert narrow_ok and size == 4 * S
    assert (quad[4 * S:] == GUARD_VALUE).all(), "written past four words per slot"
    rec = quad[:4 * S].reshape(S, 4)
    want = np.stack([cols[0], cols[1], cols[2], slot_node.view(np.int32)], axis=1)
    assert np.array_equal(rec, want)
    # the test's own view of what those columns hold: real slots scaled by the column's gcd, the others the never-fitting value
    real = slot_node != NO
    assert slot_node[S - 1] == NO and (rec[~real, :3] == NARROW_NEVER).all() and real.sum() == n
    if layout == "general" and n >= 4:
        assert slot_node[2] == NO and S == len(X) + len(set(D) - set(X)) + 1   # the unknown name's slot stays, empty
    unit = [int(np.gcd.reduce(np.abs(avail[:, j]))) or 1 for j in range(3)]
    nodes = slot_node[real].astype(np.int64)
    for j in range(3):
        assert np.array_equal(rec[real, j].astype(np.int64) * unit[j], avail[nodes, j])


def test_no_narrow_form_no_records_promised(shim):
    """A value at 2^30 units: the twin does not exist (narrow_ok false) and nothing behind the record region was touched."""
    avail = [[1, 6, 0], [1 << 30, 9, 0], [5, 12, 0]]
    S, narrow_ok, size, cols, slot_node, quad = _fill(shim, avail, [0, 1, 2], [0, 1, 2], False)
    assert not narrow_ok and size == 4 * S and (quad[4 * S:] == GUARD_VALUE).all()
