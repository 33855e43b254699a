"""The label plan (csrc/gangfit_label_plan.h: plan_labels) against a plain-Python restatement, on the CPU: the header is pure host
code, so a small extern "C" shim (tests/label_plan_shim.cpp) compiled with g++ is all it takes — no HIP, no libgangfit.so.  The
same cases run once more in a stand-alone program (tests/label_plan_main.cpp) built with AddressSanitizer and UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 0xFFFFFFFF
INCLUDES = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "k8s-spark-scheduler_amd", "csrc")]
FIELDS = ("device_route", "driver_active", "exec_active", "which", "max_rank", "width", "passes")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("label_plan") / "label_plan_shim.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", *INCLUDES,
                           os.path.join(REPO, "tests", "label_plan_shim.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.lp_plan.restype = None
    return lib


def run_shim(lib, dl, el, on_device=True):
    arrays = [None if r is None else np.ascontiguousarray(r, dtype=np.uint32) for r in (dl, el)]
    n = next((len(a) for a in arrays if a is not None), 0)
    # (an empty numpy array still has an address: plan_labels must not read it)
    ptrs = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrays]
    out = (ctypes.c_uint32 * 7)()
    lib.lp_plan(ctypes.c_uint32(n), ptrs[0], ptrs[1], int(on_device), out)
    return dict(zip(FIELDS, out))


def restate(dl, el, on_device=True):
    """An array re-sorts something ("active") when it holds two different values; L is the driver array when it is active, else
    the executor array when that is; the label group's key is the rank itself, "not ranked" the largest ranked value of L + 1,
    its field the bits of that, sorted eight bits per pass.  The slot tables are built on the device unless the option says host."""
    active = [r is not None and len(set(int(v) for v in r)) > 1 for r in (dl, el)]
    which = 1 if active[0] else (2 if active[1] else 0)
    max_rank = width = passes = 0
    if which:
        max_rank = max([int(v) for v in (dl, el)[which - 1] if int(v) != U], default=0)
        width = (max_rank + 1).bit_length()
        passes = (width + 7) // 8
    return dict(device_route=int(on_device), driver_active=int(active[0]), exec_active=int(active[1]), which=which,
                max_rank=max_rank, width=width, passes=passes)


CASES = {
    "no arrays": (None, None),
    "empty": ([], []),
    "all unranked": ([U] * 5, [U] * 5),
    "all equal": ([7] * 9, None),
    "one node": ([3], [U]),
    "max 0": ([0, U, 0], None),
    "max 0 exec": (None, [U, 0]),
    "max 254": ([254, 0, U], None),
    "max 255": ([0, 255], None),
    "max 256": ([256, U, 1], None),
    "max 2^32-2": ([U - 1, 0, U], None),
    "all ranked": ([0, 1, 2, 3], None),
    "driver is L": ([0, 1, U], [5, 9, 5]),
    "exec is L": (None, [5, 9, 5]),
    "exec is L behind a driver array that re-sorts nothing": ([4, 4, 4], [5, 9, U]),
    "driver is L beside an executor array that re-sorts nothing": ([4, 1, 4], [U, U, U]),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("on_device", [True, False])
def test_plan_matches_restatement(shim, name, on_device):
    dl, el = CASES[name]
    assert run_shim(shim, dl, el, on_device) == restate(dl, el, on_device)


def test_known_answers(shim):
    """Width and pass count at the byte edges, pinned as numbers (the restatement shares the rule, not the arithmetic)."""
    for max_rank, width, passes in ((0, 1, 1), (254, 8, 1), (255, 9, 2), (256, 9, 2), (65534, 16, 2), (65535, 17, 3),
                                    (2**24 - 2, 24, 3), (2**24 - 1, 25, 4), (U - 1, 32, 4)):
        p = run_shim(shim, [max_rank, U], None)
        assert (p["which"], p["max_rank"], p["width"], p["passes"]) == (1, max_rank, width, passes)
    p = run_shim(shim, [U, U], [1, 0])
    assert (p["which"], p["driver_active"], p["exec_active"], p["width"]) == (2, 0, 1, 2)


def test_random_arrays(shim):
    rng = np.random.default_rng(11)
    for _ in range(200):
        n = int(rng.integers(0, 40))
        top = int(rng.choice([1, 2, 255, 256, 257, 70000, U]))
        draw = lambda: None if rng.random() < 0.2 else np.where(rng.random(n) < 0.3, U, rng.integers(0, top, size=n)).astype(np.uint32)
        dl, el = draw(), draw()
        assert run_shim(shim, dl, el) == restate(dl, el)


def test_standalone_program_under_sanitizers(tmp_path):
    """The same planner over the same kind of cases in a program of its own, with AddressSanitizer and UBSan: exact-size heap
    arrays, so a read past an end aborts the program."""
    exe = tmp_path / "label_plan_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", *INCLUDES, os.path.join(REPO, "tests", "label_plan_main.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "label plan ok" in out.stdout, out.stdout + out.stderr
