"""The round arithmetic of the resident worker (csrc/gangfit_worker_rounds.h) against the literal per-lane definition, restated in
Python, on the CPU: the header is pure code, so a small extern "C" shim (tests/worker_rounds_shim.cpp) compiled with g++ is all it
takes — no HIP, no libgangfit.so.

The definition (gangfit_worker.inc): in round `round` workgroup bs of a set of blocks_per_set workgroups acts as workgroup
bsr = (bs + round) mod blocks_per_set; lane l < 16 of it owns the applications f = 16 bsr + l, f + app_stride, ... below n_apps,
app_stride = 16 blocks_per_set: cnt_l = (n_apps - 1 - f) // app_stride + 1 of them (0 when f >= n_apps).  share = the sum of cnt_l;
total = 16 cnt_0 hand-out positions; position i is application f0 + i mod 16 + (i div 16) app_stride."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = ctypes.c_uint32


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("worker_rounds") / "worker_rounds_shim.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", os.path.join(REPO, "k8s-spark-scheduler_amd", "csrc"),
                           os.path.join(REPO, "tests", "worker_rounds_shim.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    for f in (lib.wr_stride_div, lib.wr_div, lib.wr_walk, lib.wr_round, lib.wr_app_index):
        f.restype = None
    lib.wr_wave_of_round.restype = U32
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _n_apps_values(app_stride):
    return np.concatenate([np.arange(0, 2 * app_stride + 18), [1000, 10000]]).astype(np.int64)


def test_walked_rotation_is_the_defined_one(shim):
    for bps in range(1, 49):
        n_rounds = 2 * bps + 2
        for bs in range(bps):
            walked, defined, f0 = (np.zeros(n_rounds, np.uint32) for _ in range(3))
            shim.wr_walk(U32(bps), U32(bs), U32(n_rounds), _p(walked), _p(defined), _p(f0))
            want = (bs + np.arange(n_rounds)) % bps
            assert np.array_equal(walked, want) and np.array_equal(defined, want), (bps, bs)
            assert np.array_equal(f0, 16 * want), (bps, bs)
    for wave in range(16):
        for rnd in (0, 1, 15, 16, 17, 31, 1000, 2**32 - 1):
            assert shim.wr_wave_of_round(U32(wave), U32(rnd)) == (wave + rnd) % 16


def test_total_and_share_are_the_per_lane_sums(shim):
    lanes = np.arange(16, dtype=np.int64)
    for bps in range(1, 49):
        stride = 16 * bps
        n_rounds = 2 * bps + 2
        walked, defined, f0r = (np.zeros(n_rounds, np.uint32) for _ in range(3))
        shim.wr_walk(U32(bps), U32(0), U32(n_rounds), _p(walked), _p(defined), _p(f0r))  # workgroup 0 meets every bsr, twice
        napps = _n_apps_values(stride)
        F0, N = np.meshgrid(f0r.astype(np.int64), napps, indexing="ij")
        F0, N = F0.ravel(), N.ravel()
        f = F0[:, None] + lanes[None, :]
        cnt = np.where(f < N[:, None], (N[:, None] - 1 - f) // stride + 1, 0)
        want_share = cnt.sum(axis=1)
        want_total = 16 * cnt[:, 0]
        total, share = np.zeros(len(N), np.uint32), np.zeros(len(N), np.uint32)
        f0_u, n_u = _u32(F0), _u32(N)
        shim.wr_round(U32(bps), U32(len(N)), _p(f0_u), _p(n_u), _p(total), _p(share))
        assert np.array_equal(total, want_total), bps
        assert np.array_equal(share, want_share), bps
        # every workgroup's share adds up to the ticket (the completion count of the ticket)
        per_ticket = want_share.reshape(n_rounds, len(napps))[:bps].sum(axis=0)
        assert np.array_equal(per_ticket, napps), bps


def test_app_index_is_lane_of_row(shim):
    for bps in range(1, 49):
        stride = 16 * bps
        for f0 in sorted({0, 16 * (bps // 2), 16 * (bps - 1)}):
            i = _u32(np.arange(0, 16 * 700 // bps + 48))  # past the rows of a 10 000-application ticket
            a = np.zeros(len(i), np.uint32)
            shim.wr_app_index(U32(bps), U32(f0), U32(len(i)), _p(i), _p(a))
            ii = i.astype(np.int64)
            assert np.array_equal(a, f0 + ii % 16 + (ii // 16) * stride), (bps, f0)
    # the positions below total that name an application below n_apps are exactly the workgroup's applications, each once
    for bps, f0, n in ((1, 0, 17), (3, 16, 101), (5, 64, 165), (21, 320, 1000), (48, 0, 10000)):
        stride = 16 * bps
        total, share = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        shim.wr_round(U32(bps), U32(1), _p(_u32([f0])), _p(_u32([n])), _p(total), _p(share))
        i = _u32(np.arange(int(total[0])))
        a = np.zeros(len(i), np.uint32)
        shim.wr_app_index(U32(bps), U32(f0), U32(len(i)), _p(i), _p(a))
        mine = sorted(int(x) for x in a if x < n)
        want = sorted(x for x in range(n) if (x % stride) // 16 == f0 // 16)
        assert mine == want and len(mine) == int(share[0]), (bps, f0, n)


def test_the_multiplier_divides_exactly(shim):
    for b in range(1, 257):
        stride = 16 * b
        md = (U32 * 2)()
        shim.wr_stride_div(U32(b), md)
        assert md[0] <= 2**29 + 1 and 28 <= md[1] <= 36, (b, md[0], md[1])
        mult = np.arange(0, 2**20 + stride, stride, dtype=np.int64)
        nums = np.concatenate([[0], mult - 1, mult, mult + 1, [2**31 - 1, 2**31, 2**31 + 1, 2**32 - 1]])
        nums = np.unique(nums[(nums >= 0) & (nums < 2**32)])
        q = np.zeros(len(nums), np.uint32)
        nums_u = _u32(nums)
        shim.wr_div(U32(b), U32(len(nums)), _p(nums_u), _p(q))
        assert np.array_equal(q.astype(np.int64), nums // stride), b
