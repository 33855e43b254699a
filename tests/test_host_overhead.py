"""The flat Filter route on a cluster with overhead (host/extender.cpp::selectDriverNodeFlat): the overhead columns stay
resident, a Filter sends the rows that changed (gf_overhead_update) and every answer is the one the string-keyed route gives.
The C++ program host/tests/host_overhead_test.cpp does the checking; this file runs it the way test_host_mirror.py runs
host_test: `cpu` needs no GPU (the row diff against a brute-force compare), `gpu` drives the device through the C ABI."""
import os
import subprocess

import pytest

from gangfit import build


def _binary():
    build.build_native()
    build.build_host()
    assert os.path.exists(build.HOST_OVERHEAD_TEST_PATH), "host_overhead_test was not built"
    return build.HOST_OVERHEAD_TEST_PATH


def _run(mode):
    p = subprocess.run([_binary(), mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and " 0 failed" in p.stdout, p.stdout[-4000:]
    return p.stdout


def test_overhead_row_diff_cpu_half():
    out = _run("cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_filters_with_overhead_through_the_device():
    out = _run("gpu")
    assert "gpu:" in out
