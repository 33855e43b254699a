"""The executor Filter answered from the resident cluster (host/extender.cpp::rescheduleExecutorFlat -> gf_cluster_executor_fit):
the same node, outcome and error as rescheduleExecutor on the reference's dynamic-allocation and minimal-fragmentation scenarios
and on a zoned cluster with overhead and reservations, a refused call falls back, and the driver Filter after it resumes.  The
C++ program host/tests/host_executor_resident_test.cpp does the checking; this file runs it the way test_host_cluster_scan.py
runs host_cluster_scan_test: `cpu` needs no GPU, `gpu` drives the device through the C ABI."""
import os
import subprocess

import pytest

from gangfit import build


def _binary():
    build.build_native()
    build.build_host()
    assert os.path.exists(build.HOST_EXECUTOR_RESIDENT_TEST_PATH), "host_executor_resident_test was not built"
    return build.HOST_EXECUTOR_RESIDENT_TEST_PATH


def _run(mode):
    p = subprocess.run([_binary(), mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and " 0 failed" in p.stdout, p.stdout[-4000:]
    return p.stdout


def test_executor_resident_cpu_half():
    out = _run("cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_resident_executor_filter_through_the_device():
    out = _run("gpu")
    assert "gpu:" in out
