"""The executor Filter answered from the resident cluster (host/extender.cpp::rescheduleExecutorFlat -> gf_cluster_executor_fit):
the same node, outcome and error as rescheduleExecutor on the reference's dynamic-allocation and minimal-fragmentation scenarios
and on a zoned cluster with overhead and reservations, a refused call falls back, and the driver Filter after it resumes.  The
C++ program host/tests/host_executor_resident_test.cpp does the checking; this file runs it the way test_host_cluster_scan.py
runs host_cluster_scan_test: `cpu` needs no GPU, `gpu` drives the device through the C ABI."""
import pytest

from gangfit import build
from host_programs import _run


def test_executor_resident_cpu_half():
    out = _run(build.HOST_EXECUTOR_RESIDENT_TEST_PATH, "cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_resident_executor_filter_through_the_device():
    out = _run(build.HOST_EXECUTOR_RESIDENT_TEST_PATH, "gpu")
    assert "gpu:" in out
