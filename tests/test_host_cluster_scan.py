"""The UnschedulablePodMarker's scan next to the Filter's installed snapshot (host/extender.cpp::scanForUnschedulablePodsResident
-> gf_cluster_fit_feasible): the same (pod, exceeds) list as scanForUnschedulablePods on the scenarios of the reference's
unschedulablepods_test.go and on a zoned cluster with overhead and a node selection, the Filter after it resumes, a refused
question falls back.  The C++ program host/tests/host_cluster_scan_test.cpp does the checking; this file runs it the way
test_host_overhead.py runs host_overhead_test: `cpu` needs no GPU, `gpu` drives the device through the C ABI."""
import pytest

from gangfit import build
from host_programs import _run


def test_cluster_scan_cpu_half():
    out = _run(build.HOST_CLUSTER_SCAN_TEST_PATH, "cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_resident_scan_through_the_device():
    out = _run(build.HOST_CLUSTER_SCAN_TEST_PATH, "gpu")
    assert "gpu:" in out
