"""The UnschedulablePodMarker's whole minute in one call (host/extender.cpp::scanForUnschedulablePodsAllGroups ->
gf_cluster_fit_feasible_sets): three instance groups plus a pod of a group nobody names give the same (pod, exceeds) list as one
scanForUnschedulablePods per group merged in listing order; the resident route answers after a flat Filter and not before one;
gf_generation stays.  The C++ program host/tests/host_cluster_scan_sets_test.cpp does the checking; this file runs it the way
test_host_cluster_scan.py runs host_cluster_scan_test: `cpu` needs no GPU, `gpu` drives the device through the C ABI."""
import pytest

from gangfit import build
from host_programs import _run


def test_cluster_scan_sets_cpu_half():
    out = _run(build.HOST_CLUSTER_SCAN_SETS_TEST_PATH, "cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_all_groups_scan_through_the_device():
    out = _run(build.HOST_CLUSTER_SCAN_SETS_TEST_PATH, "gpu")
    assert "gpu:" in out
