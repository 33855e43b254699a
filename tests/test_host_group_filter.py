"""Driver Filters of several instance groups on one resident cluster (host/extender.cpp::selectDriverNodeFlatGroup ->
gf_snapshot_build_resident_set): the Filters of three groups alternate, an all-groups scan and an executor Filter run in between,
every answer equals selectDriverNode on that group's nodes, gf_cluster_set is sent once and the same group's Filter twice in a row
rebuilds nothing.  The C++ program host/tests/host_group_filter_test.cpp does the checking; this file runs it the way
test_host_cluster_scan_sets.py runs host_cluster_scan_sets_test: `cpu` needs no GPU, `gpu` drives the device through the C ABI."""
import pytest

from gangfit import build
from host_programs import _run


def test_group_filter_cpu_half():
    out = _run(build.HOST_GROUP_FILTER_TEST_PATH, "cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_group_filters_through_the_device():
    out = _run(build.HOST_GROUP_FILTER_TEST_PATH, "gpu")
    assert "gpu:" in out
