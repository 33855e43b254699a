"""The failover reconciler's findNodes for every instance group answered from the resident cluster
(host/failover.cpp::findNodesForStaleApplicationsResident -> gf_cluster_find_nodes): the rows and create_rank the mirror builds
for a three-group cluster name the reference's per-group node lists; on a device the resident reconcile of three groups equals the
per-group route and a literal map-keyed findNodes (names, `reserved`, availableResources afterwards), a refused call falls back,
and the driver Filter behind the resident reconcile resumes.  The C++ program host/tests/host_cluster_find_nodes_test.cpp does the
checking; this file runs it the way test_host_executor_resident.py runs its program: `cpu` needs no GPU, `gpu` drives the device
through the C ABI."""
import pytest

from gangfit import build
from host_programs import _run


def test_cluster_find_nodes_cpu_half():
    out = _run(build.HOST_CLUSTER_FIND_NODES_TEST_PATH, "cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_resident_reconcile_through_the_device():
    out = _run(build.HOST_CLUSTER_FIND_NODES_TEST_PATH, "gpu")
    assert "gpu:" in out
