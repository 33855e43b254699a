"""Node rows of the resident cluster changed in place, through the host mirror (host/extender.cpp: FlatCluster::BuildWithSpare /
Rebuild, and syncResident's gf_cluster_update route).  The C++ program host/tests/host_cluster_update_test.cpp does the checking:
`cpu` holds Rebuild to a brute-force restatement (stable indices over join, leave and rejoin, ranks, rows_out, the carried-entry
rule, spare exhaustion, a changed zone label set) and needs no GPU; `gpu` runs group Filters, a marker scan, an executor Filter and
a reconcile across node join, leave, cordon and resize against a fresh extender on a fresh Build, and reads the counters: one
gf_cluster_set, one usage replay."""
import pytest

from gangfit import build
from host_programs import _run


def test_rebuild_against_the_restatement_cpu_half():
    out = _run(build.HOST_CLUSTER_UPDATE_TEST_PATH, "cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_node_changes_through_the_device():
    out = _run(build.HOST_CLUSTER_UPDATE_TEST_PATH, "gpu")
    assert "gpu:" in out
