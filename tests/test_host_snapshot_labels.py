"""gf_snapshot_build with a prioritized node label against the string-keyed host mirror of NodeSorter.PotentialNodes, and the route
the build reports (gf_snapshot_build_info).  The C++ program host/tests/host_snapshot_labels_test.cpp does the checking; this
file runs it the way test_host_mirror.py runs host_test: `cpu` needs no GPU (the mirror's lists for drivers confined to one label
value share one order), `gpu` drives the device through the C ABI."""
import pytest

from gangfit import build
from host_programs import _run


def test_confined_lists_share_one_order_cpu_half():
    out = _run(build.HOST_SNAPSHOT_LABELS_TEST_PATH, "cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_labelled_builds_report_their_route_through_the_device():
    out = _run(build.HOST_SNAPSHOT_LABELS_TEST_PATH, "gpu")
    assert "gpu:" in out and "confined drivers: route 1" in out
