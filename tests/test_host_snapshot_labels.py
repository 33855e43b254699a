"""gf_snapshot_build with a prioritized node label against the string-keyed host mirror of NodeSorter.PotentialNodes, and the route
the build reports (gf_snapshot_build_info).  The C++ program host/tests/host_snapshot_labels_test.cpp does the checking; this
file runs it the way test_host_mirror.py runs host_test: `cpu` needs no GPU (the mirror's lists for drivers confined to one label
value share one order), `gpu` drives the device through the C ABI."""
import os
import subprocess

import pytest

from gangfit import build


def _binary():
    build.build_native()
    build.build_host()
    assert os.path.exists(build.HOST_SNAPSHOT_LABELS_TEST_PATH), "host_snapshot_labels_test was not built"
    return build.HOST_SNAPSHOT_LABELS_TEST_PATH


def _run(mode):
    p = subprocess.run([_binary(), mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and " 0 failed" in p.stdout, p.stdout[-4000:]
    return p.stdout


def test_confined_lists_share_one_order_cpu_half():
    out = _run("cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_labelled_builds_report_their_route_through_the_device():
    out = _run("gpu")
    assert "gpu:" in out and "confined drivers: route 1" in out
