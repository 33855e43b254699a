"""Driver Filters of several instance groups on one resident cluster (host/extender.cpp::selectDriverNodeFlatGroup ->
gf_snapshot_build_resident_set): the Filters of three groups alternate, an all-groups scan and an executor Filter run in between,
every answer equals selectDriverNode on that group's nodes, gf_cluster_set is sent once and the same group's Filter twice in a row
rebuilds nothing.  The C++ program host/tests/host_group_filter_test.cpp does the checking; this file runs it the way
test_host_cluster_scan_sets.py runs host_cluster_scan_sets_test: `cpu` needs no GPU, `gpu` drives the device through the C ABI."""
import os
import subprocess

import pytest

from gangfit import build


def _binary():
    build.build_native()
    build.build_host()
    assert os.path.exists(build.HOST_GROUP_FILTER_TEST_PATH), "host_group_filter_test was not built"
    return build.HOST_GROUP_FILTER_TEST_PATH


def _run(mode):
    p = subprocess.run([_binary(), mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and " 0 failed" in p.stdout, p.stdout[-4000:]
    return p.stdout


def test_group_filter_cpu_half():
    out = _run("cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_group_filters_through_the_device():
    out = _run("gpu")
    assert "gpu:" in out
