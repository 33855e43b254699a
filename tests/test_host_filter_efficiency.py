"""SelectNodeResult::efficiency of the host mirror's driver Filters (host/extender.cpp -> gf_filter_efficiency): a Filter with two
earlier drivers through the string route, the flat route and the group route reports the cluster-wide average packing efficiency
against the chain's residual, bit for bit what the host computes from gf_packing_efficiencies' rows in the summation tree of
include/gangfit.h.  The C++ program host/tests/host_filter_efficiency_test.cpp does the checking; this file runs it the way
test_host_cluster_scan_sets.py runs host_cluster_scan_sets_test: `cpu` needs no GPU, `gpu` drives the device through the C ABI."""
import pytest

from gangfit import build
from host_programs import _run


def test_filter_efficiency_cpu_half():
    out = _run(build.HOST_FILTER_EFFICIENCY_TEST_PATH, "cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_filter_efficiency_through_the_device():
    out = _run(build.HOST_FILTER_EFFICIENCY_TEST_PATH, "gpu")
    assert "gpu:" in out
