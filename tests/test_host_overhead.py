"""The flat Filter route on a cluster with overhead (host/extender.cpp::selectDriverNodeFlat): the overhead columns stay
resident, a Filter sends the rows that changed (gf_overhead_update) and every answer is the one the string-keyed route gives.
The C++ program host/tests/host_overhead_test.cpp does the checking; this file runs it the way test_host_mirror.py runs
host_test: `cpu` needs no GPU (the row diff against a brute-force compare), `gpu` drives the device through the C ABI."""
import pytest

from gangfit import build
from host_programs import _run


def test_overhead_row_diff_cpu_half():
    out = _run(build.HOST_OVERHEAD_TEST_PATH, "cpu")
    assert "cpu:" in out


@pytest.mark.gpu
def test_filters_with_overhead_through_the_device():
    out = _run(build.HOST_OVERHEAD_TEST_PATH, "gpu")
    assert "gpu:" in out
