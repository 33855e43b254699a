"""tests/cluster_executor_cases.py against what it promises (no GPU): the helper reproduces the reference's dynamic-allocation
cases of tests/test_executor_fit.py (resource_test.go:172-372), each constructed case has two candidate answers that really
differ, and the random generator makes the oracle answer both ways at every size."""
import numpy as np
import pytest

import cluster_executor_cases as xc
from oracle import binding as ob
from oracle import pysnapshot as ps
from test_executor_fit import T2_CASES, T2_ZONE


@pytest.mark.parametrize("name,avail,order,want", T2_CASES, ids=[c[0] for c in T2_CASES])
def test_the_helper_reproduces_the_reference_dynamic_allocation_cases(name, avail, order, want):
    c = xc._plain(avail)
    if name == "same AZ as the application":  # resource_test.go:262-292: the zone step narrows the candidates to zone2 = {node2}
        kw = dict(node_zone=T2_ZONE["node_zone"], req_zone=[T2_ZONE["app_zone"]])
    else:  # the order the case states is the one the helper's snapshot produces
        kw = {}
        assert ps.build(c["alloc"], c["flags"], c["name_rank"])[3].tolist() == order
    assert xc.expected(c, None, None, None, None, [[1000, 1, 0]], **kw) == [want]


def test_the_same_az_case_answers_per_zone():
    c = xc._plain(T2_ZONE["avail"])
    got = xc.expected(c, None, None, None, None, [[1000, 1, 0]] * 4, node_zone=T2_ZONE["node_zone"], req_zone=[1, 0, xc.ANY, 7])
    assert got == [1, 0, 0, xc.NO]  # zone2 -> node2; zone1 -> node1; anywhere -> node1; an empty zone: failure-fit


@pytest.mark.parametrize("case", xc.CONSTRUCTED, ids=[f.__name__ for f in xc.CONSTRUCTED])
def test_constructed_cases_have_two_answers_that_differ(case):
    c, res_node, res_req, kw, right, wrong = case()
    assert right != wrong
    assert xc.expected(c, res_node, res_req, **kw) == [right]


def test_subset_zone_ranks_the_other_answer_is_the_filtered_full_order():
    c, _, _, kw, right, wrong = xc.case_subset_zone_ranks()
    avail, _, _, X = ps.build(c["alloc"], c["flags"], c["name_rank"], zone=c["zone"], n_zones=c["n_zones"])
    assert X.tolist() == [2, 0, 1]
    filtered = [x for x in X.tolist() if kw["sets"][0][x]]
    assert ob.executor_fit(avail, kw["exe"][0], filtered) == wrong


def test_zero_valued_entry_the_other_answer_is_what_the_sums_say():
    c, res_node, res_req, kw, right, wrong = xc.case_zero_valued_entry()
    assert not res_req.any()
    assert xc.expected(c, None, None, **kw) == [wrong]  # without the entry the overhead counts once
    avail = c["alloc"] - c["overhead"]
    assert (avail[0] >= kw["exe"][0]).all() and not (avail[0] - c["overhead"][0] >= kw["exe"][0]).all()


def test_hosting_beats_capacity_the_other_answer_is_without_the_hint():
    c, _, _, kw, right, wrong = xc.case_hosting_beats_capacity()
    assert xc.expected(c, None, None, **dict(kw, hosts=None)) == [wrong]
    assert ob.node_capacity(c["alloc"][0], [0, 0, 0], kw["exe"][0]) > ob.node_capacity(c["alloc"][1], [0, 0, 0], kw["exe"][0])


@pytest.mark.parametrize("zones", xc.ZONE_CONFIGS)
@pytest.mark.parametrize("n", xc.NODE_COUNTS)
def test_the_generator_answers_both_ways(n, zones):
    seed = 1000 * n + xc.ZONE_CONFIGS.index(zones)
    c = xc.cluster(seed, n, zones)
    exe = xc.requests(seed)
    for mf in (False, True):
        got = np.array(xc.expected(c, c["res_node"], c["res_req"], None, None, exe, minimal_fragmentation=mf), dtype=np.uint64)
        assert (got == xc.NO).any() and (got != xc.NO).any(), (n, zones, mf)
        assert (got[got != xc.NO] < n).all()
    assert (c["res_node"] >= n).any() or n < 20  # entries outside the cluster
    assert not c["res_req"][c["res_node"] < n].any(axis=1).all()  # entries of all zeros on nodes of the cluster


def test_entries_outside_the_set_do_not_count():
    """An entry names n1 only: restricted to {n0}, n0 carries no reservation and its overhead counts once."""
    c, _, _, kw, _, _ = xc.case_zero_valued_entry()
    sets = np.array([[1, 0]], dtype=bool)
    assert xc.expected(c, [1], [[0, 0, 0]], sets, [0], kw["exe"]) == [0]
    assert xc.expected(c, [0], [[0, 0, 0]], sets, [0], kw["exe"]) == [xc.NO]
