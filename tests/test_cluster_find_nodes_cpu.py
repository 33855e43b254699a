"""tests/cluster_find_nodes_cases.py against what it promises (no GPU): `expected` equals the dict-shaped restatement of the
reconciler's loop (oracle.pyoracle.find_nodes_chain) on every case, and no family of cases can pass vacuously — each holds a
request that is filled, one that ends partial, an over-add on a full node, a visit of a node whose available was already
negative, and a request whose chained answer differs from its unchained one."""
import numpy as np
import pytest

import cluster_find_nodes_cases as fc
from oracle import pyoracle as po


def _dict_shaped(c, chained):
    """(names per request, reserved per request in units of exe, table afterwards) through the reference's map shapes"""
    A = fc.available(c)
    n = len(A)
    exe = [[int(v) for v in e] for e in c["exe"]]
    k = [int(v) for v in c["k"]]
    table = {str(i): [int(v) for v in a] for i, a in enumerate(A)}
    names, reserved = [None] * len(k), [None] * len(k)
    for member, qs in fc.groups(c):
        O = [str(int(x)) for x in fc.order_of(c, member)]
        if chained:
            got = po.find_nodes_chain([(k[q], exe[q]) for q in qs], table, O)
        else:
            got = [po.find_nodes(k[q], exe[q], {s: list(v) for s, v in table.items()}, O) if k[q] > 0 else ([], {}) for q in qs]
        for q, (nm, rs) in zip(qs, got):
            names[q], reserved[q] = [int(s) for s in nm], rs
    return names, reserved, [table[str(i)] for i in range(n)]


def _hold(c):
    for chained in (True, False):
        want = fc.expected(c, chained=chained)
        names, reserved, after = _dict_shaped(c, chained)
        for q in range(len(c["k"])):
            o = int(want["off"][q])
            assert names[q] == want["exec_nodes"][o:o + int(want["placed"][q])].tolist(), (q, chained)
            e = [int(v) for v in c["exe"][q]]
            for node in np.nonzero(want["adds"][q])[0]:
                assert reserved[q][str(int(node))] == [int(want["adds"][q, node]) * v for v in e], (q, int(node), chained)
            assert len(reserved[q]) == int(np.count_nonzero(want["adds"][q])), (q, chained)  # no entry behind the last node
            hit = [int(s) for s in reserved[q]]
            assert int(want["last"][q]) == (hit[-1] if hit else fc.NO), (q, chained)  # (a dict keeps insertion order)
        assert after == want["residual"].tolist(), chained


@pytest.mark.parametrize("n", fc.NODE_COUNTS)
@pytest.mark.parametrize("family", fc.FAMILIES)
def test_expected_equals_the_dict_shaped_restatement(family, n):
    for rank_kind in fc.RANKS:
        _hold(fc.case(family, n, rank_kind))


def test_expected_equals_the_dict_shaped_restatement_on_the_two_single_cases():
    _hold(fc.case_k_max())
    _hold(fc.case_big())


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_no_family_can_pass_vacuously(family):
    have = set()
    for n in fc.NODE_COUNTS:
        for rank_kind in fc.RANKS:
            have |= fc.kinds_present(fc.case(family, n, rank_kind))
    assert have == fc.ALL_KINDS, fc.ALL_KINDS - have


def test_every_size_above_one_node_holds_every_kind():
    """... and not only the family as a whole: from 63 nodes on, every single case does."""
    for family in fc.FAMILIES:
        for n in fc.NODE_COUNTS[1:]:
            c = fc.case(family, n, "random")
            assert fc.kinds_present(c) == fc.ALL_KINDS, (family, n, fc.ALL_KINDS - fc.kinds_present(c))


def test_the_cases_hold_what_the_issue_lists():
    c = fc.case("eight", 300, "random")
    assert len(c["sets"]) == 10 and not c["sets"][8].any()  # eight scattered rows, an empty one, one without a ready node
    assert c["sets"][9].any() and len(fc.order_of(c, c["sets"][9])) == 0
    assert (c["sets"].sum(axis=0) <= 1).all()  # disjoint: what a chained call demands
    assert sorted(c["create_rank"].tolist()) == list(range(300))
    assert (fc.available(c) < 0).any()
    counts = np.bincount(c["req_set"], minlength=10)
    assert counts[:8].min() >= 1 and counts[:8].max() <= 12 and counts[8] == 2 and counts[9] == 1
    assert len(set(np.diff(c["req_set"].astype(np.int64)).tolist())) > 2  # interleaved across rows in q
    assert (c["k"] == 0).any() and (c["k"] == 1).any()
    assert (np.asarray(c["exe"]) == [0, 0, 1]).all(axis=1).any() and (np.asarray(c["exe"]) == 0).all(axis=1).any()
    assert ((c["k"].astype(np.int64) + 1) * np.asarray(c["exe"]).max(axis=1) < (1 << 62)).all()
    km = fc.case_k_max()
    assert km["k"][0] == fc.MAX_K and not km["exe"][0].any()
    want = fc.expected(km)
    assert want["placed"][0] == fc.MAX_K and len(set(want["exec_nodes"][: fc.MAX_K].tolist())) == 1  # clamps at K on one node
