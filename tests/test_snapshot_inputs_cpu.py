"""tests/snapshot_inputs.py keeps its promises (no GPU): every merged-layout problem of tests/magnitudes.py, as inputs of the
snapshot build, is admissible for gf_snapshot_build and replays — through the numpy restatement oracle/pysnapshot.py — to
exactly the availabilities the problem was drawn for."""
import numpy as np
import pytest

import magnitudes as mg
import snapshot_inputs as si
from oracle import pysnapshot as ps


def _merged_cases(regime):
    return [(name, p) for name, p, _ in mg.cases(regime) if "merged" in name]


def test_there_are_twenty_merged_cases():
    assert sum(len(_merged_cases(r)) for r in mg.REGIMES) == 20


@pytest.mark.parametrize("candidates", si.CANDIDATES)
@pytest.mark.parametrize("regime", mg.REGIMES)
def test_build_inputs_replay_to_the_problem(regime, candidates):
    for name, p in _merged_cases(regime):
        where = f"{regime} {name} {candidates}"
        c = si.as_build_inputs(p, np.random.default_rng(0), candidates)
        n = len(p[0])
        # 1. the restatement gives back the clamped tables, exactly
        want_avail = np.maximum(p[0], -(mg.QMAX - 1))
        want_sched = np.maximum(np.maximum(p[1], want_avail), 0)
        lowered = want_sched - want_avail > 2 * si.ENTRY_MAX
        want_sched = np.where(lowered, np.maximum(want_avail, 0), want_sched)
        avail, sched, D, X = ps.build(**c)
        assert np.array_equal(avail, want_avail) and np.array_equal(sched, want_sched), where
        a2, s2 = si.tables(p)
        assert np.array_equal(a2, want_avail) and np.array_equal(s2, want_sched), where
        # 2. the availabilities are the problem's own but for -QMAX (which no two entries below 2^61 reach)
        changed = avail != p[0]
        assert (p[0][changed] == -mg.QMAX).all(), where
        assert int(changed.sum()) <= (4 if regime == "huge" else 0), where
        assert avail.max() <= mg.QMAX and avail.min() >= -(mg.QMAX - 1), where
        # what gf_cluster_set and check_reservations (gangfit_api_snapshot.cpp) admit
        assert c["overhead"] is None and c["alloc"].min() >= 0 and c["alloc"].max() <= mg.QMAX, where
        assert len(c["res_node"]) == len(c["res_req"]) and c["res_node"].max(initial=0) < n, where
        assert c["res_req"].min(initial=0) >= 0 and c["res_req"].max(initial=0) <= si.ENTRY_MAX, where
        per_node = np.bincount(c["res_node"], minlength=n)
        assert per_node.max(initial=0) <= 2, where
        assert per_node.max(initial=0) * int(c["res_req"].max(initial=0)) < 1 << 62, where
        # the zones travel as they are: sparse ids, the empty ones in between declared
        assert np.array_equal(c["zone"], p[2]) and c["n_zones"] == int(p[2].max()) + 1, where
        assert sorted(c["name_rank"].tolist()) == list(range(n)), where
        full = ps.READY | ps.DRIVER_CANDIDATE
        assert (c["node_flags"][:si.EDGE_NODES] == full).all(), where
        if candidates == "all":
            assert (c["node_flags"] == full).all() and len(D) == n and np.array_equal(D, X), where
        else:
            assert 0 < len(D) < n and 0 < len(X) < n, where


def test_huge_reaches_the_entry_limit():
    """The largest entry the conversion hands to the build is 2^61 - 1, the largest one it admits: the huge regime gets there."""
    top = 0
    for name, p in _merged_cases("huge"):
        c = si.as_build_inputs(p, np.random.default_rng(0), "all")
        top = max(top, int(c["res_req"].max()))
    assert top == si.ENTRY_MAX
