"""Zone facts built on the device (gangfit_snapshot.hip): the zone sums of metadata_kernel, the zone ranks (the priority sort's own
ranking up to 64 declared zones, zone_rank_kernel past that), the first-driver-slot / has-an-executor facts of
finalize_slots_kernel (combined in LDS up to kZoneLdsMax = 512 declared zones, global atomics past that), the evaluation list of
finalize_reduce_kernel and the per-zone masks of finalize_narrow_zones_kernel — at the declared zone counts where those paths
change, with few populated zones at sparse ids.  Against oracle/pysnapshot.build and the oracle's decisions on the restated
snapshot, under both finalize settings.  The oracle binding takes zone ids as they are (oracle/gangfit_oracle.c collects the
zones it sees): nothing is relabelled for it.  `python -m pytest tests/test_gpu_snapshot_zones.py -m gpu`."""
import numpy as np
import pytest

import gangfit
import stress_lib
from gangfit import workloads as wl
from oracle import binding as ob
from oracle import pysnapshot as ps
from test_snapshot_build import _cluster

IND, FIFO = gangfit.GF_MODE_INDEPENDENT, gangfit.GF_MODE_FIFO_CHAIN
PACKERS = (0, 3, 4, 5)
SIZES = (130, 1000)                  # three chunks | sixteen, the last one ragged in both
DECLARED = (64, 65, 512, 513, 4096)  # 64 | 65: the sort ranks the zones itself | zone_rank_kernel; 512 | 513: kZoneLdsMax
SCALARS_ONLY = 512
FULL = ps.READY | ps.DRIVER_CANDIDATE


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _zoned_cluster(n, nz):
    """The cluster of test_snapshot_build._cluster with six populated zones among nz declared ones.  Returns (inputs, ids):
      t1, t2   twins: t2's nodes are copies of t1's (allocatable, overhead, reservations), so the two zones have equal free
               memory and cpu sums and the zone id decides; ids 0 and 63 (64 declared zones) or 64 (more)
      last     about 40 % of the nodes, so it ranks last; its only driver candidate is the last node of the whole order
      d_only   driver candidates only      x_only   executor candidates only      none   neither
    d_only, x_only and none must be absent from the evaluation list."""
    c = _cluster(7000 + n + nz, n, min(n, 300), 1)
    rng = np.random.default_rng(31 * n + nz)
    high = 63 if nz == 64 else 64
    rest = [z for z in (nz - 1, 1, 2, 5, 7) if z not in (0, high)][:4]
    ids = dict(t1=0, t2=high, last=rest[0], d_only=rest[1], x_only=rest[2], none=rest[3])
    nt, small = n * 15 // 100, n // 10
    cuts = np.cumsum([nt, nt, small, small, small])
    t1, t2, d_only, x_only, none, last = np.split(rng.permutation(n), cuts)
    zone = np.empty(n, dtype=np.uint32)
    for name, nodes in (("t1", t1), ("t2", t2), ("d_only", d_only), ("x_only", x_only), ("none", none), ("last", last)):
        zone[nodes] = ids[name]
    alloc, over = c["alloc"].copy(), c["overhead"].copy()
    alloc[t2], over[t2] = alloc[t1], over[t1]
    partner = np.full(n + 3, -1, dtype=np.int64)
    partner[t1] = t2
    keep = ~np.isin(c["res_node"], t2)
    res_node, res_req = c["res_node"][keep], c["res_req"][keep]
    twin = partner[res_node] >= 0
    res_node = np.concatenate([res_node, partner[res_node[twin]].astype(np.uint32)])
    res_req = np.concatenate([res_req, res_req[twin]])
    f = c["node_flags"].copy()
    f[d_only] &= ~np.uint32(ps.READY)
    f[d_only[0]] |= ps.DRIVER_CANDIDATE
    f[x_only] &= ~np.uint32(ps.DRIVER_CANDIDATE)
    f[x_only[0]] = ps.READY
    f[none] = rng.choice([0, ps.UNSCHEDULABLE, ps.UNSCHEDULABLE | ps.READY], size=len(none)).astype(np.uint32)
    f[last] &= ~np.uint32(ps.DRIVER_CANDIDATE)
    f[t1[0]] = f[t2[0]] = FULL
    c = dict(c, alloc=alloc, overhead=over, res_node=res_node, res_req=res_req, zone=zone, n_zones=nz, node_flags=f)
    order = ps.build(**dict(c, node_flags=np.full(n, FULL, dtype=np.uint32)))[2]  # every node: the priority order itself
    f[order[-1]] = FULL
    return c, ids


def _check_promises(n, nz, c, ids, ref):
    avail, sched, D, X = ref
    zone = c["zone"]
    order = ps.build(**dict(c, node_flags=np.full(n, FULL, dtype=np.uint32)))[2]
    assert len(set(ids.values())) == 6 and max(ids.values()) < nz
    assert {0, 63 if nz == 64 else 64, nz - 1} <= set(ids.values())
    assert sorted(set(zone.tolist())) == sorted(ids.values())
    for j in (0, 1):  # the twins tie on (free memory, free cpu): the zone id decides
        assert avail[zone == ids["t1"], j].sum() == avail[zone == ids["t2"], j].sum()
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    assert pos[zone == ids["t1"]].max() < pos[zone == ids["t2"]].min()  # whole zones, lower id first
    dz, xz = set(zone[D].tolist()), set(zone[X].tolist())
    assert dz & xz == {ids["t1"], ids["t2"], ids["last"]}
    assert ids["d_only"] in dz - xz and ids["x_only"] in xz - dz and ids["none"] not in dz | xz
    in_last = D[zone[D] == ids["last"]]
    assert len(in_last) == 1 and pos[in_last[0]] == n - 1 and n % 64 != 0  # alone, in the ragged last chunk
    assert (sched >= 0).all()


_REFS = {}


def _case(n, nz):
    if (n, nz) not in _REFS:
        c, ids = _zoned_cluster(n, nz)
        ref = ps.build(**c)
        avail, sched, D, X = ref
        w = wl.config(2, n_nodes=16, n_apps=64)
        flags = np.ones(len(w.k), dtype=np.uint32)
        oapps = ob.make_apps(w.drv, w.exe, w.k, flags)
        refs = {algo: (ob.fit_independent(algo, avail, oapps, D, X, sched=sched, zone=c["zone"]),
                       ob.fit_fifo_chain(algo, avail, oapps, D, X, sched=sched, zone=c["zone"])) for algo in PACKERS}
        _REFS[(n, nz)] = (c, ids, ref, gangfit.make_apps(w.drv, w.exe, w.k, flags), refs)
    return _REFS[(n, nz)]


@pytest.mark.parametrize("nz", DECLARED)
@pytest.mark.parametrize("n", SIZES)
def test_clusters_hold_what_they_promise(n, nz):
    """No GPU: the generated clusters have the zones the GPU test is about."""
    c, ids, ref, _, refs = _case(n, nz)
    _check_promises(n, nz, c, ids, ref)
    assert all(refs[algo][0].results["has_capacity"].any() for algo in PACKERS)


@pytest.mark.gpu
@pytest.mark.parametrize("setting,setting_name", [(0, "device"), (1, "host")])
@pytest.mark.parametrize("nz", DECLARED)
@pytest.mark.parametrize("n", SIZES)
def test_zone_facts_and_decisions(gf_ctx, n, nz, setting, setting_name):
    c, ids, ref, apps, refs = _case(n, nz)
    avail, sched, rD, rX = ref
    where = f"n={n} declared={nz} finalize={setting_name}"
    gf_ctx.set_option("snapshot_finalize_host", setting)
    try:
        D, X = gf_ctx.build_snapshot(**c)
        info = gf_ctx.build_info()
        if setting == 0:
            assert info[:3] == (1, 0, 0) and info[3] <= SCALARS_ONLY, (where, info)
        else:
            assert info[:3] == (2, 0, 0), (where, info)
        got_avail, got_sched = gf_ctx.snapshot()
        assert np.array_equal(got_avail, avail) and np.array_equal(got_sched, sched), where
        assert np.array_equal(D, rD) and np.array_equal(X, rX), where
        for algo in PACKERS:
            ind, fifo = refs[algo]
            gpu = gf_ctx.fit_batch(IND, algo, apps)
            assert stress_lib.same(gpu, ind, False) is None, (where, algo, stress_lib.same(gpu, ind, False))
            assert np.array_equal(gf_ctx.fit_feasible(algo, apps), ind.results["has_capacity"].astype(bool)), (where, algo)
            assert np.array_equal(_bits(gf_ctx.avg_packing_efficiency(algo, apps, gpu)), _bits(ind.avg_eff)), (where, algo)
            gpu = gf_ctx.fit_batch(FIFO, algo, apps)
            assert stress_lib.same(gpu, fifo, True) is None, (where, algo, stress_lib.same(gpu, fifo, True))
            assert np.array_equal(gf_ctx.residual(), fifo.avail_after), (where, algo)
    finally:
        gf_ctx.set_option("snapshot_finalize_host", 0)
