"""The resident worker's round bookkeeping (csrc/gangfit_worker_rounds.h, the hand-out word, the ticket carried from one round to
the next) on small geometries: streams long enough that the rotation of the workgroups wraps and the eight count and hand-out
words recycle, with a different n_apps in every ticket — at and around 16 and app_stride, where a row is full, ragged or absent.
Every ticket answers what a launch (gf_fit_batch_dev) answers on the same records, bit for bit."""
import numpy as np
import pytest

import gangfit
from gangfit import _native as N
from gangfit import workloads as wl

pytestmark = pytest.mark.gpu

IND = gangfit.GF_MODE_INDEPENDENT
TIGHT, EVEN, MINFRAG = gangfit.GF_ALGO_TIGHTLY_PACK, gangfit.GF_ALGO_DISTRIBUTE_EVENLY, gangfit.GF_ALGO_MINIMAL_FRAGMENTATION
SAZ = gangfit.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK
GEOMETRIES = [(1, 1), (1, 2), (3, 2), (2, 5)]
N_APPS_MAX = 2 * 16 * 5 + 5


def _n_apps_values(b):
    stride = 16 * b
    return [1, 15, 16, 17, stride - 1, stride, stride + 1, 2 * stride + 5]


@pytest.fixture(scope="module")
def problem():
    """~300 nodes, 165 records in one device array (a ticket of n applications is its first n records), and per packer the launch's
    answer for every n the streams below use — computed once, never written again."""
    import torch

    w = wl.config(2, n_nodes=300, n_apps=N_APPS_MAX)
    s = w.snapshot
    zone = (wl.splitmix64(0xA7, len(s.avail), 9) % np.uint64(3)).astype(np.uint32)
    apps, total_k = gangfit.with_offsets(gangfit.make_apps(w.drv, w.exe, w.k))
    assert len(apps) == N_APPS_MAX
    dev = torch.device("cuda:0")
    d_apps = torch.from_numpy(apps.view(np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    want = {}
    ctx = gangfit.Context(0)
    try:
        ctx.set_snapshot(s.avail, s.sched)
        ctx.set_zones(zone)
        ctx.set_orders(s.driver_order, s.exec_order)
        for algo in (TIGHT, EVEN, MINFRAG, SAZ):
            for n in sorted({n for _, b in GEOMETRIES for n in _n_apps_values(b)}):
                res = torch.zeros(N_APPS_MAX * 16, dtype=torch.uint8, device=dev)
                exe = torch.zeros(total_k + 1, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                ctx.fit_batch_dev(IND, algo, n, d_apps.data_ptr(), res.data_ptr(), exe.data_ptr(), total_k)
                torch.cuda.synchronize()
                # the placement words of the records the launch found room for (an infeasible record has no placement)
                feas = res.cpu().numpy().view(N.RESULT_DTYPE)["has_capacity"][:n] != 0
                mask = np.zeros(total_k + 1, dtype=bool)
                for a in np.nonzero(feas)[0]:
                    mask[int(apps["exec_off"][a]): int(apps["exec_off"][a]) + int(apps["k"][a])] = True
                want[(algo, n)] = (res, exe, torch.from_numpy(mask).to(dev), bool(feas.any()), bool((~feas).any()))
    finally:
        ctx.close()
    assert any(v[3] for v in want.values())
    return dict(snapshot=s, zone=zone, d_apps=d_apps, total_k=total_k, want=want)


@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "open"])
@pytest.mark.parametrize("sets,bps", GEOMETRIES)
@pytest.mark.parametrize("algo", [TIGHT, EVEN, MINFRAG, SAZ], ids=["tightly-pack", "distribute-evenly", "minimal-fragmentation", "single-az"])
def test_streams_on_small_geometries(problem, algo, sets, bps, bounded):
    import torch

    s, total_k, d_apps = problem["snapshot"], problem["total_k"], problem["d_apps"]
    dev = torch.device("cuda:0")
    values = _n_apps_values(bps)
    n_tickets = sets * (2 * bps + 9)  # every set serves 2 b + 9 rounds: the rotation wraps twice, every LDS word is used twice
    # ticket t is round t // sets of set t % sets: consecutive rounds of a set get consecutive values, every set meets all eight
    n_of = [values[(t // sets + 3 * (t % sets)) % 8] for t in range(n_tickets)]
    ctx = gangfit.Context(0, options={"worker_sets": sets, "worker_blocks_per_set": bps})
    try:
        ctx.set_snapshot(s.avail, s.sched)
        ctx.set_zones(problem["zone"])
        ctx.set_orders(s.driver_order, s.exec_order)
        res = [torch.zeros(N_APPS_MAX * 16, dtype=torch.uint8, device=dev) for _ in range(n_tickets)]
        exe = [torch.zeros(total_k + 1, dtype=torch.int32, device=dev) for _ in range(n_tickets)]
        torch.cuda.synchronize()
        batches = [(n_of[t], d_apps.data_ptr(), res[t].data_ptr(), exe[t].data_ptr(), total_k) for t in range(n_tickets)]
        with pytest.raises(gangfit.GangfitError):  # an empty ticket is refused by the host, it never reaches the kernel
            ctx.worker_submit_dev(algo, [(0, d_apps.data_ptr(), res[0].data_ptr(), exe[0].data_ptr(), total_k)])
        if bounded:
            first = ctx.worker_submit_prepared(algo, ctx.worker_batches(batches, leave_after=True))
        else:
            first = ctx.worker_submit_dev(algo, batches)
        ctx.worker_wait(first, n_tickets)
        assert ctx.worker_geometry() == (sets, bps)
        ctx.worker_stop()
        torch.cuda.synchronize()
        bad = []
        for t in range(n_tickets):
            w_res, w_exe, mask, _, _ = problem["want"][(algo, n_of[t])]
            if not torch.equal(res[t], w_res):
                bad.append((t, n_of[t], "results"))
            if not torch.equal(exe[t][mask], w_exe[mask]):
                bad.append((t, n_of[t], "placements"))
        assert not bad, bad[:8]
        st = ctx.worker_stats()
        assert st["posted"] == st["complete"] == n_tickets and not st["resident"]
    finally:
        ctx.close()
