"""What the node-range sharding entry points of the C ABI refuse, with which code and which message: gf_shard_set, the four
gf_shard_*_dev and the four gf_shard_mf_*_dev steps, gf_shard_layout and gf_shard_mf_layout, for every packer, in every state a
caller can get wrong.  The expectations are literals: the order of the checks, the codes and the texts are part of the
contract (the two families of steps do not agree with each other, and must keep disagreeing).

The cluster has 4 nodes in 2 zones and the batch one application with k = 1; the steps that are not refused run on it as one
shard of one (every buffer zeroed, each step fed by the one before it)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import gangfit

pytestmark = pytest.mark.gpu
N = gangfit._native
OK, INVALID, STATE, UNSUPPORTED = N.GF_OK, N.GF_ERR_INVALID, N.GF_ERR_STATE, N.GF_ERR_UNSUPPORTED
TP, DE, MF = N.GF_ALGO_TIGHTLY_PACK, N.GF_ALGO_DISTRIBUTE_EVENLY, N.GF_ALGO_MINIMAL_FRAGMENTATION
AZA, SAZ, SAZMF = N.GF_ALGO_AZ_AWARE_TIGHTLY_PACK, N.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK, N.GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION
ALGOS = (TP, DE, SAZ, AZA, MF, SAZMF)

# the phrase that tells one refusal from every other
PHRASES = {
    "multi": "a multi-device context runs the shard steps and their exchanges itself",
    "orders": "gf_snapshot_set + gf_orders_set must precede a sharded fit",
    "merged": "node-range sharding needs the merged slot layout",
    "old-only": "single-az-tightly-pack and az-aware-tightly-pack only",
    "mf-only": "the gf_shard_mf_* steps serve minimal-fragmentation and single-az-minimal-fragmentation only",
    "zone-sched": "zone-aware packers compare packing efficiencies",
    "mf-sched": "single-az-minimal-fragmentation compares packing efficiencies",
    "null": "device pointers must not be NULL",
    "half": "half must be at least 1",
}
OLD_STEPS = ("partials", "drivers", "emit", "finish")
MF_STEPS = ("mf_counts", "mf_drivers", "mf_emit", "mf_finish")

AVAIL = np.array([[8000, 8 << 30, 0]] * 4, dtype=np.int64)
ZONE = np.array([0, 0, 1, 1], dtype=np.uint32)
EVERY = np.arange(4, dtype=np.uint32)
APPS = gangfit.make_apps([[1000, 1 << 30, 0]], [[1000, 1 << 30, 0]], np.array([1], dtype=np.int32))
HALF = 2  # sum of k + 1
LAYOUT_HALF = 11


def _observe(ctx, algo, null=False, half=HALF, layout_half=LAYOUT_HALF):
    """{entry point: (return code, key of the phrase in last_error() — "" when the call succeeded — [, the layout])}"""
    import torch

    lib, h = ctx._lib, ctx._h
    seen = {}

    def note(name, rc, *values):
        why = ""
        if rc != OK:
            msg = ctx.last_error()
            hits = [k for k, text in PHRASES.items() if text in msg]
            assert len(hits) == 1, (name, rc, msg)
            why = hits[0]
        seen[name] = (rc, why) + (values if rc == OK else ())

    d_apps = torch.from_numpy(gangfit.with_offsets(APPS)[0].view(np.uint8).copy()).to("cuda:0")
    buf = {name: torch.zeros(1 << 12, dtype=torch.uint8, device="cuda:0")
           for name in ("part", "drv", "res", "exec", "mf_part", "mf_cnt", "mf_drv", "mf_res", "mf_exec")}
    torch.cuda.synchronize()
    p = {name: None if null else C.c_void_p(t.data_ptr()) for name, t in buf.items()}
    da = None if null else C.c_void_p(d_apps.data_ptr())
    n = len(APPS)
    note("partials", lib.gf_shard_partials_dev(h, algo, n, da, p["part"], None))
    note("drivers", lib.gf_shard_drivers_dev(h, algo, n, da, p["part"], p["drv"], None))
    note("emit", lib.gf_shard_emit_dev(h, algo, n, da, p["part"], p["drv"], p["res"], p["exec"], half, None))
    note("finish", lib.gf_shard_finish_dev(h, algo, n, da, p["part"], p["drv"], p["res"], p["exec"], half, None))
    note("mf_counts", lib.gf_shard_mf_counts_dev(h, algo, n, da, p["mf_part"], p["mf_cnt"], None))
    note("mf_drivers", lib.gf_shard_mf_drivers_dev(h, algo, n, da, p["mf_part"], p["mf_drv"], None))
    note("mf_emit", lib.gf_shard_mf_emit_dev(h, algo, n, da, p["mf_part"], p["mf_drv"], p["mf_cnt"], p["mf_res"], p["mf_exec"], half, None))
    note("mf_finish", lib.gf_shard_mf_finish_dev(h, algo, n, da, p["mf_part"], p["mf_drv"], p["mf_res"], p["mf_exec"], half, None))
    rec, row, words, red = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    rc = lib.gf_shard_layout(h, algo, layout_half, C.byref(rec), C.byref(words), C.byref(red))
    note("layout", rc, (rec.value, words.value, red.value))
    rc = lib.gf_shard_mf_layout(h, algo, layout_half, C.byref(rec), C.byref(row), C.byref(words), C.byref(red))
    note("mf_layout", rc, (rec.value, row.value, words.value, red.value))
    torch.cuda.synchronize()
    return seen


def _expect(old_steps, layout, mf_steps, mf_layout):
    """One code for the four steps of a family, or one per step."""
    out = {}
    for names, codes in ((OLD_STEPS, old_steps), (MF_STEPS, mf_steps)):
        out.update(zip(names, [codes] * 4 if not isinstance(codes[0], tuple) else codes))
    out["layout"], out["mf_layout"] = layout, mf_layout
    return out


def _install(ctx, sched=True, orders=(EVERY, EVERY)):
    ctx.set_snapshot(AVAIL, AVAIL if sched else None)
    ctx.set_zones(ZONE)
    ctx.set_orders(*orders)
    assert ctx._lib.gf_shard_set(ctx._h, 0, 1) == OK


# the layouts of the six packers on 2 zones with half = 11 (gf_shard_layout: records, words, reduced words; gf_shard_mf_layout:
# records, bytes of a count row, words, reduced words)
LAYOUT = {TP: (1, 22, 11), DE: (1, 22, 22), SAZ: (2, 22, 22), AZA: (3, 33, 33)}
MF_LAYOUT = {MF: (1, 512, 11, 11), SAZMF: (2, 512, 22, 22)}
OLD_ONLY, MF_ONLY = (UNSUPPORTED, "old-only"), (UNSUPPORTED, "mf-only")
NULL = (INVALID, "null")


def _served(algo, steps_ok=(OK, ""), mf_steps_ok=(OK, ""), half_zero=False):
    """Everything installed: each family serves its own packers and names them to the others."""
    layout = (INVALID, "half") if half_zero else None
    if algo in LAYOUT:
        return _expect(steps_ok, layout or (OK, "", LAYOUT[algo]), MF_ONLY, layout or MF_ONLY)
    return _expect(OLD_ONLY, layout or OLD_ONLY, mf_steps_ok, layout or (OK, "", MF_LAYOUT[algo]))


def test_multi_device_context_refuses_every_entry_point():
    multi = (UNSUPPORTED, "multi")
    with gangfit.Context(devices=[0, 0]) as g:
        g.set_snapshot(AVAIL, AVAIL)
        g.set_zones(ZONE)
        g.set_orders(EVERY, EVERY)
        assert g._lib.gf_shard_set(g._h, 0, 1) == UNSUPPORTED and PHRASES["multi"] in g.last_error()
        for algo in ALGOS:
            assert _observe(g, algo) == _expect(multi, multi, multi, multi), algo
            assert _observe(g, algo, null=True) == _expect(multi, multi, multi, multi), algo  # (the first check of all)
            assert _observe(g, algo, half=0, layout_half=0) == _expect(multi, multi, multi, multi), algo


def test_no_orders_installed():
    orders = (STATE, "orders")
    with gangfit.Context(0) as ctx:
        assert ctx._lib.gf_shard_set(ctx._h, 0, 1) == OK
        for algo in ALGOS:
            assert _observe(ctx, algo) == _expect(orders, orders, orders, orders), algo
        ctx.set_snapshot(AVAIL, AVAIL)
        ctx.set_zones(ZONE)
        for algo in ALGOS:
            assert _observe(ctx, algo) == _expect(orders, orders, orders, orders), algo


def test_orders_that_do_not_merge():
    """The gf_shard_* steps look at the layout before the packer, the gf_shard_mf_* steps at the packer first."""
    merged = (UNSUPPORTED, "merged")
    with gangfit.Context(0) as ctx:
        _install(ctx, orders=([0, 1, 2], [2, 1, 0]))
        for algo in (TP, DE, SAZ, AZA):
            assert _observe(ctx, algo) == _expect(merged, merged, MF_ONLY, MF_ONLY), algo
        for algo in (MF, SAZMF):
            assert _observe(ctx, algo) == _expect(merged, merged, merged, merged), algo


def test_snapshot_without_the_schedulable_columns():
    """GF_ERR_UNSUPPORTED from the zone-aware tightly-pack packers, GF_ERR_STATE from single-az-minimal-fragmentation."""
    with gangfit.Context(0) as ctx:
        _install(ctx, sched=False)
        for algo in (TP, DE, MF):
            assert _observe(ctx, algo) == _served(algo), algo
        for algo in (SAZ, AZA):
            zs = (UNSUPPORTED, "zone-sched")
            assert _observe(ctx, algo) == _expect(zs, zs, MF_ONLY, MF_ONLY), algo
        ms = (STATE, "mf-sched")
        assert _observe(ctx, SAZMF) == _expect(OLD_ONLY, OLD_ONLY, ms, ms)


def test_packer_of_the_other_family_and_the_layouts():
    with gangfit.Context(0) as ctx:
        _install(ctx)
        for algo in ALGOS:
            assert _observe(ctx, algo) == _served(algo), algo
        for algo in (6, 99):  # no packer at all
            assert _observe(ctx, algo) == _expect(OLD_ONLY, OLD_ONLY, MF_ONLY, MF_ONLY), algo


def test_null_device_pointers():
    """Refused before the packer, the orders or the layout are looked at; the layout queries take no device pointer."""
    with gangfit.Context(0) as ctx:
        for algo in ALGOS:  # (nothing installed)
            assert _observe(ctx, algo, null=True) == _expect(NULL, (STATE, "orders"), NULL, (STATE, "orders")), algo
        _install(ctx)
        for algo in ALGOS:
            want = _served(algo)
            want.update(dict.fromkeys(OLD_STEPS + MF_STEPS, NULL))  # (the other family's packers too: before the packer is looked at)
            assert _observe(ctx, algo, null=True) == want, algo
        # n_apps == 0 asks for no pointer
        assert ctx._lib.gf_shard_partials_dev(ctx._h, TP, 0, None, None, None) == OK
        assert ctx._lib.gf_shard_mf_counts_dev(ctx._h, MF, 0, None, None, None, None) == OK
        assert ctx._lib.gf_shard_partials_dev(ctx._h, MF, 0, None, None, None) == UNSUPPORTED and PHRASES["old-only"] in ctx.last_error()


def test_half_of_zero():
    """emit and finish refuse it with the text of the pointer check, whatever the packer; the layout queries with their own."""
    with gangfit.Context(0) as ctx:
        _install(ctx)
        for algo in ALGOS:
            want = _served(algo, half_zero=True)
            for name in ("emit", "finish", "mf_emit", "mf_finish"):
                want[name] = NULL
            assert _observe(ctx, algo, half=0, layout_half=0) == want, algo
