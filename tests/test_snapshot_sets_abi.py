"""gf_snapshot_build_resident_set / gf_snapshot_set_info at the drop-in boundary: declared, exported and bound, and every refusal
leaves the generations and the installed snapshot as they were."""
import ctypes

import numpy as np
import pytest

import gangfit
from gangfit import _native as N
from gangfit import build
from oracle import pysnapshot as ps

GIB = 1 << 30
CAND = ps.READY | ps.DRIVER_CANDIDATE


def test_declared_exported_and_bound():
    lib = ctypes.CDLL(build.build_native())
    L = N.load()
    for name, n_args in (("gf_snapshot_build_resident_set", 14), ("gf_snapshot_set_info", 2)):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
        f = getattr(L, name)
        assert f.restype is ctypes.c_int32 and len(f.argtypes) == n_args


def _raw_build(ctx, words, n_res=0):
    """The C call itself: Context.build_snapshot_resident_set packs its own rows and cannot express a bit beyond the cluster."""
    w = None if words is None else np.ascontiguousarray(words, dtype=np.uint64)
    return ctx._lib.gf_snapshot_build_resident_set(ctx._h, N.ptr(w), n_res, None, None, None, None, None, None, None, None, None,
                                                   None, None)


def _raw_parent(ctx, n_res=0):
    return ctx._lib.gf_snapshot_build_resident(ctx._h, n_res, None, None, None, None, None, None, None, None, None, None, None)


def _state(ctx):
    return ctx.generation(), ctx.snapshot(), ctx.snapshot_set_info(), ctx.build_info()


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1]) and a[2:] == b[2:]


@pytest.mark.gpu
def test_refusals_change_nothing(gf_ctx):
    n = 65
    alloc = np.tile(np.array([[16000, 64 * GIB, 0]], dtype=np.int64), (n, 1))
    gf_ctx.set_cluster(alloc, np.full(n, CAND, dtype=np.uint32), np.arange(n, dtype=np.uint32))
    members = np.arange(n) % 2 == 0
    gf_ctx.build_snapshot_resident_set(members)
    before = _state(gf_ctx)
    assert before[2] == (1, 33, 34, 1)
    # a bit at or beyond n_nodes: node 65 (bit 1 of the last word), and the last bit of the last word
    for last in (0b10, 0b11, 1 << 63):
        assert _raw_build(gf_ctx, [1, last]) == N.GF_ERR_INVALID
        assert "beyond" in gf_ctx.last_error()
        assert _same(_state(gf_ctx), before)
    # what gf_snapshot_build_resident refuses: NULL entry columns
    assert _raw_build(gf_ctx, [1, 1], n_res=3) == N.GF_ERR_INVALID
    assert _same(_state(gf_ctx), before)
    # on a view: GF_ERR_STATE, like every installer
    with gf_ctx.view() as v:
        assert _raw_build(v, [1, 1]) == N.GF_ERR_STATE and _raw_build(v, None) == N.GF_ERR_STATE
        assert v.snapshot_set_info() == before[2]  # a view reports its parent's layout
    assert _same(_state(gf_ctx), before)
    # the row [1, 1] itself is fine: nodes 0 and 64
    assert _raw_build(gf_ctx, [1, 1]) == N.GF_OK
    assert gf_ctx.snapshot_set_info() == (1, 2, 3, 1)


@pytest.mark.gpu
def test_without_cluster_and_without_orders():
    with gangfit.Context(0) as fresh:
        out = np.zeros(4, dtype=np.uint32)
        assert fresh._lib.gf_snapshot_set_info(fresh._h, N.ptr(out)) == N.GF_ERR_STATE  # no orders
        assert fresh._lib.gf_snapshot_set_info(fresh._h, None) == N.GF_ERR_INVALID
        gen = fresh.generation()
        assert _raw_build(fresh, [1]) == N.GF_ERR_STATE  # gf_cluster_set must come first
        assert _raw_build(fresh, None) == N.GF_ERR_STATE
        assert fresh.generation() == gen and fresh.build_info() == (0, 0, 0, 0)
        assert fresh._lib.gf_snapshot_set_info(fresh._h, N.ptr(out)) == N.GF_ERR_STATE
        # a snapshot without orders is still "without orders"
        fresh.set_snapshot(np.zeros((4, 3), dtype=np.int64))
        assert fresh._lib.gf_snapshot_set_info(fresh._h, N.ptr(out)) == N.GF_ERR_STATE
        fresh.set_orders([0, 1], [0, 1, 2])
        assert fresh.snapshot_set_info()[:2] == (0, 4)


def _after_a_failed_update(ctx):
    """Unusable usage or overhead after an update that failed half way (option "update_fault" leaves the host flags such an
    update leaves): GF_ERR_STATE from the build, with a row and with NULL, and nothing moves; gf_usage_reset / gf_cluster_set lift it."""
    n = 130
    rng = np.random.default_rng(3)
    alloc = np.tile(np.array([[16000, 64 * GIB, 0]], dtype=np.int64), (n, 1))
    over = np.stack([rng.integers(0, 4, size=n) * 250, rng.integers(0, 4, size=n) * GIB, np.zeros(n, dtype=np.int64)], axis=1)
    flags, ranks = np.full(n, CAND, dtype=np.uint32), rng.permutation(n).astype(np.uint32)
    entries = rng.integers(0, n, size=40).astype(np.uint32)
    requests = np.tile(np.array([[1000, 2 * GIB, 0]], dtype=np.int64), (40, 1))
    row = np.zeros(3, dtype=np.uint64)
    row[:] = (0x5555555555555555, 0xFFFF, 0b11)  # 32 + 16 + 2 members, the last node among them
    RESIDENT = N.GF_RESIDENT_USAGE

    def install():
        ctx.set_cluster(alloc, flags, ranks, overhead=over)
        ctx.n_nodes = n  # (the raw calls below go past the wrapper that keeps it)
        ctx.usage_apply(entries, requests, +1)
        assert _raw_build(ctx, row, RESIDENT) == N.GF_OK
        assert ctx.snapshot_set_info() == (1, 50, 51, 1)
        return _state(ctx)

    # ---- the usage is unknown: builds from the resident sums are refused, builds whose entries travel are not
    before = install()
    ctx.set_option("update_fault", 1)
    for words in (row, None):
        assert _raw_build(ctx, words, RESIDENT) == N.GF_ERR_STATE and "usage" in ctx.last_error()
        assert _same(_state(ctx), before)
    assert _raw_parent(ctx, RESIDENT) == N.GF_ERR_STATE
    with pytest.raises(gangfit.GangfitError) as e:
        ctx.usage_apply(entries[:1], requests[:1], +1)
    assert e.value.code == N.GF_ERR_STATE and _same(_state(ctx), before)
    assert _raw_build(ctx, row, 0) == N.GF_OK  # no entry: nothing of the resident usage is read
    assert ctx.generation()[1:] == before[0][1:] and ctx.snapshot_set_info() == before[2]
    assert np.array_equal(ctx.snapshot()[0], ctx.snapshot()[1])  # available = schedulable: no usage
    ctx.usage_reset()  # lifts it
    ctx.usage_apply(entries, requests, +1)
    assert _raw_build(ctx, row, RESIDENT) == N.GF_OK
    now = _state(ctx)
    assert np.array_equal(now[1][0], before[1][0]) and np.array_equal(now[1][1], before[1][1]) and now[2] == before[2]
    # ---- the overhead is unknown: every build is refused, whatever its row and wherever its entries come from
    before = _state(ctx)
    ctx.set_option("update_fault", 2)
    for words in (row, None):
        for n_res in (RESIDENT, 0):
            assert _raw_build(ctx, words, n_res) == N.GF_ERR_STATE and "overhead" in ctx.last_error()
            assert _same(_state(ctx), before)
    assert _raw_parent(ctx, 0) == N.GF_ERR_STATE
    with pytest.raises(gangfit.GangfitError) as e:
        ctx.overhead_update([0], [[250, GIB, 0]])
    assert e.value.code == N.GF_ERR_STATE and _same(_state(ctx), before)
    ctx.usage_reset()  # ... does not lift it
    assert _raw_build(ctx, row, 0) == N.GF_ERR_STATE
    after = install()  # gf_cluster_set does
    assert np.array_equal(after[1][0], before[1][0]) and np.array_equal(after[1][1], before[1][1])
    # ---- both at once, and the switch's own refusals
    ctx.set_option("update_fault", 3)
    assert _raw_build(ctx, row, RESIDENT) == N.GF_ERR_STATE and _raw_build(ctx, None, 0) == N.GF_ERR_STATE
    assert _same(_state(ctx), after)
    install()
    with pytest.raises(gangfit.GangfitError) as e:
        ctx.set_option("update_fault", 0)
    assert e.value.code == N.GF_ERR_INVALID
    assert _raw_build(ctx, row, RESIDENT) == N.GF_OK


@pytest.mark.gpu
def test_unusable_usage_or_overhead_after_a_failed_update(gf_ctx):
    _after_a_failed_update(gf_ctx)


@pytest.mark.gpu
def test_unusable_usage_or_overhead_on_a_multi_device_context():
    """Every device is marked, as each_device marks them when an update reached only some of them."""
    with gangfit.Context(devices=[0, 0]) as g:
        _after_a_failed_update(g)
