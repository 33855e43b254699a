"""Node-range sharding of an independent gang-fit batch across the GPUs of one box.

One process per GPU.  Every rank holds a gf_ctx with the same snapshot and orders and owns one contiguous range of the
priority order (gf_shard_set); a batch is four device steps (include/gangfit.h, csrc/gangfit_shard.inc) with one small
exchange between consecutive steps:

    partials -> all-gather (16 B/app) -> drivers -> all-gather (16 B/app) -> emit -> all-reduce(SUM) of the placement
    buffer (4 B/executor) -> finish

after which every rank holds the full result, bit-identical to the single-GPU gf_fit_batch.  The exchanges are the only
collectives on the data path; on the GPU box they run over RCCL/xGMI (`torch.distributed`, backend "nccl") on device
tensors, in stream order with the kernels.  The messages are KB-sized, i.e. latency-bound: sharding the node table pays
only when one GPU's scan of the table is slower than ~3 collective latencies (50k+ nodes x 10k apps, BASELINE config 4);
for the headline size the throughput path is app sharding with no collective (bench.py).  The FIFO chain does not shard
(each commit must be visible to the next scan): it runs as replicas.

The zone-aware tightly-pack packers (single-az-tightly-pack, az-aware-tightly-pack) run the same steps once per candidate view
— every zone, plus the plain order for az-aware —, with records and placement regions per view; how many, and how much of
the placement buffer the all-reduce sums, comes from the library (gf_shard_layout, HipShardEngine.layout).

The minimal-fragmentation packers (minimal-fragmentation, single-az-minimal-fragmentation) walk the whole executor order for
every application — "the smallest capacity >= K" is a minimum over every candidate —, so theirs is the walk that divides by the
number of shards.  Their first exchange carries, next to the 16-byte records, a row of capacity counts per application and
view (512 B), from which every rank makes the same plan and emits its own range's runs: the C ABI has entry points of their own
for that (gf_shard_mf_*; ShardedMinfragBatch, sharded_fit_minfrag).  Still three exchanges per batch.

Both batches are one class (_Batch: the records' offsets, the upload, `step`, `step_timed`, `fetch`); ShardedBatch and
ShardedMinfragBatch add the packers they serve, their layout query and their four steps.  Below the C ABI it is the same
shape: every step receives one record (ShardBatch, csrc/gangfit_device.h) and picks its kernel by the packer's family.

This file is orchestration only: no arithmetic on placements happens in Python, and there is no CPU fallback —
`HipShardEngine` raises when libgangfit or the GPU is missing.  `Comm`/engine are small interfaces so that the N > 1 control
flow is also exercised on CPU (tests/test_sharded_cpu.py: world_size-2 gloo with a numpy engine from tests/).
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import List, Optional

import numpy as np

from . import _native as N
from .context import BatchOut, Context, with_offsets


# ------------------------------------------------------------------------------------------------ communicators
class Comm:
    """What the orchestrator needs from a process group."""

    rank: int = 0
    world: int = 1

    def all_gather(self, t):  # -> tensor [world, *t.shape], same device as t
        raise NotImplementedError

    def all_reduce_sum_(self, t):  # in place
        raise NotImplementedError


class SingleComm(Comm):
    """world_size 1: the exchanges degenerate to views."""

    def all_gather(self, t):
        return t.unsqueeze(0)

    def all_reduce_sum_(self, t):
        return t


class TorchComm(Comm):
    """torch.distributed process group.  "nccl" (= RCCL on ROCm) moves device tensors over xGMI; with a "gloo" group
    device tensors are staged through the host (CPU tests, and two processes sharing one GPU)."""

    def __init__(self, group=None):
        import torch.distributed as dist

        self._dist = dist
        self._group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        self._host_staged = dist.get_backend(group) != "nccl"

    def all_gather(self, t):
        import torch

        src = t.contiguous()
        stacked = (self.world,) + tuple(src.shape)
        flat = (self.world * src.shape[0],) + tuple(src.shape[1:])  # concatenated form: accepted by nccl and gloo
        if self._host_staged and src.is_cuda:
            out = torch.empty(flat, dtype=src.dtype)
            self._dist.all_gather_into_tensor(out, src.cpu(), group=self._group)
            return out.view(stacked).to(t.device)
        out = torch.empty(flat, dtype=src.dtype, device=src.device)
        self._dist.all_gather_into_tensor(out, src, group=self._group)
        return out.view(stacked)

    def all_reduce_sum_(self, t):
        if self._host_staged and t.is_cuda:
            h = t.cpu()
            self._dist.all_reduce(h, group=self._group)
            t.copy_(h)
            return t
        self._dist.all_reduce(t, group=self._group)
        return t


class ThreadGroup:
    """In-process stand-in for a process group: `world` threads, one shard each (one GPU, several gf_ctx).  Used by the
    single-GPU parity tests of the sharded path."""

    def __init__(self, world: int):
        self.world = world
        self._barrier = threading.Barrier(world)
        self._slots: List[Optional[object]] = [None] * world

    def comm(self, rank: int) -> "ThreadComm":
        return ThreadComm(self, rank)


class ThreadComm(Comm):
    def __init__(self, group: ThreadGroup, rank: int):
        self._g = group
        self.rank = rank
        self.world = group.world

    def _exchange(self, t):
        import torch

        g = self._g
        if t.is_cuda:
            torch.cuda.current_stream().synchronize()
        g._slots[self.rank] = t
        g._barrier.wait()
        parts = list(g._slots)
        g._barrier.wait()
        return parts

    def all_gather(self, t):
        import torch

        return torch.stack(self._exchange(t.contiguous()), dim=0)

    def all_reduce_sum_(self, t):
        import torch

        parts = self._exchange(t.clone())
        t.copy_(torch.stack(parts, dim=0).sum(dim=0))
        return t


# ------------------------------------------------------------------------------------------------ the HIP engine
_first_look = threading.Lock()


class HipShardEngine:
    """The four device steps through the C ABI, on torch device tensors (torch only owns memory and the stream)."""

    def __init__(self, ctx: Context, shard: int, n_shards: int, device):
        import torch

        with _first_look:  # (one thread at a time: shards of one device as a thread group may all get here first)
            have_gpu = torch.cuda.is_available()
        if not have_gpu:
            raise RuntimeError("HipShardEngine needs an MI355X: the HIP path is the only product path")
        self.ctx = ctx
        self.device = torch.device(device)
        self.shard, self.n_shards = shard, n_shards
        ctx._check(ctx._lib.gf_shard_set(ctx._h, shard, n_shards))
        self._torch = torch
        # one explicit stream for kernels, torch copies and the collectives: the legacy default stream has handle 0,
        # which the C ABI reads as "use the context's own stream" — work split over two streams would race
        self.stream = torch.cuda.Stream(self.device)

    def stream_context(self):
        return self._torch.cuda.stream(self.stream)

    def _stream(self):
        return C.c_void_p(self.stream.cuda_stream)

    def upload_apps(self, apps_off: np.ndarray):
        return self._torch.from_numpy(apps_off.view(np.uint8).copy()).to(self.device)

    def layout(self, algo: int, half: int):
        """(records per application, words of the placement buffer, leading words of it the all-reduce sums) of a batch of
        `algo` with sum of k = half - 1 on the context's installed snapshot, zones and orders (gf_shard_layout)."""
        rec, words, red = C.c_uint32(), C.c_uint64(), C.c_uint64()
        c = self.ctx
        c._check(c._lib.gf_shard_layout(c._h, algo, half, C.byref(rec), C.byref(words), C.byref(red)))
        return int(rec.value), int(words.value), int(red.value)

    def partials(self, algo: int, d_apps, n_apps: int, records: int = 1):
        out = self._torch.empty((records * n_apps, 2), dtype=self._torch.int64, device=self.device)
        c = self.ctx
        c._check(c._lib.gf_shard_partials_dev(c._h, algo, n_apps, C.c_void_p(d_apps.data_ptr()),
                                              C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def drivers(self, algo: int, d_apps, n_apps: int, all_part, records: int = 1):
        out = self._torch.empty((records * n_apps, 4), dtype=self._torch.int32, device=self.device)
        c = self.ctx
        c._check(c._lib.gf_shard_drivers_dev(c._h, algo, n_apps, C.c_void_p(d_apps.data_ptr()),
                                             C.c_void_p(all_part.data_ptr()), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def emit(self, algo: int, d_apps, n_apps: int, all_part, all_drv, half: int, words: Optional[int] = None):
        res = self._torch.empty(n_apps * 16, dtype=self._torch.uint8, device=self.device)
        exec2 = self._torch.empty(2 * half if words is None else words, dtype=self._torch.int32, device=self.device)
        c = self.ctx
        c._check(c._lib.gf_shard_emit_dev(c._h, algo, n_apps, C.c_void_p(d_apps.data_ptr()),
                                          C.c_void_p(all_part.data_ptr()), C.c_void_p(all_drv.data_ptr()),
                                          C.c_void_p(res.data_ptr()), C.c_void_p(exec2.data_ptr()), half, self._stream()))
        return res, exec2

    def finish(self, algo: int, d_apps, n_apps: int, all_part, all_drv, res, exec2, half: int):
        c = self.ctx
        c._check(c._lib.gf_shard_finish_dev(c._h, algo, n_apps, C.c_void_p(d_apps.data_ptr()),
                                            C.c_void_p(all_part.data_ptr()), C.c_void_p(all_drv.data_ptr()),
                                            C.c_void_p(res.data_ptr()), C.c_void_p(exec2.data_ptr()), half,
                                            self._stream()))

    # ---- the minimal-fragmentation family (gf_shard_mf_*)
    def mf_layout(self, algo: int, half: int):
        """(records per application, bytes of a count row, words of the placement buffer, leading words of it the all-reduce
        sums) of a minimal-fragmentation batch with sum of k = half - 1 (gf_shard_mf_layout)."""
        rec, row, words, red = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        c = self.ctx
        c._check(c._lib.gf_shard_mf_layout(c._h, algo, half, C.byref(rec), C.byref(row), C.byref(words), C.byref(red)))
        return int(rec.value), int(row.value), int(words.value), int(red.value)

    def mf_counts(self, algo: int, d_apps, n_apps: int, records: int, row_bytes: int):
        """This shard's records and count rows in ONE buffer (what the first exchange carries): records * n_apps 16-byte records,
        then records * n_apps rows."""
        n = records * n_apps
        out = self._torch.empty(n * (16 + row_bytes), dtype=self._torch.uint8, device=self.device)
        c = self.ctx
        c._check(c._lib.gf_shard_mf_counts_dev(c._h, algo, n_apps, C.c_void_p(d_apps.data_ptr()), C.c_void_p(out.data_ptr()),
                                               C.c_void_p(out.data_ptr() + n * 16), self._stream()))
        return out

    def mf_split(self, gathered, n_apps: int, records: int):
        """The gathered [world, bytes] buffers of mf_counts as the two tables the later steps read: [world][records][n_apps]
        records, and the rows in the same order."""
        n = records * n_apps
        return gathered[:, : n * 16].contiguous(), gathered[:, n * 16:].contiguous()

    def mf_drivers(self, algo: int, d_apps, n_apps: int, all_part, records: int):
        out = self._torch.empty((records * n_apps, 4), dtype=self._torch.int32, device=self.device)
        c = self.ctx
        c._check(c._lib.gf_shard_mf_drivers_dev(c._h, algo, n_apps, C.c_void_p(d_apps.data_ptr()),
                                                C.c_void_p(all_part.data_ptr()), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def mf_emit(self, algo: int, d_apps, n_apps: int, all_part, all_drv, all_cnt, half: int, words: int):
        res = self._torch.empty(n_apps * 16, dtype=self._torch.uint8, device=self.device)
        exec2 = self._torch.empty(words, dtype=self._torch.int32, device=self.device)
        c = self.ctx
        c._check(c._lib.gf_shard_mf_emit_dev(c._h, algo, n_apps, C.c_void_p(d_apps.data_ptr()), C.c_void_p(all_part.data_ptr()),
                                             C.c_void_p(all_drv.data_ptr()), C.c_void_p(all_cnt.data_ptr()),
                                             C.c_void_p(res.data_ptr()), C.c_void_p(exec2.data_ptr()), half, self._stream()))
        return res, exec2

    def mf_finish(self, algo: int, d_apps, n_apps: int, all_part, all_drv, res, exec2, half: int):
        c = self.ctx
        c._check(c._lib.gf_shard_mf_finish_dev(c._h, algo, n_apps, C.c_void_p(d_apps.data_ptr()),
                                               C.c_void_p(all_part.data_ptr()), C.c_void_p(all_drv.data_ptr()),
                                               C.c_void_p(res.data_ptr()), C.c_void_p(exec2.data_ptr()), half, self._stream()))


# ------------------------------------------------------------------------------------------------ orchestration
class _Batch:
    """One pending-app table prepared for repeated sharded evaluation (bench.py times `step`).  A family of packers adds which
    ones it serves (ALGOS, REFUSAL), its layout query (_layout: records, reduce_words and what its steps need besides) and its
    steps (_steps(mark): the four device steps and the three exchanges, mark(2 i) before and mark(2 i + 1) behind exchange i)."""

    ALGOS: tuple = ()
    REFUSAL = ""

    def __init__(self, engine, comm: Comm, algo: int, apps: np.ndarray):
        if algo not in self.ALGOS:
            raise N.GangfitError(N.GF_ERR_UNSUPPORTED, self.REFUSAL)
        self.engine, self.comm, self.algo = engine, comm, algo
        apps = np.ascontiguousarray(apps, dtype=N.APP_DTYPE)
        self.apps_off, self.total_k = with_offsets(apps)
        self.n_apps = len(apps)
        self.half = self.total_k + 1
        self._layout()
        with engine.stream_context():
            self.d_apps = engine.upload_apps(self.apps_off)
        self.res = self.exec2 = None

    def _placements(self):
        """What the all-reduce carries: the leading reduce_words of the buffer — tightly-pack's placements, distribute-evenly's
        placements and pass-1 capacities, or every candidate view's placement region."""
        return self.exec2 if self.reduce_words >= len(self.exec2) else self.exec2[: self.reduce_words]

    def step(self):
        self._steps(lambda i: None)

    def step_timed(self):
        """step(), with a pair of events on the engine's stream around each of the three exchanges (GPU engines only).  Returns
        [first all-gather (the partials, or the records and count rows), all-gather of the drivers, all-reduce of the placements]
        in microseconds of device time — what the data-path collectives of one batch cost (bench.py:
        config.node_sharded.exchange_us)."""
        import torch

        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        self._steps(lambda i: ev[i].record(self.engine.stream))
        self.engine.stream.synchronize()
        return [ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(3)]

    def fetch(self) -> BatchOut:
        with self.engine.stream_context():
            res = self.res.cpu().numpy().view(N.RESULT_DTYPE).copy()
            ex = self.exec2[: self.total_k].cpu().numpy().view(np.uint32).copy()
        return BatchOut(res, self.apps_off["exec_off"].copy(), ex, -1)


SHARDED_ALGOS = (N.GF_ALGO_TIGHTLY_PACK, N.GF_ALGO_DISTRIBUTE_EVENLY, N.GF_ALGO_SINGLE_AZ_TIGHTLY_PACK,
                 N.GF_ALGO_AZ_AWARE_TIGHTLY_PACK)


class ShardedBatch(_Batch):
    """The plain and the zone-aware tightly-pack packers: partials -> all-gather -> drivers -> all-gather -> emit ->
    all-reduce(SUM) of the placement buffer -> finish."""

    ALGOS = SHARDED_ALGOS
    REFUSAL = ("node-range sharding serves tightly-pack, distribute-evenly, single-az-tightly-pack and az-aware-tightly-pack "
               "only")

    def _layout(self):
        # from the library (HipShardEngine.layout); an engine without the query serves the plain packers, whose layout is
        # fixed: one record per application, [0, half) placements + [half, 2 half) distribute-evenly's capacities
        if hasattr(self.engine, "layout"):
            self.records, words, self.reduce_words = self.engine.layout(self.algo, self.half)
            self._rec_kw, self._emit_kw = {"records": self.records}, {"words": words}
        elif self.algo in (N.GF_ALGO_TIGHTLY_PACK, N.GF_ALGO_DISTRIBUTE_EVENLY):
            self.records = 1
            self.reduce_words = 2 * self.half if self.algo == N.GF_ALGO_DISTRIBUTE_EVENLY else self.half
            self._rec_kw, self._emit_kw = {}, {}
        else:
            raise N.GangfitError(N.GF_ERR_UNSUPPORTED, "this shard engine serves the plain packers only")

    def _steps(self, mark):
        e, c, algo, n = self.engine, self.comm, self.algo, self.n_apps
        with e.stream_context():
            part = e.partials(algo, self.d_apps, n, **self._rec_kw)
            mark(0)
            all_part = c.all_gather(part)
            mark(1)
            drv = e.drivers(algo, self.d_apps, n, all_part, **self._rec_kw)
            mark(2)
            all_drv = c.all_gather(drv)
            mark(3)
            self.res, self.exec2 = e.emit(algo, self.d_apps, n, all_part, all_drv, self.half, **self._emit_kw)
            mark(4)
            c.all_reduce_sum_(self._placements())
            mark(5)
            e.finish(algo, self.d_apps, n, all_part, all_drv, self.res, self.exec2, self.half)


def sharded_fit(engine, comm: Comm, algo: int, apps: np.ndarray) -> BatchOut:
    """gf_fit_batch(GF_MODE_INDEPENDENT) with the node table sharded by priority-order range over comm.world GPUs."""
    b = ShardedBatch(engine, comm, algo, apps)
    b.step()
    return b.fetch()


MINFRAG_ALGOS = (N.GF_ALGO_MINIMAL_FRAGMENTATION, N.GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION)


class ShardedMinfragBatch(_Batch):
    """The minimal-fragmentation packers: counts -> all-gather (records and count rows, one buffer) -> drivers -> all-gather ->
    emit -> all-reduce(SUM) of the placement buffer -> finish."""

    ALGOS = MINFRAG_ALGOS
    REFUSAL = "the minimal-fragmentation shard steps serve minimal-fragmentation and single-az-minimal-fragmentation only"

    def _layout(self):
        self.records, self.row_bytes, self.words, self.reduce_words = self.engine.mf_layout(self.algo, self.half)

    def first_exchange_bytes_per_app(self) -> int:
        """What one rank contributes to the first all-gather per application (every view's record and count row)."""
        return self.records * (16 + self.row_bytes)

    def _steps(self, mark):
        e, c, algo, n, rec = self.engine, self.comm, self.algo, self.n_apps, self.records
        with e.stream_context():
            mine = e.mf_counts(algo, self.d_apps, n, rec, self.row_bytes)
            mark(0)
            gathered = c.all_gather(mine)
            mark(1)
            all_part, all_cnt = e.mf_split(gathered, n, rec)
            drv = e.mf_drivers(algo, self.d_apps, n, all_part, rec)
            mark(2)
            all_drv = c.all_gather(drv)
            mark(3)
            self.res, self.exec2 = e.mf_emit(algo, self.d_apps, n, all_part, all_drv, all_cnt, self.half, self.words)
            mark(4)
            c.all_reduce_sum_(self._placements())
            mark(5)
            e.mf_finish(algo, self.d_apps, n, all_part, all_drv, self.res, self.exec2, self.half)


def sharded_fit_minfrag(engine, comm: Comm, algo: int, apps: np.ndarray) -> BatchOut:
    """gf_fit_batch(GF_MODE_INDEPENDENT) of a minimal-fragmentation packer with the node table sharded by priority-order range
    over comm.world GPUs."""
    b = ShardedMinfragBatch(engine, comm, algo, apps)
    b.step()
    return b.fetch()
