// gangfit_api_group.cpp — node-range sharding: the gf_shard_* steps for one process per GPU, and gf_fit_batch on a multi-device
// context (one gf_ctx over several devices: exchanges by peer stores over xGMI or by RCCL).
#include "gangfit_ctx.h"

using namespace gfapi;

namespace gfapi {

using gangfit::ShardFamily;

// the packer has zone views (after shard_serves): the zoned family and single-az-minimal-fragmentation
static bool shard_has_zones(gf_algo algo) {
    return gangfit::shard_family_of(algo) == ShardFamily::zoned || algo == GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION;
}

// GF_OK when node-range sharding serves `algo` on this context (orders installed) through the steps asked for — mf_steps: the
// gf_shard_mf_* entry points, which serve the minfrag family; else gf_shard_*, which serve the other two —, else why not, in
// ctx->err when `report` (the entry points; a multi-device context quietly runs the batch on its first device instead).  The two
// sets of steps are part of the ABI as they answer today: gf_shard_mf_* look at the packer before the layout and call missing
// schedulable columns a GF_ERR_STATE, gf_shard_* look at the layout first and call them GF_ERR_UNSUPPORTED.
static int shard_serves(gf_ctx* ctx, gf_algo algo, bool mf_steps, bool report) {
    char why[256];
    int rc = GF_ERR_UNSUPPORTED;
    const std::optional<ShardFamily> family = gangfit::shard_family_of(algo);
    const bool served = family && (*family == ShardFamily::minfrag) == mf_steps;
    const bool views = served && shard_has_zones(algo);
    const uint32_t n_cand = candidate_views(ctx, algo);
    if (mf_steps && !served)
        std::snprintf(why, sizeof why, "the gf_shard_mf_* steps serve minimal-fragmentation and single-az-minimal-fragmentation only");
    else if (!ctx->merged)
        std::snprintf(why, sizeof why, "node-range sharding needs the merged slot layout (driver and executor orders must be "
                                       "subsequences of one priority order)");
    else if (!served)
        std::snprintf(why, sizeof why, "node-range sharding serves tightly-pack, distribute-evenly, single-az-tightly-pack "
                                       "and az-aware-tightly-pack only");
    else if (views && !ctx->have_sched) {
        if (mf_steps) rc = GF_ERR_STATE;
        std::snprintf(why, sizeof why, "%s packing efficiencies: node-range sharding needs the schedulable columns of gf_snapshot_set",
                      mf_steps ? "single-az-minimal-fragmentation compares" : "zone-aware packers compare");
    } else if (views && (n_cand == 0 || n_cand > 64))
        std::snprintf(why, sizeof why, "node-range sharding of %s needs 1 to 64 candidate views (zones of the evaluation list%s), not %u",
                      mf_steps ? "single-az-minimal-fragmentation" : "a zone-aware packer", mf_steps ? "" : ", plus one for az-aware", n_cand);
    else
        return GF_OK;
    return report ? fail(ctx, rc, "%s", why) : rc;
}

static void shard_range_of(gf_ctx* ctx, gangfit::ShardRange* r);

static int shard_ready(gf_ctx* ctx, gf_algo algo, bool mf_steps, gangfit::ShardRange* r) {
    if (!ctx->have_orders) return fail(ctx, GF_ERR_STATE, "gf_snapshot_set + gf_orders_set must precede a sharded fit");
    if (const int rc = shard_serves(ctx, algo, mf_steps, true); rc != GF_OK) return rc;
    shard_range_of(ctx, r);
    return GF_OK;
}

static void shard_range_of(gf_ctx* ctx, gangfit::ShardRange* r) {
    const uint64_t xc = ((uint64_t)ctx->n_x + 63) / 64;  // chunks of the merged order (the sentinel slot hosts nothing)
    r->c_lo = (uint32_t)(xc * ctx->shard / ctx->n_shards);
    r->c_hi = (uint32_t)(xc * (ctx->shard + 1) / ctx->n_shards);
    r->shard = ctx->shard;
    r->n_shards = ctx->n_shards;
    // the range's sub-slots of the sparse gpu view (gangs of gpu executors are summed and emitted from it: gangfit_shard.inc)
    r->g_lo = r->g_hi = 0;
    if (ctx->n_g != 0 && !ctx->g_prefix.empty()) {
        const size_t last = ctx->g_prefix.size() - 1;
        r->g_lo = ctx->g_prefix[r->c_lo < last ? r->c_lo : last];
        r->g_hi = ctx->g_prefix[r->c_hi < last ? r->c_hi : last];
    }
}
// (a context without the prefix table — a view — takes the full order)
static gangfit::SparseTable shard_sparse(gf_ctx* ctx) {
    return (ctx->n_g != 0 && !ctx->g_prefix.empty()) ? make_sparse(ctx) : gangfit::SparseTable{};
}
// What of a ShardBatch comes from the context alone (after shard_ready): the tables and the packer's candidate views.  The
// caller adds the shards, the records and the stream.
static void shard_batch_of(gf_ctx* ctx, gf_algo algo, gangfit::ShardBatch* b) {
    b->table = make_table(ctx, ctx->d_snap.ptr);
    b->gpu_view = shard_sparse(ctx);
    b->has_zones = shard_has_zones(algo);
    if (!b->has_zones) return;
    gangfit::ShardZones& z = b->zones;
    z.xmask = ctx->d_zmasks.ptr;
    z.dmask = ctx->d_zmasks.ptr + (size_t)ctx->zd_row0 * ctx->zstride;
    z.span = ctx->zspan_ok ? ctx->d_zspan.ptr : nullptr;
    z.sched = ctx->d_sched.ptr;
    z.n_zones = ctx->n_zones;
    z.stride = ctx->zstride;
    z.n_cand = candidate_views(ctx, algo);
    z.az_aware = algo == GF_ALGO_AZ_AWARE_TIGHTLY_PACK ? 1u : 0u;
}
// What a batch's buffers hold (gf_shard_layout, gf_shard_mf_layout): records per application and view, placement buffer words,
// words to reduce
struct ShardLayout {
    uint32_t records;
    uint64_t exec2_words, reduce_words;
};
static ShardLayout shard_layout_of(const gf_ctx* ctx, gf_algo algo, uint64_t half) {
    // plain: [0, half) the placements, [half, 2 half) the capacities of distribute-evenly's pass 1
    if (gangfit::shard_family_of(algo) == ShardFamily::plain) return ShardLayout{1u, 2 * half, algo == GF_ALGO_DISTRIBUTE_EVENLY ? 2 * half : half};
    const uint32_t v = candidate_views(ctx, algo);
    return ShardLayout{v, (uint64_t)v * half, (uint64_t)v * half};  // region c: view c's placement, all of it reduced
}

// ---- the submitting threads (GroupPool, gangfit_ctx.h)
GroupPool::GroupPool(uint32_t n_devices) : parties(n_devices) {
    for (uint32_t d = 1; d < n_devices; ++d) threads.emplace_back([this, d] { worker(d); });
}
GroupPool::~GroupPool() {
    {
        std::lock_guard<std::mutex> l(m);
        quit = true;
        generation.fetch_add(1, std::memory_order_release);
    }
    cv.notify_all();
    for (std::thread& t : threads) t.join();
}
void GroupPool::worker(uint32_t d) {
    uint64_t seen = 0;
    for (;;) {
        // a short spin (batches that follow each other find the thread awake), then the condition variable
        const auto t0 = std::chrono::steady_clock::now();
        while (generation.load(std::memory_order_acquire) == seen) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [&] { return generation.load(std::memory_order_acquire) != seen; });
                break;
            }
        }
        seen = generation.load(std::memory_order_acquire);
        if (quit) return;
        (*job)(d);
        remaining.fetch_sub(1, std::memory_order_acq_rel);
    }
}
void GroupPool::run(const std::function<void(uint32_t)>& j) {
    job = &j;
    remaining.store(parties - 1, std::memory_order_release);
    {
        std::lock_guard<std::mutex> l(m);
        generation.fetch_add(1, std::memory_order_release);
    }
    cv.notify_all();
    j(0);
    while (remaining.load(std::memory_order_acquire) != 0) std::this_thread::yield();
}
void GroupPool::barrier() {
    const uint32_t gen = bar_gen.load(std::memory_order_acquire);
    if (bar_count.fetch_add(1, std::memory_order_acq_rel) + 1 == parties) {
        bar_count.store(0, std::memory_order_relaxed);
        bar_gen.fetch_add(1, std::memory_order_release);
    } else {
        uint32_t spins = 0;
        while (bar_gen.load(std::memory_order_acquire) == gen)
            if ((++spins & 0xFFFu) == 0) std::this_thread::yield();
    }
}

// gf_fit_batch on a multi-device context.  Independent batches of the two plain packers, of the zone-aware tightly-pack
// packers and of the two minimal-fragmentation packers are node-range sharded across the sub-contexts (the
// four steps of gangfit_shard.inc with the three exchanges done by peer access — the producing kernels write straight into every
// device's gathered table, the minimal-fragmentation packers' count rows like their records, shard_reduce_pull_kernel collects
// the placements — or by RCCL); everything else — FIFO chains (each commit must be visible to the next scan), orders that do not
// merge, zone-aware batches without the schedulable columns or with more than 64 candidate views — runs on the first device.
//
// One sub-context = one DEVICE and the shards it hosts: per step ONE launch per device (a grid row per hosted shard), one
// upload of the records, one gathered table and one placement buffer per device.  With several devices device d's calls are
// issued by submitting thread d (GroupPool); between the steps the threads meet at a host barrier, because stream t may only
// be told to wait for event s once event s has been recorded.
int group_fit_batch(gf_ctx* g, gf_mode mode, gf_algo algo, uint32_t n_apps, const gf_app* apps, gf_result* results,
                    uint32_t* exec_nodes, uint64_t exec_nodes_cap, int32_t* chain_failed_at) {
    std::lock_guard<std::recursive_mutex> glock(g->mu);
    gf_ctx* const first = g->group[0];
    const std::optional<ShardFamily> family = gangfit::shard_family_of(algo);
    const bool minfrag = family == ShardFamily::minfrag;  // (the gf_shard_mf_* steps: count rows travel with the records)
    bool sharded = mode == GF_MODE_INDEPENDENT && n_apps > 0 && !g->g_shard_off;
    for (gf_ctx* s : g->group) sharded = sharded && s->have_orders && shard_serves(s, algo, minfrag, false) == GF_OK;
    if (!sharded) {
        const int rc = gf_fit_batch(first, mode, algo, n_apps, apps, results, exec_nodes, exec_nodes_cap, chain_failed_at);
        if (rc != GF_OK) g->err = first->err;
        return rc;
    }
    if (!apps || !results) return fail(g, GF_ERR_INVALID, "apps/results must not be NULL");
    if (chain_failed_at) *chain_failed_at = -1;
    const uint32_t D = (uint32_t)g->group.size();  // devices (sub-contexts)
    const uint32_t S = g->g_total_shards;          // shards of the priority order
    GF_HIP(g, hipSetDevice(first->device));
    GF_HIP(g, g->h_apps.reserve(n_apps));
    uint64_t total_k = 0;
    if (const int rc = check_apps(g, n_apps, apps, g->h_apps.ptr, &total_k); rc != GF_OK) return rc;
    if (total_k > exec_nodes_cap || (total_k > 0 && !exec_nodes))
        return fail(g, GF_ERR_CAPACITY, "exec_nodes holds %llu entries, %llu needed", (unsigned long long)exec_nodes_cap,
                    (unsigned long long)total_k);
    const uint64_t half = total_k + 1;
    // records per application and view, the placement buffer and what the reduce of it carries (shard_layout_of)
    const ShardLayout lay = shard_layout_of(first, algo, half);
    const uint32_t rec = lay.records;
    const size_t row_words = gangfit::kShardMfRowBytes / sizeof(uint32_t);  // (minimal-fragmentation: a count row per record)
    const size_t reduce_words = (size_t)lay.reduce_words;
    GF_HIP(g, g->h_results.reserve(n_apps));
    GF_HIP(g, g->h_exec.reserve(total_k + 1));
    // ---- buffers on every device (growth only: no-ops from the second batch of a size on) and what each device's kernels
    //      must know about the others: every gathered table, every placement buffer
    std::vector<gangfit::ShardBatch> batch(D);  // what the steps of each device receive
    gangfit::PeerPtrs part_all{}, drv_all{}, cnt_all{}, exec_others{};
    for (uint32_t d = 0; d < D; ++d) {
        gf_ctx* c = g->group[d];
        GF_HIP(g, hipSetDevice(c->device));
        gangfit::ShardSet& set = batch[d].set;
        set.n_shards = S;
        for (uint32_t sh : c->my_shards) {
            c->shard = sh;
            c->n_shards = S;
            gangfit::ShardRange r{};
            if (const int rc = shard_ready(c, algo, minfrag, &r); rc != GF_OK) {
                g->err = c->err;
                return rc;
            }
            const uint32_t q = set.n++;
            set.c_lo[q] = r.c_lo;
            set.c_hi[q] = r.c_hi;
            set.shard[q] = sh;
            set.g_lo[q] = r.g_lo;
            set.g_hi[q] = r.g_hi;
        }
        shard_batch_of(c, algo, &batch[d]);
        GF_HIP(g, c->d_apps.reserve(n_apps));
        GF_HIP(g, c->d_results.reserve(n_apps));
        GF_HIP(g, c->g_part_loc.reserve((size_t)c->my_shards.size() * rec * n_apps));
        GF_HIP(g, c->g_drv_loc.reserve((size_t)c->my_shards.size() * rec * n_apps));
        GF_HIP(g, c->g_part_all.reserve((size_t)S * rec * n_apps));
        GF_HIP(g, c->g_drv_all.reserve((size_t)S * rec * n_apps));
        GF_HIP(g, c->g_exec2.reserve(lay.exec2_words));
        if (minfrag) {
            GF_HIP(g, c->g_cnt_loc.reserve((size_t)c->my_shards.size() * rec * n_apps * row_words));
            GF_HIP(g, c->g_cnt_all.reserve((size_t)S * rec * n_apps * row_words));
            cnt_all.p[d] = c->g_cnt_all.ptr;
        }
        part_all.p[d] = c->g_part_all.ptr;
        drv_all.p[d] = c->g_drv_all.ptr;
        if (d > 0) exec_others.p[exec_others.n++] = c->g_exec2.ptr;
        gangfit::ShardBatch& b = batch[d];
        b.n_apps = n_apps;
        b.d_apps = c->d_apps.ptr;
        b.d_part = c->g_part_loc.ptr;
        b.d_all_part = c->g_part_all.ptr;
        b.d_drv = c->g_drv_loc.ptr;
        b.d_all_drv = c->g_drv_all.ptr;
        b.d_counts = minfrag ? c->g_cnt_loc.ptr : nullptr;
        b.d_all_counts = minfrag ? c->g_cnt_all.ptr : nullptr;
        b.d_results = c->d_results.ptr;
        b.d_exec2 = c->g_exec2.ptr;
        b.half = half;
        b.n_shards = S;
        b.stream = c->stream;
    }
    part_all.n = drv_all.n = cnt_all.n = D;
    const bool use_rccl = g->g_comms.size() == D && D == S;
    if (!use_rccl)  // the producing kernels write into every device's gathered table
        for (gangfit::ShardBatch& b : batch) {
            b.part_dsts = part_all;
            b.drv_dsts = drv_all;
            if (minfrag) b.count_dsts = cnt_all;
        }
    std::vector<int> rc_of(D, GF_OK);
    auto hip_ok = [&](uint32_t d, hipError_t e, const char* what) {
        if (e == hipSuccess || rc_of[d] != GF_OK) return e == hipSuccess;
        rc_of[d] = fail(g->group[d], GF_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
        return false;
    };
#define GF_STEP(d, call) hip_ok((d), (call), #call)
    // the steps of ONE device, each issued on that device's stream by whichever thread runs them
    auto step_partials = [&](uint32_t d) {
        gf_ctx* c = g->group[d];
        if (!GF_STEP(d, hipSetDevice(c->device))) return;
        if (!GF_STEP(d, hipMemcpyAsync(c->d_apps.ptr, g->h_apps.ptr, (size_t)n_apps * sizeof(gf_app), hipMemcpyHostToDevice, c->stream))) return;
        if (!GF_STEP(d, gangfit::launch_shard_first(algo, batch[d]))) return;
        if (g->g_fault == 2 && d > 0 && !use_rccl) {  // fault injection: this device's capacity sums arrive as zeros everywhere
            for (uint32_t t = 0; t < D; ++t)
                for (uint32_t sh : c->my_shards)
                    (void)GF_STEP(d, hipMemsetAsync(static_cast<gf_shard_partial*>(part_all.p[t]) + (size_t)sh * rec * n_apps, 0,
                                                   (size_t)rec * n_apps * sizeof(gf_shard_partial), c->stream));
        } else if (g->g_fault == 2 && d > 0) {
            (void)GF_STEP(d, hipMemsetAsync(c->g_part_loc.ptr, 0, (size_t)rec * n_apps * sizeof(gf_shard_partial), c->stream));
        }
        if (D > 1 && !use_rccl) (void)GF_STEP(d, hipEventRecord(c->g_ev[0], c->stream));
    };
    auto wait_others = [&](uint32_t d, int which) {  // this device's stream continues only behind event `which` of every other
        gf_ctx* c = g->group[d];
        for (uint32_t s2 = 0; s2 < D; ++s2)
            if (s2 != d && !GF_STEP(d, hipStreamWaitEvent(c->stream, g->group[s2]->g_ev[which], 0))) return;
    };
    auto step_drivers = [&](uint32_t d) {
        gf_ctx* c = g->group[d];
        if (rc_of[d] != GF_OK || !GF_STEP(d, hipSetDevice(c->device))) return;
        if (D > 1 && !use_rccl) wait_others(d, 0);
        if (!GF_STEP(d, gangfit::launch_shard_drivers(algo, batch[d]))) return;
        if (D > 1 && !use_rccl) (void)GF_STEP(d, hipEventRecord(c->g_ev[1], c->stream));
    };
    auto step_emit = [&](uint32_t d) {
        gf_ctx* c = g->group[d];
        if (rc_of[d] != GF_OK || !GF_STEP(d, hipSetDevice(c->device))) return;
        if (D > 1 && !use_rccl) wait_others(d, 1);
        if (!GF_STEP(d, gangfit::launch_shard_emit(algo, batch[d]))) return;
        if (D > 1) (void)GF_STEP(d, hipEventRecord(c->g_ev[2], c->stream));
    };
    auto step_finish = [&]() {  // the first device only: sum of the slices (each entry written by exactly one shard), finish, D2H
        if (rc_of[0] != GF_OK || !GF_STEP(0, hipSetDevice(first->device))) return;
        if (!use_rccl) {
            for (uint32_t s2 = 1; s2 < D; ++s2)
                if (!GF_STEP(0, hipStreamWaitEvent(first->stream, g->group[s2]->g_ev[2], 0))) return;
            if (g->g_fault != 1 && D > 1)  // fault injection: the other devices' placement slices never arrive
                if (!GF_STEP(0, gangfit::launch_shard_reduce_pull(exec_others, first->g_exec2.ptr, reduce_words, first->stream))) return;
        }
        if (!GF_STEP(0, gangfit::launch_shard_finish(algo, batch[0]))) return;
        if (!GF_STEP(0, hipMemcpyAsync(g->h_results.ptr, first->d_results.ptr, (size_t)n_apps * sizeof(gf_result), hipMemcpyDeviceToHost, first->stream))) return;
        if (total_k && !GF_STEP(0, hipMemcpyAsync(g->h_exec.ptr, first->g_exec2.ptr, (size_t)total_k * sizeof(uint32_t), hipMemcpyDeviceToHost, first->stream))) return;
        (void)GF_STEP(0, gf_wait_stream(first->stream));
    };
    // An error must not return while the other devices' kernels, their peer stores into every gathered table, or pending
    // reads of the pinned records are still running: the next batch reuses all of those buffers.  Every stream is waited
    // for first; when even that fails the context stops sharding and serves from its first device.
    auto drain_all = [&]() {
        bool ok = true;
        for (uint32_t d = 0; d < D; ++d) {
            gf_ctx* c = g->group[d];
            if (hipSetDevice(c->device) != hipSuccess || gf_wait_stream(c->stream) != hipSuccess) ok = false;
        }
        (void)hipGetLastError();
        (void)hipSetDevice(first->device);
        if (!ok) g->g_shard_off = true;
    };
    auto fail_drained = [&](const char* what) {
        drain_all();
        return fail(g, GF_ERR_HIP, "%s", what);
    };
    if (use_rccl) {
        // RCCL exchange (one shard per device): every device's collective is enqueued on its own stream inside one group call
        // issued by THIS thread; the library orders the streams against each other
        // (with_rows: the minimal-fragmentation packers' count rows travel in the same grouped call as their records)
        auto rccl_all_gather = [&](auto loc, auto all, size_t bytes_each, bool with_rows = false) -> int {
            if (rccl().GroupStart() != 0) return -1;
            int bad = 0;
            for (uint32_t s2 = 0; s2 < D; ++s2) {
                gf_ctx* c = g->group[s2];
                if (hipSetDevice(c->device) != hipSuccess) bad = 1;
                bad |= rccl().AllGather(loc(c), all(c), bytes_each, Rccl::kChar, g->g_comms[s2], c->stream);
                if (with_rows)
                    bad |= rccl().AllGather(c->g_cnt_loc.ptr, c->g_cnt_all.ptr, (size_t)rec * n_apps * gangfit::kShardMfRowBytes, Rccl::kChar,
                                            g->g_comms[s2], c->stream);
            }
            return rccl().GroupEnd() | bad;
        };
        for (uint32_t d = 0; d < D; ++d) step_partials(d);
        if (rccl_all_gather([](gf_ctx* c) { return (const void*)c->g_part_loc.ptr; }, [](gf_ctx* c) { return (void*)c->g_part_all.ptr; },
                            (size_t)rec * n_apps * sizeof(gf_shard_partial), minfrag) != 0)
            return fail_drained("ncclAllGather of the capacity sums failed");
        for (uint32_t d = 0; d < D; ++d) step_drivers(d);
        if (rccl_all_gather([](gf_ctx* c) { return (const void*)c->g_drv_loc.ptr; }, [](gf_ctx* c) { return (void*)c->g_drv_all.ptr; },
                            (size_t)rec * n_apps * sizeof(gf_shard_driver)) != 0)
            return fail_drained("ncclAllGather of the driver records failed");
        for (uint32_t d = 0; d < D; ++d) step_emit(d);
        // the reduction north_star names: sum of the placement slices onto the first device, over xGMI
        if (rccl().GroupStart() != 0) return fail_drained("ncclGroupStart failed");
        int bad = 0;
        for (uint32_t d = 0; d < D; ++d) {
            gf_ctx* c = g->group[d];
            if (hipSetDevice(c->device) != hipSuccess) bad = 1;
            bad |= rccl().Reduce(c->g_exec2.ptr, first->g_exec2.ptr, reduce_words, Rccl::kUint32, Rccl::kSum, 0, g->g_comms[d], c->stream);
        }
        if ((rccl().GroupEnd() | bad) != 0) return fail_drained("ncclReduce of the placements failed");
        step_finish();
    } else if (D == 1 || g->g_pool == nullptr) {
        for (uint32_t d = 0; d < D; ++d) step_partials(d);
        for (uint32_t d = 0; d < D; ++d) step_drivers(d);
        for (uint32_t d = 0; d < D; ++d) step_emit(d);
        step_finish();
    } else {
        // one submitting thread per device; a host barrier behind every step that records an event another device waits for
        GroupPool& pool = *g->g_pool;
        const std::function<void(uint32_t)> job = [&](uint32_t d) {
            step_partials(d);
            pool.barrier();
            step_drivers(d);
            pool.barrier();
            step_emit(d);
            pool.barrier();
            if (d == 0) step_finish();
        };
        pool.run(job);
    }
#undef GF_STEP
    for (uint32_t d = 0; d < D; ++d)
        if (rc_of[d] != GF_OK) {
            drain_all();  // (step_finish returned without waiting for anything when an earlier step had failed)
            g->err = g->group[d]->err;
            return rc_of[d];
        }
    std::memcpy(results, g->h_results.ptr, (size_t)n_apps * sizeof(gf_result));
    if (total_k) std::memcpy(exec_nodes, g->h_exec.ptr, (size_t)total_k * sizeof(uint32_t));
    // ---- self-check: the first sharded batch of each packer family (plain, zone-aware, minimal-fragmentation) on every newly installed snapshot is
    //      also answered by the first device alone.  A wrong exchange (peer stores that did not land, a collective that reduced
    //      something else) must not decide a Filter: on a mismatch the context stops sharding, says why, and serves the first
    //      device's answer.
    uint64_t& verified = g->g_verified_epoch[(int)*family];  // (plain, zoned, minfrag)
    if (g->g_verify && first->snap_epoch != verified) {
        std::vector<gf_result> ref_res(n_apps);
        std::vector<uint32_t> ref_exec((size_t)total_k + 1);
        const int rc = gf_fit_batch(first, mode, algo, n_apps, apps, ref_res.data(), ref_exec.data(), total_k, nullptr);
        if (rc != GF_OK) {
            g->err = first->err;
            return rc;
        }
        bool same = std::memcmp(ref_res.data(), results, (size_t)n_apps * sizeof(gf_result)) == 0;
        for (uint32_t a = 0; a < n_apps && same; ++a)
            if (ref_res[a].has_capacity)
                same = std::memcmp(ref_exec.data() + g->h_apps.ptr[a].exec_off, exec_nodes + g->h_apps.ptr[a].exec_off,
                                   (size_t)ref_res[a].exec_len * sizeof(uint32_t)) == 0;
        if (same) {
            verified = first->snap_epoch;
        } else {
            g->g_shard_off = true;
            g->err = "the node-range sharded batch disagreed with the first device's own answer: sharding is off for this context";
            std::memcpy(results, ref_res.data(), (size_t)n_apps * sizeof(gf_result));
            if (total_k) std::memcpy(exec_nodes, ref_exec.data(), (size_t)total_k * sizeof(uint32_t));
        }
    }
    return GF_OK;
}

// ---- the entry points of one process per GPU
// Every one of them begins here: a multi-device context runs the steps itself.
static int shard_single_device(gf_ctx* ctx) {
    if (ctx != nullptr && !ctx->group.empty())
        return fail(ctx, GF_ERR_UNSUPPORTED, "a multi-device context runs the shard steps and their exchanges itself (gf_fit_batch)");
    return ctx ? GF_OK : GF_ERR_INVALID;
}
// The preamble of a step (mf_steps: one of gf_shard_mf_*): the context, then the step's own pointer check — made by the caller,
// which knows its pointers, and judged here, where its place among the checks is —, then whether the packer is served; on GF_OK
// *b holds everything that does not depend on the step: tables, views, the context's shard and the stream.
static int shard_step_begin(gf_ctx* ctx, gf_algo algo, bool mf_steps, bool pointers_ok, void* stream, gangfit::ShardBatch* b) {
    if (const int rc = shard_single_device(ctx); rc != GF_OK) return rc;
    if (!pointers_ok) return fail(ctx, GF_ERR_INVALID, "device pointers must not be NULL");
    gangfit::ShardRange r{};
    if (const int rc = shard_ready(ctx, algo, mf_steps, &r); rc != GF_OK) return rc;
    shard_batch_of(ctx, algo, b);
    b->set = gangfit::shard_set_of(r);
    b->n_shards = ctx->n_shards;
    b->stream = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    return GF_OK;
}
// ... and of a layout query
static int shard_layout_begin(gf_ctx* ctx, gf_algo algo, bool mf_steps, uint64_t half, ShardLayout* lay) {
    if (const int rc = shard_single_device(ctx); rc != GF_OK) return rc;
    if (half == 0) return fail(ctx, GF_ERR_INVALID, "half must be at least 1 (sum of k + 1)");
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    gangfit::ShardRange r{};
    if (const int rc = shard_ready(ctx, algo, mf_steps, &r); rc != GF_OK) return rc;
    *lay = shard_layout_of(ctx, algo, half);
    return GF_OK;
}

// (both families: the packer's family decides which steps serve it, the search is the same)
static int shard_drivers_dev(gf_ctx* ctx, gf_algo algo, bool mf_steps, uint32_t n_apps, const gf_app* d_apps,
                             const gf_shard_partial* d_all_partials, gf_shard_driver* d_out, void* stream) {
    gangfit::ShardBatch b;
    if (const int rc = shard_step_begin(ctx, algo, mf_steps, n_apps == 0 || (d_apps && d_all_partials && d_out), stream, &b); rc != GF_OK)
        return rc;
    b.n_apps = n_apps;
    b.d_apps = d_apps;
    b.d_all_part = d_all_partials;
    b.d_drv = d_out;
    GF_HIP(ctx, gangfit::launch_shard_drivers(algo, b));
    return GF_OK;
}
// emit and finish of both families take the same buffers (d_all_counts: gf_shard_mf_emit_dev alone)
static int shard_emit_or_finish_dev(gf_ctx* ctx, gf_algo algo, bool mf_steps, bool emit, uint32_t n_apps, const gf_app* d_apps,
                                    const gf_shard_partial* d_all_partials, const gf_shard_driver* d_all_drivers,
                                    const void* d_all_counts, gf_result* d_results, uint32_t* d_exec2, uint64_t half, void* stream) {
    const bool counts_ok = !(mf_steps && emit) || d_all_counts;
    gangfit::ShardBatch b;
    if (const int rc = shard_step_begin(ctx, algo, mf_steps,
                                        n_apps == 0 || (d_apps && d_all_partials && d_all_drivers && counts_ok && d_results && d_exec2 && half != 0),
                                        stream, &b);
        rc != GF_OK)
        return rc;
    b.n_apps = n_apps;
    b.d_apps = d_apps;
    b.d_all_part = d_all_partials;
    b.d_all_drv = d_all_drivers;
    b.d_all_counts = static_cast<const uint32_t*>(d_all_counts);
    b.d_results = d_results;
    b.d_exec2 = d_exec2;
    b.half = half;
    GF_HIP(ctx, emit ? gangfit::launch_shard_emit(algo, b) : gangfit::launch_shard_finish(algo, b));
    return GF_OK;
}

}  // namespace gfapi

extern "C" {

int gf_shard_set(gf_ctx* ctx, uint32_t shard, uint32_t n_shards) {
    if (const int rc = shard_single_device(ctx); rc != GF_OK) return rc;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    if (n_shards == 0 || shard >= n_shards || n_shards > 1024)
        return fail(ctx, GF_ERR_INVALID, "shard %u of %u", shard, n_shards);
    ctx->shard = shard;
    ctx->n_shards = n_shards;
    return GF_OK;
}

int gf_shard_partials_dev(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, const gf_app* d_apps, gf_shard_partial* d_out,
                          void* stream) {
    gangfit::ShardBatch b;
    if (const int rc = shard_step_begin(ctx, algo, false, n_apps == 0 || (d_apps && d_out), stream, &b); rc != GF_OK) return rc;
    b.n_apps = n_apps;
    b.d_apps = d_apps;
    b.d_part = d_out;
    GF_HIP(ctx, gangfit::launch_shard_first(algo, b));
    return GF_OK;
}

int gf_shard_drivers_dev(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, const gf_app* d_apps,
                         const gf_shard_partial* d_all_partials, gf_shard_driver* d_out, void* stream) {
    return shard_drivers_dev(ctx, algo, false, n_apps, d_apps, d_all_partials, d_out, stream);
}

int gf_shard_emit_dev(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, const gf_app* d_apps,
                      const gf_shard_partial* d_all_partials, const gf_shard_driver* d_all_drivers, gf_result* d_results,
                      uint32_t* d_exec2, uint64_t half, void* stream) {
    return shard_emit_or_finish_dev(ctx, algo, false, true, n_apps, d_apps, d_all_partials, d_all_drivers, nullptr, d_results, d_exec2, half,
                                    stream);
}
int gf_shard_finish_dev(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, const gf_app* d_apps,
                        const gf_shard_partial* d_all_partials, const gf_shard_driver* d_all_drivers,
                        gf_result* d_results, uint32_t* d_exec2, uint64_t half, void* stream) {
    return shard_emit_or_finish_dev(ctx, algo, false, false, n_apps, d_apps, d_all_partials, d_all_drivers, nullptr, d_results, d_exec2, half,
                                    stream);
}

int gf_shard_layout(gf_ctx* ctx, gf_algo algo, uint64_t half, uint32_t* records_per_app, uint64_t* exec2_words,
                    uint64_t* reduce_words) {
    ShardLayout lay{};
    if (const int rc = shard_layout_begin(ctx, algo, false, half, &lay); rc != GF_OK) return rc;
    if (records_per_app) *records_per_app = lay.records;
    if (exec2_words) *exec2_words = lay.exec2_words;
    if (reduce_words) *reduce_words = lay.reduce_words;
    return GF_OK;
}

// ---- the minimal-fragmentation family (gangfit_shard.inc: the shard_mf_* kernels)
int gf_shard_mf_layout(gf_ctx* ctx, gf_algo algo, uint64_t half, uint32_t* records_per_app, uint32_t* count_bytes_per_record,
                       uint64_t* exec2_words, uint64_t* reduce_words) {
    ShardLayout lay{};
    if (const int rc = shard_layout_begin(ctx, algo, true, half, &lay); rc != GF_OK) return rc;
    if (records_per_app) *records_per_app = lay.records;
    if (count_bytes_per_record) *count_bytes_per_record = gangfit::kShardMfRowBytes;
    if (exec2_words) *exec2_words = lay.exec2_words;
    if (reduce_words) *reduce_words = lay.reduce_words;
    return GF_OK;
}

int gf_shard_mf_counts_dev(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, const gf_app* d_apps, gf_shard_partial* d_part_out,
                           void* d_counts_out, void* stream) {
    gangfit::ShardBatch b;
    if (const int rc = shard_step_begin(ctx, algo, true, n_apps == 0 || (d_apps && d_part_out && d_counts_out), stream, &b); rc != GF_OK)
        return rc;
    b.n_apps = n_apps;
    b.d_apps = d_apps;
    b.d_part = d_part_out;
    b.d_counts = static_cast<uint32_t*>(d_counts_out);
    GF_HIP(ctx, gangfit::launch_shard_first(algo, b));
    return GF_OK;
}

int gf_shard_mf_drivers_dev(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, const gf_app* d_apps,
                            const gf_shard_partial* d_all_partials, gf_shard_driver* d_out, void* stream) {
    return shard_drivers_dev(ctx, algo, true, n_apps, d_apps, d_all_partials, d_out, stream);
}

int gf_shard_mf_emit_dev(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, const gf_app* d_apps, const gf_shard_partial* d_all_partials,
                         const gf_shard_driver* d_all_drivers, const void* d_all_counts, gf_result* d_results, uint32_t* d_exec2,
                         uint64_t half, void* stream) {
    return shard_emit_or_finish_dev(ctx, algo, true, true, n_apps, d_apps, d_all_partials, d_all_drivers, d_all_counts, d_results, d_exec2, half,
                                    stream);
}

int gf_shard_mf_finish_dev(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, const gf_app* d_apps,
                           const gf_shard_partial* d_all_partials, const gf_shard_driver* d_all_drivers, gf_result* d_results,
                           uint32_t* d_exec2, uint64_t half, void* stream) {
    return shard_emit_or_finish_dev(ctx, algo, true, false, n_apps, d_apps, d_all_partials, d_all_drivers, nullptr, d_results, d_exec2, half,
                                    stream);
}

}  // extern "C"
