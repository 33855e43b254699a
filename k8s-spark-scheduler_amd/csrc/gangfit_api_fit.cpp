// gangfit_api_fit.cpp — the decision side of the C ABI: table views; route_of, the one place that decides which kernels serve a
// (mode, packer) on a context, and launch, which runs them (one function per route family: independent batches,
// the plain chain, the LDS chains with their generic twin, the generic chain); the incremental chain cache, gf_fit_batch /
// gf_fit_batch_dev / gf_fit_feasible / gf_spark_binpack, single executors, findNodes and the packing efficiencies.
#include "gangfit_ctx.h"
#include "gangfit_floor_units.h"

using namespace gfapi;

namespace gfapi {

NodeTable make_table(gf_ctx* ctx, int64_t* base) {
    NodeTable t;
    t.cpu = base;
    t.mem = base + ctx->n_slots;
    t.gpu = base + 2 * (size_t)ctx->n_slots;
    t.slot_node = ctx->d_slot_node.ptr;
    t.dslot = ctx->d_dslot.ptr;
    t.node_slot = ctx->d_node_slot.ptr;
    t.cmax = ctx->d_cmax.ptr;
    t.n_chunks = ctx->n_chunks;
    t.n_x = ctx->n_x;
    t.n_d = ctx->n_d;
    t.n_slots = ctx->n_slots;
    t.n_nodes = ctx->n_nodes;
    t.d_identity = ctx->d_identity ? 1u : 0u;
    t.xmask = ctx->d_masks.ptr;
    t.dmask = ctx->d_masks.ptr + ctx->n_chunks;
    // the snapshot's scaled int32 twin travels with the SNAPSHOT only (a chain's working copy has its own, in the chain's units)
    if (ctx->narrow_ok && base == ctx->d_snap.ptr && ctx->d_nsnap.ptr != nullptr) {
        t.ncpu = ctx->d_nsnap.ptr;
        t.nmem = t.ncpu + ctx->n_slots;
        t.ngpu = t.nmem + ctx->n_slots;
        t.nquad = reinterpret_cast<const int4*>(ctx->d_nquad.ptr);  // (written with the columns: current whenever they are)
        for (int j = 0; j < 3; ++j) t.nunit[j] = ctx->unit[j] > 0 ? ctx->unit[j] : 1;
    }
    return t;
}

gangfit::SparseTable make_sparse(gf_ctx* ctx) {
    gangfit::SparseTable g{};
    if (ctx->n_g == 0) return g;
    g.cpu = ctx->d_gtab.ptr;
    g.mem = g.cpu + ctx->n_gpad;
    g.gpu = g.mem + ctx->n_gpad;
    g.slot_node = ctx->d_gidx.ptr;
    g.sub_of_slot = ctx->d_gidx.ptr + ctx->n_gpad;
    g.cmax = ctx->d_gcmax.ptr;
    g.xmask = ctx->d_gmask.ptr;
    g.n_x = ctx->n_g;
    g.n_chunks = ctx->n_gpad / 64;
    g.zmask = g.xmask + g.n_chunks;
    g.slot_of_sub = g.sub_of_slot + ctx->n_slots;
    return g;
}

gangfit::EffTables slot_eff_tables(gf_ctx* ctx, const int64_t* avail_base) {
    gangfit::EffTables e;
    for (int j = 0; j < 3; ++j) {
        e.avail[j] = avail_base + (size_t)j * ctx->n_slots;
        e.sched[j] = ctx->d_sched.ptr + (size_t)j * ctx->n_slots;
    }
    return e;
}

// minimalFragmentation never records its placements in `reserved` (minimal_fragmentation.go:59-91)
bool reserves_executors(gf_algo algo) {
    return algo != GF_ALGO_MINIMAL_FRAGMENTATION && algo != GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION;
}
bool is_zone_algo(gf_algo algo) {
    return algo == GF_ALGO_AZ_AWARE_TIGHTLY_PACK || algo == GF_ALGO_SINGLE_AZ_TIGHTLY_PACK ||
           algo == GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION;
}
bool is_plain_algo(gf_algo algo) {
    return algo == GF_ALGO_TIGHTLY_PACK || algo == GF_ALGO_DISTRIBUTE_EVENLY || algo == GF_ALGO_MINIMAL_FRAGMENTATION;
}
// candidate views of one application: every zone of the evaluation list (plus the plain order for az-aware), else one
uint32_t candidate_views(const gf_ctx* ctx, gf_algo algo) {
    return is_zone_algo(algo) ? ctx->n_zones + (algo == GF_ALGO_AZ_AWARE_TIGHTLY_PACK ? 1u : 0u) : 1u;
}

// Checks request record a: k in [0, GF_MAX_K], every quantity in [0, 2^62).
static int check_app(gf_ctx* ctx, uint32_t a, const gf_app& in) {
    if (in.k < 0 || in.k > GF_MAX_K) return fail(ctx, GF_ERR_INVALID, "apps[%u].k = %d outside [0, %d]", a, in.k, GF_MAX_K);
    for (int j = 0; j < 3; ++j)
        if (in.drv[j] < 0 || in.drv[j] >= GF_MAX_ABS_QUANTITY || in.exe[j] < 0 || in.exe[j] >= GF_MAX_ABS_QUANTITY)
            return fail(ctx, GF_ERR_INVALID, "apps[%u] request outside [0, 2^62)", a);
    return GF_OK;
}

// Checks the request records (check_app) and sums their executors into *total_k; out (nullable) receives a copy of the
// records with exec_off set.
int check_apps(gf_ctx* ctx, uint32_t n_apps, const gf_app* apps, gf_app* out, uint64_t* total_k) {
    uint64_t t = 0;
    for (uint32_t a = 0; a < n_apps; ++a) {
        const gf_app& in = apps[a];
        if (const int rc = check_app(ctx, a, in); rc != GF_OK) return rc;
        if (out != nullptr) {
            out[a] = in;
            out[a].exec_off = t;
        }
        t += (uint64_t)in.k;
    }
    *total_k = t;
    return GF_OK;
}

// Rows of the per-wave multiplicity scratch: enough waves to fill the chip, bounded to 256 MiB.
int ensure_cnt(gf_ctx* ctx, uint64_t n_decisions, hipStream_t stream) {
    uint64_t rows = n_decisions < 1024 ? n_decisions : 1024;
    const uint64_t cap = (UINT64_C(256) << 20) / (4 * (uint64_t)ctx->n_slots);
    if (rows > cap) rows = cap;
    if (rows < 1) rows = 1;
    if (rows <= ctx->cnt_rows && ctx->cnt_slots == ctx->n_slots) return GF_OK;
    if (rows < ctx->cnt_rows) rows = ctx->cnt_rows;
    GF_HIP(ctx, gf_wait_stream(stream));
    GF_HIP(ctx, ctx->d_cnt.reserve(rows * ctx->n_slots));
    GF_HIP(ctx, hipMemsetAsync(ctx->d_cnt.ptr, 0, rows * ctx->n_slots * sizeof(uint32_t), stream));
    ctx->cnt_rows = (uint32_t)rows;
    ctx->cnt_slots = ctx->n_slots;
    return GF_OK;
}


// The narrow (scaled int32) working table of one FIFO chain.  The table's units are the gcds of its own columns; a batch
// whose requests are finer than that (a 2 GiB driver on a cluster whose free memory happens to be a multiple of 4 GiB)
// would have no scaled form and fall to the wide kernels.  When the host sees the batch (h_apps; gf_fit_batch) the units are
// therefore refined to gcd(table unit, every request of the batch) and the working copy is multiplied up by the ratio —
// as long as every scaled magnitude stays below 2^30; comparisons, subtractions and floor divisions are invariant under a
// common factor, so the chain is bit-identical.  Device-resident batches (gf_fit_batch_dev) keep the table's units.
// *proven (nullable): every request of the batch is a multiple of the resulting units and fits the narrow range, i.e. the
// narrow kernel will not hand the batch to its wide twin (what prepare_app tests on the device).
void narrow_units(const gf_ctx* ctx, const gf_app* h_apps, uint32_t n_apps, int64_t eff[3], int32_t factor[3], bool* proven) {
    refine_units(ctx->unit, ctx->nmax, h_apps, n_apps, eff, factor, proven);  // (gangfit_floor_units.h: the exact form)
}

// The smallest and largest table value per dimension, which the floored form is decided from: kept at install for a table the host
// built; a snapshot built on the device reads back magnitudes only, so the first chain that asks fetches them (one small kernel and
// a copy of six words, once per snapshot, on a route that had no narrow form before).
int table_range(gf_ctx* ctx) {
    if (ctx->range_known) return GF_OK;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, ctx->d_frange.reserve(6));
    GF_HIP(ctx, gangfit::launch_table_range(ctx->d_snap.ptr, ctx->d_slot_node.ptr, ctx->n_slots, ctx->d_frange.ptr, ctx->stream));
    int64_t h[6];
    GF_HIP(ctx, hipMemcpyAsync(h, ctx->d_frange.ptr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP(ctx, gf_wait_stream(ctx->stream));
    for (int j = 0; j < 3; ++j) {
        ctx->tmin[j] = h[j];
        ctx->tmax[j] = h[3 + j];
    }
    ctx->range_known = true;
    return GF_OK;
}

// The floored narrow form of a queue on this context (gangfit_floor_units.h), for a caller that knows the exact form does not serve:
// the table has none, or refine_units did not prove the queue.  true: unit[] divides every request and the floored table fits.
// Like chain_plan's scan of the exact form, a queue that shares a prefix with a cached floored chain is only scanned behind it:
// the cached units divide the prefix by construction and the table fits them, so when they divide the new applications too they
// are a valid set of units for this queue — and the checkpoints are scaled in them.  known_common (nullable): the length of that
// prefix, where the caller has counted it.
bool floor_plan(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, const gf_app* h_apps, int64_t unit[3], const uint32_t* known_common = nullptr) {
    if (!ctx->narrow_floor || !ctx->merged || ctx->fifo_generic || h_apps == nullptr) return false;
    const gf_ctx::ChainCache& C = ctx->chain;
    if (C.valid && C.floored && C.epoch == ctx->snap_epoch && C.algo == (int)algo && C.n_apps > 0) {
        uint32_t common = 0;
        if (known_common != nullptr) {
            common = *known_common;
        } else {
            const uint32_t lim = (n_apps < C.n_apps ? n_apps : C.n_apps) - 1;
            while (common < lim && std::memcmp(&h_apps[common], &C.apps[common], sizeof(gf_app)) == 0) ++common;
        }
        bool ok = common > 0;
        for (uint32_t i = common; i < n_apps && ok; ++i) {
            ok = h_apps[i].k >= 0 && h_apps[i].k <= GF_MAX_K;
            for (int j = 0; j < 3 && ok; ++j)
                for (const int64_t v : {h_apps[i].drv[j], h_apps[i].exe[j]})
                    ok = ok && v >= 0 && v % C.unit[j] == 0 && v / C.unit[j] < kNarrowBound;
        }
        if (ok) {
            for (int j = 0; j < 3; ++j) unit[j] = C.unit[j];
            return true;
        }
    }
    if (table_range(ctx) != GF_OK) {  // the range is not known: no floored form, the batch takes the route it took without one
        (void)hipGetLastError();
        ctx->err.clear();  // (not this call's failure: whatever is wrong with the device, the launch reports it)
        return false;
    }
    return floor_units(ctx->tmin, ctx->tmax, h_apps, n_apps, unit);
}

// How one FIFO chain of gf_fit_batch uses the chain cache (decided by chain_plan before the launch).
struct ChainRun {
    uint32_t a_begin = 0;        // first application this launch evaluates (a multiple of 1 << shift); 0 = from the snapshot
    bool record = false;         // dump checkpoints into ctx->chain.d_ckpt
    bool narrow_proven = false;  // every request has a scaled form (checked on the host): the wide twin is not launched
    uint32_t common = 0;         // leading applications identical to the cached queue's (>= a_begin): the cache keeps them
    bool from_tip = false;       // the launch starts from the cached chain's tip (a_begin = its tip_at, any value) instead of a checkpoint
    bool write_tip = false;      // the launch leaves its own tip in ctx->chain.d_tip
    int64_t eff[3] = {0, 0, 0};  // the narrow units of the queue and their factors (narrow_units): narrow_begin does not scan it again
    int32_t factor[3] = {1, 1, 1};
    // The chain runs on the FLOORED narrow form in units eff (factor = 1, narrow_proven): decided by gf_fit_batch before the route
    // where the table has no exact form, by chain_plan where the exact form did not prove the queue.  Such a run is handed on even
    // when the chain cache is not used (record = false, a_begin = 0): the launch needs its units.
    bool floored = false;
    uint32_t exact_fails_at = 0;  // ... and the shortest prefix of the queue that has no exact form (0: the table has none at all)
};

// One call's batch, as launch() and its helpers see it: the WHOLE queue on the device — q.n_apps, d_apps, d_results,
// d_exec_nodes, half (= placements + 1), d_chain_failed_at and stream; the rest of q is the launch's own — and what the caller
// knows beyond it.  gf_fit_batch_dev knows nothing: no records on the host, no plan, no offer.
struct FitCall {
    gangfit::ChainBatch q;
    const gf_app* h_apps = nullptr;  // the same records on the host (with exec_off)
    const ChainRun* run = nullptr;   // gf_fit_batch's plan for a FIFO chain that uses the chain cache
    struct HostIo {  // gf_fit_batch's offer to a FIFO chain: the device addresses of the pinned h_apps / h_results / h_exec /
                     // h_failed, where its first kernel may read the records and its last one write the answers (apps == nullptr: none)
        const gf_app* apps = nullptr;
        gf_result* results = nullptr;
        uint32_t* exec = nullptr;
        int32_t* failed = nullptr;
        bool apps_done = false;  // a kernel of this call writes (or a copy wrote) the records to d_apps
        bool out_done = false;   // the last kernel of this call writes the answers to the host buffers
    } host;
};

// restore (nullable): a checkpoint of an earlier chain in the SAME units — the working copy starts from it instead of the
// snapshot (incremental chains).
// The copies themselves are left to the chain's first kernel (io).
int narrow_begin(gf_ctx* ctx, const FitCall& call, gangfit::NarrowTable* nt, gangfit::ChainIo* io, const int32_t* restore = nullptr,
                 bool restore_dirty_chunks = false) {
    int64_t own_eff[3];
    int32_t own_factor[3];
    if (call.run == nullptr) narrow_units(ctx, call.h_apps, call.q.n_apps, own_eff, own_factor, nullptr);  // a call without a plan
    const int64_t* eff = call.run != nullptr ? call.run->eff : own_eff;
    const int32_t* factor = call.run != nullptr ? call.run->factor : own_factor;
    nt->cpu = ctx->d_nwork.ptr;
    nt->mem = nt->cpu + ctx->n_slots;
    nt->gpu = nt->mem + ctx->n_slots;
    for (int j = 0; j < 3; ++j) nt->unit[j] = eff[j];
    const size_t table_bytes = 3 * (size_t)ctx->n_slots * sizeof(int32_t);
    const bool whole = restore != nullptr && !restore_dirty_chunks;  // the checkpoint is the whole table
    const int32_t* src = nullptr;  // what the working copy starts from, when a plain copy makes it
    if (call.run != nullptr && call.run->floored) {
        // the floored snapshot in these units takes the place of d_nsnap: built once per (snapshot epoch, units)
        const size_t S = ctx->n_slots, C = ctx->n_chunks;
        if (ctx->floor_epoch != ctx->snap_epoch || std::memcmp(ctx->floor_unit, eff, sizeof ctx->floor_unit) != 0) {
            ctx->floor_epoch = 0;
            GF_HIP(ctx, ctx->d_fsnap.reserve(3 * S));
            GF_HIP(ctx, ctx->d_fcmax.reserve(3 * C));
            GF_HIP(ctx, ctx->d_frem.reserve(3 * S));
            GF_HIP(ctx, gangfit::launch_floor_snapshot(ctx->d_snap.ptr, ctx->d_slot_node.ptr, ctx->n_slots, ctx->n_chunks, eff,
                                                       ctx->d_fsnap.ptr, ctx->d_fcmax.ptr, ctx->d_frem.ptr, call.q.stream));
            std::memcpy(ctx->floor_unit, eff, sizeof ctx->floor_unit);
            ctx->floor_epoch = ctx->snap_epoch;
        }
        GF_HIP(ctx, ctx->d_nwork.reserve(3 * S));  // (a table without an exact form has none yet)
        nt->cpu = ctx->d_nwork.ptr;
        nt->mem = nt->cpu + S;
        nt->gpu = nt->mem + S;
        src = whole ? restore : ctx->d_fsnap.ptr;
        nt->cmax = ctx->d_fcmax.ptr;
    } else if (factor[0] == 1 && factor[1] == 1 && factor[2] == 1) {
        src = whole ? restore : ctx->d_nsnap.ptr;
        nt->cmax = ctx->d_ncmax.ptr;
    } else {
        GF_HIP(ctx, ctx->d_ncmax_w.reserve(3 * (size_t)ctx->n_chunks));
        GF_HIP(ctx, gangfit::launch_narrow_rescale(ctx->d_nsnap.ptr, ctx->d_nwork.ptr, ctx->n_slots, ctx->d_ncmax.ptr,
                                                   ctx->d_ncmax_w.ptr, ctx->n_chunks, factor, call.q.stream));
        if (whole) src = restore;
        nt->cmax = ctx->d_ncmax_w.ptr;
    }
    if (src != nullptr) {
        io->copy_src[0] = reinterpret_cast<const uint32_t*>(src);
        io->copy_dst[0] = reinterpret_cast<uint32_t*>(ctx->d_nwork.ptr);
        io->copy_words[0] = table_bytes / sizeof(uint32_t);
    }
    // ... or only the chunks that differ from the snapshot (in the chain's units), laid over it
    if (restore != nullptr && restore_dirty_chunks) {
        io->overlay = ctx->chain.d_ckpt.ptr;  // checkpoints 1 .. count, the latest delta of a chunk wins (delta format)
        io->overlay_stride = ctx->chain.slot_words;
        io->overlay_count = (uint32_t)((size_t)(restore - ctx->chain.d_ckpt.ptr) / ctx->chain.slot_words) + 1u;
        io->overlay_dst = ctx->d_nwork.ptr;
        io->overlay_slots = ctx->n_slots;
        io->overlay_chunks = ctx->n_chunks;
    }
    return GF_OK;
}

// The checkpoint arguments of a chain kernel and the table it starts from.
gangfit::ChainCkpt chain_ckpt_args(gf_ctx* ctx, const ChainRun* run, const int32_t** restore) {
    gangfit::ChainCkpt ck{nullptr, run ? run->a_begin : 0u, ctx->chain.shift, ctx->chain.slot_words, nullptr, nullptr};
    *restore = nullptr;
    if (run != nullptr && (run->record || run->a_begin > 0)) {
        ck.base = ctx->chain.d_ckpt.ptr;
        if (run->write_tip) ck.tip = ctx->chain.d_tip.ptr;
        if (run->a_begin > 0 && run->from_tip) {
            *restore = ctx->chain.d_tip.ptr;
        } else if (run->a_begin > 0) {
            *restore = ck.base + (size_t)((run->a_begin >> ck.shift) - 1u) * ctx->chain.slot_words;
            if (ctx->chain.dirty_format)
                ck.resume_mask = reinterpret_cast<const unsigned long long*>(*restore + 3 * (size_t)ctx->n_slots + (ctx->n_slots & 1u));
        }
    }
    return ck;
}

// The flag word of the chain being launched ("a request has no scaled form") and the ChainIo that goes with a launch on
// the records [a0, n_apps): the records come from the pinned host buffer when gf_fit_batch offered it, the answers go to
// the host buffers when the translate step is the last kernel to write them (answers_final).
int32_t* wide_flag(gf_ctx* ctx) { return ctx->d_wide_needed.ptr + (ctx->wide_seq & 1u); }
int chain_io_begin(gf_ctx* ctx, const FitCall& call, uint32_t a0, bool answers_final, gangfit::ChainIo* io) {
    if (ctx->wide_dirty) {
        GF_HIP(ctx, hipMemsetAsync(ctx->d_wide_needed.ptr, 0, 2 * sizeof(int32_t), call.q.stream));
        ctx->wide_dirty = false;
    }
    io->wide_clear = ctx->d_wide_needed.ptr + ((ctx->wide_seq & 1u) ^ 1u);
    const FitCall::HostIo& h = call.host;
    if (h.apps != nullptr && !h.apps_done) io->apps_src = h.apps + a0;
    if (h.apps != nullptr && answers_final) {
        io->h_results = h.results + a0;
        io->h_exec = h.exec;
        io->h_failed = h.failed;
    }
    ctx->wide_dirty = true;  // until chain_io_end: a launch that fails half way leaves the flag words in an unknown state
    return GF_OK;
}
void chain_io_end(gf_ctx* ctx, FitCall* call, const gangfit::ChainIo& io) {
    ctx->wide_dirty = false;
    ++ctx->wide_seq;
    if (io.apps_src != nullptr) call->host.apps_done = true;
    if (io.h_results != nullptr) call->host.out_done = true;
}
// Launch paths whose first kernel does not take the records from the host: an ordinary copy, once per gf_fit_batch.
int apps_to_device(gf_ctx* ctx, FitCall* call) {
    FitCall::HostIo& h = call->host;
    if (h.apps == nullptr || h.apps_done) return GF_OK;
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_apps.ptr, ctx->h_apps.ptr, (size_t)call->q.n_apps * sizeof(gf_app), hipMemcpyHostToDevice,
                               call->q.stream));
    h.apps_done = true;
    return GF_OK;
}

// Table slots the solo chain kernel keeps in LDS (whole 64-slot chunk blocks of 784 bytes next to its fixed tables).
uint32_t solo_lds_slots(const gf_ctx* ctx) {
    const size_t fixed = gangfit::fifo_solo_lds_bytes(0, ctx->n_chunks);
    const size_t per_chunk = gangfit::fifo_solo_lds_bytes(64, ctx->n_chunks) - fixed;
    const size_t fit = ctx->lds_budget > fixed ? (ctx->lds_budget - fixed) / per_chunk : 0;
    const size_t whole = (ctx->n_slots + 63u) / 64u;
    return (uint32_t)((fit < whole ? fit : whole) * 64u);
}
// ... and the wide chain kernel: as much of the table front as fits next to its fixed LDS needs stays in LDS for the whole chain
uint32_t wide_lds_slots(const gf_ctx* ctx) {
    const size_t fixed = gangfit::fifo_v2_lds_bytes(0, ctx->n_chunks);
    const uint32_t fit = ctx->lds_budget > fixed ? (uint32_t)((ctx->lds_budget - fixed) / 24) : 0;
    return fit >= (ctx->n_slots + 63) / 64 * 64 ? ctx->n_slots : fit / 64 * 64;  // the whole table (padded to full steps), or whole steps
}

// Geometry of the LDS-resident chains of the zone-aware tightly-pack packers (gangfit_fifo_zoned.inc) and of the
// minimal-fragmentation packers (gangfit_fifo_minfrag.inc); false = the tables do not fit and the generic chain serves.
bool zoned_lds_geometry(const gf_ctx* ctx, bool az_aware, uint32_t* n_shapes, uint32_t* lds_slots) {
    const uint32_t nz = ctx->n_zones;
    if (nz + (az_aware ? 1u : 0u) > 16) return false;
    // as many shape-index rows as LDS allows next to the masks (64 down to 4), then as much of the table as fits
    uint32_t ns = 64;
    const uint32_t n_cand = nz + (az_aware ? 1u : 0u);
    while (ns > 4 && gangfit::fifo_zoned_lds_bytes(64, ctx->n_chunks, nz, n_cand, ns) > ctx->lds_budget) ns /= 2;
    const size_t fixed = gangfit::fifo_zoned_lds_bytes(0, ctx->n_chunks, nz, n_cand, ns);
    if (ctx->lds_budget <= fixed + 12 * 64) return false;
    uint32_t slots = (uint32_t)((ctx->lds_budget - fixed) / 12);
    *lds_slots = slots >= ctx->n_slots ? ctx->n_slots : slots / 64 * 64;
    *n_shapes = ns;
    return true;
}
bool minfrag_lds_geometry(const gf_ctx* ctx, bool zoned, uint32_t* n_idx, uint32_t* lds_slots) {
    const uint32_t nz = ctx->n_zones;
    if (zoned && (nz == 0 || nz > 16)) return false;
    const uint32_t zviews = zoned ? nz : 0u;
    // 64 shape ids per role (rows of the capacity matrix, histograms); as many of them as LDS allows next to the masks also
    // get chunk-index rows (64 down to 0 — the histogram path does without), then as much of the table as fits
    uint32_t ni = 64;
    while (ni > 0 && gangfit::fifo_minfrag_lds_bytes(64, ctx->n_chunks, zviews, ni) > ctx->lds_budget) ni /= 2;
    const size_t fixed = gangfit::fifo_minfrag_lds_bytes(0, ctx->n_chunks, zviews, ni);
    if (ctx->lds_budget <= fixed + 12 * 64) return false;
    uint32_t slots = (uint32_t)((ctx->lds_budget - fixed) / 12);
    *lds_slots = slots >= ctx->n_slots ? ctx->n_slots : slots / 64 * 64;
    *n_idx = ni;
    return true;
}
// The whole record of that chain: the route's geometry and its global-memory tables — 64 shape ids per role; the capacity matrix,
// one int32 per (request shape, slot), unless it would exceed 1 GiB or option "minfrag_matrix" is off (capacities are then
// recomputed per pass); with it, the capacity histograms (option "minfrag_hist").
int minfrag_lds_chain(gf_ctx* ctx, bool zoned, uint32_t lds_slots, uint32_t n_idx, gangfit::MinfragLdsChain* m) {
    m->zoned = zoned;
    m->lds_slots = lds_slots;
    m->n_shapes = 64;
    m->n_idx = n_idx;
    m->d_capmat = m->d_hist = nullptr;
    if ((uint64_t)m->n_shapes * ctx->n_slots * sizeof(int32_t) <= (UINT64_C(1) << 30) && ctx->fifo_minfrag_matrix) {
        GF_HIP(ctx, ctx->d_capmat.reserve((size_t)m->n_shapes * ctx->n_slots + 2048));  // rows are read 2048 slots at a time
        m->d_capmat = ctx->d_capmat.ptr;
    }
    if (m->d_capmat != nullptr && ctx->fifo_minfrag_hist) {
        GF_HIP(ctx, ctx->d_mfhist.reserve(gangfit::fifo_minfrag_hist_words(zoned ? ctx->n_zones : 0u, m->n_shapes)));
        m->d_hist = ctx->d_mfhist.ptr;
    }
    return GF_OK;
}

// What serves a batch of (mode, packer) on this context: the kernel route and the geometry of its chain kernel.  It depends
// on the context's state and options only, never on the batch (what a batch adds — the narrow proof, the resume point —
// is ChainRun's), with one exception: on a table without an exact narrow form, `floored` (route_of's last argument) says that
// this queue has the floored one (floor_plan), which is as good a table for the LDS chain kernels.
struct Route {
    enum Kind {
        kPlain,       // independent, plain packers: fit_independent_kernel
        kZonedFused,  // independent, zone-aware packers in one launch: fit_zoned_fused_kernel
        kZonedFour,   // ... in four: fit_independent_kernel (az-aware) -> fit_zoned_kernel -> avg_efficiency_kernel -> zone_select_kernel
        kSolo,        // FIFO chain, tightly-pack / distribute-evenly: fit_fifo_solo_kernel, fit_fifo_chain_kernel as its wide twin
        kWide,        // ... fit_fifo_chain_kernel alone
        kZonedLds,    // FIFO chain, zone-aware tightly-pack: fit_fifo_zoned_lds_kernel, fit_fifo_generic_kernel as its wide twin
        kMinfragLds,  // FIFO chain, minimal-fragmentation packers: fit_fifo_minfrag_lds_kernel, the same twin
        kGeneric,     // FIFO chain of the zone-aware or minimal-fragmentation packers: fit_fifo_generic_kernel alone
    } kind = kPlain;
    int inner = GF_ALGO_TIGHTLY_PACK;  // the packer of one candidate view
    bool zoned = false, az_aware = false;
    uint32_t n_cand = 1;       // candidate views of an application
    uint32_t lds_slots = 0;    // LDS chain kernels: table slots kept in LDS
    uint32_t lds_slots_wide = 0;  // kSolo, kWide: ... by fit_fifo_chain_kernel
    uint32_t n_shapes = 0;     // kZonedLds: shape-index rows; kMinfragLds: shape ids with chunk-index rows (n_idx)
    bool table_in_lds = false; // LDS chain kernels: the whole table
    bool lds_chain() const { return kind == kSolo || kind == kZonedLds || kind == kMinfragLds; }
};

// Refusals in order: no orders (GF_ERR_STATE), a packer without a device path, an unknown mode (GF_ERR_UNSUPPORTED),
// a zone-aware packer without the schedulable columns (GF_ERR_STATE), a zone-aware FIFO chain with more than 63 zones
// (GF_ERR_UNSUPPORTED).
int route_of(gf_ctx* ctx, gf_mode mode, gf_algo algo, Route* r, bool floored = false) {
    *r = Route{};
    if (!ctx->have_orders) return fail(ctx, GF_ERR_STATE, "gf_snapshot_set + gf_orders_set must precede a fit");
    const bool zoned = is_zone_algo(algo);
    if (!zoned && !is_plain_algo(algo)) return fail(ctx, GF_ERR_UNSUPPORTED, "gf_algo %d is not served by the device path", (int)algo);
    if (mode != GF_MODE_INDEPENDENT && mode != GF_MODE_FIFO_CHAIN) return fail(ctx, GF_ERR_UNSUPPORTED, "unknown gf_mode %d", (int)mode);
    if (zoned && !ctx->have_sched)
        return fail(ctx, GF_ERR_STATE, "zone-aware packers compare packing efficiencies: gf_snapshot_set needs the schedulable columns");
    const uint32_t nz = ctx->n_zones;
    r->zoned = zoned;
    r->az_aware = algo == GF_ALGO_AZ_AWARE_TIGHTLY_PACK;
    r->inner = algo == GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION ? GF_ALGO_MINIMAL_FRAGMENTATION : (zoned ? GF_ALGO_TIGHTLY_PACK : (int)algo);
    r->n_cand = candidate_views(ctx, algo);
    if (mode == GF_MODE_INDEPENDENT) {
        r->kind = !zoned ? Route::kPlain : (ctx->zoned_fused && nz + 1 <= 64 ? Route::kZonedFused : Route::kZonedFour);
        return GF_OK;
    }
    if (zoned && nz + 1 > 64) return fail(ctx, GF_ERR_UNSUPPORTED, "more than 63 zones in a FIFO chain");
    // the LDS chain kernels work on the narrow table of the merged layout
    const bool lds = ctx->merged && (ctx->narrow_ok || floored) && !ctx->fifo_generic;
    if (r->inner != GF_ALGO_MINIMAL_FRAGMENTATION && !zoned) {
        r->kind = lds ? Route::kSolo : Route::kWide;
        if (lds) r->lds_slots = solo_lds_slots(ctx);
        r->lds_slots_wide = wide_lds_slots(ctx);
    } else if (r->inner == GF_ALGO_TIGHTLY_PACK) {
        r->kind = lds && zoned_lds_geometry(ctx, r->az_aware, &r->n_shapes, &r->lds_slots) ? Route::kZonedLds : Route::kGeneric;
    } else {
        r->kind = lds && minfrag_lds_geometry(ctx, zoned, &r->n_shapes, &r->lds_slots) ? Route::kMinfragLds : Route::kGeneric;
    }
    r->table_in_lds = r->lds_chain() && r->lds_slots >= ctx->n_slots;
    return GF_OK;
}

// What the resident worker serves (gf_worker_fit, gf_worker_submit_dev): route_of's rules for an independent batch, then the
// worker's own.  Refusals in order, all before anything touches the device: a view or a multi-device parent
// (GF_ERR_UNSUPPORTED); route_of's — no orders, a zone-aware packer without the schedulable columns (GF_ERR_STATE), a packer
// without a device path (GF_ERR_UNSUPPORTED) —; a zone-aware packer on a context without a zone assignment (gf_zones_set was not
// called since the snapshot, or the evaluation list is empty), with more than 64 candidate views — the one-launch kernel's
// bound —, or single-az-minimal-fragmentation, whose view code has no worker instance (GF_ERR_UNSUPPORTED each).
int worker_route_of(gf_ctx* ctx, gf_algo algo) {
    if (!ctx->group.empty() || ctx->view_of != nullptr)
        return fail(ctx, GF_ERR_UNSUPPORTED, "the resident worker serves plain contexts (no views, one device)");
    Route r;
    if (const int rc = route_of(ctx, GF_MODE_INDEPENDENT, algo, &r); rc != GF_OK) return rc;
    if (!r.zoned) return GF_OK;
    if (ctx->zone.empty() || ctx->n_zones == 0)
        return fail(ctx, GF_ERR_UNSUPPORTED, "the resident worker serves a zone-aware packer on installed zones (gf_zones_set)");
    if (r.n_cand > 64)
        return fail(ctx, GF_ERR_UNSUPPORTED, "the resident worker serves at most 64 candidate views (%u zones%s)", ctx->n_zones,
                    r.az_aware ? " + the plain order" : "");
    if (r.inner != GF_ALGO_TIGHTLY_PACK)
        return fail(ctx, GF_ERR_UNSUPPORTED, "the resident worker does not serve single-az-minimal-fragmentation");
    return GF_OK;
}

gangfit::ZoneTable zone_table(const gf_ctx* ctx) {
    return gangfit::ZoneTable{ctx->d_zmasks.ptr, ctx->d_zmasks.ptr + (size_t)ctx->zd_row0 * ctx->zstride, ctx->n_zones, ctx->zstride};
}

// What every LDS chain kernel's launch starts with: the scaled records, the checkpoint arguments, the ChainIo and the narrow
// working table (the copies themselves are left to the chain's first kernel).  chain_io_end(ctx, call, b->io) follows the launch.
int lds_chain_begin(gf_ctx* ctx, const FitCall& call, bool answers_final, bool restore_dirty_chunks, gangfit::ChainBatch* b,
                    gangfit::NarrowTable* nt) {
    GF_HIP(ctx, ctx->d_napps.reserve(call.q.n_apps));
    const int32_t* restore = nullptr;
    b->ckpt = chain_ckpt_args(ctx, call.run, &restore);
    if (const int rc = chain_io_begin(ctx, call, b->ckpt.a_base, answers_final, &b->io); rc != GF_OK) return rc;
    return narrow_begin(ctx, call, nt, &b->io, restore, restore_dirty_chunks);
}

// Which chains resume: every packer, when its LDS-resident chain kernel serves (the route) and every request has a scaled
// form.  Returns false when the chain cache is not used for this call (run is then not handed on; only its
// a_begin = 0 is read).
bool chain_plan(gf_ctx* ctx, const Route& route, gf_algo algo, uint32_t n_apps, const gf_app* h_apps, ChainRun* run) {
    const ChainRun before = *run;  // (gf_fit_batch has decided the floored form where the table has no exact one)
    *run = ChainRun{};
    if (before.floored && route.lds_chain()) {
        run->floored = run->narrow_proven = true;
        for (int j = 0; j < 3; ++j) run->eff[j] = before.eff[j];
    }
    gf_ctx::ChainCache& C = ctx->chain;
    // (the LDS chain kernels dump and restore the checkpoints.)  Without the cache the host proves nothing about an exact table's
    // queue — narrow_begin scans the units, the guarded twin stands by — and so the floored form is not tried there either: with
    // option "chain_cache" = 0 or the counters on, a table that HAS an exact form keeps today's route for every queue.
    if (!route.lds_chain() || !ctx->chain_cache_on || ctx->stats_on) return false;
    const bool solo = route.kind == Route::kSolo, table_in_lds = route.table_in_lds;
    // The narrow units of the queue and the proof that every request has a scaled form.  A scan of the whole queue is twelve
    // 64-bit divisions per application — more host time than a resumed chain takes on the device —, so a queue that shares a
    // prefix with the cached one is only scanned behind it: the cached units divide the prefix by construction, and when they
    // divide the new applications too they ARE a valid set of units for this queue (any common divisor keeps the chain exact;
    // the checkpoints are scaled in them).  Otherwise: the full scan, and the chain replays.
    int64_t(&eff)[3] = run->eff;
    int32_t(&factor)[3] = run->factor;
    bool proven = false;
    uint32_t common = 0;  // applications this queue shares with the cached one, from the front (the last of either excluded)
    bool units_from_cache = false;
    const bool cached = C.valid && C.epoch == ctx->snap_epoch && C.algo == (int)algo && C.n_apps > 0;
    if (cached) {
        const uint32_t lim = (n_apps < C.n_apps ? n_apps : C.n_apps) - 1;
        while (common < lim && std::memcmp(&h_apps[common], &C.apps[common], sizeof(gf_app)) == 0) ++common;
    }
    // The floored form (gangfit_floor_units.h) serves only a queue the exact form does not prove.  Decided before the route where
    // the table has no exact form; else here, behind the scan that did not prove the queue — or without that scan, when the cached
    // chain is a floored one and this queue still begins with the prefix that had no exact form then (exact_fails_at): it has none now.
    bool floor_tried = false;
    if (run->floored) {
        proven = units_from_cache = true;  // (nothing left to scan; `same` below compares the units with the cached chain's)
    } else if (cached && C.floored) {
        if (common >= C.exact_fails_at) {
            floor_tried = true;
            if (floor_plan(ctx, algo, n_apps, h_apps, eff, &common)) {
                run->floored = run->narrow_proven = proven = units_from_cache = true;  // (whatever becomes of the cache below)
                run->exact_fails_at = C.exact_fails_at;
            }
        }
    } else if (cached) {
        bool ok = common > 0;
        for (uint32_t i = common; i < n_apps && ok; ++i) {
            ok = h_apps[i].k >= 0 && h_apps[i].k <= GF_MAX_K;
            for (int j = 0; j < 3 && ok; ++j)
                for (const int64_t v : {h_apps[i].drv[j], h_apps[i].exe[j]})
                    ok = ok && v >= 0 && v % C.unit[j] == 0 && v / C.unit[j] < (INT64_C(1) << 30);
        }
        if (ok) {
            units_from_cache = proven = true;
            for (int j = 0; j < 3; ++j) {
                eff[j] = C.unit[j];
                factor[j] = (int32_t)(ctx->unit[j] / C.unit[j]);  // (the cached chain passed the range check with these)
            }
        }
    }
    if (!units_from_cache) {
        narrow_units(ctx, h_apps, n_apps, eff, factor, &proven);
        if (!proven && !floor_tried) {
            int64_t fu[3];
            if (floor_plan(ctx, algo, n_apps, h_apps, fu, cached ? &common : nullptr)) {
                run->floored = run->narrow_proven = proven = true;  // (whatever becomes of the cache below)
                run->exact_fails_at = exact_fails_at(ctx->unit, ctx->nmax, h_apps, n_apps);
                for (int j = 0; j < 3; ++j) {
                    eff[j] = fu[j];
                    factor[j] = 1;
                }
            }
        }
    }
    if (!proven) return false;
    // checkpoint interval: 32 applications while a dump is cheap — the whole table from LDS, or (solo kernel, table with a
    // global tail) only the chunks that differ from the snapshot; 128 where a dump copies a table that lives in global memory
    // (the zone-aware and minimal-fragmentation chains beyond their LDS front); wider when 128 dumps would not fit 2 GiB
    const size_t slot_words = gangfit::chain_ckpt_stride(ctx->n_slots, ctx->n_chunks);
    const bool dirty_format = solo && !table_in_lds;
    uint32_t shift = (table_in_lds || solo) ? 5 : 7;
    while (shift < 12 && (size_t)(4096u >> shift) * slot_words * sizeof(int32_t) > (UINT64_C(2) << 30)) ++shift;
    const size_t n_ck = (size_t)((n_apps - 1) >> shift);
    if (n_ck * slot_words * sizeof(int32_t) > (UINT64_C(4) << 30)) return false;
    uint32_t a_begin = 0;
    const bool same = C.valid && C.epoch == ctx->snap_epoch && C.algo == (int)algo && C.shift == shift && C.dirty_format == dirty_format &&
                      C.slot_words == slot_words && C.unit[0] == eff[0] && C.unit[1] == eff[1] && C.unit[2] == eff[2] &&
                      C.floored == run->floored;
    if (same) {
        // longest common prefix of the two queues, the last application of either excluded (nothing is committed behind
        // the driver being filtered: its table is not a state of the longer chain)
        uint32_t c = common >> shift;
        if (c > C.n_ckpt) c = C.n_ckpt;
        a_begin = c << shift;
    }
    // The cached chain's TIP (whole table in LDS): the table before the application that chain ended at.  A queue
    // that agrees with the cached one up to there — the Filter of the next driver in creation order, the same Filter again —
    // resumes from it and evaluates one or two applications instead of everything since the last checkpoint.  Not when this
    // chain would cross a checkpoint boundary: it then starts from the checkpoint, so that the boundary's dump is made (the
    // kernel dumps where a refill of its staging buffer falls, every 32 applications from ITS first one).
    const bool tip_possible = table_in_lds;  // (every LDS chain kernel leaves a tip when its whole table sits in LDS)
    bool from_tip = false;
    if (same && tip_possible && C.tip_valid && C.d_tip.ptr != nullptr && C.tip_at > a_begin && C.tip_at <= common &&
        ((n_apps - 1) >> shift) == (C.tip_at >> shift)) {
        a_begin = C.tip_at;
        from_tip = true;
    }
    if (tip_possible && slot_words > C.d_tip.cap) {
        if (C.d_tip.ptr) (void)gf_wait_stream(ctx->stream);
        if (C.d_tip.reserve(slot_words) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        C.tip_valid = false;
        if (from_tip) {  // (cannot happen: a valid tip lives in a buffer of this size)
            from_tip = false;
            a_begin = 0;
        }
    }
    // the checkpoint buffer keeps what it holds when it grows
    if (n_ck * slot_words > C.d_ckpt.cap) {
        size_t want = C.d_ckpt.cap ? C.d_ckpt.cap : 32 * slot_words;
        while (want < n_ck * slot_words) want *= 2;
        int32_t* fresh = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&fresh), want * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        const size_t keep = (size_t)(a_begin >> shift) * slot_words;
        if (keep && hipMemcpy(fresh, C.d_ckpt.ptr, keep * sizeof(int32_t), hipMemcpyDeviceToDevice) != hipSuccess) {
            (void)hipFree(fresh);
            return false;
        }
        if (C.d_ckpt.ptr) {
            (void)gf_wait_stream(ctx->stream);
            (void)hipFree(C.d_ckpt.ptr);
        }
        C.d_ckpt.ptr = fresh;
        C.d_ckpt.cap = want;
    }
    if (!same) C.valid = false;
    C.shift = shift;
    C.slot_words = slot_words;
    C.dirty_format = dirty_format;
    for (int j = 0; j < 3; ++j) C.unit[j] = eff[j];
    C.floored = run->floored;
    C.exact_fails_at = run->exact_fails_at;
    run->a_begin = a_begin;
    run->common = same ? common : 0;
    run->record = true;
    run->from_tip = from_tip;
    run->write_tip = tip_possible;
    run->narrow_proven = true;
    return true;
}

// The chain that just ran becomes the cached one (h_results / h_exec hold the complete answer, prefix included).
void chain_commit(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, uint64_t total_k, int32_t failed_at, const ChainRun& run) {
    gf_ctx::ChainCache& C = ctx->chain;
    // what the cached queue already holds stays: records up to the common prefix, answers up to the first application evaluated
    const uint32_t keep_apps = C.valid ? (run.common < n_apps ? run.common : n_apps) : 0u;
    const uint32_t keep_res = C.valid ? run.a_begin : 0u;
    const uint64_t keep_exec = keep_res > 0 ? ctx->h_apps.ptr[keep_res].exec_off : 0;
    C.apps.resize(n_apps);
    std::memcpy(C.apps.data() + keep_apps, ctx->h_apps.ptr + keep_apps, (size_t)(n_apps - keep_apps) * sizeof(gf_app));
    C.results.resize(n_apps);
    std::memcpy(C.results.data() + keep_res, ctx->h_results.ptr + keep_res, (size_t)(n_apps - keep_res) * sizeof(gf_result));
    C.exec.resize(total_k);
    if (total_k > keep_exec)
        std::memcpy(C.exec.data() + keep_exec, ctx->h_exec.ptr + keep_exec, (size_t)(total_k - keep_exec) * sizeof(uint32_t));
    C.n_apps = n_apps;
    C.failed_at = failed_at;
    C.algo = (int)algo;
    C.epoch = ctx->snap_epoch;
    // the chain reached application `last` (the one it aborted at, else the filtered driver): dumps exist up to there
    const uint32_t last = failed_at >= 0 ? (uint32_t)failed_at : n_apps - 1;
    C.n_ckpt = last >> C.shift;
    C.tip_valid = run.write_tip;  // the epilogue left the table before application `last`
    C.tip_at = last;
    C.valid = true;
    ctx->chain_stat[0] += 1;
    ctx->chain_stat[1] += run.a_begin > 0 ? 1 : 0;
    ctx->chain_stat[2] += (failed_at >= 0 ? (uint32_t)failed_at + 1 : n_apps) - run.a_begin;
    ctx->chain_stat[3] += run.a_begin;
}

// The tables of a chain: the wide working table, nt — its scaled twin —, the zones, and the remainders when nt is the floored form.
gangfit::ChainTables chain_tables(gf_ctx* ctx, const Route& r, const gangfit::NarrowTable& nt, bool floored = false) {
    return gangfit::ChainTables{make_table(ctx, ctx->d_work.ptr), nt, r.zoned ? zone_table(ctx) : gangfit::ZoneTable{nullptr, nullptr, 0, 0},
                                r.zoned ? ctx->d_sched.ptr : nullptr, floored ? ctx->d_frem.ptr : nullptr};
}
// Makes b — the whole queue with its ckpt and io set — the batch of the queue's tail [b->ckpt.a_base, n_apps), once the context's
// buffers have their sizes: exec_off is absolute, so the record, scaled-record and result pointers are all that moves.
void chain_batch_tail(gf_ctx* ctx, gangfit::ChainBatch* b) {
    const uint32_t a0 = b->ckpt.a_base;
    b->n_apps -= a0;
    b->d_apps += a0;
    b->d_napps = ctx->d_napps.ptr + a0;
    b->d_wide_needed = wide_flag(ctx);
    b->d_results += a0;
    b->d_scratch = ctx->d_scratch.ptr;
    b->d_zexec = ctx->d_zexec.ptr;
    b->d_stats = ctx->stats_on ? ctx->d_stats.ptr : nullptr;
}

// Behind a chain on the floored narrow form: its epilogue left q' * unit in the wide working table, the residuals are q' * unit + r.
int floor_residuals(gf_ctx* ctx, hipStream_t stream) {
    GF_HIP(ctx, gangfit::launch_floor_residual(ctx->d_work.ptr, ctx->d_frem.ptr, ctx->n_slots, stream));
    return GF_OK;
}

// Independent batches: every application against the snapshot.  The FitBatch of n_apps records and their answers on the context's
// tables and buffers as they stand — of a FitCall's queue, or (gf_fit_feasible, which then puts its own buffers in) of records alone.
gangfit::FitBatch fit_batch_of(gf_ctx* ctx, const Route& r, uint32_t n_apps, const gf_app* d_apps, gf_result* d_results,
                               uint32_t* d_exec_nodes, uint64_t half, hipStream_t stream) {
    return gangfit::FitBatch{.table = make_table(ctx, ctx->d_snap.ptr), .gpu_view = make_sparse(ctx),
                             .zones = r.zoned ? zone_table(ctx) : gangfit::ZoneTable{nullptr, nullptr, 0, 0},
                             .d_sched = r.zoned ? ctx->d_sched.ptr : nullptr, .n_apps = n_apps, .d_apps = d_apps, .d_results = d_results,
                             .d_exec_nodes = d_exec_nodes, .d_scratch = ctx->d_scratch.ptr, .half = half, .d_zexec = ctx->d_zexec.ptr,
                             .d_stats = ctx->stats_on ? ctx->d_stats.ptr : nullptr, .stream = stream};
}
gangfit::FitBatch fit_batch_of(gf_ctx* ctx, const Route& r, const FitCall& c) {
    return fit_batch_of(ctx, r, c.q.n_apps, c.q.d_apps, c.q.d_results, c.q.d_exec_nodes, c.q.half, c.q.stream);
}
int launch_plain(gf_ctx* ctx, const Route& r, FitCall* call) {
    if (const int arc = apps_to_device(ctx, call); arc != GF_OK) return arc;
    GF_HIP(ctx, gangfit::launch_fit_independent((gf_algo)r.inner, fit_batch_of(ctx, r, *call)));
    return GF_OK;
}
// ... of the zone-aware packers in one launch: a workgroup per application decides every candidate view, chooses and writes the
// final answer — d_apps / d_results / d_exec_nodes may be device-mapped host memory (gf_fit_batch)
int launch_zoned_fused(gf_ctx* ctx, const Route& r, FitCall* call) {
    GF_HIP(ctx, ctx->d_zexec.reserve(((uint64_t)ctx->n_zones + 1) * call->q.half));
    if (const int arc = apps_to_device(ctx, call); arc != GF_OK) return arc;
    GF_HIP(ctx, gangfit::launch_fit_zoned_fused(r.inner, r.az_aware, fit_batch_of(ctx, r, *call)));
    return GF_OK;
}
// ... in four
int launch_zoned_four(gf_ctx* ctx, const Route& r, FitCall* call) {
    const uint32_t nz = ctx->n_zones;
    const uint64_t half = call->q.half, n_dec = (uint64_t)call->q.n_apps * (nz ? nz : 1);
    GF_HIP(ctx, ctx->d_zres.reserve(n_dec));
    GF_HIP(ctx, ctx->d_zexec.reserve(((uint64_t)nz + 1) * half));
    GF_HIP(ctx, ctx->d_zavg.reserve(4 * n_dec));
    if (const int rc = ensure_cnt(ctx, n_dec < 16 ? 16 : n_dec, call->q.stream); rc != GF_OK) return rc;
    if (const int arc = apps_to_device(ctx, call); arc != GF_OK) return arc;
    const gangfit::ZoneBuffers zb{ctx->d_zres.ptr, ctx->d_zavg.ptr, ctx->d_cnt.ptr, ctx->cnt_rows};
    GF_HIP(ctx, gangfit::launch_fit_zoned(r.inner, r.az_aware, r.inner != GF_ALGO_MINIMAL_FRAGMENTATION, slot_eff_tables(ctx, ctx->d_snap.ptr),
                                          zb, fit_batch_of(ctx, r, *call)));
    return GF_OK;
}

// FIFO chain of tightly-pack / distribute-evenly: the solo kernel (kSolo) with the wide kernel as its guarded twin unless
// the host has proven every request's scaled form, or the wide kernel alone (kWide).
int launch_plain_chain(gf_ctx* ctx, const Route& r, FitCall* call) {
    gangfit::FifoPlan plan{};
    plan.narrow = r.kind == Route::kSolo;
    plan.wide = !(plan.narrow && call->run != nullptr && call->run->narrow_proven);
    plan.lds_slots_v2 = r.lds_slots_wide;
    plan.lds_slots_solo = r.lds_slots;
    // every chain starts from the snapshot: availableNodesSchedulingMetadata is rebuilt per request (resource.go:303).
    // The solo kernel rewrites every real slot of the wide working table in its epilogue: the copy is only needed by the
    // wide kernel.  Like the narrow table's, the copy is made by the chain's first kernel (ChainIo).
    gangfit::ChainBatch b = call->q;
    gangfit::NarrowTable nt{};
    b.ckpt.shift = ctx->chain.shift;
    if (plan.narrow) {
        if (const int rc = lds_chain_begin(ctx, *call, true, ctx->chain.dirty_format, &b, &nt); rc != GF_OK) return rc;
    } else if (const int rc = chain_io_begin(ctx, *call, 0, true, &b.io); rc != GF_OK) {
        return rc;
    }
    if (plan.wide) {
        b.io.copy_src[1] = reinterpret_cast<const uint32_t*>(ctx->d_snap.ptr);
        b.io.copy_dst[1] = reinterpret_cast<uint32_t*>(ctx->d_work.ptr);
        b.io.copy_words[1] = 3 * (size_t)ctx->n_slots * (sizeof(int64_t) / sizeof(uint32_t));
    }
    ctx->work_valid = true;
    chain_batch_tail(ctx, &b);
    const uint64_t heads_lo = b.ckpt.a_base > 0 ? call->h_apps[b.ckpt.a_base].exec_off : 0;  // placements of the skipped prefix
    const bool floored = plan.narrow && call->run != nullptr && call->run->floored;
    GF_HIP(ctx, gangfit::launch_fit_fifo((gf_algo)r.inner, plan, chain_tables(ctx, r, nt, floored), b, heads_lo));
    chain_io_end(ctx, call, b.io);
    return floored ? floor_residuals(ctx, call->q.stream) : GF_OK;
}

// FIFO chains of the zone-aware and minimal-fragmentation packers.  What the generic chain kernel needs before anything of
// the chain is launched; twin_runs = false: the LDS chain serves for certain and rewrites every real slot of the wide working
// table in its epilogue — no record copy, no table copy.
int generic_chain_begin(gf_ctx* ctx, const Route& r, FitCall* call, bool twin_runs) {
    const uint32_t nz = r.zoned ? ctx->n_zones : 0u;
    GF_HIP(ctx, ctx->d_zexec.reserve(((uint64_t)nz + 1) * (call->q.half)));
    if (r.zoned) {
        const uint64_t n_dec = (uint64_t)call->q.n_apps * (nz ? nz : 1);
        if (const int rc = ensure_cnt(ctx, n_dec < 16 ? 16 : n_dec, call->q.stream); rc != GF_OK) return rc;
        if (ctx->cnt_rows < 16) return fail(ctx, GF_ERR_HIP, "multiplicity scratch too small");
    }
    // every chain starts from the snapshot: availableNodesSchedulingMetadata is rebuilt per request (resource.go:303)
    if (twin_runs) {
        if (const int arc = apps_to_device(ctx, call); arc != GF_OK) return arc;  // the generic kernel reads d_apps
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_work.ptr, ctx->d_snap.ptr, 3 * (size_t)ctx->n_slots * sizeof(int64_t),
                                   hipMemcpyDeviceToDevice, call->q.stream));
    }
    ctx->work_valid = true;
    return GF_OK;
}
// The generic chain kernel on the whole queue (one wavefront per candidate view, the working table in global memory), behind
// generic_chain_begin; run_if (nullable): the flag word of the LDS chain it is the twin of — it only runs when a request had no
// scaled form.
int launch_generic_chain(gf_ctx* ctx, const Route& r, FitCall* call, const int32_t* run_if) {
    const gangfit::GenericChain g{r.inner, r.zoned, r.az_aware, r.zoned ? ctx->d_cnt.ptr : nullptr, run_if};
    gangfit::ChainBatch b = call->q;
    chain_batch_tail(ctx, &b);
    GF_HIP(ctx, gangfit::launch_fit_fifo_generic(g, chain_tables(ctx, r, gangfit::NarrowTable{}), b));
    return GF_OK;
}

// The LDS chain kernel (kZonedLds, kMinfragLds), with the generic chain kernel as its guarded twin unless the host has proven
// every request's scaled form.
int launch_lds_chain(gf_ctx* ctx, const Route& r, FitCall* call) {
    const bool proven = call->run != nullptr && call->run->narrow_proven;
    if (const int rc = generic_chain_begin(ctx, r, call, !proven); rc != GF_OK) return rc;
    GF_HIP(ctx, ctx->d_zexec.reserve(32 * (call->q.half)));
    gangfit::ChainBatch b = call->q;
    gangfit::NarrowTable nt{};
    if (const int rc = lds_chain_begin(ctx, *call, proven, false, &b, &nt); rc != GF_OK) return rc;
    chain_batch_tail(ctx, &b);
    const bool floored = proven && call->run->floored;
    if (r.kind == Route::kZonedLds) {
        GF_HIP(ctx, gangfit::launch_fit_fifo_zoned_lds(r.az_aware, r.lds_slots, r.n_shapes, chain_tables(ctx, r, nt, floored), b));
    } else {
        gangfit::MinfragLdsChain m;
        if (const int rc = minfrag_lds_chain(ctx, r.zoned, r.lds_slots, /* n_idx */ r.n_shapes, &m); rc != GF_OK) return rc;
        GF_HIP(ctx, gangfit::launch_fit_fifo_minfrag_lds(m, chain_tables(ctx, r, nt, floored), b));
    }
    chain_io_end(ctx, call, b.io);
    if (floored) return floor_residuals(ctx, call->q.stream);
    return proven ? GF_OK : launch_generic_chain(ctx, r, call, b.d_wide_needed);
}

// Launches the route's kernels.
int launch(gf_ctx* ctx, const Route& r, FitCall* call) {
    GF_HIP(ctx, ctx->d_scratch.reserve(2 * (call->q.half)));
    switch (r.kind) {
    case Route::kPlain:
        return launch_plain(ctx, r, call);
    case Route::kZonedFused:
        return launch_zoned_fused(ctx, r, call);
    case Route::kZonedFour:
        return launch_zoned_four(ctx, r, call);
    case Route::kSolo:
    case Route::kWide:
        return launch_plain_chain(ctx, r, call);
    case Route::kZonedLds:
    case Route::kMinfragLds:
        return launch_lds_chain(ctx, r, call);
    case Route::kGeneric:
        if (const int rc = generic_chain_begin(ctx, r, call, true); rc != GF_OK) return rc;
        return launch_generic_chain(ctx, r, call, nullptr);
    }
    return fail(ctx, GF_ERR_INVALID, "unknown kernel route %d", (int)r.kind);
}

// gf_call_phases of a blocking call, from its five time stamps: stage | launch | wait | copy-out | total
using call_clock = std::chrono::steady_clock;
void set_call_phases(gf_ctx* ctx, call_clock::time_point entry, call_clock::time_point staged, call_clock::time_point launched,
                     call_clock::time_point done, call_clock::time_point out) {
    const call_clock::time_point t[5] = {entry, staged, launched, done, out};
    for (int i = 0; i < 4; ++i) ctx->call_phase_us[i] = std::chrono::duration<double, std::micro>(t[i + 1] - t[i]).count();
    ctx->call_phase_us[4] = std::chrono::duration<double, std::micro>(out - entry).count();
}

}  // namespace gfapi

extern "C" {

int gf_chain_cache_stats(gf_ctx* ctx, int reset, uint64_t out[4]) {
    GF_DELEGATE(ctx, gf_chain_cache_stats(ctx, reset, out));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    if (out)
        for (int i = 0; i < 4; ++i) out[i] = ctx->chain_stat[i];
    if (reset)
        for (uint64_t& v : ctx->chain_stat) v = 0;
    return GF_OK;
}

int gf_chain_units(gf_ctx* ctx, int64_t out[4]) {
    GF_DELEGATE(ctx, gf_chain_units(ctx, out));
    if (!ctx || !out) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    for (int i = 0; i < 4; ++i) out[i] = ctx->chain_unit_last[i];
    return GF_OK;
}

int gf_fit_batch(gf_ctx* ctx, gf_mode mode, gf_algo algo, uint32_t n_apps, const gf_app* apps, gf_result* results,
                 uint32_t* exec_nodes, uint64_t exec_nodes_cap, int32_t* chain_failed_at) {
    if (ctx != nullptr && !ctx->group.empty())
        return group_fit_batch(ctx, mode, algo, n_apps, apps, results, exec_nodes, exec_nodes_cap, chain_failed_at);
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_VIEW_ENTER(ctx)
    if (n_apps > 0 && (!apps || !results)) return fail(ctx, GF_ERR_INVALID, "apps/results must not be NULL");
    if (chain_failed_at) *chain_failed_at = -1;
    if (n_apps == 0) return GF_OK;
    const auto t_entry = call_clock::now();
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, ctx->h_apps.reserve(n_apps));
    uint64_t total_k = 0;
    if (const int rc = check_apps(ctx, n_apps, apps, ctx->h_apps.ptr, &total_k); rc != GF_OK) return rc;
    if (total_k > exec_nodes_cap || (total_k > 0 && !exec_nodes))
        return fail(ctx, GF_ERR_CAPACITY, "exec_nodes holds %llu entries, %llu needed",
                    (unsigned long long)exec_nodes_cap, (unsigned long long)total_k);
    // A table without an exact narrow form takes the wide kernels — unless this queue has the floored form (floor_plan), which
    // the route has to know: the LDS chain kernels then serve it as they serve an exact table.
    ChainRun run;
    if (mode == GF_MODE_FIFO_CHAIN && ctx->have_orders && !ctx->narrow_ok && floor_plan(ctx, algo, n_apps, ctx->h_apps.ptr, run.eff))
        run.floored = true;
    Route route;
    if (const int rc = route_of(ctx, mode, algo, &route, run.floored); rc != GF_OK) {
        ctx->chain.valid = false;
        return rc;
    }
    GF_HIP(ctx, ctx->d_apps.reserve(n_apps));
    GF_HIP(ctx, ctx->d_results.reserve(n_apps));
    GF_HIP(ctx, ctx->d_exec.reserve(total_k + 1));
    GF_HIP(ctx, ctx->h_results.reserve(n_apps));
    GF_HIP(ctx, ctx->h_exec.reserve(total_k + 1));
    hipStream_t st = ctx->stream;
    FitCall call;  // (the device arrays are chosen below)
    call.q.n_apps = n_apps;
    call.q.half = total_k + 1;
    call.q.d_chain_failed_at = ctx->d_failed.ptr;
    call.q.stream = st;
    call.h_apps = ctx->h_apps.ptr;
    // Small independent batches of the plain packers skip the three staging copies: the kernel reads the app records from
    // the pinned staging buffer and writes results and placements straight into pinned host memory (posted PCIe writes,
    // visible when the kernel has completed).  A copy engine round trip costs more than the whole kernel at these sizes.
    if (ctx->zero_copy && (route.kind == Route::kPlain || route.kind == Route::kZonedFused) &&
        (uint64_t)n_apps * sizeof(gf_app) + total_k * sizeof(uint32_t) <= (UINT64_C(4) << 20)) {
        void *da = ctx->h_apps.dev, *dr = ctx->h_results.dev, *de = ctx->h_exec.dev;
        if (da != nullptr && dr != nullptr && de != nullptr) {
            const auto t_staged = call_clock::now();
            call.q.d_apps = static_cast<const gf_app*>(da);
            call.q.d_results = static_cast<gf_result*>(dr);
            call.q.d_exec_nodes = static_cast<uint32_t*>(de);
            const int rc0 = launch(ctx, route, &call);
            if (rc0 != GF_OK) return rc0;
            const auto t_launched = call_clock::now();
            GF_HIP(ctx, gf_wait_stream(st));
            const auto t_done = call_clock::now();
            std::memcpy(results, ctx->h_results.ptr, (size_t)n_apps * sizeof(gf_result));
            if (total_k) std::memcpy(exec_nodes, ctx->h_exec.ptr, (size_t)total_k * sizeof(uint32_t));
            set_call_phases(ctx, t_entry, t_staged, t_launched, t_done, call_clock::now());
            return GF_OK;
        }
    }
    // ---- FIFO chains of the plain packers on the solo kernel: resume from the last chain's checkpoints where the queues agree
    const bool use_cache = chain_plan(ctx, route, algo, n_apps, ctx->h_apps.ptr, &run);
    const uint32_t a0 = run.a_begin;
    const uint64_t k0 = a0 > 0 ? ctx->h_apps.ptr[a0].exec_off : 0;  // placements of the skipped prefix
    // The answers travel to the pinned host buffers by posted writes of a kernel when the buffers are device-mapped: three
    // copy-engine transfers behind the last kernel are three hand-overs between the compute queue and a copy engine — a
    // visible part of a resumed chain, and what keeps chains on different streams from overlapping.  A FIFO chain goes
    // further: its first kernel reads the records from the pinned buffer and its last one writes the answers there
    // (FitCall::HostIo), which makes a Filter three launches and no copy.
    void *da = ctx->h_apps.dev, *dr = ctx->h_results.dev, *de = ctx->h_exec.dev, *df = ctx->h_failed.dev;
    const bool mapped = ctx->zero_copy && dr != nullptr && de != nullptr && df != nullptr;
    call.q.d_apps = ctx->d_apps.ptr;
    call.q.d_results = ctx->d_results.ptr;
    call.q.d_exec_nodes = ctx->d_exec.ptr;
    call.run = use_cache || run.floored ? &run : nullptr;  // (a floored chain needs its units even when nothing is cached)
    if (mapped && mode == GF_MODE_FIFO_CHAIN && da != nullptr) {
        call.host.apps = static_cast<const gf_app*>(da);
        call.host.results = static_cast<gf_result*>(dr);
        call.host.exec = static_cast<uint32_t*>(de);
        call.host.failed = static_cast<int32_t*>(df);
    } else {
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_apps.ptr + a0, ctx->h_apps.ptr + a0, (size_t)(n_apps - a0) * sizeof(gf_app),
                                   hipMemcpyHostToDevice, st));
    }
    const int rc = launch(ctx, route, &call);
    if (rc != GF_OK) {
        ctx->chain.valid = false;
        return rc;
    }
    if (call.host.out_done) {
        // the chain's last kernel wrote results, placements and the abort index to the host buffers
    } else if (mapped) {
        gangfit::CopyOut co{};
        co.src[0] = reinterpret_cast<const uint32_t*>(ctx->d_results.ptr + a0);
        co.dst[0] = reinterpret_cast<uint32_t*>(static_cast<gf_result*>(dr) + a0);
        co.words[0] = (size_t)(n_apps - a0) * (sizeof(gf_result) / 4);
        co.src[1] = ctx->d_exec.ptr + k0;
        co.dst[1] = static_cast<uint32_t*>(de) + k0;
        co.words[1] = (size_t)(total_k - k0);
        co.src[2] = reinterpret_cast<const uint32_t*>(ctx->d_failed.ptr);
        co.dst[2] = static_cast<uint32_t*>(df);
        co.words[2] = mode == GF_MODE_FIFO_CHAIN ? 1 : 0;
        GF_HIP(ctx, gangfit::launch_copy_out(co, st));
    } else {
        (void)hipGetLastError();
        GF_HIP(ctx, hipMemcpyAsync(ctx->h_results.ptr + a0, ctx->d_results.ptr + a0, (size_t)(n_apps - a0) * sizeof(gf_result),
                                   hipMemcpyDeviceToHost, st));
        if (total_k > k0)
            GF_HIP(ctx, hipMemcpyAsync(ctx->h_exec.ptr + k0, ctx->d_exec.ptr + k0, (size_t)(total_k - k0) * sizeof(uint32_t),
                                       hipMemcpyDeviceToHost, st));
        if (mode == GF_MODE_FIFO_CHAIN)
            GF_HIP(ctx, hipMemcpyAsync(ctx->h_failed.ptr, ctx->d_failed.ptr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    const hipError_t we = gf_wait_stream(st);
    if (we != hipSuccess) {
        ctx->chain.valid = false;
        return fail(ctx, GF_ERR_HIP, "waiting for the batch failed: %s", hipGetErrorString(we));
    }
    int32_t failed_at = mode == GF_MODE_FIFO_CHAIN ? ctx->h_failed.ptr[0] : -1;
    if (a0 > 0) {  // the prefix the chain did not replay comes from the cache, straight to the caller; the kernel counted from a0
        std::memcpy(results, ctx->chain.results.data(), (size_t)a0 * sizeof(gf_result));
        if (k0) std::memcpy(exec_nodes, ctx->chain.exec.data(), (size_t)k0 * sizeof(uint32_t));
        if (failed_at >= 0) failed_at += (int32_t)a0;
    }
    if (use_cache) chain_commit(ctx, algo, n_apps, total_k, failed_at, run);
    if (call.run != nullptr && route.lds_chain() && run.narrow_proven) {  // gf_chain_units: an LDS chain kernel served for certain
        for (int j = 0; j < 3; ++j) ctx->chain_unit_last[j] = run.eff[j];
        ctx->chain_unit_last[3] = run.floored ? 1 : 0;
    }
    std::memcpy(results + a0, ctx->h_results.ptr + a0, (size_t)(n_apps - a0) * sizeof(gf_result));
    if (total_k > k0) std::memcpy(exec_nodes + k0, ctx->h_exec.ptr + k0, (size_t)(total_k - k0) * sizeof(uint32_t));
    if (mode == GF_MODE_FIFO_CHAIN && chain_failed_at) *chain_failed_at = failed_at;
    return GF_OK;
}

int gf_fit_feasible(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, const gf_app* apps, uint8_t* has_capacity) {
    if (!ctx) return GF_ERR_INVALID;
    if (n_apps > 0 && (!apps || !has_capacity)) return fail(ctx, GF_ERR_INVALID, "apps/has_capacity must not be NULL");
    if (n_apps == 0) return GF_OK;
    // the plain packers and the one-launch zone route have a feasibility-only kernel.  A multi-device context, the four-kernel
    // zone route or a refusal: the full batch, of which only HasCapacity is handed on (gf_fit_batch reports the refusal)
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    Route route;
    if (!ctx->group.empty() || route_of(ctx, GF_MODE_INDEPENDENT, algo, &route) != GF_OK || route.kind == Route::kZonedFour) {
        uint64_t total_k = 0;
        if (const int rc = check_apps(ctx, n_apps, apps, nullptr, &total_k); rc != GF_OK) return rc;  // the sizes below come from it
        std::vector<gf_result> res;
        std::vector<uint32_t> exec;
        try {  // no exception crosses the C ABI
            res.resize(n_apps);
            exec.resize((size_t)total_k + 1);
        } catch (const std::exception&) {
            return fail(ctx, GF_ERR_CAPACITY, "gf_fit_feasible: no host memory for %u results + %llu placements", n_apps,
                        (unsigned long long)total_k);
        }
        const int rc = gf_fit_batch(ctx, GF_MODE_INDEPENDENT, algo, n_apps, apps, res.data(), exec.data(), total_k, nullptr);
        if (rc != GF_OK) return rc;
        for (uint32_t a = 0; a < n_apps; ++a) has_capacity[a] = res[a].has_capacity ? 1 : 0;
        return GF_OK;
    }
    GF_VIEW_ENTER(ctx)
    if (n_apps >= 0x80000000u) return fail(ctx, GF_ERR_INVALID, "n_apps = %u", n_apps);
    const auto t_entry = call_clock::now();
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, ctx->h_apps.reserve(n_apps));
    uint64_t total_k = 0;  // the placements are still made (same decision code): into device memory, where they stay
    if (const int rc = check_apps(ctx, n_apps, apps, ctx->h_apps.ptr, &total_k); rc != GF_OK) return rc;
    const uint64_t half = total_k + 1;
    GF_HIP(ctx, ctx->d_feas_exec.reserve(total_k + 1));  // private to this entry point: see gf_ctx::d_feas_exec
    GF_HIP(ctx, ctx->d_feas_scratch.reserve(2 * half));
    GF_HIP(ctx, ctx->h_feasible.reserve((size_t)n_apps + 4));  // the kernel writes whole words
    hipStream_t st = ctx->stream;
    {  // the collection words start at zero; the kernel's collecting workgroup leaves them at zero again
        const uint32_t* before = ctx->d_feasible_sync.ptr;
        GF_HIP(ctx, ctx->d_feasible_sync.reserve(((size_t)n_apps + 3) / 4 + 4));
        if (ctx->d_feasible_sync.ptr != before || ctx->feasible_sync_dirty) {
            GF_HIP(ctx, hipMemsetAsync(ctx->d_feasible_sync.ptr, 0, ctx->d_feasible_sync.cap * sizeof(uint32_t), st));
            ctx->feasible_sync_dirty = false;
        }
    }
    const gf_app* d_apps = ctx->h_apps.dev;
    uint8_t* d_feas = ctx->h_feasible.dev;
    const bool mapped = ctx->zero_copy && d_apps != nullptr && d_feas != nullptr &&
                        (uint64_t)n_apps * sizeof(gf_app) <= (UINT64_C(4) << 20);
    DeviceBuf<uint8_t> staged;  // (hosts without mapped pinned memory, or very large batches: two copies around the kernel)
    if (!mapped) {
        GF_HIP(ctx, ctx->d_apps.reserve(n_apps));
        GF_HIP(ctx, staged.reserve((size_t)n_apps + 4));
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_apps.ptr, ctx->h_apps.ptr, (size_t)n_apps * sizeof(gf_app), hipMemcpyHostToDevice, st));
        d_apps = ctx->d_apps.ptr;
        d_feas = staged.ptr;
    }
    // Mapped staging: the answers announce themselves.  Every byte of the pinned array is preset to "not yet"; the kernel's
    // collecting workgroup writes the whole array with system-scope (written-through) stores, and the caller watches the bytes
    // arrive instead of waiting for the kernel-end write-back and the stream's completion signal (6-8 us of a 12-15 us wait:
    // profiles/r5h_feasible_call.txt).  A byte that has arrived is final, so no ordering between them is needed; when all have
    // arrived every wavefront has read its record and made its decision — what the kernel still owes (placement stores to device
    // memory, its end) goes to buffers only this entry point uses (d_feas_*), and the next gf_fit_feasible is ordered behind it
    // on the context's stream: an entry point that launches on a caller's stream, or copies on the null stream, shares nothing
    // with the tail of this kernel.  gf_fit_batch cannot do the same:
    // 13 000 placement words written through over the host link cost more than the signal they replace (round 4: 30.3 us
    // against 23.3).
    constexpr uint8_t kNotYet = 0xFF;
    // (GANGFIT_WAIT=block: the host cannot spare a core for the duration of a call — no spinning on the answers either)
    const bool announce = mapped && ctx->feasible_announce && !wait_blocking();
    if (announce) std::memset(ctx->h_feasible.ptr, kNotYet, n_apps);
    const auto t_staged = call_clock::now();
    hipError_t e = route.kind == Route::kZonedFused ? ctx->d_feas_zexec.reserve(((uint64_t)ctx->n_zones + 1) * half) : hipSuccess;
    if (e == hipSuccess) {
        // no result records; the placements stay in this entry point's own buffers
        gangfit::FitBatch b = fit_batch_of(ctx, route, n_apps, d_apps, nullptr, ctx->d_feas_exec.ptr, half, st);
        b.d_scratch = ctx->d_feas_scratch.ptr;
        b.d_zexec = ctx->d_feas_zexec.ptr;
        b.d_stats = nullptr;
        b.feasible = gangfit::FeasibleOut{d_feas, ctx->d_feasible_sync.ptr, ctx->eff_nonneg};
        e = route.kind == Route::kZonedFused ? gangfit::launch_fit_zoned_fused(route.inner, route.az_aware, b)
                                             : gangfit::launch_fit_independent((gf_algo)route.inner, b);
    }
    if (e == hipSuccess && !mapped)
        e = hipMemcpyAsync(ctx->h_feasible.ptr, staged.ptr, n_apps, hipMemcpyDeviceToHost, st);
    const auto t_launched = call_clock::now();
    bool arrived = false;
    if (e == hipSuccess && announce) {
        const volatile uint8_t* f = ctx->h_feasible.ptr;
        uint32_t next = 0;  // everything before it has arrived
        for (uint32_t spin = 0;; ++spin) {
            while (next < n_apps && f[next] != kNotYet) ++next;
            if (next == n_apps) {
                arrived = true;
                break;
            }
            __builtin_ia32_pause();
            // a kernel that faulted never writes: after 2 ms the stream is asked (it reports the error, or completes)
            if ((spin & 255u) == 255u && call_clock::now() - t_launched > std::chrono::milliseconds(2)) break;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (e == hipSuccess && !arrived) e = gf_wait_stream(st);
    if (e != hipSuccess) ctx->feasible_sync_dirty = true;  // the collection may have stopped anywhere
    const auto t_done = call_clock::now();
    staged.release();
    if (e != hipSuccess) return fail(ctx, GF_ERR_HIP, "gf_fit_feasible failed: %s", hipGetErrorString(e));
    std::memcpy(has_capacity, ctx->h_feasible.ptr, n_apps);
    set_call_phases(ctx, t_entry, t_staged, t_launched, t_done, call_clock::now());
    return GF_OK;
}

int gf_fit_batch_dev(gf_ctx* ctx, gf_mode mode, gf_algo algo, uint32_t n_apps, const gf_app* d_apps,
                     gf_result* d_results, uint32_t* d_exec_nodes, uint64_t exec_nodes_len, int32_t* d_chain_failed_at,
                     void* stream) {
    GF_DELEGATE(ctx, gf_fit_batch_dev(ctx, mode, algo, n_apps, d_apps, d_results, d_exec_nodes, exec_nodes_len, d_chain_failed_at, stream));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_VIEW_ENTER(ctx)  // launch() grows buffers and flips state flags
    if (n_apps > 0 && (!d_apps || !d_results)) return fail(ctx, GF_ERR_INVALID, "device apps/results must not be NULL");
    if (mode == GF_MODE_FIFO_CHAIN && !d_chain_failed_at) d_chain_failed_at = ctx->d_failed.ptr;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    Route route;
    if (const int rc = route_of(ctx, mode, algo, &route); rc != GF_OK) return rc;
    FitCall call;  // no host records, no plan, no offer
    call.q.n_apps = n_apps;
    call.q.d_apps = d_apps;
    call.q.d_results = d_results;
    call.q.d_exec_nodes = d_exec_nodes;
    call.q.half = exec_nodes_len + 1;
    call.q.d_chain_failed_at = d_chain_failed_at;
    call.q.stream = st;
    return launch(ctx, route, &call);
}


int gf_spark_binpack(gf_ctx* ctx, gf_algo algo, const gf_app* app, gf_result* result, uint32_t* exec_nodes,
                     uint64_t exec_nodes_cap) {
    return gf_fit_batch(ctx, GF_MODE_INDEPENDENT, algo, 1, app, result, exec_nodes, exec_nodes_cap, nullptr);
}

int gf_executor_fit(gf_ctx* ctx, int minimal_fragmentation, uint32_t n_req, const int64_t* exe, const int64_t* reserved,
                    const uint32_t* hosts_app, uint32_t* node_out) {
    return gf_executor_fit_zoned(ctx, minimal_fragmentation, n_req, exe, reserved, hosts_app, nullptr, nullptr, node_out);
}

int gf_executor_fit_zoned(gf_ctx* ctx, int minimal_fragmentation, uint32_t n_req, const int64_t* exe, const int64_t* reserved,
                          const uint32_t* hosts_app, const uint32_t* node_zone, const uint32_t* req_zone, uint32_t* node_out) {
    GF_DELEGATE(ctx, gf_executor_fit_zoned(ctx, minimal_fragmentation, n_req, exe, reserved, hosts_app, node_zone, req_zone, node_out));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_VIEW_ENTER(ctx)
    if (n_req == 0) return GF_OK;
    if (!exe || !node_out) return fail(ctx, GF_ERR_INVALID, "exe/node_out must not be NULL");
    if (!ctx->have_orders) return fail(ctx, GF_ERR_STATE, "gf_snapshot_set + gf_orders_set must precede gf_executor_fit");
    if ((node_zone == nullptr) != (req_zone == nullptr))
        return fail(ctx, GF_ERR_INVALID, "node_zone and req_zone come together (both NULL: no zone step)");
    for (size_t i = 0; i < 3 * (size_t)n_req; ++i)
        if (exe[i] < 0 || exe[i] >= GF_MAX_ABS_QUANTITY) return fail(ctx, GF_ERR_INVALID, "executor request outside [0, 2^62)");
    const uint32_t n = ctx->n_nodes;
    if (node_zone)
        for (uint32_t i = 0; i < n; ++i)
            if (node_zone[i] == GF_ANY_ZONE) return fail(ctx, GF_ERR_INVALID, "node_zone[%u] is GF_ANY_ZONE: a node has a zone", i);
    if (reserved)
        for (size_t i = 0; i < 3 * (size_t)n; ++i)
            if (reserved[i] < 0 || reserved[i] >= GF_MAX_ABS_QUANTITY)
                return fail(ctx, GF_ERR_INVALID, "reserved[%zu] outside [0, 2^62)", i);
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t words = (n + 31) / 32;
    GF_HIP(ctx, ctx->d_xexe.reserve(3 * (size_t)n_req));
    GF_HIP(ctx, ctx->d_xout.reserve(n_req));
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_xexe.ptr, exe, 3 * (size_t)n_req * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (reserved) {
        GF_HIP(ctx, ctx->d_xreserved.reserve(3 * (size_t)n + 1));
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_xreserved.ptr, reserved, 3 * (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    const bool with_hosts = minimal_fragmentation && hosts_app && words > 0;
    if (with_hosts) {
        GF_HIP(ctx, ctx->d_xhosts.reserve((size_t)n_req * words));
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_xhosts.ptr, hosts_app, (size_t)n_req * words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    if (node_zone) {
        GF_HIP(ctx, ctx->d_xnzone.reserve((size_t)n + 1));
        GF_HIP(ctx, ctx->d_xqzone.reserve(n_req));
        if (n) GF_HIP(ctx, hipMemcpyAsync(ctx->d_xnzone.ptr, node_zone, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_xqzone.ptr, req_zone, (size_t)n_req * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    GF_HIP(ctx, gangfit::launch_executor_fit(minimal_fragmentation != 0, make_table(ctx, ctx->d_snap.ptr),
                                             reserved ? ctx->d_xreserved.ptr : nullptr, n_req, ctx->d_xexe.ptr,
                                             with_hosts ? ctx->d_xhosts.ptr : nullptr, words, node_zone ? ctx->d_xnzone.ptr : nullptr,
                                             node_zone ? ctx->d_xqzone.ptr : nullptr, ctx->d_xout.ptr, st));
    GF_HIP(ctx, hipMemcpyAsync(node_out, ctx->d_xout.ptr, (size_t)n_req * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GF_HIP(ctx, gf_wait_stream(st));
    return GF_OK;
}

int gf_find_nodes(gf_ctx* ctx, int chained, uint32_t n_req, const int64_t* exe, const int32_t* k, gf_find_result* results,
                  uint32_t* exec_nodes, uint64_t exec_nodes_cap, uint32_t* reserved_adds) {
    GF_DELEGATE(ctx, gf_find_nodes(ctx, chained, n_req, exe, k, results, exec_nodes, exec_nodes_cap, reserved_adds));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_VIEW_ENTER(ctx)
    if (n_req == 0) return GF_OK;
    if (!exe || !k || !results) return fail(ctx, GF_ERR_INVALID, "exe/k/results must not be NULL");
    if (!ctx->have_orders) return fail(ctx, GF_ERR_STATE, "gf_snapshot_set + gf_orders_set must precede gf_find_nodes");
    for (size_t i = 0; i < 3 * (size_t)n_req; ++i)
        if (exe[i] < 0 || exe[i] >= GF_MAX_ABS_QUANTITY) return fail(ctx, GF_ERR_INVALID, "executor request outside [0, 2^62)");
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, ctx->h_foff.reserve(n_req));
    uint64_t total_k = 0;
    for (uint32_t q = 0; q < n_req; ++q) {
        if (k[q] < 0 || k[q] > GF_MAX_K) return fail(ctx, GF_ERR_INVALID, "k[%u] = %d outside [0, %d]", q, k[q], GF_MAX_K);
        ctx->h_foff.ptr[q] = total_k;
        total_k += (uint64_t)k[q];
    }
    if (total_k > exec_nodes_cap || (total_k > 0 && !exec_nodes))
        return fail(ctx, GF_ERR_CAPACITY, "exec_nodes holds %llu entries, %llu needed", (unsigned long long)exec_nodes_cap,
                    (unsigned long long)total_k);
    const uint32_t n = ctx->n_nodes;
    hipStream_t st = ctx->stream;
    GF_HIP(ctx, ctx->d_xexe.reserve(3 * (size_t)n_req));
    GF_HIP(ctx, ctx->d_fk.reserve(n_req));
    GF_HIP(ctx, ctx->d_foff.reserve(n_req));
    GF_HIP(ctx, ctx->d_fres.reserve(n_req));
    GF_HIP(ctx, ctx->d_exec.reserve(total_k + 1));
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_xexe.ptr, exe, 3 * (size_t)n_req * sizeof(int64_t), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_fk.ptr, k, (size_t)n_req * sizeof(int32_t), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_foff.ptr, ctx->h_foff.ptr, (size_t)n_req * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    uint32_t* d_adds = nullptr;
    if (reserved_adds && n > 0) {
        GF_HIP(ctx, ctx->d_fadds.reserve((size_t)n_req * n));
        GF_HIP(ctx, hipMemsetAsync(ctx->d_fadds.ptr, 0, (size_t)n_req * n * sizeof(uint32_t), st));
        d_adds = ctx->d_fadds.ptr;
    }
    if (chained) {  // every reconcile starts from the snapshot (availableResourcesPerInstanceGroup, failover.go:286-322)
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_work.ptr, ctx->d_snap.ptr, 3 * (size_t)ctx->n_slots * sizeof(int64_t),
                                   hipMemcpyDeviceToDevice, st));
        ctx->work_valid = true;
    }
    GF_HIP(ctx, gangfit::launch_find_nodes(chained != 0, make_table(ctx, chained ? ctx->d_work.ptr : ctx->d_snap.ptr), n_req,
                                           ctx->d_xexe.ptr, ctx->d_fk.ptr, ctx->d_foff.ptr, ctx->d_fres.ptr, ctx->d_exec.ptr,
                                           d_adds, st));
    GF_HIP(ctx, hipMemcpyAsync(results, ctx->d_fres.ptr, (size_t)n_req * sizeof(gf_find_result), hipMemcpyDeviceToHost, st));
    if (total_k)
        GF_HIP(ctx, hipMemcpyAsync(exec_nodes, ctx->d_exec.ptr, (size_t)total_k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (d_adds)
        GF_HIP(ctx, hipMemcpyAsync(reserved_adds, d_adds, (size_t)n_req * n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GF_HIP(ctx, gf_wait_stream(st));
    return GF_OK;
}


int gf_avg_packing_efficiency(gf_ctx* ctx, gf_algo algo, uint32_t n_apps, const gf_app* apps, const gf_result* results,
                              const uint32_t* exec_nodes, uint64_t exec_nodes_len, gf_avg_efficiency* out) {
    GF_DELEGATE(ctx, gf_avg_packing_efficiency(ctx, algo, n_apps, apps, results, exec_nodes, exec_nodes_len, out));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_VIEW_ENTER(ctx)
    if (n_apps > 0 && (!apps || !results || !out)) return fail(ctx, GF_ERR_INVALID, "apps/results/out must not be NULL");
    if (n_apps == 0) return GF_OK;
    if (!ctx->have_orders) return fail(ctx, GF_ERR_STATE, "gf_snapshot_set + gf_orders_set must precede");
    if (!ctx->have_sched) return fail(ctx, GF_ERR_STATE, "efficiencies need the schedulable columns of gf_snapshot_set");
    if (int mrc = materialize_host(ctx); mrc != GF_OK) return mrc;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    // validate the lists on the host: every placed node must own a slot (it came out of one of the two orders)
    uint64_t total_k = 0;
    GF_HIP(ctx, ctx->h_apps.reserve(n_apps));
    for (uint32_t a = 0; a < n_apps; ++a) {
        gf_app& o = ctx->h_apps.ptr[a];
        o = apps[a];
        if (const int rc = check_app(ctx, a, o); rc != GF_OK) return rc;
        o.exec_off = total_k;
        if (results[a].has_capacity) {
            const uint32_t d = results[a].driver_node;
            if (d >= ctx->n_nodes || ctx->h_node_slot[d] == GF_NO_NODE)
                return fail(ctx, GF_ERR_INVALID, "results[%u].driver_node is not a candidate node", a);
            if (total_k + (uint64_t)o.k > exec_nodes_len || (o.k > 0 && !exec_nodes))
                return fail(ctx, GF_ERR_CAPACITY, "exec_nodes too short");
            for (int32_t i = 0; i < o.k; ++i) {
                const uint32_t n = exec_nodes[total_k + i];
                if (n >= ctx->n_nodes || ctx->h_node_slot[n] == GF_NO_NODE)
                    return fail(ctx, GF_ERR_INVALID, "exec_nodes[%llu] is not a candidate node",
                                (unsigned long long)(total_k + i));
            }
        }
        total_k += (uint64_t)o.k;
    }
    hipStream_t st = ctx->stream;
    GF_HIP(ctx, ctx->d_apps.reserve(n_apps));
    GF_HIP(ctx, ctx->d_results.reserve(n_apps));
    GF_HIP(ctx, ctx->d_exec.reserve(total_k + 1));
    GF_HIP(ctx, ctx->d_avg.reserve(4 * (size_t)n_apps));
    GF_HIP(ctx, ctx->h_avg.reserve(4 * (size_t)n_apps));
    int rc = ensure_cnt(ctx, n_apps, st);
    if (rc != GF_OK) return rc;
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_apps.ptr, ctx->h_apps.ptr, (size_t)n_apps * sizeof(gf_app), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_results.ptr, results, (size_t)n_apps * sizeof(gf_result), hipMemcpyHostToDevice, st));
    if (total_k && exec_nodes)
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_exec.ptr, exec_nodes, (size_t)(total_k <= exec_nodes_len ? total_k : exec_nodes_len) * sizeof(uint32_t),
                                   hipMemcpyHostToDevice, st));
    GF_HIP(ctx, gangfit::launch_avg_efficiency(reserves_executors(algo), make_table(ctx, ctx->d_snap.ptr),
                                               slot_eff_tables(ctx, ctx->d_snap.ptr), ctx->d_cnt.ptr, ctx->cnt_rows,
                                               n_apps, ctx->d_apps.ptr, ctx->d_results.ptr, ctx->d_exec.ptr,
                                               ctx->d_avg.ptr, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->h_avg.ptr, ctx->d_avg.ptr, 4 * (size_t)n_apps * sizeof(double), hipMemcpyDeviceToHost, st));
    GF_HIP(ctx, gf_wait_stream(st));
    static_assert(sizeof(gf_avg_efficiency) == 4 * sizeof(double), "gf_avg_efficiency layout");
    std::memcpy(out, ctx->h_avg.ptr, 4 * (size_t)n_apps * sizeof(double));
    return GF_OK;
}

int gf_packing_efficiencies(gf_ctx* ctx, gf_algo algo, const gf_app* app, const gf_result* result,
                            const uint32_t* exec_nodes, double* eff_out) {
    GF_DELEGATE(ctx, gf_packing_efficiencies(ctx, algo, app, result, exec_nodes, eff_out));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_VIEW_ENTER(ctx)
    if (!app || !result || !eff_out) return fail(ctx, GF_ERR_INVALID, "app/result/eff_out must not be NULL");
    if (!ctx->have_snapshot || !ctx->have_sched)
        return fail(ctx, GF_ERR_STATE, "efficiencies need gf_snapshot_set with the schedulable columns");
    if (const int rc = check_app(ctx, 0, *app); rc != GF_OK) return rc;
    if (result->has_capacity && app->k > 0 && !exec_nodes) return fail(ctx, GF_ERR_INVALID, "exec_nodes must not be NULL");
    const uint32_t n = ctx->n_nodes;
    if (n == 0) return GF_OK;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    GF_HIP(ctx, ctx->d_apps.reserve(1));
    GF_HIP(ctx, ctx->d_results.reserve(1));
    GF_HIP(ctx, ctx->d_exec.reserve((size_t)app->k + 1));
    GF_HIP(ctx, ctx->d_reserved.reserve(3 * (size_t)n));
    GF_HIP(ctx, ctx->d_eff.reserve(3 * (size_t)n));
    GF_HIP(ctx, ctx->h_apps.reserve(1));
    ctx->h_apps.ptr[0] = *app;
    ctx->h_apps.ptr[0].exec_off = 0;
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_apps.ptr, ctx->h_apps.ptr, sizeof(gf_app), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_results.ptr, result, sizeof(gf_result), hipMemcpyHostToDevice, st));
    if (result->has_capacity && app->k > 0)
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_exec.ptr, exec_nodes, (size_t)app->k * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    gangfit::EffTables e;
    for (int j = 0; j < 3; ++j) {
        e.avail[j] = ctx->d_node_tab.ptr + (size_t)j * n;
        e.sched[j] = ctx->d_node_tab.ptr + (size_t)(3 + j) * n;
    }
    GF_HIP(ctx, gangfit::launch_node_efficiencies(reserves_executors(algo), e, n, app->k, ctx->d_apps.ptr,
                                                  ctx->d_results.ptr, ctx->d_exec.ptr, ctx->d_reserved.ptr,
                                                  ctx->d_eff.ptr, st));
    GF_HIP(ctx, hipMemcpyAsync(eff_out, ctx->d_eff.ptr, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    GF_HIP(ctx, gf_wait_stream(st));
    return GF_OK;
}

}  // extern "C"
