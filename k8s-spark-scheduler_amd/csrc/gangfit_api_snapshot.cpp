// gangfit_api_snapshot.cpp — the snapshot side of the C ABI.  gf_snapshot_set / gf_zones_set record the snapshot; gf_orders_set plans
// and fills the slot layout on the host (gangfit_slot_layout.h: pure code), uploads it and commits it through install_layout — the
// one place a layout becomes current, shared with the on-device finalize of gf_snapshot_build*.  Then the resident cluster columns
// and usage sums, and gf_snapshot_build* (reservation replay + metadata + priority sort, slot tables on the device or the host).
#include "gangfit_ctx.h"
#include "gangfit_label_plan.h"

using namespace gfapi;

namespace gfapi {

// After a device-side gf_snapshot_build the host mirrors of the snapshot are fetched only when something asks for them.
int materialize_host(gf_ctx* ctx) {
    if (!ctx->host_stale) return GF_OK;
    const size_t N = ctx->n_nodes;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, ctx->h_bcols.reserve(6 * N + 1));
    GF_HIP(ctx, ctx->h_border.reserve(N + 1));
    if (N) {
        GF_HIP(ctx, hipMemcpyAsync(ctx->h_bcols.ptr, ctx->d_node_tab.ptr, 6 * N * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        GF_HIP(ctx, hipMemcpyAsync(ctx->h_border.ptr, ctx->d_node_slot.ptr, N * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    GF_HIP(ctx, gf_wait_stream(ctx->stream));
    for (int j = 0; j < 3; ++j) {
        ctx->avail[j].assign(ctx->h_bcols.ptr + (size_t)j * N, ctx->h_bcols.ptr + (size_t)(j + 1) * N);
        ctx->sched[j].assign(ctx->h_bcols.ptr + (size_t)(3 + j) * N, ctx->h_bcols.ptr + (size_t)(4 + j) * N);
    }
    ctx->h_node_slot.assign(ctx->h_border.ptr, ctx->h_border.ptr + N);
    ctx->host_stale = false;
    return GF_OK;
}

}  // namespace gfapi

namespace {

// A call every device of a multi-device context repeats (each keeps the same resident data): the sub-contexts in order, under the
// group's lock; the first failure stops the round and its error becomes the group's.  A failure past the first device leaves
// the devices apart: `poison` (usage_ok, cl_over_ok or none) is then cleared on every one of them.
template <class Call>
int each_device(gf_ctx* g, bool gf_ctx::*poison, Call call) {
    std::lock_guard<std::recursive_mutex> glock(g->mu);
    for (size_t i = 0; i < g->group.size(); ++i) {
        const int rc = call(g->group[i], i == 0);
        if (rc == GF_OK) continue;
        g->err = g->group[i]->err;
        if (i > 0 && poison != nullptr)
            for (gf_ctx* sub : g->group) sub->*poison = false;
        return rc;
    }
    return GF_OK;
}

// Reserve the device buffer (never left NULL) and copy n elements from pinned memory behind the stream.
template <typename T>
hipError_t upload(DeviceBuf<T>& d, const T* src, size_t n, hipStream_t st) {
    const hipError_t e = d.reserve(n + 1);
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpyAsync(d.ptr, src, n * sizeof(T), hipMemcpyHostToDevice, st);
}

// The one place a layout becomes current: gf_orders_set's host-built tables and the on-device finalize both end here.
void install_layout(gf_ctx* ctx, LayoutFacts&& f) {
    ctx->n_x = f.n_x;
    ctx->n_d = f.n_d;
    ctx->n_slots = f.n_slots;
    ctx->n_chunks = f.n_chunks;
    ctx->merged = f.merged;
    ctx->d_identity = f.identity;
    ctx->narrow_ok = f.narrow_ok;
    for (int j = 0; j < 3; ++j) {
        ctx->unit[j] = f.unit[j];
        ctx->nmax[j] = f.nmax[j];
        ctx->tmin[j] = f.tmin[j];
        ctx->tmax[j] = f.tmax[j];
    }
    ctx->range_known = f.range_known;
    ctx->floor_epoch = 0;  // the floored snapshot of the old table, and what gf_chain_units reports
    for (int64_t& u : ctx->chain_unit_last) u = 0;
    ctx->n_g = f.n_g;
    ctx->n_gpad = f.n_gpad;
    ctx->g_prefix = std::move(f.g_prefix);
    ctx->n_zones = f.n_zones;
    ctx->zstride = f.zstride;
    ctx->zd_row0 = f.zd_row0;
    ctx->zspan_ok = f.zspan_ok;
    ctx->host_stale = f.host_stale;
    if (!f.host_stale) ctx->h_node_slot = std::move(f.node_slot);  // else materialize_host fetches it on demand
    ctx->have_orders = true;
    ctx->work_valid = false;
    ++ctx->snap_epoch;  // drops the chain cache
}

}  // namespace

extern "C" {

int gf_snapshot_set(gf_ctx* ctx, uint32_t n_nodes, const int64_t* avail_cpu_milli, const int64_t* avail_mem_bytes,
                    const int64_t* avail_gpu, const int64_t* sched_cpu_milli, const int64_t* sched_mem_bytes,
                    const int64_t* sched_gpu) {
    GF_EACH(ctx, gf_snapshot_set(ctx, n_nodes, avail_cpu_milli, avail_mem_bytes, avail_gpu, sched_cpu_milli, sched_mem_bytes, sched_gpu));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    InstallGuard install_guard(ctx);
    if (n_nodes > 0 && (!avail_cpu_milli || !avail_mem_bytes || !avail_gpu))
        return fail(ctx, GF_ERR_INVALID, "available arrays must not be NULL");
    if (n_nodes >= GF_NO_NODE) return fail(ctx, GF_ERR_INVALID, "too many nodes");
    const int64_t* av[3] = {avail_cpu_milli, avail_mem_bytes, avail_gpu};
    const int64_t* sc[3] = {sched_cpu_milli, sched_mem_bytes, sched_gpu};
    for (int j = 0; j < 3; ++j)
        for (uint32_t n = 0; n < n_nodes; ++n)
            if (av[j][n] >= GF_MAX_ABS_QUANTITY || av[j][n] <= -GF_MAX_ABS_QUANTITY)
                return fail(ctx, GF_ERR_INVALID, "available[%d][%u] outside (-2^62, 2^62)", j, n);
    ctx->have_sched = sc[0] && sc[1] && sc[2];
    if (ctx->have_sched)
        for (int j = 0; j < 3; ++j)
            for (uint32_t n = 0; n < n_nodes; ++n)
                if (sc[j][n] < 0 || sc[j][n] >= GF_MAX_ABS_QUANTITY)
                    return fail(ctx, GF_ERR_INVALID, "schedulable[%d][%u] outside [0, 2^62)", j, n);
    ctx->zone.clear();
    ctx->host_stale = false;
    ctx->eff_nonneg = ctx->have_sched;  // (fit_zoned_fused_kernel's feasibility instantiation: when no efficiency can be negative)
    for (int j = 0; j < 3 && ctx->eff_nonneg; ++j)
        for (uint32_t n = 0; n < n_nodes; ++n)
            if (av[j][n] > sc[j][n]) {
                ctx->eff_nonneg = false;
                break;
            }
    for (int j = 0; j < 3; ++j) {
        ctx->avail[j].assign(av[j], av[j] + n_nodes);
        if (ctx->have_sched)
            ctx->sched[j].assign(sc[j], sc[j] + n_nodes);
        else
            ctx->sched[j].clear();
    }
    ctx->n_nodes = n_nodes;
    ctx->have_snapshot = true;
    ctx->have_orders = false;
    ctx->work_valid = false;
    ++ctx->snap_epoch;  // drops the chain cache
    // node-indexed copy for the per-node efficiency map (gf_packing_efficiencies)
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, gf_wait_stream(ctx->stream));
    GF_HIP(ctx, ctx->d_node_tab.reserve(6 * (size_t)n_nodes + 1));
    for (int j = 0; j < 3 && n_nodes; ++j) {
        GF_HIP(ctx, hipMemcpy(ctx->d_node_tab.ptr + (size_t)j * n_nodes, av[j], (size_t)n_nodes * sizeof(int64_t),
                              hipMemcpyHostToDevice));
        if (ctx->have_sched)
            GF_HIP(ctx, hipMemcpy(ctx->d_node_tab.ptr + (size_t)(3 + j) * n_nodes, sc[j],
                                  (size_t)n_nodes * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    return GF_OK;
}

int gf_zones_set(gf_ctx* ctx, const uint32_t* zone_of_node) {
    GF_EACH(ctx, gf_zones_set(ctx, zone_of_node));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    InstallGuard install_guard(ctx);
    if (!ctx->have_snapshot) return fail(ctx, GF_ERR_STATE, "gf_snapshot_set must precede gf_zones_set");
    if (ctx->n_nodes > 0 && !zone_of_node) return fail(ctx, GF_ERR_INVALID, "zone array must not be NULL");
    ctx->zone.assign(zone_of_node, zone_of_node + ctx->n_nodes);
    ctx->have_orders = false;  // the zone views are built by gf_orders_set
    ++ctx->snap_epoch;
    return GF_OK;
}

int gf_orders_set(gf_ctx* ctx, const uint32_t* driver_order, uint32_t n_d, const uint32_t* exec_order, uint32_t n_x) {
    GF_EACH(ctx, gf_orders_set(ctx, driver_order, n_d, exec_order, n_x));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    InstallGuard install_guard(ctx);
    if (!ctx->have_snapshot) return fail(ctx, GF_ERR_STATE, "gf_snapshot_set must precede gf_orders_set");
    if (int mrc = materialize_host(ctx); mrc != GF_OK) return mrc;
    if ((n_d > 0 && !driver_order) || (n_x > 0 && !exec_order))
        return fail(ctx, GF_ERR_INVALID, "order arrays must not be NULL");
    GF_HIP(ctx, hipSetDevice(ctx->device));
    // ---- plan: nothing of the context changes before the layout has been accepted
    LayoutInput in;
    in.n_nodes = ctx->n_nodes;
    for (int j = 0; j < 3; ++j) {
        in.avail[j] = ctx->avail[j].data();
        in.sched[j] = ctx->have_sched ? ctx->sched[j].data() : nullptr;
    }
    in.zone = ctx->zone.empty() ? nullptr : ctx->zone.data();
    in.driver_order = driver_order;
    in.n_d = n_d;
    in.exec_order = exec_order;
    in.n_x = n_x;
    in.force_general_layout = ctx->force_general_layout;
    in.sparse_gpu = ctx->sparse_gpu;
    LayoutPlan plan = plan_layout(in);
    if (plan.code != GF_OK) return fail(ctx, plan.code, "%s", plan.error.c_str());
    const LayoutSizes& z = plan.sizes;
    LayoutFacts& f = plan.facts;
    // ---- reserve the pinned staging, fill it
    GF_HIP(ctx, ctx->h_table.reserve(z.table + z.sched));
    GF_HIP(ctx, ctx->h_index.reserve(z.index + z.zspan + 1));
    GF_HIP(ctx, ctx->h_masks.reserve(z.masks));
    GF_HIP(ctx, ctx->h_cmax.reserve(z.cmax));
    GF_HIP(ctx, ctx->h_ntable.reserve(z.ntable + z.nquad));
    GF_HIP(ctx, ctx->h_gtab.reserve(z.gtab));
    GF_HIP(ctx, ctx->h_gidx.reserve(z.gidx));
    GF_HIP(ctx, ctx->h_zmasks.reserve(z.zmasks + z.gmask + 1));
    LayoutTables t;
    t.table = ctx->h_table.ptr;
    t.sched = t.table + z.table;
    t.index = ctx->h_index.ptr;
    t.zspan = t.index + z.index;
    t.masks = ctx->h_masks.ptr;
    t.cmax = ctx->h_cmax.ptr;
    t.ntable = ctx->h_ntable.ptr;
    t.nquad = t.ntable + z.ntable;
    t.gtab = ctx->h_gtab.ptr;
    t.gidx = ctx->h_gidx.ptr;
    t.zmasks = ctx->h_zmasks.ptr;
    t.gmask = t.zmasks + z.zmasks;
    fill_layout(in, plan, t);
    // ---- upload
    hipStream_t st = ctx->stream;
    const size_t S = f.n_slots, C = f.n_chunks, G = f.n_gpad;
    GF_HIP(ctx, gf_wait_stream(st));  // nothing in flight may still read the old tables
    if (f.narrow_ok) {
        GF_HIP(ctx, upload(ctx->d_nsnap, t.ntable, 3 * S, st));
        GF_HIP(ctx, ctx->d_nwork.reserve(3 * S));
        GF_HIP(ctx, upload(ctx->d_ncmax, t.ntable + 3 * S, 3 * C, st));
        GF_HIP(ctx, upload(ctx->d_nquad, t.nquad, 4 * S, st));
    }
    GF_HIP(ctx, upload(ctx->d_cmax, t.cmax, 3 * C, st));
    GF_HIP(ctx, upload(ctx->d_masks, t.masks, 2 * C, st));
    GF_HIP(ctx, upload(ctx->d_snap, t.table, 3 * S, st));
    GF_HIP(ctx, ctx->d_work.reserve(3 * S));
    GF_HIP(ctx, upload(ctx->d_slot_node, t.index, S, st));
    GF_HIP(ctx, upload(ctx->d_dslot, t.index + S, f.n_d, st));
    GF_HIP(ctx, upload(ctx->d_node_slot, t.index + S + f.n_d, in.n_nodes, st));
    if (f.n_g != 0) {
        GF_HIP(ctx, upload(ctx->d_gtab, t.gtab, 3 * G, st));
        GF_HIP(ctx, upload(ctx->d_gcmax, t.gtab + 3 * G, 3 * (G / 64), st));
        GF_HIP(ctx, upload(ctx->d_gidx, t.gidx, z.gidx, st));
        GF_HIP(ctx, upload(ctx->d_gmask, t.gmask, z.gmask, st));
    }
    GF_HIP(ctx, ctx->d_sched.reserve(3 * S));
    if (z.sched != 0)
        GF_HIP(ctx, upload(ctx->d_sched, t.sched, z.sched, st));
    else
        GF_HIP(ctx, hipMemsetAsync(ctx->d_sched.ptr, 0, 3 * S * sizeof(int64_t), st));
    GF_HIP(ctx, upload(ctx->d_zmasks, t.zmasks, z.zmasks, st));
    GF_HIP(ctx, upload(ctx->d_zspan, t.zspan, z.zspan, st));
    GF_HIP(ctx, gf_wait_stream(st));  // the caller's arrays and the staging are free again
    install_layout(ctx, std::move(f));
    return GF_OK;
}

int gf_cluster_set(gf_ctx* ctx, uint32_t n_nodes, const int64_t* alloc_cpu_milli, const int64_t* alloc_mem_bytes,
                   const int64_t* alloc_gpu, const int64_t* over_cpu_milli, const int64_t* over_mem_bytes,
                   const int64_t* over_gpu, const uint32_t* node_flags, const uint32_t* zone_of_node, uint32_t n_zones,
                   const uint32_t* name_rank) {
    GF_EACH(ctx, gf_cluster_set(ctx, n_nodes, alloc_cpu_milli, alloc_mem_bytes, alloc_gpu, over_cpu_milli, over_mem_bytes,
                                over_gpu, node_flags, zone_of_node, n_zones, name_rank));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    ctx->have_cluster = false;
    const uint32_t n = n_nodes;
    if (n >= GF_NO_NODE) return fail(ctx, GF_ERR_INVALID, "too many nodes");
    if (n > 0 && (!alloc_cpu_milli || !alloc_mem_bytes || !alloc_gpu || !node_flags || !name_rank))
        return fail(ctx, GF_ERR_INVALID, "allocatable / node_flags / name_rank must not be NULL");
    const bool with_over = over_cpu_milli || over_mem_bytes || over_gpu;
    if (with_over && !(over_cpu_milli && over_mem_bytes && over_gpu))
        return fail(ctx, GF_ERR_INVALID, "overhead columns must be all NULL or all set");
    if (zone_of_node == nullptr) n_zones = 1;
    if (n_zones == 0 || n_zones > 4096) return fail(ctx, GF_ERR_INVALID, "n_zones = %u outside [1, 4096]", n_zones);
    {  // name_rank must be a permutation: it seeds the stable sort with the name order (nodesorting.go:92)
        std::vector<uint8_t> seen(n, 0);
        for (uint32_t i = 0; i < n; ++i) {
            if (name_rank[i] >= n || seen[name_rank[i]]) return fail(ctx, GF_ERR_INVALID, "name_rank is not a permutation");
            seen[name_rank[i]] = 1;
        }
        if (zone_of_node)
            for (uint32_t i = 0; i < n; ++i)
                if (zone_of_node[i] >= n_zones) return fail(ctx, GF_ERR_INVALID, "zone_of_node[%u] >= n_zones", i);
    }
    const int64_t* cols[3] = {alloc_cpu_milli, alloc_mem_bytes, alloc_gpu};
    const int64_t* ocols[3] = {over_cpu_milli, over_mem_bytes, over_gpu};
    const int64_t lim = GF_MAX_ABS_QUANTITY >> 1;
    for (int j = 0; j < 3; ++j) {
        ctx->cl_max_over[j] = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (cols[j][i] < 0 || cols[j][i] >= GF_MAX_ABS_QUANTITY || (with_over && (ocols[j][i] < 0 || ocols[j][i] >= lim)))
                return fail(ctx, GF_ERR_INVALID, "allocatable / overhead value out of range at node %u", i);
            if (with_over && ocols[j][i] > ctx->cl_max_over[j]) ctx->cl_max_over[j] = ocols[j][i];
        }
    }
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t N = n;
    GF_HIP(ctx, gf_wait_stream(st));  // nothing in flight may still read the columns that are about to be replaced
    GF_HIP(ctx, ctx->d_cl_i64.reserve(6 * N + 1));
    GF_HIP(ctx, ctx->d_cl_u32.reserve(3 * N + 1));
    for (int j = 0; j < 3 && N; ++j) {
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_cl_i64.ptr + j * N, cols[j], N * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (with_over)
            GF_HIP(ctx, hipMemcpyAsync(ctx->d_cl_i64.ptr + (3 + j) * N, ocols[j], N * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    if (N) {
        if (zone_of_node)
            GF_HIP(ctx, hipMemcpyAsync(ctx->d_cl_u32.ptr, zone_of_node, N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        else
            GF_HIP(ctx, hipMemsetAsync(ctx->d_cl_u32.ptr, 0, N * sizeof(uint32_t), st));
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_cl_u32.ptr + N, name_rank, N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_cl_u32.ptr + 2 * N, node_flags, N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    GF_HIP(ctx, ctx->d_cl_usage.reserve(3 * N + 1));
    GF_HIP(ctx, hipMemsetAsync(ctx->d_cl_usage.ptr, 0, (3 * N + 1) * sizeof(int64_t), st));  // a new node set: no usage yet
    GF_HIP(ctx, ctx->d_cl_x32.reserve(2 * N + 1));
    if (N) GF_HIP(ctx, hipMemsetAsync(ctx->d_cl_x32.ptr, 0, N * sizeof(uint32_t), st));  // ... and no reservation entry
    if (N) GF_HIP(ctx, hipMemcpyAsync(ctx->d_cl_x32.ptr + N, node_flags, N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    for (int j = 0; j < 3; ++j) ctx->usage_total[j] = 0;
    GF_HIP(ctx, gf_wait_stream(st));  // the caller's arrays are free again
    ctx->cl_alloc.resize(3 * N);
    for (int j = 0; j < 3 && N; ++j) std::copy(cols[j], cols[j] + N, ctx->cl_alloc.begin() + (size_t)j * N);
    ctx->cl_flags.assign(node_flags, node_flags + n);
    ctx->cl_default_flags = ctx->cl_flags;
    ctx->d_flags_default = true;
    ctx->usage_ok = true;
    ctx->cl_over_ok = true;
    ++ctx->cluster_gen;
    ++ctx->usage_gen;
    if (zone_of_node)
        ctx->cl_zone.assign(zone_of_node, zone_of_node + n);
    else
        ctx->cl_zone.clear();
    ctx->cl_n = n;
    ctx->cl_zones = n_zones;
    ctx->cl_over = with_over;
    ctx->have_cluster = true;
    return GF_OK;
}

int gf_snapshot_build(gf_ctx* ctx, uint32_t n_nodes, const int64_t* alloc_cpu_milli, const int64_t* alloc_mem_bytes,
                      const int64_t* alloc_gpu, const int64_t* over_cpu_milli, const int64_t* over_mem_bytes,
                      const int64_t* over_gpu, uint32_t n_res, const uint32_t* res_node, const int64_t* res_cpu_milli,
                      const int64_t* res_mem_bytes, const int64_t* res_gpu, const uint32_t* node_flags,
                      const uint32_t* zone_of_node, uint32_t n_zones, const uint32_t* name_rank,
                      const uint32_t* driver_label_rank, const uint32_t* exec_label_rank, uint32_t* driver_order_out,
                      uint32_t* n_d_out, uint32_t* exec_order_out, uint32_t* n_x_out) {
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);  // cluster + build are one sequence
    const int rc = gf_cluster_set(ctx, n_nodes, alloc_cpu_milli, alloc_mem_bytes, alloc_gpu, over_cpu_milli, over_mem_bytes,
                                  over_gpu, node_flags, zone_of_node, n_zones, name_rank);
    if (rc != GF_OK) return rc;
    return gf_snapshot_build_resident(ctx, n_res, res_node, res_cpu_milli, res_mem_bytes, res_gpu, nullptr, driver_label_rank,
                                      exec_label_rank, driver_order_out, n_d_out, exec_order_out, n_x_out);
}

int gf_usage_reset(gf_ctx* ctx) {
    GF_EACH(ctx, gf_usage_reset(ctx));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    if (!ctx->have_cluster) return fail(ctx, GF_ERR_STATE, "gf_cluster_set must precede gf_usage_reset");
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, hipMemsetAsync(ctx->d_cl_usage.ptr, 0, (3 * (size_t)ctx->cl_n + 1) * sizeof(int64_t), ctx->stream));
    if (ctx->cl_n) GF_HIP(ctx, hipMemsetAsync(ctx->d_cl_x32.ptr, 0, (size_t)ctx->cl_n * sizeof(uint32_t), ctx->stream));  // the entry counts
    for (int j = 0; j < 3; ++j) ctx->usage_total[j] = 0;
    ctx->usage_ok = true;
    ++ctx->usage_gen;
    return GF_OK;
}

int gf_usage_apply(gf_ctx* ctx, uint32_t n_entries, const uint32_t* res_node, const int64_t* res_cpu_milli,
                   const int64_t* res_mem_bytes, const int64_t* res_gpu, int sign) {
    // every device keeps the same sums; an update that reaches some devices and fails on another leaves them apart:
    // the resident usage is then unusable everywhere until gf_usage_reset
    if (ctx != nullptr && !ctx->group.empty())
        return each_device(ctx, &gf_ctx::usage_ok, [&](gf_ctx* sub, bool) {
            return gf_usage_apply(sub, n_entries, res_node, res_cpu_milli, res_mem_bytes, res_gpu, sign);
        });
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    if (!ctx->have_cluster) return fail(ctx, GF_ERR_STATE, "gf_cluster_set must precede gf_usage_apply");
    if (!ctx->usage_ok) return fail(ctx, GF_ERR_STATE, "an earlier update failed half way: gf_usage_reset must rebuild the resident usage");
    if (sign != 1 && sign != -1) return fail(ctx, GF_ERR_INVALID, "sign must be +1 or -1");
    if (n_entries == 0) return GF_OK;
    if (!res_node || !res_cpu_milli || !res_mem_bytes || !res_gpu) return fail(ctx, GF_ERR_INVALID, "entry columns must not be NULL");
    const int64_t* rcols[3] = {res_cpu_milli, res_mem_bytes, res_gpu};
    const int64_t lim = GF_MAX_ABS_QUANTITY >> 1;
    __int128 total[3];
    for (int j = 0; j < 3; ++j) {
        __int128 sum = 0;
        for (uint32_t i = 0; i < n_entries; ++i) {
            if (rcols[j][i] < 0 || rcols[j][i] >= lim) return fail(ctx, GF_ERR_INVALID, "entry %u out of range", i);
            if (res_node[i] < ctx->cl_n) sum += rcols[j][i];
        }
        total[j] = ctx->usage_total[j] + (sign > 0 ? sum : -sum);
        // every node's sum lies between 0 and the sum of everything applied: that (plus the overhead) must stay below 2^62
        if (total[j] < 0) return fail(ctx, GF_ERR_INVALID, "more usage removed than was ever added (dimension %d)", j);
        if (total[j] + (__int128)ctx->cl_max_over[j] >= (__int128)GF_MAX_ABS_QUANTITY)
            return fail(ctx, GF_ERR_INVALID, "the resident usage can sum past 2^62: not representable");
    }
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t R = n_entries;
    GF_HIP(ctx, gf_wait_stream(st));  // an earlier update may still read the staging buffers that are about to grow
    GF_HIP(ctx, ctx->d_delta_i64.reserve(3 * R));
    GF_HIP(ctx, ctx->d_delta_u32.reserve(R));
    for (int j = 0; j < 3; ++j)
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_delta_i64.ptr + j * R, rcols[j], R * sizeof(int64_t), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_delta_u32.ptr, res_node, R * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, ctx->d_flag32.reserve(1));
    if (sign < 0) GF_HIP(ctx, hipMemsetAsync(ctx->d_flag32.ptr, 0, sizeof(uint32_t), st));
    ++ctx->usage_gen;
    ctx->usage_ok = false;  // until the update is known to have been applied in full
    GF_HIP(ctx, gangfit::launch_usage_apply(n_entries, ctx->cl_n, ctx->d_delta_u32.ptr, ctx->d_delta_i64.ptr, sign,
                                            ctx->d_cl_usage.ptr, ctx->d_cl_x32.ptr, ctx->d_flag32.ptr, st));
    if (sign < 0)
        GF_HIP(ctx, hipMemcpyAsync(ctx->h_failed.ptr, ctx->d_flag32.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GF_HIP(ctx, gf_wait_stream(st));  // the caller's arrays are free again
    if (sign < 0 && ctx->h_failed.ptr[0] != 0) {
        // an entry was removed from a node that never carried it: the node's sum went negative (the snapshot would report
        // available > allocatable).  Put the update back and refuse it.
        GF_HIP(ctx, gangfit::launch_usage_apply(n_entries, ctx->cl_n, ctx->d_delta_u32.ptr, ctx->d_delta_i64.ptr, +1,
                                                ctx->d_cl_usage.ptr, ctx->d_cl_x32.ptr, nullptr, st));
        GF_HIP(ctx, gf_wait_stream(st));
        ctx->usage_ok = true;
        return fail(ctx, GF_ERR_INVALID, "an entry was removed from a node that never carried it (a node's usage went negative)");
    }
    ctx->usage_ok = true;
    for (int j = 0; j < 3; ++j) ctx->usage_total[j] = total[j];
    return GF_OK;
}

int gf_overhead_update(gf_ctx* ctx, uint32_t n_rows, const uint32_t* node, const int64_t* over_cpu_milli, const int64_t* over_mem_bytes,
                       const int64_t* over_gpu) {
    // every device keeps the same columns; an update that reaches some devices and fails on another leaves them apart:
    // the resident cluster is then unusable everywhere until gf_cluster_set
    if (ctx != nullptr && !ctx->group.empty())
        return each_device(ctx, &gf_ctx::cl_over_ok, [&](gf_ctx* sub, bool) {
            return gf_overhead_update(sub, n_rows, node, over_cpu_milli, over_mem_bytes, over_gpu);
        });
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    if (!ctx->have_cluster) return fail(ctx, GF_ERR_STATE, "gf_cluster_set must precede gf_overhead_update");
    if (!ctx->cl_over_ok)
        return fail(ctx, GF_ERR_STATE, "an earlier update failed half way: gf_cluster_set must replace the resident cluster");
    if (n_rows == 0) return GF_OK;
    if (!node || !over_cpu_milli || !over_mem_bytes || !over_gpu) return fail(ctx, GF_ERR_INVALID, "row columns must not be NULL");
    const int64_t* ocols[3] = {over_cpu_milli, over_mem_bytes, over_gpu};
    const int64_t lim = GF_MAX_ABS_QUANTITY >> 1;
    int64_t row_max[3] = {0, 0, 0};
    for (int j = 0; j < 3; ++j) {
        for (uint32_t i = 0; i < n_rows; ++i) {
            if (ocols[j][i] < 0 || ocols[j][i] >= lim) return fail(ctx, GF_ERR_INVALID, "row %u out of range", i);
            if (ocols[j][i] > row_max[j]) row_max[j] = ocols[j][i];
        }
        // what gf_usage_apply keeps true — (everything applied) + (the largest overhead) < 2^62 — must survive the new rows
        if (ctx->usage_total[j] + (__int128)row_max[j] >= (__int128)GF_MAX_ABS_QUANTITY)
            return fail(ctx, GF_ERR_INVALID, "the resident usage plus this overhead can sum past 2^62: not representable");
    }
    for (uint32_t i = 0; i < n_rows; ++i)
        if (node[i] >= ctx->cl_n) return fail(ctx, GF_ERR_INVALID, "row %u names node %u of %u", i, node[i], ctx->cl_n);
    if (ctx->cl_row_stamp.size() != ctx->cl_n || ctx->cl_row_call == UINT32_MAX) {
        ctx->cl_row_stamp.assign(ctx->cl_n, 0);
        ctx->cl_row_call = 0;
    }
    ++ctx->cl_row_call;
    for (uint32_t i = 0; i < n_rows; ++i) {
        if (ctx->cl_row_stamp[node[i]] == ctx->cl_row_call) return fail(ctx, GF_ERR_INVALID, "node %u is named twice in one update", node[i]);
        ctx->cl_row_stamp[node[i]] = ctx->cl_row_call;
    }
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t R = n_rows, N = ctx->cl_n;
    GF_HIP(ctx, gf_wait_stream(st));  // an earlier update may still read the staging buffers that are about to grow
    GF_HIP(ctx, ctx->d_delta_i64.reserve(3 * R));
    GF_HIP(ctx, ctx->d_delta_u32.reserve(R));
    // ---- from here on the device changes: a runtime failure leaves the columns unknown
    ctx->cl_over_ok = false;
    int64_t* d_over = ctx->d_cl_i64.ptr + 3 * N;
    if (!ctx->cl_over)  // installed without overhead columns: the build read none; now it must, and the other rows are zero
        GF_HIP(ctx, hipMemsetAsync(d_over, 0, 3 * N * sizeof(int64_t), st));
    for (int j = 0; j < 3; ++j)
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_delta_i64.ptr + j * R, ocols[j], R * sizeof(int64_t), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_delta_u32.ptr, node, R * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, gangfit::launch_overhead_update(n_rows, ctx->cl_n, ctx->d_delta_u32.ptr, ctx->d_delta_i64.ptr, d_over, st));
    GF_HIP(ctx, gf_wait_stream(st));  // the caller's arrays are free again
    ctx->cl_over = true;
    ctx->cl_over_ok = true;
    for (int j = 0; j < 3; ++j)
        if (row_max[j] > ctx->cl_max_over[j]) ctx->cl_max_over[j] = row_max[j];  // a bound: a replaced row never lowers it
    ++ctx->cluster_gen;
    return GF_OK;
}

int gf_cluster_update(gf_ctx* ctx, uint32_t n_rows, const uint32_t* node, const int64_t* alloc_cpu_milli, const int64_t* alloc_mem_bytes,
                      const int64_t* alloc_gpu, const uint32_t* node_flags, const uint32_t* zone_of_node, const uint32_t* name_rank) {
    // every device keeps the same columns; an update that reaches some devices and fails on another leaves them apart:
    // the resident cluster is then unusable everywhere until gf_cluster_set
    if (ctx != nullptr && !ctx->group.empty())
        return each_device(ctx, &gf_ctx::cl_over_ok, [&](gf_ctx* sub, bool) {
            return gf_cluster_update(sub, n_rows, node, alloc_cpu_milli, alloc_mem_bytes, alloc_gpu, node_flags, zone_of_node, name_rank);
        });
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    if (!ctx->have_cluster) return fail(ctx, GF_ERR_STATE, "gf_cluster_set must precede gf_cluster_update");
    if (!ctx->cl_over_ok)
        return fail(ctx, GF_ERR_STATE, "an earlier update failed half way: gf_cluster_set must replace the resident cluster");
    if (n_rows == 0 && name_rank == nullptr) return GF_OK;
    if (n_rows > 0 && (!node || !alloc_cpu_milli || !alloc_mem_bytes || !alloc_gpu || !node_flags))
        return fail(ctx, GF_ERR_INVALID, "row columns must not be NULL");
    const int64_t* cols[3] = {alloc_cpu_milli, alloc_mem_bytes, alloc_gpu};
    for (int j = 0; j < 3; ++j)
        for (uint32_t i = 0; i < n_rows; ++i)
            if (cols[j][i] < 0 || cols[j][i] >= GF_MAX_ABS_QUANTITY) return fail(ctx, GF_ERR_INVALID, "allocatable of row %u out of range", i);
    for (uint32_t i = 0; i < n_rows; ++i)
        if (node[i] >= ctx->cl_n) return fail(ctx, GF_ERR_INVALID, "row %u names node %u of %u", i, node[i], ctx->cl_n);
    if (n_rows > 0 && zone_of_node != nullptr) {
        bool any = false;
        for (uint32_t i = 0; i < n_rows; ++i) {
            if (zone_of_node[i] >= ctx->cl_zones) return fail(ctx, GF_ERR_INVALID, "zone_of_node[%u] >= n_zones = %u", i, ctx->cl_zones);
            any |= zone_of_node[i] != 0;
        }
        if (ctx->cl_zone.empty()) {  // installed without zones: every node is in zone 0, and zeros say nothing new
            if (any) return fail(ctx, GF_ERR_INVALID, "the cluster was installed without zones: a zone id needs gf_cluster_set");
            zone_of_node = nullptr;
        }
    }
    if (n_rows == 0) zone_of_node = nullptr;
    if (name_rank != nullptr) {  // a permutation, as in gf_cluster_set
        std::vector<uint8_t> seen(ctx->cl_n, 0);
        for (uint32_t i = 0; i < ctx->cl_n; ++i) {
            if (name_rank[i] >= ctx->cl_n || seen[name_rank[i]]) return fail(ctx, GF_ERR_INVALID, "name_rank is not a permutation");
            seen[name_rank[i]] = 1;
        }
    }
    if (n_rows > 0) {
        if (ctx->cl_row_stamp.size() != ctx->cl_n || ctx->cl_row_call == UINT32_MAX) {
            ctx->cl_row_stamp.assign(ctx->cl_n, 0);
            ctx->cl_row_call = 0;
        }
        ++ctx->cl_row_call;
        for (uint32_t i = 0; i < n_rows; ++i) {
            if (ctx->cl_row_stamp[node[i]] == ctx->cl_row_call) return fail(ctx, GF_ERR_INVALID, "node %u is named twice in one update", node[i]);
            ctx->cl_row_stamp[node[i]] = ctx->cl_row_call;
        }
    }
    const size_t R = n_rows, N = ctx->cl_n;
    if (N == 0) return GF_OK;  // (name_rank of no node: nothing to replace)
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    GF_HIP(ctx, gf_wait_stream(st));  // an earlier update may still read the staging buffers that are about to grow
    GF_HIP(ctx, ctx->d_delta_i64.reserve(3 * R));
    GF_HIP(ctx, ctx->d_delta_u32.reserve(3 * R));  // node | flags | zone
    // ---- from here on the device changes: a runtime failure leaves the columns unknown
    ctx->cl_over_ok = false;
    if (R) {
        uint32_t* const d_rows32 = ctx->d_delta_u32.ptr;
        for (int j = 0; j < 3; ++j)
            GF_HIP(ctx, hipMemcpyAsync(ctx->d_delta_i64.ptr + j * R, cols[j], R * sizeof(int64_t), hipMemcpyHostToDevice, st));
        GF_HIP(ctx, hipMemcpyAsync(d_rows32, node, R * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        GF_HIP(ctx, hipMemcpyAsync(d_rows32 + R, node_flags, R * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (zone_of_node) GF_HIP(ctx, hipMemcpyAsync(d_rows32 + 2 * R, zone_of_node, R * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        // (while the build's flag column holds a request's candidate flags, d_flags_default == false, the next build uploads the
        // whole default column from cl_default_flags below; the kernel's stores there are then overwritten)
        GF_HIP(ctx, gangfit::launch_cluster_update(n_rows, ctx->cl_n, d_rows32, ctx->d_delta_i64.ptr, d_rows32 + R,
                                                   zone_of_node ? d_rows32 + 2 * R : nullptr, ctx->d_cl_i64.ptr, ctx->d_cl_u32.ptr,
                                                   ctx->d_cl_u32.ptr + 2 * N, ctx->d_cl_x32.ptr + N, st));
    }
    if (name_rank) GF_HIP(ctx, hipMemcpyAsync(ctx->d_cl_u32.ptr + N, name_rank, N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, gf_wait_stream(st));  // the caller's arrays are free again
    for (uint32_t i = 0; i < n_rows; ++i) {  // the host copies follow the rows: the build's host route and the range checks read them
        const uint32_t n = node[i];
        for (int j = 0; j < 3; ++j) ctx->cl_alloc[(size_t)j * N + n] = cols[j][i];
        ctx->cl_default_flags[n] = node_flags[i];
        if (zone_of_node) ctx->cl_zone[n] = zone_of_node[i];
    }
    if (n_rows > 0) ctx->cl_flags = ctx->cl_default_flags;  // no request's candidate flags outlive the update
    ctx->cl_over_ok = true;
    ++ctx->cluster_gen;
    return GF_OK;
}

}  // extern "C"

namespace {

// Where gf_snapshot_build_resident hands back the two candidate lists; every pointer may be NULL.
struct OrderOuts {
    uint32_t* driver_order;
    uint32_t* n_d;
    uint32_t* exec_order;
    uint32_t* n_x;
    bool any() const { return driver_order || n_d || exec_order || n_x; }
    void counts(uint32_t nd, uint32_t nx) const {
        if (n_d) *n_d = nd;
        if (n_x) *n_x = nx;
    }
};

// The two candidate lists (nodesorting.go:47-63) from the sorted permutation and the node flags: written to the outputs that are
// not NULL; returns the two counts through nd / nx.
void candidate_lists(const uint32_t* perm, size_t n, const uint32_t* flags, uint32_t* drivers, uint32_t* execs, uint32_t* nd,
                     uint32_t* nx) {
    *nd = *nx = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t node = perm[i], fl = flags[node];
        if (fl & GF_NODE_DRIVER_CANDIDATE) {
            if (drivers) drivers[*nd] = node;
            ++*nd;
        }
        if (!(fl & GF_NODE_UNSCHEDULABLE) && (fl & GF_NODE_READY)) {
            if (execs) execs[*nx] = node;
            ++*nx;
        }
    }
}

// The reservation columns of one build: ranges, and the per-node sums (usage + overhead) must stay below 2^62 — the device
// accumulates in 64 bits and would wrap silently.  Coarse bound first (every entry on one node); only when that fails, the real
// per-node entry counts.
int check_reservations(gf_ctx* ctx, uint32_t n_res, const uint32_t* res_node, const int64_t* const rcols[3]) {
    const int64_t lim = GF_MAX_ABS_QUANTITY >> 1;
    int64_t max_res[3] = {0, 0, 0};
    for (int j = 0; j < 3; ++j)
        for (uint32_t i = 0; i < n_res; ++i) {
            if (rcols[j][i] < 0 || rcols[j][i] >= lim) return fail(ctx, GF_ERR_INVALID, "reservation %u out of range", i);
            if (rcols[j][i] > max_res[j]) max_res[j] = rcols[j][i];
        }
    if ((uint64_t)n_res >= (1ull << 32) - 1) return fail(ctx, GF_ERR_INVALID, "too many reservations");
    auto fits = [&](uint64_t count) {
        for (int j = 0; j < 3; ++j)
            if ((unsigned __int128)count * (uint64_t)max_res[j] + (uint64_t)ctx->cl_max_over[j] >= (unsigned __int128)GF_MAX_ABS_QUANTITY)
                return false;
        return true;
    };
    if (fits(n_res)) return GF_OK;
    std::vector<uint32_t> cnt(ctx->cl_n, 0);
    uint32_t most = 0;
    for (uint32_t i = 0; i < n_res; ++i)
        if (res_node[i] < ctx->cl_n && ++cnt[res_node[i]] > most) most = cnt[res_node[i]];
    if (fits(most)) return GF_OK;
    return fail(ctx, GF_ERR_INVALID, "the reservations of one node (%u entries) can sum past 2^62: not representable", most);
}

// The device memory of one build: the resident cluster columns and the two scratch buffers, carved.
struct BuildScratch {
    int64_t *alloc, *over;                                                         // d_cl_i64
    uint32_t *zone, *name_rank, *flags;                                            // d_cl_u32
    int64_t *usage, *avail, *sched, *keys_a, *keys_b, *keys_c, *res_req, *zone_sum;  // d_bi64 ...
    unsigned long long* gcd_part;  // gcd partials | magnitude partials
    long long* units;
    uint32_t *perm_a, *perm_b, *perm_c, *res_node, *zone_order, *zone_rank, *zfirst, *zhasx, *zeval, *scalars;  // d_bu32
    uint32_t *label_d, *label_x, *perm_p, *ppos;  // the request's label ranks | the priority order and its inverse (label group)
    unsigned long long* merge_summary;            // LabelMerge::d_summary
    uint32_t n;                                   // nodes the build runs over: the cluster's, or the members of a node set
    // a node-set build (gf_snapshot_build_resident_set; members == nullptr otherwise): alloc .. flags above are then the members'
    // compact columns, and what the finalize indexes by node is the members' until launch_snapshot_set_scatter has run
    const std::vector<uint32_t>* members;  // member -> cluster index, ascending
    uint64_t *set_words, *set_nbits;       // d_set64 ...
    int64_t *set_usage, *set_node_tab;
    uint32_t *set_prefix, *set_node, *set_node_slot;  // d_set32 ...
};

int carve_build_scratch(gf_ctx* ctx, uint32_t n, size_t R, BuildScratch* out) {
    const size_t N = n, Z = ctx->cl_zones;
    const size_t NCH = (N + 1 + 63) / 64;  // chunks of the slot space (nodes + sentinel)
    GF_HIP(ctx, ctx->d_bi64.reserve(9 * N + 3 * N + 3 * R + 3 * Z + 6 * NCH + 16 + 4 * (size_t)gangfit::kLabelMergeUnits));
    GF_HIP(ctx, ctx->d_bu32.reserve(3 * N + R + 5 * Z + 16 + 4 * N));
    BuildScratch& s = *out;
    s.n = n;
    s.members = nullptr;
    s.alloc = ctx->d_cl_i64.ptr;
    s.over = s.alloc + 3 * (size_t)ctx->cl_n;
    s.zone = ctx->d_cl_u32.ptr;
    s.name_rank = s.zone + ctx->cl_n;
    s.flags = s.name_rank + ctx->cl_n;
    s.usage = ctx->d_bi64.ptr;
    s.avail = s.usage + 3 * N;
    s.sched = s.avail + 3 * N;
    s.keys_a = s.sched + 3 * N;
    s.keys_b = s.keys_a + N;
    s.keys_c = s.keys_b + N;
    s.res_req = s.keys_c + N;
    s.zone_sum = s.res_req + 3 * R;
    s.gcd_part = reinterpret_cast<unsigned long long*>(s.zone_sum + 3 * Z);
    s.units = reinterpret_cast<long long*>(s.gcd_part + 6 * NCH);
    s.perm_a = ctx->d_bu32.ptr;
    s.perm_b = s.perm_a + N;
    s.perm_c = s.perm_b + N;
    s.res_node = s.perm_c + N;
    s.zone_order = s.res_node + R;
    s.zone_rank = s.zone_order + Z;
    s.zfirst = s.zone_rank + Z;
    s.zhasx = s.zfirst + Z;
    s.zeval = s.zhasx + Z;
    s.scalars = s.zeval + Z;  // 16 words
    s.label_d = s.scalars + 16;
    s.label_x = s.label_d + N;
    s.perm_p = s.label_x + N;
    s.ppos = s.perm_p + N;
    s.merge_summary = reinterpret_cast<unsigned long long*>(s.units + 8);  // (units: 6 words)
    return GF_OK;
}

// The scratch of a node-set build behind carve_build_scratch(m): the row, its name-order twin, the prefix counts, the usage sums of
// entries that travel (by cluster index) and the members' compact columns, which replace the resident ones in *out.
int carve_set_scratch(gf_ctx* ctx, const std::vector<uint32_t>& members, BuildScratch* out) {
    const size_t N = ctx->cl_n, W = (N + 63) / 64, M = members.size();
    GF_HIP(ctx, ctx->d_set64.reserve(2 * W + 3 * N + 9 * M + 6 * M + 1));
    GF_HIP(ctx, ctx->d_set32.reserve(2 * W + 5 * M + 2));
    BuildScratch& s = *out;
    s.members = &members;
    s.set_words = reinterpret_cast<uint64_t*>(ctx->d_set64.ptr);
    s.set_nbits = s.set_words + W;
    s.set_usage = ctx->d_set64.ptr + 2 * W;
    s.alloc = s.set_usage + 3 * N;
    s.over = s.alloc + 3 * M;
    s.usage = s.over + 3 * M;  // (the compact sums: the build reads them as resident ones)
    s.set_node_tab = s.usage + 3 * M;
    s.set_prefix = ctx->d_set32.ptr;
    s.zone = s.set_prefix + 2 * W;
    s.name_rank = s.zone + M;
    s.flags = s.name_rank + M;
    s.set_node = s.flags + M;
    s.set_node_slot = s.set_node + M;
    return GF_OK;
}

gangfit::SnapshotBuild build_args(gf_ctx* ctx, const BuildScratch& s, uint32_t n_res, bool usage_resident, const LabelPlan& lp) {
    gangfit::SnapshotBuild b{};
    b.n_nodes = s.n;
    b.n_res = n_res;
    b.n_zones = ctx->cl_zones;
    b.d_alloc = s.alloc;
    b.d_overhead = ctx->cl_over ? s.over : nullptr;
    b.d_res_node = s.res_node;
    b.d_res_req = s.res_req;
    b.d_zone = s.zone;
    b.d_name_rank = s.name_rank;
    if (s.members != nullptr) usage_resident = true;  // the members' sums were gathered: neither zeroed nor scattered into
    b.d_usage = (usage_resident && s.members == nullptr) ? ctx->d_cl_usage.ptr : s.usage;
    b.usage_resident = usage_resident;
    b.d_avail = s.avail;
    b.d_sched = s.sched;
    b.d_zone_sum = s.zone_sum;
    b.d_zone_order = s.zone_order;
    b.d_zone_rank = s.zone_rank;
    b.d_perm_a = s.perm_a;
    b.d_perm_b = s.perm_b;
    b.d_keys_a = s.keys_a;
    b.d_keys_b = s.keys_b;
    b.d_keys_c = s.keys_c;
    b.d_perm_c = s.perm_c;
    b.sort_fault = ctx->sort_fault;
    b.d_zfirst = s.zfirst;  // the finalize step's accumulators start clean with everything else (one clearing launch)
    b.d_zhasx = s.zhasx;
    b.zhasx_to_scalars_words = 2 * (size_t)ctx->cl_zones + 16;  // d_zhasx | d_zeval | d_scalars
    b.d_sort_work = ctx->d_sortwork.ptr;
    if (lp.device_route && lp.which != 0) {  // the label key group: d_perm_b receives C, d_perm_p keeps the priority order
        b.d_label = lp.which == 1 ? s.label_d : s.label_x;
        b.label_max = lp.max_rank;
        b.label_width = lp.width;
        b.d_perm_p = s.perm_p;
        b.d_ppos = s.ppos;
    }
    return b;
}

// What gf_snapshot_build_info reports; a build commits it when it has succeeded.
struct BuildInfo {
    uint32_t route = 0, label_group = 0, merge_failed = 0;
    uint64_t d2h_bytes = 0;
};

// The slot tables on the device too: nothing of size O(n_nodes) returns to the host unless the caller asks for the orders.
// Behind a label key group s.perm_b holds C, not the priority order: when the merge check has flagged it (the two lists are not
// both subsequences of C) nothing is installed, info->merge_failed is set and the caller takes the host route.
int finalize_on_device(gf_ctx* ctx, const BuildScratch& s, const OrderOuts& out, BuildInfo* info) {
    hipStream_t st = ctx->stream;
    const uint32_t n = s.n, n_slots = n + 1, n_chunks = (n_slots + 63) / 64;
    const bool set = s.members != nullptr;  // n members: their slots and the sentinel, node-indexed tables at the cluster's size
    const size_t N = ctx->cl_n, S = n_slots, C = n_chunks, Z = ctx->cl_zones;
    GF_HIP(ctx, ctx->d_snap.reserve(3 * S));
    GF_HIP(ctx, ctx->d_work.reserve(3 * S));
    GF_HIP(ctx, ctx->d_sched.reserve(3 * S));
    GF_HIP(ctx, ctx->d_slot_node.reserve(S));
    GF_HIP(ctx, ctx->d_dslot.reserve(S + 1));
    GF_HIP(ctx, ctx->d_node_slot.reserve(N + 1));
    GF_HIP(ctx, ctx->d_cmax.reserve(3 * C));
    GF_HIP(ctx, ctx->d_masks.reserve(2 * C));
    GF_HIP(ctx, ctx->d_node_tab.reserve(6 * N + 1));
    GF_HIP(ctx, ctx->d_zmasks.reserve(2 * Z * C + 1));
    GF_HIP(ctx, ctx->d_nsnap.reserve(3 * S));
    GF_HIP(ctx, ctx->d_nwork.reserve(3 * S));
    GF_HIP(ctx, ctx->d_ncmax.reserve(3 * C));
    GF_HIP(ctx, ctx->d_nquad.reserve(4 * S));
    gangfit::SnapshotFinalize f{};
    f.n_nodes = n;
    f.n_slots = n_slots;
    f.n_chunks = n_chunks;
    f.n_zones = ctx->cl_zones;
    f.d_avail = s.avail;
    f.d_sched = s.sched;
    f.d_perm = s.perm_b;
    f.d_zone = s.zone;
    f.d_flags = s.flags;
    f.d_snap = ctx->d_snap.ptr;
    f.d_sched_slot = ctx->d_sched.ptr;
    f.d_slot_node = ctx->d_slot_node.ptr;
    f.d_node_slot = set ? s.set_node_slot : ctx->d_node_slot.ptr;
    f.d_dslot = ctx->d_dslot.ptr;
    f.d_masks = ctx->d_masks.ptr;
    f.d_cmax = ctx->d_cmax.ptr;
    f.d_node_tab = set ? s.set_node_tab : ctx->d_node_tab.ptr;
    f.d_gcd_part = s.gcd_part;
    f.d_units = s.units;
    f.d_zfirst = s.zfirst;
    f.d_zhasx = s.zhasx;
    f.d_zeval = s.zeval;
    f.d_scalars = s.scalars;
    f.d_zmasks = ctx->d_zmasks.ptr;
    f.d_nsnap = ctx->d_nsnap.ptr;
    f.d_ncmax = ctx->d_ncmax.ptr;
    f.d_nquad = reinterpret_cast<int4*>(ctx->d_nquad.ptr);
    GF_HIP(ctx, ctx->h_bcols.reserve(6 * N + 8));
    GF_HIP(ctx, ctx->h_border.reserve(N + 16));
    // everything the host needs back is one range of sixteen words (SnapshotFinalize::d_scalars): the kernels write it into
    // pinned memory as they produce it (no copy on the stream), or ONE copy where that memory is not mapped to the device
    uint32_t* h_scalars = ctx->h_border.ptr;
    if (ctx->h_border.dev != nullptr) {
        std::memset(h_scalars, 0, 16 * sizeof(uint32_t));
        f.h_out = ctx->h_border.dev;
    }
    GF_HIP(ctx, gangfit::launch_snapshot_finalize(f, ctx->d_sortwork.ptr + gangfit::snapshot_sort_error_word(), st));
    if (set) {
        gangfit::SnapshotSetScatter sc{};
        sc.n_nodes = ctx->cl_n;
        sc.n_members = n;
        sc.d_words = s.set_words;
        sc.d_prefix = s.set_prefix;
        sc.c_node = s.set_node;
        sc.c_node_slot = s.set_node_slot;
        sc.c_node_tab = s.set_node_tab;
        sc.d_node_slot = ctx->d_node_slot.ptr;
        sc.d_node_tab = ctx->d_node_tab.ptr;
        sc.d_status = s.scalars + 3;  // (finalize_reduce_kernel has written it)
        sc.d_slot_node = ctx->d_slot_node.ptr;
        sc.d_nquad = reinterpret_cast<int4*>(ctx->d_nquad.ptr);
        GF_HIP(ctx, gangfit::launch_snapshot_set_scatter(sc, st));
    }
    if (f.h_out == nullptr) GF_HIP(ctx, hipMemcpyAsync(h_scalars, s.scalars, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GF_HIP(ctx, gf_wait_stream(st));
    info->d2h_bytes += 16 * sizeof(uint32_t);
    if (h_scalars[3] & 1u) return fail(ctx, GF_ERR_HIP, "the priority sort's grid barrier gave up (device oversubscribed?)");
    if (h_scalars[3] & 2u) {
        info->merge_failed = 1;
        return GF_OK;
    }
    // ---- the snapshot itself (what gf_snapshot_set + gf_zones_set record on the host path) ...
    ctx->have_sched = h_scalars[2] == 0;  // a negative schedulable value (overhead above allocatable) disables the efficiencies
    ctx->n_nodes = ctx->cl_n;
    ctx->have_snapshot = true;
    ctx->zone = ctx->cl_zone;
    ctx->eff_nonneg = false;  // nothing compared available with schedulable
    // ---- ... and its layout: every node has a slot, in the sorted order, and one sentinel
    LayoutFacts lf;
    lf.n_slots = n_slots;
    lf.n_x = lf.n_d = n;
    lf.n_chunks = n_chunks;
    lf.merged = lf.identity = true;
    lf.narrow_ok = h_scalars[1] == 0;
    for (int j = 0; j < 3; ++j) {  // 3 units, then the 3 largest scaled magnitudes, as pairs of words
        lf.unit[j] = (int64_t)((uint64_t)h_scalars[4 + 2 * j] | ((uint64_t)h_scalars[5 + 2 * j] << 32));
        lf.nmax[j] = (int64_t)((uint64_t)h_scalars[10 + 2 * j] | ((uint64_t)h_scalars[11 + 2 * j] << 32));
    }
    // n_g = 0: the sparse gpu view is built by gf_orders_set only; the full order serves here
    lf.n_zones = h_scalars[0];
    lf.zstride = n_chunks;
    lf.zd_row0 = ctx->cl_zones;  // the device lays the driver rows behind one row per zone of the cluster
    lf.zspan_ok = false;         // the zone masks were built on the device: the shards scan every zone over their whole range
    lf.host_stale = true;
    install_layout(ctx, std::move(lf));
    if (out.any()) {  // the two lists, for callers that want them (a set's order in cluster indices: its slots' nodes)
        GF_HIP(ctx, hipMemcpyAsync(ctx->h_border.ptr, set ? ctx->d_slot_node.ptr : s.perm_b, (size_t)n * sizeof(uint32_t),
                                   hipMemcpyDeviceToHost, st));
        GF_HIP(ctx, gf_wait_stream(st));
        uint32_t nd, nx;
        candidate_lists(ctx->h_border.ptr, n, ctx->cl_flags.data(), out.driver_order, out.exec_order, &nd, &nx);
        out.counts(nd, nx);
    }
    return GF_OK;
}

// The sorted snapshot returns to the host and is installed through the public setters: the optional stable label re-sorts
// (nodesorting.go:161-199) can break the merged layout, which only gf_orders_set handles.  Taken when the label merge check has
// failed (the re-sorted lists are not both subsequences of the sort's one order), with option "snapshot_finalize_host" = 1, and
// never otherwise: label ranks whose lists still merge are finalized on the device (gangfit_label_plan.h).
// d_order: the priority order on the device (s.perm_b, or s.perm_p behind a label key group).
int finalize_on_host(gf_ctx* ctx, const BuildScratch& s, const uint32_t* d_order, const uint32_t* driver_label_rank,
                     const uint32_t* exec_label_rank, const OrderOuts& out, BuildInfo* info) {
    hipStream_t st = ctx->stream;
    const uint32_t n = s.n;
    const size_t N = n;
    GF_HIP(ctx, ctx->h_bcols.reserve(6 * N));
    GF_HIP(ctx, ctx->h_border.reserve(N + 8));
    GF_HIP(ctx, hipMemcpyAsync(ctx->h_bcols.ptr, s.avail, 6 * N * sizeof(int64_t), hipMemcpyDeviceToHost, st));  // avail | sched
    GF_HIP(ctx, hipMemcpyAsync(ctx->h_border.ptr, d_order, N * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    info->d2h_bytes += 6 * N * sizeof(int64_t) + N * sizeof(uint32_t) + sizeof(uint32_t);
    GF_HIP(ctx, hipMemcpyAsync(ctx->h_failed.ptr, ctx->d_sortwork.ptr + gangfit::snapshot_sort_error_word(), sizeof(uint32_t),
                               hipMemcpyDeviceToHost, st));
    GF_HIP(ctx, gf_wait_stream(st));
    if (ctx->h_failed.ptr[0] != 0) return fail(ctx, GF_ERR_HIP, "the priority sort's grid barrier gave up (device oversubscribed?)");
    const int64_t* h_avail = ctx->h_bcols.ptr;
    const int64_t* h_sched = ctx->h_bcols.ptr + 3 * N;
    bool sched_ok = true;
    for (size_t i = 0; i < 3 * N && sched_ok; ++i) sched_ok = h_sched[i] >= 0;  // (a node set: over its members only)
    // a node set: rows and order in cluster indices — the members' rows, zeros for every other node
    const uint32_t n_inst = ctx->cl_n;
    std::vector<int64_t> wide;
    if (s.members != nullptr) {
        const std::vector<uint32_t>& mem = *s.members;
        const size_t CN = n_inst;
        wide.assign(6 * CN, 0);
        for (size_t c = 0; c < N; ++c) {
            for (int j = 0; j < 6; ++j) wide[(size_t)j * CN + mem[c]] = ctx->h_bcols.ptr[(size_t)j * N + c];
            ctx->h_border.ptr[c] = mem[ctx->h_border.ptr[c]];
        }
        h_avail = wide.data();
        h_sched = wide.data() + 3 * CN;
    }
    const size_t NI = n_inst;
    std::vector<uint32_t> D(N), X(N);
    uint32_t nd, nx;
    candidate_lists(ctx->h_border.ptr, N, ctx->cl_flags.data(), D.data(), X.data(), &nd, &nx);
    D.resize(nd);
    X.resize(nx);
    auto by_rank = [](std::vector<uint32_t>& v, const uint32_t* rank) {
        std::stable_sort(v.begin(), v.end(), [rank](uint32_t a, uint32_t b) { return rank[a] < rank[b]; });
    };
    if (driver_label_rank) by_rank(D, driver_label_rank);
    if (exec_label_rank) by_rank(X, exec_label_rank);
    int rc = gf_snapshot_set(ctx, n_inst, h_avail, h_avail + NI, h_avail + 2 * NI, sched_ok ? h_sched : nullptr,
                             sched_ok ? h_sched + NI : nullptr, sched_ok ? h_sched + 2 * NI : nullptr);
    if (rc != GF_OK) return rc;
    if (!ctx->cl_zone.empty() && (rc = gf_zones_set(ctx, ctx->cl_zone.data())) != GF_OK) return rc;
    if ((rc = gf_orders_set(ctx, D.data(), nd, X.data(), nx)) != GF_OK) return rc;
    out.counts(nd, nx);
    if (out.driver_order) std::memcpy(out.driver_order, D.data(), D.size() * sizeof(uint32_t));
    if (out.exec_order) std::memcpy(out.exec_order, X.data(), X.size() * sizeof(uint32_t));
    return GF_OK;
}

}  // namespace

namespace {

// gf_snapshot_build_resident (member_words == nullptr: every node of the resident cluster) and gf_snapshot_build_resident_set (the
// members of the row) on one device.
int build_resident(gf_ctx* ctx, const uint64_t* member_words, uint32_t n_res, const uint32_t* res_node, const int64_t* res_cpu_milli,
                   const int64_t* res_mem_bytes, const int64_t* res_gpu, const uint32_t* node_flags, const uint32_t* driver_label_rank,
                   const uint32_t* exec_label_rank, const OrderOuts& out) {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    InstallGuard install_guard(ctx);
    if (!ctx->have_cluster)
        return fail(ctx, GF_ERR_STATE, "gf_cluster_set must precede gf_snapshot_build_resident%s", member_words ? "_set" : "");
    const uint32_t n = ctx->cl_n;
    const bool set = member_words != nullptr;
    std::vector<uint32_t> members;  // member -> cluster index, ascending
    if (set) {
        const uint32_t W = (n + 63u) / 64u;
        if ((n & 63u) != 0 && (member_words[W - 1] >> (n & 63u)) != 0)
            return fail(ctx, GF_ERR_INVALID, "the member row has a bit at or beyond n_nodes = %u", n);
        for (uint32_t w = 0; w < W; ++w)
            for (uint64_t bits = member_words[w]; bits != 0; bits &= bits - 1) members.push_back(w * 64u + (uint32_t)__builtin_ctzll(bits));
    }
    const uint32_t m = set ? (uint32_t)members.size() : n;  // nodes the build runs over
    const bool usage_resident = n_res == GF_RESIDENT_USAGE;  // the sums gf_usage_apply maintains: no entry travels
    if (usage_resident) n_res = 0;
    if (n_res > 0 && (!res_node || !res_cpu_milli || !res_mem_bytes || !res_gpu))
        return fail(ctx, GF_ERR_INVALID, "reservation columns must not be NULL");
    if (usage_resident && !ctx->usage_ok)
        return fail(ctx, GF_ERR_STATE, "the resident usage is unknown (a failed update): gf_usage_reset must rebuild it");
    if (!ctx->cl_over_ok)
        return fail(ctx, GF_ERR_STATE, "the resident overhead is unknown (a failed gf_overhead_update): gf_cluster_set must replace it");
    // this request's candidate flags; NULL = the flags of gf_cluster_set (not those of the previous request)
    if (node_flags)
        ctx->cl_flags.assign(node_flags, node_flags + n);
    else
        ctx->cl_flags = ctx->cl_default_flags;
    const uint32_t* const flags_upload = node_flags ? node_flags : (ctx->d_flags_default ? nullptr : ctx->cl_default_flags.data());
    const int64_t* const rcols[3] = {res_cpu_milli, res_mem_bytes, res_gpu};
    if (int rc = check_reservations(ctx, n_res, res_node, rcols); rc != GF_OK) return rc;
    BuildInfo info;
    auto done = [&](int rc, uint32_t route) {  // what gf_snapshot_build_info reports: the last build that succeeded
        if (rc != GF_OK) return rc;
        ctx->build_info[0] = route;
        ctx->build_info[1] = info.label_group;
        ctx->build_info[2] = info.merge_failed;
        ctx->build_info[3] = info.d2h_bytes > UINT32_MAX ? UINT32_MAX : (uint32_t)info.d2h_bytes;
        if (set) {  // (every install behind this point moves snap_epoch on: the layout is a set's while the two are equal)
            ctx->set_epoch = ctx->snap_epoch;
            ctx->set_members = m;
        }
        return rc;
    };
    if (m == 0) {  // no node (or no member): an empty layout; a set keeps the node-indexed rows of the cluster, all zero
        const std::vector<int64_t> zeros(n, 0);
        const int64_t* const z = zeros.data();
        int rc = n == 0 ? gf_snapshot_set(ctx, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) : gf_snapshot_set(ctx, n, z, z, z, z, z, z);
        if (rc != GF_OK) return rc;
        if (n != 0 && !ctx->cl_zone.empty() && (rc = gf_zones_set(ctx, ctx->cl_zone.data())) != GF_OK) return rc;
        out.counts(0, 0);
        return done(gf_orders_set(ctx, nullptr, 0, nullptr, 0), 2);
    }
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t N = n, M = m, R = n_res;
    GF_HIP(ctx, gf_wait_stream(st));  // nothing in flight may still read buffers that are about to grow
    // a set's label ranks travel as its members' rows: the plan, the key width and the route are those of the members alone.
    // (Staged in the context's pinned memory, which outlives an early return with the copy still on the stream.)
    const uint32_t* label_in[2] = {driver_label_rank, exec_label_rank};
    if (set && (label_in[0] != nullptr || label_in[1] != nullptr)) {
        GF_HIP(ctx, ctx->h_set_labels.reserve(2 * M));
        for (int r = 0; r < 2; ++r)
            if (label_in[r] != nullptr) {
                uint32_t* const row = ctx->h_set_labels.ptr + (size_t)r * M;
                for (uint32_t c = 0; c < m; ++c) row[c] = label_in[r][members[c]];
                label_in[r] = row;
            }
    }
    const LabelPlan lp = plan_labels(m, label_in[0], label_in[1], ctx->snapshot_finalize_on_device);
    const bool label_group = lp.device_route && lp.which != 0;
    BuildScratch s;
    if (int rc = carve_build_scratch(ctx, m, R, &s); rc != GF_OK) return rc;
    const uint32_t* const d_cl_flags = s.flags;
    if (set)
        if (int rc = carve_set_scratch(ctx, members, &s); rc != GF_OK) return rc;
    for (int j = 0; j < 3 && R; ++j)
        GF_HIP(ctx, hipMemcpyAsync(s.res_req + j * R, rcols[j], R * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (R) GF_HIP(ctx, hipMemcpyAsync(s.res_node, res_node, R * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (flags_upload) {
        GF_HIP(ctx, hipMemcpyAsync(const_cast<uint32_t*>(d_cl_flags), flags_upload, N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        ctx->d_flags_default = node_flags == nullptr;
    }
    if (label_group) {  // the rank arrays that re-sort something: 4 bytes per node each, like the flags
        if (lp.driver_active) GF_HIP(ctx, hipMemcpyAsync(s.label_d, label_in[0], M * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (lp.exec_active) GF_HIP(ctx, hipMemcpyAsync(s.label_x, label_in[1], M * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    if (set) {  // the row (8 bytes per 64 nodes), then the members' columns gathered on the device
        const size_t W = (N + 63) / 64;
        GF_HIP(ctx, hipMemcpyAsync(s.set_words, member_words, W * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        // nbits, and behind it the sums of entries that travel: by cluster index, so that an entry on a non-member is never read
        GF_HIP(ctx, hipMemsetAsync(s.set_nbits, 0, (W + (usage_resident ? 0 : 3 * N)) * sizeof(uint64_t), st));
        if (R)
            GF_HIP(ctx, gangfit::launch_usage_apply(n_res, n, s.res_node, s.res_req, +1, s.set_usage, nullptr, nullptr, st));
        gangfit::SnapshotSetGather g{};
        g.n_nodes = n;
        g.n_members = m;
        g.d_words = s.set_words;
        g.d_nbits = s.set_nbits;
        g.d_prefix = s.set_prefix;
        g.d_alloc = ctx->d_cl_i64.ptr;
        g.d_overhead = ctx->cl_over ? ctx->d_cl_i64.ptr + 3 * N : nullptr;
        g.d_usage = usage_resident ? ctx->d_cl_usage.ptr : s.set_usage;
        g.d_zone = ctx->d_cl_u32.ptr;
        g.d_name_rank = ctx->d_cl_u32.ptr + N;
        g.d_flags = d_cl_flags;
        g.c_alloc = s.alloc;
        g.c_overhead = s.over;
        g.c_usage = s.usage;
        g.c_zone = s.zone;
        g.c_flags = s.flags;
        g.c_name_rank = s.name_rank;
        g.c_node = s.set_node;
        GF_HIP(ctx, gangfit::launch_snapshot_set_gather(g, st));
    }
    GF_HIP(ctx, ctx->d_sortwork.reserve(gangfit::snapshot_sort_work_words()));
    GF_HIP(ctx, gangfit::launch_snapshot_build(build_args(ctx, s, set ? 0 : n_res, usage_resident, lp), st));
    if (lp.device_route) {
        if (label_group) {
            info.label_group = 1;
            gangfit::LabelMerge mc{};
            mc.n_nodes = m;
            mc.d_order = s.perm_b;
            mc.d_flags = s.flags;
            mc.d_ppos = s.ppos;
            mc.d_rank[0] = lp.driver_active ? s.label_d : nullptr;
            mc.d_rank[1] = lp.exec_active ? s.label_x : nullptr;
            mc.d_summary = s.merge_summary;
            mc.d_fail = ctx->d_sortwork.ptr + gangfit::snapshot_sort_error_word() + 1;
            GF_HIP(ctx, gangfit::launch_label_merge_check(mc, st));
        }
        const int rc = finalize_on_device(ctx, s, out, &info);
        if (rc != GF_OK || !info.merge_failed) return done(rc, 1);
    }
    // (behind a label key group the sort left the priority order itself in perm_p)
    return done(finalize_on_host(ctx, s, label_group ? s.perm_p : s.perm_b, driver_label_rank, exec_label_rank, out, &info), 2);
}

// ... on every device of a multi-device context (the caller's order lists come from the first device only)
int build_resident_each(gf_ctx* ctx, const uint64_t* member_words, uint32_t n_res, const uint32_t* res_node, const int64_t* res_cpu_milli,
                        const int64_t* res_mem_bytes, const int64_t* res_gpu, const uint32_t* node_flags, const uint32_t* driver_label_rank,
                        const uint32_t* exec_label_rank, const OrderOuts& out) {
    if (!ctx) return GF_ERR_INVALID;
    if (ctx->group.empty())
        return build_resident(ctx, member_words, n_res, res_node, res_cpu_milli, res_mem_bytes, res_gpu, node_flags, driver_label_rank,
                              exec_label_rank, out);
    return each_device(ctx, nullptr, [&](gf_ctx* sub, bool first) {
        return build_resident(sub, member_words, n_res, res_node, res_cpu_milli, res_mem_bytes, res_gpu, node_flags, driver_label_rank,
                              exec_label_rank, first ? out : OrderOuts{nullptr, nullptr, nullptr, nullptr});
    });
}

}  // namespace

extern "C" int gf_snapshot_build_resident(gf_ctx* ctx, uint32_t n_res, const uint32_t* res_node, const int64_t* res_cpu_milli,
                                          const int64_t* res_mem_bytes, const int64_t* res_gpu, const uint32_t* node_flags,
                                          const uint32_t* driver_label_rank, const uint32_t* exec_label_rank,
                                          uint32_t* driver_order_out, uint32_t* n_d_out, uint32_t* exec_order_out, uint32_t* n_x_out) {
    return build_resident_each(ctx, nullptr, n_res, res_node, res_cpu_milli, res_mem_bytes, res_gpu, node_flags, driver_label_rank,
                               exec_label_rank, OrderOuts{driver_order_out, n_d_out, exec_order_out, n_x_out});
}

extern "C" int gf_snapshot_build_resident_set(gf_ctx* ctx, const uint64_t* member_words, uint32_t n_res, const uint32_t* res_node,
                                              const int64_t* res_cpu_milli, const int64_t* res_mem_bytes, const int64_t* res_gpu,
                                              const uint32_t* node_flags, const uint32_t* driver_label_rank,
                                              const uint32_t* exec_label_rank, uint32_t* driver_order_out, uint32_t* n_d_out,
                                              uint32_t* exec_order_out, uint32_t* n_x_out) {
    return build_resident_each(ctx, member_words, n_res, res_node, res_cpu_milli, res_mem_bytes, res_gpu, node_flags, driver_label_rank,
                               exec_label_rank, OrderOuts{driver_order_out, n_d_out, exec_order_out, n_x_out});
}

extern "C" {

int gf_snapshot_get(gf_ctx* ctx, int64_t* avail_out, int64_t* sched_out) {
    GF_DELEGATE(ctx, gf_snapshot_get(ctx, avail_out, sched_out));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_VIEW_ENTER(ctx)
    if (!ctx->have_snapshot) return fail(ctx, GF_ERR_STATE, "no snapshot");
    if (int mrc = materialize_host(ctx); mrc != GF_OK) return mrc;
    for (uint32_t i = 0; i < ctx->n_nodes; ++i)
        for (int j = 0; j < 3; ++j) {
            if (avail_out) avail_out[3 * (size_t)i + j] = ctx->avail[j][i];
            if (sched_out) sched_out[3 * (size_t)i + j] = ctx->have_sched ? ctx->sched[j][i] : 0;
        }
    return GF_OK;
}

int gf_residual_get(gf_ctx* ctx, int64_t* avail_out) {
    GF_DELEGATE(ctx, gf_residual_get(ctx, avail_out));
    if (!ctx || !avail_out) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_VIEW_ENTER(ctx)
    if (!ctx->have_orders || !ctx->work_valid) return fail(ctx, GF_ERR_STATE, "no FIFO chain has run on the current orders");
    if (int mrc = materialize_host(ctx); mrc != GF_OK) return mrc;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, ctx->h_table.reserve(3 * (size_t)ctx->n_slots));
    GF_HIP(ctx, hipMemcpyAsync(ctx->h_table.ptr, ctx->d_work.ptr, 3 * (size_t)ctx->n_slots * sizeof(int64_t),
                               hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP(ctx, gf_wait_stream(ctx->stream));
    const int64_t* t = ctx->h_table.ptr;
    for (uint32_t n = 0; n < ctx->n_nodes; ++n) {
        const uint32_t s = ctx->h_node_slot[n];
        for (int j = 0; j < 3; ++j)
            avail_out[3 * (size_t)n + j] = (s == GF_NO_NODE) ? ctx->avail[j][n] : t[(size_t)j * ctx->n_slots + s];
    }
    return GF_OK;
}

int gf_snapshot_build_info(gf_ctx* ctx, uint32_t out[4]) {
    GF_DELEGATE(ctx, gf_snapshot_build_info(ctx, out));
    if (!ctx || !out) return GF_ERR_INVALID;
    gf_ctx* const src = ctx->view_of != nullptr ? ctx->view_of : ctx;  // a view fits on its parent's snapshot: its parent's build
    std::lock_guard<std::recursive_mutex> lock(src->mu);
    for (int i = 0; i < 4; ++i) out[i] = src->build_info[i];
    return GF_OK;
}

int gf_snapshot_set_info(gf_ctx* ctx, uint32_t out[4]) {
    GF_DELEGATE(ctx, gf_snapshot_set_info(ctx, out));
    if (!ctx || !out) return GF_ERR_INVALID;
    gf_ctx* const src = ctx->view_of != nullptr ? ctx->view_of : ctx;  // a view fits on its parent's layout
    std::lock_guard<std::recursive_mutex> lock(src->mu);
    if (!src->have_snapshot || !src->have_orders) return fail(ctx, GF_ERR_STATE, "no orders installed");
    const bool set = src->set_epoch == src->snap_epoch;
    out[0] = set ? 1u : 0u;
    out[1] = set ? src->set_members : src->n_nodes;
    out[2] = src->n_slots;
    out[3] = src->n_chunks;
    return GF_OK;
}

}  // extern "C"
