// gangfit_api_scan.cpp — gf_cluster_fit_feasible and gf_cluster_fit_feasible_sets: the UnschedulablePodMarker's empty-cluster
// question answered from the resident cluster columns (gangfit_scan.inc), next to the installed snapshot instead of in its place.
// Nothing here installs: no InstallGuard, no epoch, no generation, no chain cache, no worker_quiesce — the calls only read what
// gf_cluster_set uploaded and write buffers of their own (gf_ctx::d_scan_*).  gf_cluster_executor_fit: the executor Filter answered
// the same way (gangfit_exec_scan.inc) from the columns, the resident overhead rows, the usage sums and the per-node entry counts;
// its buffers are gf_ctx::d_xs_*.
#include "gangfit_ctx.h"

using namespace gfapi;

namespace {

struct ScanQuestion {
    const int64_t* ocols[3];
    bool with_over, zoned;
};

// What both entry points refuse, in one order; *q = what the launch needs.  `who` names the entry point in the messages.
int scan_check(gf_ctx* ctx, const char* who, gf_algo algo, const int64_t* over_cpu_milli, const int64_t* over_mem_bytes,
               const int64_t* over_gpu, uint32_t n_apps, const gf_app* apps, const uint8_t* has_capacity, ScanQuestion* q) {
    if (!ctx->have_cluster) return fail(ctx, GF_ERR_STATE, "gf_cluster_set must precede %s", who);
    const bool zone_aware = is_zone_algo(algo);
    if (!zone_aware && !is_plain_algo(algo)) return fail(ctx, GF_ERR_UNSUPPORTED, "gf_algo %d is not served by the device path", (int)algo);
    const bool with_over = over_cpu_milli || over_mem_bytes || over_gpu;
    if (with_over && !(over_cpu_milli && over_mem_bytes && over_gpu))
        return fail(ctx, GF_ERR_INVALID, "overhead columns must be all NULL or all set");
    const uint32_t n = ctx->cl_n;
    const size_t N = n;
    const int64_t* ocols[3] = {over_cpu_milli, over_mem_bytes, over_gpu};
    bool over_exceeds = false;  // some node's overhead is above its allocatable: a negative schedulable quantity
    if (with_over) {
        const int64_t lim = GF_MAX_ABS_QUANTITY >> 1;
        for (int j = 0; j < 3; ++j)
            for (uint32_t i = 0; i < n; ++i) {
                if (ocols[j][i] < 0 || ocols[j][i] >= lim) return fail(ctx, GF_ERR_INVALID, "overhead value out of range at node %u", i);
                over_exceeds |= ocols[j][i] > ctx->cl_alloc[(size_t)j * N + i];
            }
    }
    if (n_apps > 0 && (!apps || !has_capacity)) return fail(ctx, GF_ERR_INVALID, "apps/has_capacity must not be NULL");
    uint64_t total_k = 0;
    if (const int rc = check_apps(ctx, n_apps, apps, nullptr, &total_k); rc != GF_OK) return rc;
    if (zone_aware) {
        // the zone-aware answer is chooseBestResult's: some zone fits AND its average Max efficiency is above 0 (single_az.go:75-97).
        // The scan skips the averages, so it only serves what makes them positive by construction (gf_fit_feasible's
        // `surely_positive`): available == schedulable >= 0 on every node, and a driver that asks for cpu or memory
        if (ctx->cl_zones > 64u)
            return fail(ctx, GF_ERR_UNSUPPORTED, "the capacity scan serves the zone-aware packers on at most 64 zones (%u)", ctx->cl_zones);
        if (over_exceeds)
            return fail(ctx, GF_ERR_UNSUPPORTED, "a node's overhead exceeds its allocatable: the zone-aware answer needs the averages");
        for (uint32_t a = 0; a < n_apps; ++a)
            if (apps[a].drv[0] == 0 && apps[a].drv[1] == 0)
                return fail(ctx, GF_ERR_UNSUPPORTED, "apps[%u]'s driver asks for neither cpu nor memory: the zone-aware answer needs the averages", a);
    }
    if (n_apps >= 0x80000000u) return fail(ctx, GF_ERR_INVALID, "n_apps = %u", n_apps);
    for (int j = 0; j < 3; ++j) q->ocols[j] = ocols[j];
    q->with_over = with_over;
    // az-aware-tightly-pack falls back to the plain order when no single zone fits (az_aware_pack_tightly.go:33-37), and a gang
    // that fits one zone fits the plain order: its answer is the plain one
    q->zoned = zone_aware && algo != GF_ALGO_AZ_AWARE_TIGHTLY_PACK;
    return GF_OK;
}

// The overhead columns and the records on their way to the device; the previous scan has left these buffers (the calls block).
int scan_upload(gf_ctx* ctx, const ScanQuestion& q, uint32_t n_apps, const gf_app* apps, hipStream_t st) {
    const size_t N = ctx->cl_n;
    GF_HIP(ctx, ctx->d_scan_over.reserve(3 * N + 1));
    GF_HIP(ctx, ctx->d_scan_apps.reserve(n_apps));
    GF_HIP(ctx, ctx->d_scan_out.reserve(n_apps));
    GF_HIP(ctx, ctx->h_scan_out.reserve(n_apps));
    if (q.with_over)
        for (int j = 0; j < 3 && N; ++j)
            GF_HIP(ctx, hipMemcpyAsync(ctx->d_scan_over.ptr + (size_t)j * N, q.ocols[j], N * sizeof(int64_t), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_scan_apps.ptr, apps, (size_t)n_apps * sizeof(gf_app), hipMemcpyHostToDevice, st));
    return GF_OK;
}

int scan_answers(gf_ctx* ctx, uint32_t n_apps, uint8_t* has_capacity, hipStream_t st) {
    GF_HIP(ctx, hipMemcpyAsync(ctx->h_scan_out.ptr, ctx->d_scan_out.ptr, n_apps, hipMemcpyDeviceToHost, st));
    GF_HIP(ctx, gf_wait_stream(st));  // the caller's arrays are free again, the answers have arrived
    std::memcpy(has_capacity, ctx->h_scan_out.ptr, n_apps);
    return GF_OK;
}

}  // namespace

extern "C" {

int gf_cluster_fit_feasible(gf_ctx* ctx, gf_algo algo, const int64_t* over_cpu_milli, const int64_t* over_mem_bytes,
                            const int64_t* over_gpu, const uint8_t* node_select, uint32_t n_apps, const gf_app* apps,
                            uint8_t* has_capacity) {
    GF_DELEGATE(ctx, gf_cluster_fit_feasible(ctx, algo, over_cpu_milli, over_mem_bytes, over_gpu, node_select, n_apps, apps, has_capacity));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    ScanQuestion q{};
    if (const int rc = scan_check(ctx, "gf_cluster_fit_feasible", algo, over_cpu_milli, over_mem_bytes, over_gpu, n_apps, apps, has_capacity, &q);
        rc != GF_OK)
        return rc;
    if (n_apps == 0) return GF_OK;
    const uint32_t n = ctx->cl_n;
    const size_t N = n;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    GF_HIP(ctx, ctx->d_scan_select.reserve(N + 1));
    if (const int rc = scan_upload(ctx, q, n_apps, apps, st); rc != GF_OK) return rc;
    if (node_select != nullptr && N) GF_HIP(ctx, hipMemcpyAsync(ctx->d_scan_select.ptr, node_select, N, hipMemcpyHostToDevice, st));
    const gangfit::ScanArgs args{.alloc = ctx->d_cl_i64.ptr, .over = q.with_over ? ctx->d_scan_over.ptr : nullptr, .zone = ctx->d_cl_u32.ptr,
                                 .select = node_select != nullptr ? ctx->d_scan_select.ptr : nullptr, .n_nodes = n, .n_apps = n_apps,
                                 .apps = ctx->d_scan_apps.ptr, .out = ctx->d_scan_out.ptr};
    GF_HIP(ctx, gangfit::launch_cluster_scan(q.zoned, args, st));
    return scan_answers(ctx, n_apps, has_capacity, st);
}

int gf_cluster_fit_feasible_sets(gf_ctx* ctx, gf_algo algo, const int64_t* over_cpu_milli, const int64_t* over_mem_bytes,
                                 const int64_t* over_gpu, uint32_t n_sets, const uint64_t* set_words, const uint32_t* app_set,
                                 uint32_t n_apps, const gf_app* apps, uint8_t* has_capacity) {
    GF_DELEGATE(ctx, gf_cluster_fit_feasible_sets(ctx, algo, over_cpu_milli, over_mem_bytes, over_gpu, n_sets, set_words, app_set, n_apps, apps, has_capacity));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    ScanQuestion q{};
    if (const int rc = scan_check(ctx, "gf_cluster_fit_feasible_sets", algo, over_cpu_milli, over_mem_bytes, over_gpu, n_apps, apps, has_capacity, &q);
        rc != GF_OK)
        return rc;
    if (n_apps == 0) return GF_OK;
    const uint32_t n = ctx->cl_n;
    const size_t W = ((size_t)n + 63) / 64;
    if (n_sets == 0) return fail(ctx, GF_ERR_INVALID, "n_sets = 0 with %u applications", n_apps);
    // (a cluster of no node has rows of no word: nothing to point at, and every set is empty)
    if ((!set_words && W > 0) || !app_set) return fail(ctx, GF_ERR_INVALID, "set_words/app_set must not be NULL");
    for (uint32_t a = 0; a < n_apps; ++a)
        if (app_set[a] >= n_sets) return fail(ctx, GF_ERR_INVALID, "app_set[%u] = %u names no set (%u sets)", a, app_set[a], n_sets);
    if ((n & 63u) != 0u) {  // the kernel trusts a bit to name a node
        const uint64_t beyond = ~UINT64_C(0) << (n & 63u);
        for (uint32_t s = 0; s < n_sets; ++s)
            if (set_words[(size_t)s * W + (W - 1)] & beyond) return fail(ctx, GF_ERR_INVALID, "set %u has a bit at or beyond node %u", s, n);
    }
    const size_t n_words = (size_t)n_sets * W;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    GF_HIP(ctx, ctx->d_scan_sets.reserve(n_words + 1));
    GF_HIP(ctx, ctx->d_scan_app_set.reserve(n_apps));
    if (const int rc = scan_upload(ctx, q, n_apps, apps, st); rc != GF_OK) return rc;
    if (n_words) GF_HIP(ctx, hipMemcpyAsync(ctx->d_scan_sets.ptr, set_words, n_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_scan_app_set.ptr, app_set, (size_t)n_apps * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    const gangfit::ScanSetsArgs args{.alloc = ctx->d_cl_i64.ptr, .over = q.with_over ? ctx->d_scan_over.ptr : nullptr, .zone = ctx->d_cl_u32.ptr,
                                     .set_words = ctx->d_scan_sets.ptr, .app_set = ctx->d_scan_app_set.ptr, .n_nodes = n, .n_apps = n_apps,
                                     .apps = ctx->d_scan_apps.ptr, .out = ctx->d_scan_out.ptr};
    GF_HIP(ctx, gangfit::launch_cluster_scan_sets(q.zoned, args, st));
    return scan_answers(ctx, n_apps, has_capacity, st);
}

// The executor Filter next to the installed snapshot: reads the resident columns, the usage sums and the entry counts; writes the
// d_xs_* buffers only.
int gf_cluster_executor_fit(gf_ctx* ctx, int minimal_fragmentation, uint32_t n_sets, const uint64_t* set_words, uint32_t n_req,
                            const int64_t* exe, const uint32_t* req_set, const uint32_t* hosts_app, const uint32_t* node_zone,
                            const uint32_t* req_zone, const uint32_t* exec_label_rank, uint32_t* node_out) {
    GF_DELEGATE(ctx, gf_cluster_executor_fit(ctx, minimal_fragmentation, n_sets, set_words, n_req, exe, req_set, hosts_app, node_zone,
                                             req_zone, exec_label_rank, node_out));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    if (!ctx->have_cluster) return fail(ctx, GF_ERR_STATE, "gf_cluster_set must precede gf_cluster_executor_fit");
    if (!ctx->usage_ok) return fail(ctx, GF_ERR_STATE, "the resident usage is unknown (a failed gf_usage_apply): gf_usage_reset must rebuild it");
    if (!ctx->cl_over_ok)
        return fail(ctx, GF_ERR_STATE, "the resident overhead is unknown (a failed gf_overhead_update): gf_cluster_set must replace it");
    if (ctx->cl_zones > 64u)
        return fail(ctx, GF_ERR_UNSUPPORTED, "the resident executor Filter ranks at most 64 zones (%u)", ctx->cl_zones);
    if (n_req == 0) return GF_OK;
    if (!exe || !node_out) return fail(ctx, GF_ERR_INVALID, "exe/node_out must not be NULL");
    if (n_req >= 0x80000000u) return fail(ctx, GF_ERR_INVALID, "n_req = %u", n_req);
    for (size_t i = 0; i < 3 * (size_t)n_req; ++i)
        if (exe[i] < 0 || exe[i] >= GF_MAX_ABS_QUANTITY) return fail(ctx, GF_ERR_INVALID, "executor request outside [0, 2^62)");
    const uint32_t n = ctx->cl_n;
    const size_t N = n, W = (N + 63) / 64;
    if (n_sets > 0) {
        if (!req_set) return fail(ctx, GF_ERR_INVALID, "req_set must not be NULL with %u sets", n_sets);
        if (!set_words && W > 0) return fail(ctx, GF_ERR_INVALID, "set_words must not be NULL with %u sets", n_sets);
        for (uint32_t q = 0; q < n_req; ++q)
            if (req_set[q] >= n_sets) return fail(ctx, GF_ERR_INVALID, "req_set[%u] = %u names no set (%u sets)", q, req_set[q], n_sets);
        if ((n & 63u) != 0u) {  // the kernel trusts a bit to name a node
            const uint64_t beyond = ~UINT64_C(0) << (n & 63u);
            for (uint32_t s = 0; s < n_sets; ++s)
                if (set_words[(size_t)s * W + (W - 1)] & beyond) return fail(ctx, GF_ERR_INVALID, "set %u has a bit at or beyond node %u", s, n);
        }
    }
    if (node_zone != nullptr && req_zone == nullptr) return fail(ctx, GF_ERR_INVALID, "node_zone comes with req_zone");
    if (node_zone)
        for (uint32_t i = 0; i < n; ++i)
            if (node_zone[i] == GF_ANY_ZONE) return fail(ctx, GF_ERR_INVALID, "node_zone[%u] is GF_ANY_ZONE: a node has a zone", i);
    const bool with_sets = n_sets > 0 && W > 0;
    const uint32_t hosts_stride = (n + 31) / 32;
    const bool with_hosts = minimal_fragmentation && hosts_app && hosts_stride > 0;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // ---- the requests: exe | set row | zone, one copy from pinned staging (the previous call has left these buffers: it blocked)
    const size_t R = n_req, req_words = 3 * R + (R + 1) / 2 * 2;
    GF_HIP(ctx, ctx->h_xs_req.reserve(req_words));
    GF_HIP(ctx, ctx->d_xs_req.reserve(req_words));
    GF_HIP(ctx, ctx->d_xs_out.reserve(R));
    GF_HIP(ctx, ctx->h_xs_out.reserve(R));
    std::memcpy(ctx->h_xs_req.ptr, exe, 3 * R * sizeof(int64_t));
    uint32_t* const h_set = reinterpret_cast<uint32_t*>(ctx->h_xs_req.ptr + 3 * R);
    uint32_t* const h_zone = h_set + (R + 1) / 2 * 2;
    for (size_t q = 0; q < R; ++q) {
        h_set[q] = with_sets ? req_set[q] : 0u;
        h_zone[q] = req_zone ? req_zone[q] : GF_ANY_ZONE;
    }
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_xs_req.ptr, ctx->h_xs_req.ptr, req_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    const uint32_t* const d_set = reinterpret_cast<const uint32_t*>(ctx->d_xs_req.ptr + 3 * R);
    const uint32_t* const d_zone = d_set + (R + 1) / 2 * 2;
    if (with_sets) {
        const size_t n_words = (size_t)n_sets * W;
        GF_HIP(ctx, ctx->d_xs_sets.reserve(n_words));
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_xs_sets.ptr, set_words, n_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    if (with_hosts) {
        GF_HIP(ctx, ctx->d_xs_hosts.reserve(R * hosts_stride));
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_xs_hosts.ptr, hosts_app, R * hosts_stride * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    if ((node_zone || exec_label_rank) && N) {  // the only O(n_nodes) arrays this call ever moves
        GF_HIP(ctx, ctx->d_xs_cols.reserve(2 * N));
        if (node_zone) GF_HIP(ctx, hipMemcpyAsync(ctx->d_xs_cols.ptr, node_zone, N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (exec_label_rank)
            GF_HIP(ctx, hipMemcpyAsync(ctx->d_xs_cols.ptr + N, exec_label_rank, N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    const gangfit::ExecScanArgs args{
        .alloc = ctx->d_cl_i64.ptr, .over = ctx->cl_over ? ctx->d_cl_i64.ptr + 3 * N : nullptr, .usage = ctx->d_cl_usage.ptr,
        .res_count = ctx->d_cl_x32.ptr, .zone = ctx->d_cl_u32.ptr, .name_rank = ctx->d_cl_u32.ptr + N, .flags = ctx->d_cl_x32.ptr + N,
        .node_zone = node_zone && N ? ctx->d_xs_cols.ptr : nullptr, .label_rank = exec_label_rank && N ? ctx->d_xs_cols.ptr + N : nullptr,
        .set_words = with_sets ? ctx->d_xs_sets.ptr : nullptr, .req_set = with_sets ? d_set : nullptr, .req_zone = req_zone ? d_zone : nullptr,
        .hosts = with_hosts ? ctx->d_xs_hosts.ptr : nullptr, .exe = reinterpret_cast<const int64_t*>(ctx->d_xs_req.ptr), .n_nodes = n,
        .n_zones = ctx->cl_zones, .n_req = n_req, .hosts_stride = hosts_stride, .out = ctx->d_xs_out.ptr};
    GF_HIP(ctx, gangfit::launch_cluster_executor_fit(minimal_fragmentation != 0, args, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->h_xs_out.ptr, ctx->d_xs_out.ptr, R * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GF_HIP(ctx, gf_wait_stream(st));  // the caller's arrays are free again, the answers have arrived
    std::memcpy(node_out, ctx->h_xs_out.ptr, R * sizeof(uint32_t));
    return GF_OK;
}

}  // extern "C"
