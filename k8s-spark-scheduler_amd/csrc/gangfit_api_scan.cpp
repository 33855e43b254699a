// gangfit_api_scan.cpp — gf_cluster_fit_feasible and gf_cluster_fit_feasible_sets: the UnschedulablePodMarker's empty-cluster
// question answered from the resident cluster columns (gangfit_scan.inc), next to the installed snapshot instead of in its place.
// Nothing here installs: no InstallGuard, no epoch, no generation, no chain cache, no worker_quiesce — the calls only read what
// gf_cluster_set uploaded and write buffers of their own (gf_ctx::d_scan_*).  gf_cluster_executor_fit: the executor Filter answered
// the same way (gangfit_exec_scan.inc) from the columns, the resident overhead rows, the usage sums and the per-node entry counts;
// its buffers are gf_ctx::d_xs_*.  gf_cluster_find_nodes: the failover reconciler's findNodes for every instance group, answered the
// same way (gangfit_find_scan.inc) on a working table of its own; its buffers are gf_ctx::d_cf_*.
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

// The set rows of the entry points that take them (n_sets rows of ceil(n_nodes / 64) words): the kernels trust a bit to name a node.
int set_rows_check(gf_ctx* ctx, uint32_t n_sets, const uint64_t* set_words) {
    const uint32_t n = ctx->cl_n;
    const size_t W = ((size_t)n + 63) / 64;
    if ((n & 63u) == 0u) return GF_OK;
    const uint64_t beyond = ~UINT64_C(0) << (n & 63u);
    for (uint32_t s = 0; s < n_sets; ++s)
        if (set_words[(size_t)s * W + (W - 1)] & beyond) return fail(ctx, GF_ERR_INVALID, "set %u has a bit at or beyond node %u", s, n);
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
    if (const int rc = set_rows_check(ctx, n_sets, set_words); rc != GF_OK) return rc;
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
        if (const int rc = set_rows_check(ctx, n_sets, set_words); rc != GF_OK) return rc;
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

// findNodes of the failover reconciler next to the installed snapshot (gangfit_find_scan.inc): reads the resident columns, the
// usage sums and the flags of gf_cluster_set; writes the d_cf_* buffers only — not d_work, not work_valid, no epoch.
int gf_cluster_find_nodes(gf_ctx* ctx, int chained, uint32_t n_sets, const uint64_t* set_words, const uint32_t* create_rank,
                          uint32_t n_req, const int64_t* exe, const int32_t* k, const uint32_t* req_set, gf_find_result* results,
                          uint32_t* exec_nodes, uint64_t exec_nodes_cap, uint32_t* reserved_adds, int64_t* residual_out) {
    GF_DELEGATE(ctx, gf_cluster_find_nodes(ctx, chained, n_sets, set_words, create_rank, n_req, exe, k, req_set, results, exec_nodes,
                                           exec_nodes_cap, reserved_adds, residual_out));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    if (!ctx->have_cluster) return fail(ctx, GF_ERR_STATE, "gf_cluster_set must precede gf_cluster_find_nodes");
    if (!ctx->usage_ok) return fail(ctx, GF_ERR_STATE, "the resident usage is unknown (a failed gf_usage_apply): gf_usage_reset must rebuild it");
    if (!ctx->cl_over_ok)
        return fail(ctx, GF_ERR_STATE, "the resident overhead is unknown (a failed gf_overhead_update): gf_cluster_set must replace it");
    if (n_req == 0) return GF_OK;
    if (!exe || !k || !results) return fail(ctx, GF_ERR_INVALID, "exe/k/results must not be NULL");
    if (n_req >= 0x80000000u) return fail(ctx, GF_ERR_INVALID, "n_req = %u", n_req);
    const uint32_t n = ctx->cl_n;
    const size_t N = n, W = (N + 63) / 64, R = n_req;
    if (!create_rank && N > 0) return fail(ctx, GF_ERR_INVALID, "create_rank must not be NULL");
    {
        std::vector<uint8_t> seen(N, 0);
        for (uint32_t i = 0; i < n; ++i) {
            if (create_rank[i] >= n || seen[create_rank[i]]) return fail(ctx, GF_ERR_INVALID, "create_rank is not a permutation (node %u)", i);
            seen[create_rank[i]] = 1;
        }
    }
    for (size_t i = 0; i < 3 * R; ++i)
        if (exe[i] < 0 || exe[i] >= GF_MAX_ABS_QUANTITY) return fail(ctx, GF_ERR_INVALID, "executor request outside [0, 2^62)");
    std::vector<uint64_t> exec_off(R);
    uint64_t total_k = 0;
    for (uint32_t q = 0; q < n_req; ++q) {
        if (k[q] < 0 || k[q] > GF_MAX_K) return fail(ctx, GF_ERR_INVALID, "k[%u] = %d outside [0, %d]", q, k[q], GF_MAX_K);
        exec_off[q] = total_k;
        total_k += (uint64_t)k[q];
    }
    if (n_sets > 0) {
        if (!req_set) return fail(ctx, GF_ERR_INVALID, "req_set must not be NULL with %u sets", n_sets);
        if (!set_words && W > 0) return fail(ctx, GF_ERR_INVALID, "set_words must not be NULL with %u sets", n_sets);
        for (uint32_t q = 0; q < n_req; ++q)
            if (req_set[q] >= n_sets) return fail(ctx, GF_ERR_INVALID, "req_set[%u] = %u names no set (%u sets)", q, req_set[q], n_sets);
        if (const int rc = set_rows_check(ctx, n_sets, set_words); rc != GF_OK) return rc;
    }
    const bool with_sets = n_sets > 0 && W > 0;
    // ---- the used rows: the rows some request names.  Under `chained` the reference keeps one table per instance group, so rows
    // of equal content are one used row, and two used rows must not share a node
    std::vector<uint32_t> row_set, req_row(R);
    if (!with_sets) {
        row_set.push_back(0u);
        std::fill(req_row.begin(), req_row.end(), 0u);
    } else {
        std::vector<uint32_t> used_of(n_sets, GF_NO_NODE);
        std::vector<uint64_t> hash;
        for (uint32_t q = 0; q < n_req; ++q) {
            const uint32_t s = req_set[q];
            if (used_of[s] == GF_NO_NODE) {
                const uint64_t* const row = set_words + (size_t)s * W;
                uint32_t u = (uint32_t)row_set.size();
                if (chained) {
                    uint64_t h = UINT64_C(0xcbf29ce484222325);
                    for (size_t w = 0; w < W; ++w) h = (h ^ row[w]) * UINT64_C(0x100000001b3);
                    for (uint32_t v = 0; v < (uint32_t)row_set.size() && u == (uint32_t)row_set.size(); ++v)
                        if (hash[v] == h && std::memcmp(set_words + (size_t)row_set[v] * W, row, W * sizeof(uint64_t)) == 0) u = v;
                    if (u == (uint32_t)row_set.size()) hash.push_back(h);
                }
                if (u == (uint32_t)row_set.size()) row_set.push_back(s);
                used_of[s] = u;
            }
            req_row[q] = used_of[s];
        }
        if (chained) {
            std::vector<uint64_t> all(W, 0);
            for (const uint32_t s : row_set) {
                const uint64_t* const row = set_words + (size_t)s * W;
                for (size_t w = 0; w < W; ++w) {
                    if (all[w] & row[w])
                        return fail(ctx, GF_ERR_INVALID, "set %u shares a node with another set of a chained call: rows are equal or disjoint", s);
                    all[w] |= row[w];
                }
            }
        }
    }
    if (total_k > exec_nodes_cap || (total_k > 0 && !exec_nodes))
        return fail(ctx, GF_ERR_CAPACITY, "exec_nodes holds %llu entries, %llu needed", (unsigned long long)exec_nodes_cap,
                    (unsigned long long)total_k);
    const size_t U = row_set.size();
    std::vector<uint64_t> row_base(U);
    uint64_t ord_len = 0;
    for (size_t u = 0; u < U; ++u) {
        row_base[u] = ord_len;
        if (!with_sets) {
            ord_len += N;
        } else {
            const uint64_t* const row = set_words + (size_t)row_set[u] * W;
            for (size_t w = 0; w < W; ++w) ord_len += (uint64_t)__builtin_popcountll(row[w]);
        }
    }
    // the requests grouped by used row, ascending q inside a row (a counting sort)
    std::vector<uint32_t> row_req(U + 1, 0), req_list(R);
    for (size_t q = 0; q < R; ++q) row_req[req_row[q] + 1]++;
    for (size_t u = 0; u < U; ++u) row_req[u + 1] += row_req[u];
    {
        std::vector<uint32_t> at(row_req.begin(), row_req.end() - 1);
        for (size_t q = 0; q < R; ++q) req_list[at[req_row[q]]++] = (uint32_t)q;
    }
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // ---- device layout.  64-bit: work 3N | exe 3R | exec_off R | row_base U.  32-bit: create_rank N | perm N | k R | row_set U |
    // row_req U + 1 | req_list R | req_row R | row_len U | ord
    const size_t o_exe = 3 * N, o_off = o_exe + 3 * R, o_base = o_off + R, n64 = o_base + U;
    const size_t o_perm = N, o_k = 2 * N, o_rset = o_k + R, o_rreq = o_rset + U, o_list = o_rreq + U + 1, o_qrow = o_list + R,
                 o_len = o_qrow + R, o_ord = o_len + U, n32 = o_ord + (size_t)ord_len;
    GF_HIP(ctx, ctx->d_cf_i64.reserve(n64));
    GF_HIP(ctx, ctx->d_cf_u32.reserve(n32 + 1));
    GF_HIP(ctx, ctx->d_cf_res.reserve(R));
    GF_HIP(ctx, ctx->d_cf_exec.reserve((size_t)total_k + 1));
    int64_t* const d64 = ctx->d_cf_i64.ptr;
    uint32_t* const d32 = ctx->d_cf_u32.ptr;
    const auto up = [st](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    GF_HIP(ctx, up(d64 + o_exe, exe, 3 * R * sizeof(int64_t)));
    GF_HIP(ctx, up(d64 + o_off, exec_off.data(), R * sizeof(uint64_t)));
    GF_HIP(ctx, up(d64 + o_base, row_base.data(), U * sizeof(uint64_t)));
    GF_HIP(ctx, up(d32, create_rank, N * sizeof(uint32_t)));  // the one O(n_nodes) array this call moves
    GF_HIP(ctx, up(d32 + o_k, k, R * sizeof(int32_t)));
    GF_HIP(ctx, up(d32 + o_rset, row_set.data(), U * sizeof(uint32_t)));
    GF_HIP(ctx, up(d32 + o_rreq, row_req.data(), (U + 1) * sizeof(uint32_t)));
    GF_HIP(ctx, up(d32 + o_list, req_list.data(), R * sizeof(uint32_t)));
    GF_HIP(ctx, up(d32 + o_qrow, req_row.data(), R * sizeof(uint32_t)));
    if (with_sets) {
        const size_t n_words = (size_t)n_sets * W;
        GF_HIP(ctx, ctx->d_cf_sets.reserve(n_words));
        GF_HIP(ctx, up(ctx->d_cf_sets.ptr, set_words, n_words * sizeof(uint64_t)));
    }
    uint32_t* d_adds = nullptr;
    if (reserved_adds && N > 0) {
        GF_HIP(ctx, ctx->d_cf_adds.reserve(R * N));
        GF_HIP(ctx, hipMemsetAsync(ctx->d_cf_adds.ptr, 0, R * N * sizeof(uint32_t), st));
        d_adds = ctx->d_cf_adds.ptr;
    }
    const gangfit::FindScanArgs args{
        .alloc = ctx->d_cl_i64.ptr, .over = ctx->cl_over ? ctx->d_cl_i64.ptr + 3 * N : nullptr, .usage = ctx->d_cl_usage.ptr,
        .flags = ctx->d_cl_x32.ptr + N, .create_rank = d32, .set_words = with_sets ? ctx->d_cf_sets.ptr : nullptr,
        .row_set = d32 + o_rset, .row_base = reinterpret_cast<const uint64_t*>(d64 + o_base), .row_req = d32 + o_rreq,
        .req_list = d32 + o_list, .req_row = d32 + o_qrow, .exe = d64 + o_exe, .k = reinterpret_cast<const int32_t*>(d32 + o_k),
        .exec_off = reinterpret_cast<const uint64_t*>(d64 + o_off), .n_nodes = n, .n_words = 0, .n_rows = (uint32_t)U, .n_req = n_req,
        .perm = d32 + o_perm, .ord = d32 + o_ord, .row_len = d32 + o_len, .work = d64, .results = ctx->d_cf_res.ptr,
        .exec_nodes = ctx->d_cf_exec.ptr, .adds_out = d_adds};
    GF_HIP(ctx, gangfit::launch_cluster_find_nodes(chained != 0, args, st));
    GF_HIP(ctx, hipMemcpyAsync(results, ctx->d_cf_res.ptr, R * sizeof(gf_find_result), hipMemcpyDeviceToHost, st));
    if (total_k)
        GF_HIP(ctx, hipMemcpyAsync(exec_nodes, ctx->d_cf_exec.ptr, (size_t)total_k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (d_adds) GF_HIP(ctx, hipMemcpyAsync(reserved_adds, d_adds, R * N * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    std::vector<int64_t> cols;
    if (residual_out && N > 0) {
        cols.resize(3 * N);
        GF_HIP(ctx, hipMemcpyAsync(cols.data(), d64, 3 * N * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    GF_HIP(ctx, gf_wait_stream(st));  // the caller's arrays are free again, the answers have arrived
    for (size_t i = 0; i < cols.size() / 3; ++i)
        for (int j = 0; j < 3; ++j) residual_out[3 * i + j] = cols[(size_t)j * N + i];
    return GF_OK;
}

}  // extern "C"
