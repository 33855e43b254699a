// gangfit_api_scan.cpp — gf_cluster_fit_feasible: the UnschedulablePodMarker's empty-cluster question answered from the resident
// cluster columns (gangfit_scan.inc), next to the installed snapshot instead of in its place.  Nothing here installs: no
// InstallGuard, no epoch, no generation, no chain cache, no worker_quiesce — the call only reads what gf_cluster_set uploaded and
// writes buffers of its own (gf_ctx::d_scan_*).
#include "gangfit_ctx.h"

using namespace gfapi;

extern "C" {

int gf_cluster_fit_feasible(gf_ctx* ctx, gf_algo algo, const int64_t* over_cpu_milli, const int64_t* over_mem_bytes,
                            const int64_t* over_gpu, const uint8_t* node_select, uint32_t n_apps, const gf_app* apps,
                            uint8_t* has_capacity) {
    GF_DELEGATE(ctx, gf_cluster_fit_feasible(ctx, algo, over_cpu_milli, over_mem_bytes, over_gpu, node_select, n_apps, apps, has_capacity));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_NOT_ON_A_VIEW(ctx);
    if (!ctx->have_cluster) return fail(ctx, GF_ERR_STATE, "gf_cluster_set must precede gf_cluster_fit_feasible");
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
    if (n_apps == 0) return GF_OK;
    if (n_apps >= 0x80000000u) return fail(ctx, GF_ERR_INVALID, "n_apps = %u", n_apps);
    // az-aware-tightly-pack falls back to the plain order when no single zone fits (az_aware_pack_tightly.go:33-37), and a gang
    // that fits one zone fits the plain order: its answer is the plain one
    const bool zoned = zone_aware && algo != GF_ALGO_AZ_AWARE_TIGHTLY_PACK;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the call is blocking, so the previous scan has left these buffers; nothing else names them
    GF_HIP(ctx, ctx->d_scan_over.reserve(3 * N + 1));
    GF_HIP(ctx, ctx->d_scan_select.reserve(N + 1));
    GF_HIP(ctx, ctx->d_scan_apps.reserve(n_apps));
    GF_HIP(ctx, ctx->d_scan_out.reserve(n_apps));
    GF_HIP(ctx, ctx->h_scan_out.reserve(n_apps));
    if (with_over)
        for (int j = 0; j < 3 && N; ++j)
            GF_HIP(ctx, hipMemcpyAsync(ctx->d_scan_over.ptr + (size_t)j * N, ocols[j], N * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (node_select != nullptr && N) GF_HIP(ctx, hipMemcpyAsync(ctx->d_scan_select.ptr, node_select, N, hipMemcpyHostToDevice, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_scan_apps.ptr, apps, (size_t)n_apps * sizeof(gf_app), hipMemcpyHostToDevice, st));
    GF_HIP(ctx, gangfit::launch_cluster_scan(zoned, n, ctx->d_cl_i64.ptr, with_over ? ctx->d_scan_over.ptr : nullptr, ctx->d_cl_u32.ptr,
                                             node_select != nullptr ? ctx->d_scan_select.ptr : nullptr, n_apps, ctx->d_scan_apps.ptr,
                                             ctx->d_scan_out.ptr, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->h_scan_out.ptr, ctx->d_scan_out.ptr, n_apps, hipMemcpyDeviceToHost, st));
    GF_HIP(ctx, gf_wait_stream(st));  // the caller's arrays are free again, the answers have arrived
    std::memcpy(has_capacity, ctx->h_scan_out.ptr, n_apps);
    return GF_OK;
}

}  // extern "C"
