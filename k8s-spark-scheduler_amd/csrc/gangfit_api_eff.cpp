// gangfit_api_eff.cpp — gf_filter_efficiency: the value selectDriverNode hands to metrics.ReportPackingEfficiency
// (internal/extender/resource.go:329, 352, 372-381), ComputeAvgPackingEfficiency over one PackingEfficiency per metadata key, summed
// on the device (gangfit_filter_eff.inc) against the installed snapshot or against what the last FIFO chain left in the working
// table.  Nothing here installs: no InstallGuard, no epoch, no generation, no chain cache, no worker_quiesce — the call reads the
// node-indexed tables, node_slot and d_work, and writes buffers of its own (gf_ctx::d_fe_*).
#include "gangfit_ctx.h"

using namespace gfapi;

extern "C" {

int gf_filter_efficiency(gf_ctx* ctx, gf_algo algo, int against, const gf_app* app, const gf_result* result,
                         const uint32_t* exec_nodes, const uint64_t* member_words, gf_avg_efficiency* out,
                         uint32_t counts_out[2]) {
    GF_DELEGATE(ctx, gf_filter_efficiency(ctx, algo, against, app, result, exec_nodes, member_words, out, counts_out));
    if (!ctx) return GF_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    GF_VIEW_ENTER(ctx)
    if (!app || !result || !out) return fail(ctx, GF_ERR_INVALID, "app/result/out must not be NULL");
    if (against != GF_EFF_AGAINST_SNAPSHOT && against != GF_EFF_AGAINST_RESIDUAL)
        return fail(ctx, GF_ERR_INVALID, "against = %d is neither GF_EFF_AGAINST_SNAPSHOT nor GF_EFF_AGAINST_RESIDUAL", against);
    gf_app rec;
    uint64_t total_k = 0;
    if (const int rc = check_apps(ctx, 1, app, &rec, &total_k); rc != GF_OK) return rc;  // k in [0, GF_MAX_K]; exec_off = 0
    if (!ctx->have_snapshot || !ctx->have_sched)
        return fail(ctx, GF_ERR_STATE, "efficiencies need gf_snapshot_set with the schedulable columns");
    const bool residual = against == GF_EFF_AGAINST_RESIDUAL;
    if (residual && (!ctx->have_orders || !ctx->work_valid))
        return fail(ctx, GF_ERR_STATE, "no FIFO chain has run on the current orders");
    const bool with_execs = reserves_executors(algo) && result->has_capacity && rec.k > 0;
    if (with_execs && !exec_nodes) return fail(ctx, GF_ERR_INVALID, "exec_nodes must not be NULL");
    const uint32_t n = ctx->n_nodes;
    const uint32_t n_words = (uint32_t)(((uint64_t)n + 63u) / 64u);
    if (member_words != nullptr && (n & 63u) != 0u && (member_words[n_words - 1] >> (n & 63u)) != 0ull)
        return fail(ctx, GF_ERR_INVALID, "member_words names a node at or beyond n_nodes = %u", n);
    static_assert(sizeof(gf_avg_efficiency) == 4 * sizeof(double), "gf_avg_efficiency layout");
    out->cpu = out->memory = out->gpu = out->max = 0.0;
    if (counts_out) counts_out[0] = counts_out[1] = 0u;
    if (!result->has_capacity || n == 0) return GF_OK;  // WorstAvgPackingEfficiency (efficiency.go:119-121): nothing is launched

    GF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    static_assert(sizeof(gf_app) == 64 && sizeof(gf_result) == 16, "the staged record");
    constexpr size_t kAppWords = sizeof(gf_app) / 8, kResWords = sizeof(gf_result) / 8;
    const size_t n_exec = with_execs ? (size_t)rec.k : 0;
    const size_t in_words = kAppWords + kResWords + (n_exec + 1) / 2;
    const uint32_t n_pad = gangfit::filter_eff_pad(n_words);
    GF_HIP(ctx, ctx->h_fe_in.reserve(in_words));
    GF_HIP(ctx, ctx->d_fe_in.reserve(in_words));
    GF_HIP(ctx, ctx->d_fe_part.reserve(4 * (size_t)n_pad));
    GF_HIP(ctx, ctx->d_fe_cnt.reserve(2 * (size_t)n_pad));
    GF_HIP(ctx, ctx->d_fe_out.reserve(1));
    GF_HIP(ctx, ctx->h_fe_out.reserve(1));
    {
        const int64_t* before = ctx->d_fe_reserved.ptr;
        GF_HIP(ctx, ctx->d_fe_reserved.reserve(3 * (size_t)n));
        if (ctx->d_fe_reserved.ptr != before) ctx->fe_reserved_clean = false;
    }
    if (!ctx->fe_reserved_clean)  // once per allocation (or after a call that failed half way), not per call
        GF_HIP(ctx, hipMemsetAsync(ctx->d_fe_reserved.ptr, 0, ctx->d_fe_reserved.cap * sizeof(int64_t), st));
    ctx->fe_reserved_clean = false;  // until the combine kernel has cleared what the scatter wrote

    uint64_t* const h = ctx->h_fe_in.ptr;
    std::memcpy(h, &rec, sizeof rec);
    std::memcpy(h + kAppWords, result, sizeof *result);
    if (n_exec) {
        h[in_words - 1] = 0;
        std::memcpy(h + kAppWords + kResWords, exec_nodes, n_exec * sizeof(uint32_t));
    }
    GF_HIP(ctx, hipMemcpyAsync(ctx->d_fe_in.ptr, h, in_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (member_words != nullptr) {
        GF_HIP(ctx, ctx->d_fe_row.reserve(n_words));
        GF_HIP(ctx, hipMemcpyAsync(ctx->d_fe_row.ptr, member_words, (size_t)n_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    gangfit::FilterEffArgs a{};
    for (int j = 0; j < 3; ++j) {
        a.tab.avail[j] = ctx->d_node_tab.ptr + (size_t)j * n;
        a.tab.sched[j] = ctx->d_node_tab.ptr + (size_t)(3 + j) * n;
    }
    a.work = residual ? ctx->d_work.ptr : nullptr;
    a.node_slot = residual ? ctx->d_node_slot.ptr : nullptr;
    a.n_slots = ctx->n_slots;
    a.n_nodes = n;
    a.n_words = n_words;
    a.n_pad = n_pad;
    a.members = member_words != nullptr ? ctx->d_fe_row.ptr : nullptr;
    a.reserved = ctx->d_fe_reserved.ptr;
    a.part = ctx->d_fe_part.ptr;
    a.part_cnt = ctx->d_fe_cnt.ptr;
    const uint64_t* const d_in = ctx->d_fe_in.ptr;
    GF_HIP(ctx, gangfit::launch_filter_efficiency(reserves_executors(algo), a, rec.k, reinterpret_cast<const gf_app*>(d_in),
                                                  reinterpret_cast<const gf_result*>(d_in + kAppWords),
                                                  reinterpret_cast<const uint32_t*>(d_in + kAppWords + kResWords),
                                                  ctx->d_fe_reserved.ptr, ctx->d_fe_out.ptr, st));
    GF_HIP(ctx, hipMemcpyAsync(ctx->h_fe_out.ptr, ctx->d_fe_out.ptr, sizeof(gangfit::FilterEffOut), hipMemcpyDeviceToHost, st));
    GF_HIP(ctx, gf_wait_stream(st));
    ctx->fe_reserved_clean = true;
    const gangfit::FilterEffOut& o = *ctx->h_fe_out.ptr;
    out->cpu = o.avg[0];
    out->memory = o.avg[1];
    out->gpu = o.avg[2];
    out->max = o.avg[3];
    if (counts_out) {
        counts_out[0] = o.counts[0];
        counts_out[1] = o.counts[1];
    }
    return GF_OK;
}

}  // extern "C"
