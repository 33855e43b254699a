// slot_layout_shim.cpp — what tests/test_slot_layout_cpu.py loads through ctypes: the two steps of gangfit_slot_layout.h behind a C
// interface, and the facts copied out.  Host code only (g++ -std=c++17 -I include -I k8s-spark-scheduler_amd/csrc).
#include <cstring>

#include "gangfit_slot_layout.h"

using namespace gfapi;

namespace {
struct Handle {
    LayoutInput in;
    LayoutPlan plan;
};
}  // namespace

extern "C" {

struct sl_facts {
    uint32_t n_slots, n_x, n_d, n_chunks, merged, identity, narrow_ok, n_g, n_gpad, n_zones, zstride, zd_row0, zspan_ok, host_stale;
    uint32_t n_node_slot, n_g_prefix;
    int64_t unit[3], nmax[3];
};

// cols: avail cpu | mem | gpu | sched cpu | mem | gpu (the last three NULL: no schedulable columns).  sizes: the eleven element
// counts in the order of LayoutSizes.  Returns the plan's code; the handle is NULL after a refusal.
int sl_plan(uint32_t n_nodes, const int64_t* const cols[6], const uint32_t* zone, const uint32_t* driver_order, uint32_t n_d,
            const uint32_t* exec_order, uint32_t n_x, int force_general_layout, int sparse_gpu, void** handle, char* error,
            size_t error_cap, uint64_t sizes[11]) {
    Handle* h = new Handle;
    h->in.n_nodes = n_nodes;
    for (int j = 0; j < 3; ++j) {
        h->in.avail[j] = cols[j];
        h->in.sched[j] = cols[3 + j];
    }
    h->in.zone = zone;
    h->in.driver_order = driver_order;
    h->in.n_d = n_d;
    h->in.exec_order = exec_order;
    h->in.n_x = n_x;
    h->in.force_general_layout = force_general_layout != 0;
    h->in.sparse_gpu = sparse_gpu != 0;
    h->plan = plan_layout(h->in);
    const int code = h->plan.code;
    std::snprintf(error, error_cap, "%s", h->plan.error.c_str());
    if (code != GF_OK) {
        delete h;
        *handle = nullptr;
        return code;
    }
    const LayoutSizes& z = h->plan.sizes;
    const size_t all[11] = {z.table, z.index, z.masks, z.cmax, z.ntable, z.gtab, z.gidx, z.gmask, z.sched, z.zmasks, z.zspan};
    for (int i = 0; i < 11; ++i) sizes[i] = all[i];
    *handle = h;
    return code;
}

// tables: eleven buffers of at least sizes[i] elements, in the same order.
void sl_fill(void* handle, void* const tables[11], sl_facts* out) {
    Handle* h = static_cast<Handle*>(handle);
    LayoutTables t;
    t.table = static_cast<int64_t*>(tables[0]);
    t.index = static_cast<uint32_t*>(tables[1]);
    t.masks = static_cast<uint64_t*>(tables[2]);
    t.cmax = static_cast<int64_t*>(tables[3]);
    t.ntable = static_cast<int32_t*>(tables[4]);
    t.gtab = static_cast<int64_t*>(tables[5]);
    t.gidx = static_cast<uint32_t*>(tables[6]);
    t.gmask = static_cast<uint64_t*>(tables[7]);
    t.sched = static_cast<int64_t*>(tables[8]);
    t.zmasks = static_cast<uint64_t*>(tables[9]);
    t.zspan = static_cast<uint32_t*>(tables[10]);
    fill_layout(h->in, h->plan, t);
    const LayoutFacts& f = h->plan.facts;
    *out = sl_facts{f.n_slots, f.n_x,     f.n_d,     f.n_chunks, f.merged,   f.identity, f.narrow_ok,  f.n_g,
                    f.n_gpad,  f.n_zones, f.zstride, f.zd_row0,  f.zspan_ok, f.host_stale, (uint32_t)f.node_slot.size(),
                    (uint32_t)f.g_prefix.size(), {f.unit[0], f.unit[1], f.unit[2]}, {f.nmax[0], f.nmax[1], f.nmax[2]}};
}

// node_slot / g_prefix of the facts, into buffers of n_node_slot / n_g_prefix words.
void sl_vectors(void* handle, uint32_t* node_slot, uint32_t* g_prefix) {
    const LayoutFacts& f = static_cast<Handle*>(handle)->plan.facts;
    if (!f.node_slot.empty()) std::memcpy(node_slot, f.node_slot.data(), f.node_slot.size() * sizeof(uint32_t));
    if (!f.g_prefix.empty()) std::memcpy(g_prefix, f.g_prefix.data(), f.g_prefix.size() * sizeof(uint32_t));
}

void sl_free(void* handle) { delete static_cast<Handle*>(handle); }

}  // extern "C"
