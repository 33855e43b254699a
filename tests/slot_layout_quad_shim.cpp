// slot_layout_quad_shim.cpp — what tests/test_slot_layout_quad_cpu.py loads through ctypes: plan_layout + fill_layout of
// gangfit_slot_layout.h with the record form of the int32 twin (LayoutTables::nquad) asked for, and the three tables the test
// compares copied out.  Host code only (g++ -std=c++17 -I include -I k8s-spark-scheduler_amd/csrc).
#include <cstring>
#include <vector>

#include "gangfit_slot_layout.h"

using namespace gfapi;

extern "C" {

// avail: cpu | mem | gpu columns.  ntable: 3 * n_slots, index: n_slots (slot_node), nquad: 4 * n_slots + guard words the fill must
// leave alone, each of capacity cap_slots slots.  Returns n_slots, or -1 when the plan is refused or a buffer is too small;
// *narrow_ok says whether the twin exists.  guard: words behind nquad's 4 * n_slots that must still hold `guard_value`.
int slq_fill(uint32_t n_nodes, const int64_t* const avail[3], const uint32_t* driver_order, uint32_t n_d, const uint32_t* exec_order,
             uint32_t n_x, int force_general_layout, uint32_t cap_slots, int32_t* ntable, uint32_t* index, int32_t* nquad, uint32_t guard,
             int32_t guard_value, int* narrow_ok, uint64_t* nquad_size) {
    LayoutInput in;
    in.n_nodes = n_nodes;
    for (int j = 0; j < 3; ++j) in.avail[j] = avail[j];
    in.driver_order = driver_order;
    in.n_d = n_d;
    in.exec_order = exec_order;
    in.n_x = n_x;
    in.force_general_layout = force_general_layout != 0;
    LayoutPlan p = plan_layout(in);
    if (p.code != GF_OK || p.facts.n_slots > cap_slots) return -1;
    const LayoutSizes& z = p.sizes;
    *nquad_size = z.nquad;
    std::vector<int64_t> table(z.table + 1), cmax(z.cmax + 1), gtab(z.gtab + 1), sched(z.sched + 1);
    std::vector<uint32_t> idx(z.index + 1), gidx(z.gidx + 1), zspan(z.zspan + 1);
    std::vector<uint64_t> masks(z.masks + 1), gmask(z.gmask + 1), zmasks(z.zmasks + 1);
    std::vector<int32_t> nt(z.ntable + 1), nq(z.nquad + guard, guard_value);
    LayoutTables t;
    t.table = table.data();
    t.index = idx.data();
    t.masks = masks.data();
    t.cmax = cmax.data();
    t.ntable = nt.data();
    t.nquad = nq.data();
    t.gtab = gtab.data();
    t.gidx = gidx.data();
    t.gmask = gmask.data();
    t.sched = sched.data();
    t.zmasks = zmasks.data();
    t.zspan = zspan.data();
    fill_layout(in, p, t);
    const size_t S = p.facts.n_slots;
    std::memcpy(ntable, nt.data(), 3 * S * sizeof(int32_t));
    std::memcpy(index, idx.data(), S * sizeof(uint32_t));
    std::memcpy(nquad, nq.data(), (z.nquad + guard) * sizeof(int32_t));
    *narrow_ok = p.facts.narrow_ok ? 1 : 0;
    return (int)S;
}

}  // extern "C"
