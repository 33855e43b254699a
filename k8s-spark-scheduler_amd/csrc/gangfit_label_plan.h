// gangfit_label_plan.h — what gf_snapshot_build* does with the label ranks of a request (driver-prioritized-node-label /
// executor-prioritized-node-label, internal/sort/nodesorting.go:161-199) as pure host code: no HIP, no context.  plan_labels scans
// the caller's rank arrays once and decides
//   - which arrays matter: an array that is NULL, empty or holds one value everywhere (every node ranked alike, or none ranked)
//     re-sorts nothing — the stable sort leaves its list as it is — and counts as absent;
//   - which array is L, the key of the priority sort's label group (priority_sort_kernel): the driver array when it matters,
//     else the executor array.  The sort then returns C = all nodes, stably by L on top of the priority order;
//   - the key of that group: a ranked value is its own key, "not ranked" (UINT32_MAX: behind every ranked node) is the largest
//     ranked value + 1; the field is bits_of(that) wide, sorted eight bits per pass (one pass for any real configuration);
//   - whether the device builds the slot tables at all (option "snapshot_finalize_host" = 0).
// The device route stands when both lists are still subsequences of C; the merge check (LabelMerge, gangfit_device.h) decides that
// on the device.  It is a SUFFICIENT condition: two lists may fit one slot order that this construction does not find; they are
// then installed through the host route like lists that conflict, with the same result.
#pragma once
#include <cstdint>

namespace gfapi {

constexpr uint32_t kLabelUnranked = 0xFFFFFFFFu;

struct LabelPlan {
    bool device_route = false;  // the slot tables are built on the device (a failed merge check still falls back to the host)
    bool driver_active = false, exec_active = false;  // the array re-sorts something: it is uploaded, and the merge check reads it
    int which = 0;              // L: 0 = no label group, 1 = the driver array, 2 = the executor array
    uint32_t max_rank = 0;      // largest ranked value of L (0 when none is ranked)
    uint32_t width = 0;         // bits of max_rank + 1, the key of "not ranked"; 0 = no label group
    uint32_t passes = 0;        // 8-bit passes of the group: (width + 7) / 8
};

struct LabelScan {
    bool uniform = true;    // no two entries differ (also: no entries)
    uint32_t max_rank = 0;  // largest entry that is not kLabelUnranked
};

inline LabelScan scan_label_ranks(uint32_t n, const uint32_t* rank) {
    LabelScan s;
    if (rank == nullptr) return s;
    for (uint32_t i = 0; i < n; ++i) {
        if (rank[i] != rank[0]) s.uniform = false;
        if (rank[i] != kLabelUnranked && rank[i] > s.max_rank) s.max_rank = rank[i];
    }
    return s;
}

inline uint32_t label_bits_of(uint64_t v) {
    uint32_t b = 0;
    while (v) {
        ++b;
        v >>= 1;
    }
    return b;
}

inline LabelPlan plan_labels(uint32_t n_nodes, const uint32_t* driver_label_rank, const uint32_t* exec_label_rank,
                             bool finalize_on_device) {
    LabelPlan p;
    p.device_route = finalize_on_device;
    const LabelScan d = scan_label_ranks(n_nodes, driver_label_rank), x = scan_label_ranks(n_nodes, exec_label_rank);
    p.driver_active = !d.uniform;
    p.exec_active = !x.uniform;
    p.which = p.driver_active ? 1 : (p.exec_active ? 2 : 0);
    if (p.which != 0) {
        p.max_rank = p.which == 1 ? d.max_rank : x.max_rank;
        p.width = label_bits_of((uint64_t)p.max_rank + 1u);
        p.passes = (p.width + 7u) / 8u;
    }
    return p;
}

}  // namespace gfapi
