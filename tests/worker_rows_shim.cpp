// worker_rows_shim.cpp — test shim for tests/test_worker_rows_cpu.py: the row arithmetic of the resident worker
// (csrc/gangfit_worker_rows.h) behind a C interface.  Host code only (g++ -std=c++17 -I k8s-spark-scheduler_amd/csrc).
#include "gangfit_worker_rows.h"

using namespace gangfit::rows;

extern "C" {

void wrow_consts(uint32_t out[4]) {
    out[0] = kRowLen;
    out[1] = kRows;
    out[2] = kRowSightings;
    out[3] = (uint32_t)kCapClamp;
}

// The row of one shape from the capacities of the executor order (caps[j]: capacity of slot j without any driver, already
// clamped): the first kRowLen slots with capacity >= 1, by the definition (NOT the kernel's build).  Returns the count.
uint32_t wrow_build(uint32_t n_x, const int32_t* caps, const uint32_t* slot_node, uint32_t* slot, uint32_t* node, int32_t* cap) {
    uint32_t fill = 0;
    for (uint32_t j = 0; j < n_x && fill < kRowLen; ++j) {
        if (caps[j] < 1) continue;
        slot[fill] = j;
        node[fill] = slot_node[j];
        cap[fill] = caps[j] < kCapClamp ? caps[j] : kCapClamp;
        ++fill;
    }
    return fill;
}

int wrow_decide(const uint32_t* slot, const uint32_t* node, const int32_t* cap, uint32_t count, uint32_t ds, int32_t c_ds, int32_t k,
                uint32_t* out) {
    return decide(slot, node, cap, count, ds, c_ds, k, out) ? 1 : 0;
}

// One directory word through a sequence of events (0 = a claim attempt, 1 = a sighting, 2 = the builder publishes): what a
// wavefront does is decided by the pure predicates alone.  builders / ready_at: how many sightings were told to build, and the
// event index at which the word became READY (-1: never).
void wrow_directory_walk(uint32_t n_events, const uint8_t* events, uint32_t* word_out, uint32_t* builders, int32_t* ready_at) {
    uint32_t w = kEmpty;
    *builders = 0;
    *ready_at = -1;
    for (uint32_t i = 0; i < n_events; ++i) {
        if (events[i] == 0) {
            if (w == kEmpty) w = kFirstSighting;  // (claim + key + publish: CLAIMED is never seen by this single walker)
        } else if (events[i] == 1) {
            if (dir_has_key(w) && !dir_ready(w) && dir_counting(w)) {
                const uint32_t old = w;
                w += 1u;
                if (dir_sighting_builds(old)) ++*builders;
            }
        } else if (!dir_ready(w) && dir_has_key(w) && !dir_counting(w)) {
            w |= kReadyBit;
            *ready_at = (int32_t)i;
        }
    }
    *word_out = w;
}

}  // extern "C"
