// gangfit_worker_rows.h — the shape rows of the resident worker (gangfit_worker.inc, tightly-pack instance) as pure functions: no
// HIP, no context, the same code for the kernel and for a CPU test (tests/worker_rows_shim.cpp).
//
// A tightly-pack placement is the sequence of (node, capacity) runs over the executor order, cut at K, and
// the capacity cap(n, 0) of a node for an executor request does not depend on the application.  So per executor SHAPE (the scaled
// request, three int32 words) the first kRowLen slots of the executor order with capacity >= 1, their node ids and their
// capacities form a ROW, and an application of that shape is decided from the row alone whenever the row covers its K.
//
// Why the row decision equals the scan (wave_tight_scan_compact with the driver reserved on slot ds):
//   * every slot outside the row has capacity 0 for this shape or lies behind the row's last entry; a slot of capacity 0
//     contributes nothing to the scan, with or without the driver's reservation (a reservation only lowers a capacity);
//   * the scan takes slots in slot order and stops where the running total reaches K; the row keeps slot order;
//   * the row's capacities are clamped at GF_MAX_K >= K, and min(min(c, GF_MAX_K), room) == min(c, room) for every room <= K: the
//     clamp does not change a cut at K;
//   * the driver's reservation lowers exactly one slot's capacity, ds's: the entry whose slot is ds takes c_ds = cap(ds, drv)
//     (possibly 0: the entry then emits nothing), every other entry is what the scan computes.
//   So when the corrected row total reaches K, the scan would have reached K inside the row's span and the runs are the scan's.
//   When it does not, the row says nothing (NOT SERVED): the gang may still fit behind the row, or with another driver, and the
//   caller decides the application as it did before rows existed.
//
// The rows live in LDS: per workgroup and per launch by design.  The worker leaves before every install of a snapshot, LDS dies
// with the launch, so a row can never outlive the snapshot it was cut from.  Nothing here waits: a row that is not READY is
// "not there".
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GF_ROWS_FN __host__ __device__ inline
#else
#define GF_ROWS_FN inline
#endif

namespace gangfit {
namespace rows {

constexpr uint32_t kRowLen = 64;       // entries of a row = lanes of a wavefront
constexpr uint32_t kRows = 40;         // rows (and directory entries) per workgroup; no eviction: further shapes are never cached
// Sightings of a shape in a workgroup before its row is built (the claim of the directory entry is the first).  Chosen by
// measurement among 4, 8 and 16 (profiles/r11a_worker_rows_summary.md): at 2 000 tickets of the headline queue the medians were
// 1 391.9, 1 379.2 and 1 356.1 M decisions/s against the parent's 1 077.1 — every workgroup has to see every shape this often before
// it is served from a row, so the smallest wins; a window of twenty tickets is the same for all three, because a bounded launch of
// fewer than kRowSightings rounds per set does not look rows up at all (gangfit_worker.inc, rows_live).  Smaller values were not
// measured: a build costs several decisions, and a shape seen once or twice in a launch must not pay it.
constexpr uint32_t kRowSightings = 4;
constexpr int32_t kCapClamp = 1 << 20; // GF_MAX_K (static_assert in gangfit_worker.inc)

// The key of a row is the scaled executor request, three int32 words, compared for equality on all three.  The directory is probed
// by all its entries at once — lane l compares entry l — so there is no hash and no probing order.

// ---- directory word: EMPTY -> CLAIMED (the key is being written) -> COUNTING(sightings) -> BUILDING -> READY.
//   0                      EMPTY
//   1                      CLAIMED: one wavefront owns the entry and writes its key; nobody else reads the key yet
//   2 .. kRowSightings     COUNTING, sightings = word - 1
//   > kRowSightings        BUILDING: the wavefront whose sighting made the word kRowSightings + 1 builds the row; later sightings
//                          only add to the low bits (harmless: nobody reads a count any more)
//   bit 31                 READY (set by an atomic OR behind the row's last word, release; the low bits are whatever they were)
constexpr uint32_t kEmpty = 0u, kClaimed = 1u, kFirstSighting = 2u, kReadyBit = 0x80000000u;
GF_ROWS_FN bool dir_ready(uint32_t w) { return (w & kReadyBit) != 0u; }
GF_ROWS_FN bool dir_has_key(uint32_t w) { return w >= kFirstSighting; }                    // COUNTING, BUILDING or READY
GF_ROWS_FN bool dir_counting(uint32_t w) { return w >= kFirstSighting && w <= kRowSightings; }
// a sighting is `fetch_add(word, 1)`; `old` is what it returned.  True for exactly one wavefront per entry: the builder.
GF_ROWS_FN bool dir_sighting_builds(uint32_t old) { return old == kRowSightings; }

// ---- the capacity an entry is good for once the driver sits on slot ds with capacity c_ds left for this shape
GF_ROWS_FN int32_t entry_cap(uint32_t slot, int32_t cap, uint32_t ds, int32_t c_ds) { return slot == ds ? c_ds : cap; }
// served <=> the corrected total reaches K (K >= 1: the caller handles K == 0 on its old path)
GF_ROWS_FN bool served(int64_t total, int32_t k) { return k >= 1 && total >= (int64_t)k; }
// the run of an entry: `before` = corrected capacities of the entries in front of it
GF_ROWS_FN int32_t run_of(int64_t before, int32_t cap, int32_t k) {
    const int64_t room = (int64_t)k - before;
    return room <= 0 ? 0 : (room < (int64_t)cap ? (int32_t)room : cap);
}

// ---- the whole row decision over the n entries of a row, sequentially: the model tests/test_worker_rows_cpu.py holds against the
// oracle (the kernel applies the same three rules — entry_cap, served, run_of — with one wave scan).  Writes the placement (node
// ids, K of them) only when served.
GF_ROWS_FN bool decide(const uint32_t* slot, const uint32_t* node, const int32_t* cap, uint32_t n, uint32_t ds, int32_t c_ds,
                       int32_t k, uint32_t* out) {
    int64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += entry_cap(slot[i], cap[i], ds, c_ds);
    if (!served(total, k)) return false;
    int64_t before = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const int32_t c = entry_cap(slot[i], cap[i], ds, c_ds);
        const int32_t t = run_of(before, c, k);
        for (int32_t j = 0; j < t; ++j) out[before + j] = node[i];
        before += c;
    }
    return true;
}

}  // namespace rows
}  // namespace gangfit
