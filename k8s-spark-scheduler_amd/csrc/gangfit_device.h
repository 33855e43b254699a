// gangfit_device.h — shared declarations between the HIP kernels (gangfit_kernels.hip) and the C-ABI host
// layer (gangfit_api*.cpp, gangfit_ctx.h).  gfx950 / CDNA4 only: wave64, no compatibility paths.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <optional>

#include "gangfit.h"
#include "gangfit_worker_rounds.h"
#include "gangfit_worker_rows.h"

namespace gangfit {

// The node table as the kernels see it, in "slot" space.  SoA, int64, one array per dimension; a wave scanning slots
// b..b+63 issues three coalesced 512-byte loads.  Two layouts (gf_orders_set picks one):
//   merged  — driverNodePriorityOrder and executorNodePriorityOrder are subsequences of one common order (they both
//             derive from getNodeNamesInPriorityOrder, internal/sort/nodesorting.go:41-64, so this is the production
//             shape): slots [0, n_x) are that common order, n_d == n_x, driver position == slot (d_identity), and the
//             per-chunk bit masks say which slots are driver / executor candidates.
//   general — the two orders disagree (different label-priority re-sorts for drivers and executors): slots [0, n_x)
//             are the executor order, driver-only nodes follow, dslot[] maps driver positions to slots.
// The last slot is a sentinel (available = -2^62) that unknown node names map to.
struct NodeTable {
    int64_t* cpu;  // milli-cores   [n_slots]
    int64_t* mem;  // bytes         [n_slots]
    int64_t* gpu;  // devices       [n_slots]
    const uint32_t* slot_node;  // [n_slots] slot -> caller's node index (what is written to exec_nodes)
    const uint32_t* dslot;      // [n_d]     position in driverNodePriorityOrder -> slot (general layout only)
    const uint32_t* node_slot;  // [n_nodes] caller's node index -> slot
    // Chunk-maxima index: cmax[d * n_chunks + c] = max over slots [64c, 64c+64) of dimension d, taken on the SNAPSHOT.
    // Upper bounds stay valid while a FIFO chain subtracts, so "cmax < request in some dimension" proves that no slot
    // of the chunk can host the request: the scans skip such chunks without loading them.  The reference's priority
    // order (least free memory first) makes this skip the whole front of the order for large executors.
    const int64_t* cmax;        // [3][n_chunks]
    const uint64_t* xmask;      // [n_chunks] bit l of xmask[c]: slot 64c+l is an executor candidate
    const uint64_t* dmask;      // [n_chunks] bit l of dmask[c]: slot 64c+l is a driver candidate (merged layout)
    uint32_t n_chunks;          // ceil(n_slots / 64)
    uint32_t n_x;               // slots scanned by the executor packers
    uint32_t n_d;               // driver candidates (positions)
    uint32_t n_slots;
    uint32_t n_nodes;
    uint32_t d_identity;        // 1: driver position == slot (merged layout)
    // The SNAPSHOT in the scaled int32 domain (value = scaled value * nunit[dimension], |scaled value| < 2^30), slot order; nullptr
    // when the snapshot has no such form.  Read by the minimal-fragmentation independent batch (gangfit_minfrag.inc), whose every
    // pass evaluates every candidate slot: a capacity there is a multiply-high instead of a 64-bit quotient.
    const int32_t* ncpu = nullptr;
    const int32_t* nmem = nullptr;
    const int32_t* ngpu = nullptr;
    int64_t nunit[3] = {1, 1, 1};
    // The same twin once more as ONE 16-byte record per slot, {ncpu[s], nmem[s], ngpu[s], slot_node[s]}, 16-byte aligned: what the
    // resident worker's tightly-pack decisions read (NarrowView, gangfit_kernels.hip) — a slot's values and its node id are always
    // wanted together there, and one address and one load bring them.  Exists exactly when the columns do.  (The last member:
    // no other MEMBER's offset moves; the arguments behind a NodeTable move by eight bytes in every kernel that takes one, and
    // WorkerKernargs, which embeds it, follows by construction.)
    const int4* nquad = nullptr;
};

// Sparse-dimension view of the executor order for the independent batch (merged layout): the executor candidates that have
// at least one free gpu, in priority order, as a compact table of their own ("sub-slots").  gpu nodes are a minority of a
// cluster, so a gang whose executors need a gpu collects them from a few slots of MANY 64-slot chunks of the full order —
// a chain of dependent round trips that makes it the slowest wavefront of a launch.  Every node left out has capacity 0 for
// such a request (available gpu <= 0 < request), so scanning the compact table instead gives the same placements.
struct SparseTable {
    const int64_t* cpu;  // [n_sub + pad] values of the sub-slots (the padding slots never fit)
    const int64_t* mem;
    const int64_t* gpu;
    const uint32_t* slot_node;    // sub-slot -> caller's node index
    const int64_t* cmax;          // [3][n_chunks] chunk maxima of the compact table
    const uint64_t* xmask;        // [n_chunks] all sub-slots are executor candidates
    const uint32_t* sub_of_slot;  // [n_slots of the full table] slot -> sub-slot, GF_NO_NODE when the slot is not in the view
    uint32_t n_x;                 // sub-slots (0 = no sparse view: the kernel uses the full table)
    uint32_t n_chunks;
    // the zone packers' one-launch kernel (fit_zoned_fused_kernel) packs a zone's gangs of gpu executors from the view too:
    const uint64_t* zmask;        // [n_zones of the evaluation list][n_chunks] the sub-slots whose node lies in the zone
    const uint32_t* slot_of_sub;  // [n_sub + pad] sub-slot -> slot of the full table (its placements are slot ids)
};

// Zone view of the two candidate orders for the single-AZ packers (LIB/binpack/single_az.go:23-72): zone zi of the
// evaluation list keeps only its own nodes of driverNodePriorityOrder / executorNodePriorityOrder, order preserved —
// i.e. the same slot table scanned through per-zone candidate bit masks.  The evaluation list is driverZonesInOrder
// (zones by first appearance in the driver order) restricted to zones that own at least one executor candidate (:36-41).
struct ZoneTable {
    const uint64_t* xmask;  // [n_zones][stride] executor-candidate bits of each zone (indexed like NodeTable::xmask)
    const uint64_t* dmask;  // [n_zones][stride] driver-candidate bits: by slot (merged layout) or by driver position (general)
    uint32_t n_zones;
    uint32_t stride;        // 64-bit words per zone row
};

// Node tables the efficiency kernels read (LIB/binpack/efficiency.go:66-156): AvailableResources and
// SchedulableResources, SoA int64, indexed by slot (hot path) or by the caller's node index (full per-node map).
struct EffTables {
    const int64_t* avail[3];
    const int64_t* sched[3];
};

// Narrow (scaled int32) domain of the FIFO chain — see gangfit_fifo_common.inc.
struct NApp {  // 64 bytes, produced by the chain prologue (prepare_app): requests divided by the table's units
    int32_t drv[3];
    int32_t k;
    int32_t exe[3];  // >= 0
    uint32_t flags;
    uint32_t mag[3];  // division by exe as a multiplication (narrow_magic, gangfit_fifo_common.inc): 2 * ceil(2^(30 + l) / exe), 0 when exe == 0
    uint32_t msh;     // the three post-shifts l = ceil(log2(exe)), 8 bits each
    uint64_t exec_off;
    uint64_t pad;
};
static_assert(sizeof(NApp) == 64, "NApp must be 64 bytes");

// d_dst = d_src * factor[dimension] for the 3 * n_slots table values and the 3 * n_chunks chunk maxima; sentinel values
// (<= INT32_MIN / 2: empty slots) are kept.
hipError_t launch_narrow_rescale(const int32_t* d_src, int32_t* d_dst, uint32_t n_slots, const int32_t* d_cmax_src,
                                 int32_t* d_cmax_dst, uint32_t n_chunks, const int32_t factor[3], hipStream_t stream);

// The floored narrow form (gangfit_floor_units.h): value = q * unit[dimension] + r, q = floor(value / unit), 0 <= r < unit.
struct FloorUnitArgs {
    int64_t unit[3];
    double rcp[3];  // 1 / (double)unit
};
// d_fsnap (3 * n_slots) = q of the wide snapshot d_snap, empty and sentinel slots kNarrowNever; d_fcmax (3 * n_chunks) its chunk
// maxima; d_frem (3 * n_slots) = r, 0 on empty and sentinel slots.  The caller has checked -2^30 < q < 2^30 for every real slot.
hipError_t launch_floor_snapshot(const int64_t* d_snap, const uint32_t* d_slot_node, uint32_t n_slots, uint32_t n_chunks,
                                 const int64_t unit[3], int32_t* d_fsnap, int32_t* d_fcmax, int64_t* d_frem, hipStream_t stream);
// d_work (3 * n_slots, q' * unit as a chain's epilogue leaves it) += d_frem: the true residuals.
hipError_t launch_floor_residual(int64_t* d_work, const int64_t* d_frem, uint32_t n_slots, hipStream_t stream);
// d_out6 = the 3 minima | 3 maxima of d_snap's dimensions over the real slots (INT64_MAX | INT64_MIN without one).
hipError_t launch_table_range(const int64_t* d_snap, const uint32_t* d_slot_node, uint32_t n_slots, int64_t* d_out6, hipStream_t stream);

struct NarrowTable {  // value = scaled value * unit[dimension]
    int32_t* cpu;  // [n_slots] working copy, scaled
    int32_t* mem;
    int32_t* gpu;
    const int32_t* cmax;  // [3][n_chunks] scaled chunk maxima of the snapshot
    int64_t unit[3];
};


// Kernel-visible counters used by tests/bench to report visited bytes honestly (SURVEY.md section 8d
// "early-exit note").  One uint64 pair per launch, accumulated with a single atomic per app.
struct ScanStats {
    unsigned long long exec_slots_visited;    // executor-order slots whose capacity was evaluated
    unsigned long long driver_slots_visited;  // driver-order positions whose fit was evaluated
    unsigned long long fifo_shader_cycles;    // s_memtime delta over the last FIFO chain kernel (shader clock)
    unsigned long long fifo_realtime_ticks;   // s_memrealtime delta over the same span (constant 100 MHz)
    unsigned long long fifo_phase_cycles[6];  // wave-0 shader cycles: stage | driver scan | executor scan | slow path | commit | steps
    // the solo chain's rare endings (gangfit_fifo_solo.inc, instrumented variant only), by return code: [1] a request without
    // a shape id, [2] the capacity bound, [3] no driver candidate, [4] the gang does not fit behind its first driver
    unsigned long long fifo_rare_count[5];
    unsigned long long fifo_rare_cycles[5];   // shader cycles inside solo_rare_app, same index
    unsigned long long fifo_hw_id;            // HW_ID of the chain's controlling wavefront (CU, SE, ...) | XCC_ID << 32
};

// What a feasibility-only launch (gf_fit_feasible) writes instead of result records and counters; d_bytes == nullptr: the full batch.
struct FeasibleOut {
    uint8_t* d_bytes = nullptr;   // n_apps HasCapacity bytes (padded to a multiple of four; device-mapped pinned memory or a device
                                  // buffer), written in whole words by the kernel's collecting workgroup
    uint32_t* d_words = nullptr;  // the collection words: ceil(n_apps / 4) of device memory, zero between launches (cleared by the same)
    bool eff_nonneg = false;      // zone-aware packers: no node's efficiency can be negative (gf_ctx::eff_nonneg)
};
// What every launcher of an independent batch (gangfit_kernels.hip) receives; it reads what it needs and leaves the rest alone.
struct FitBatch {
    NodeTable table{};
    SparseTable gpu_view{};                  // n_x == 0: none
    ZoneTable zones{nullptr, nullptr, 0, 0};  // zone-aware packers (else empty) ...
    const int64_t* d_sched = nullptr;        // ... and SchedulableResources in slot order (3 * n_slots)
    uint32_t n_apps = 0;
    const gf_app* d_apps = nullptr;
    gf_result* d_results = nullptr;
    uint32_t* d_exec_nodes = nullptr;
    uint32_t* d_scratch = nullptr;  // 2 * half uint32 (DistributeEvenly survivor lists)
    uint64_t half = 0;              // the ONE stride of d_scratch, of d_zexec and of the placements (total_k + 1)
    uint32_t* d_zexec = nullptr;    // (n_zones + 1) rows of half uint32: the candidate views' placements as SLOT ids (both zone routes)
    ScanStats* d_stats = nullptr;   // nullable
    FeasibleOut feasible{};
    hipStream_t stream = nullptr;
};
hipError_t launch_fit_independent(gf_algo algo, const FitBatch& batch);

// ---- the resident worker of the independent batch (gangfit_worker.inc; host side: gangfit_api_worker.cpp)
constexpr uint32_t kWorkerRing = 64;  // tickets in flight at most (a power of two: the host waits for ticket t - 64 before it posts t)
constexpr uint32_t kWorkerInline = 16;  // tickets a launch of the worker carries in its arguments (at most one per set)
constexpr int kWorkerWaves = 16;             // wavefronts per workgroup of the worker kernel (one workgroup fills a CU)
constexpr uint32_t kWorkerCountStride = 64;  // words between two tickets' counters: one 256-byte line (one memory channel) each

// A ticket: six self-validating 8-byte words.  word[0] = ticket number + 1; words 1..5 carry worker_tag(ticket) in their
// top sixteen bits (device and pinned-host addresses, the placement count and n_apps | flags << 32 all stay below 2^48): a
// reader that finds the right tag in every word has the whole ticket without any ordering between the words.
struct WorkerTicket {  // 64 bytes
    unsigned long long word[8];  // [0] seq, [1] apps, [2] results, [3] exec_nodes, [4] exec_len, [5] n_apps | flags << 32
};
static_assert(sizeof(WorkerTicket) == 64, "one cache line per ticket");
__host__ __device__ inline unsigned long long worker_tag(unsigned long long ticket) { return ((ticket + 1ull) & 0x7FFFull) | 0x8000ull; }

struct WorkerHostCtl {  // pinned host memory, device-mapped
    unsigned long long posted;  // host -> device: tickets posted so far (the doorbell)
    unsigned long long stop;    // host -> device: 1 = leave now; N + 2 = leave once ticket N - 1 has been relayed (N tickets in all)
    unsigned long long pad0[6];
    unsigned long long consumed;  // device -> host: tickets the leader has relayed (valid once state == 2)
    unsigned long long state;     // device -> host: 1 = the leader runs, 2 = it has left
    unsigned long long pad1[6];
    unsigned long long done[kWorkerRing];  // device -> host: done[t % ring] = t + 1 when ticket t is complete
    WorkerTicket ring[kWorkerRing];        // host -> device
};

struct WorkerDevCtl {  // fine-grained device memory
    unsigned long long quit;  // = generation of the launch whose leader has left (never reset: the next launch has another one)
    // shape rows of the tightly-pack instance (gangfit_worker_rows.h): rows built, decisions served from a row, decisions that
    // looked a row up and fell back — every workgroup adds its LDS counts once, when it leaves (gf_worker_row_stats)
    unsigned long long rows[3];
    unsigned long long pad0[4];
    uint32_t count[kWorkerRing * kWorkerCountStride];  // [slot * stride]: applications of the slot's ticket finished so far
    WorkerTicket ring[kWorkerRing];
};

struct WorkerArgs {
    WorkerHostCtl* host;
    WorkerDevCtl* dev;
    unsigned long long generation;    // of this launch (1, 2, ...): the value the leader writes into the quit word when it leaves
    unsigned long long first_ticket;  // tickets below this one were served by an earlier launch
    unsigned long long idle_ticks;    // the leader leaves after this long without a new ticket (100 MHz)
    unsigned long long leave_after;   // != 0: nothing behind ticket leave_after - 1 will be posted to this launch (GF_WORKER_LEAVE_AFTER)
    uint32_t* scratch;                // [kWorkerRing][3 * scratch_stride]: private placements, two survivor lists
    unsigned long long scratch_stride;
    uint32_t sets;
    uint32_t blocks_per_set;
    ScanStats* stats;  // nullable: slots visited, summed over every decision of the launch (gf_scan_stats)
    // The first tickets of the launch travel with it: tickets first_ticket .. first_ticket + n_inline - 1 as their six tagged
    // words, exactly as in the ring.  A set finds its first ticket in the kernel's argument segment — which every wavefront
    // reads at its start anyway — instead of waiting for the leader's look at the doorbell and its relay over the host link
    // (two round trips, ~4 us of a 60 us window of twenty tickets).  The leader relays them all the same (the ring is what
    // later rounds and the completion accounting index).
    uint32_t n_inline;
    uint32_t stride_mul;  // rounds::make_stride_div(blocks_per_set).mul: the launch's quotient by app_stride (gangfit_worker_rounds.h)
    unsigned long long inline_words[kWorkerInline][6];
    // The zone-aware tightly-pack instances only (single-az-tightly-pack, az-aware-tightly-pack; behind everything the plain
    // instances read, whose argument offsets stay where they were): the zone rows of the evaluation list — at most 64 candidate
    // views, the plain order of az-aware included — and SchedulableResources in slot order (3 * n_slots), for the averages.
    ZoneTable zones;
    const int64_t* sched;
    uint32_t stride_shift;  // ... and its shift (behind everything else: no earlier argument moves)
    uint32_t pad_stride;
};

// The argument segment of fit_worker_kernel(NodeTable, SparseTable, WorkerArgs) as the kernel itself reads it back: the three
// arguments lie in it one behind the other (each is a multiple of eight bytes, aligned to eight), so a pointer to the segment
// is a pointer to this record.  The tightly-pack worker reads operands that its narrow decision seldom touches from here, with
// scalar loads at the point of use (gangfit_worker.inc, OPERANDS), instead of holding them in registers across its round loop.
struct WorkerKernargs {
    NodeTable T;
    SparseTable G;
    WorkerArgs W;
};
static_assert(sizeof(NodeTable) % 8 == 0 && sizeof(SparseTable) % 8 == 0 && sizeof(WorkerArgs) % 8 == 0 && alignof(NodeTable) == 8 &&
                  alignof(SparseTable) == 8 && alignof(WorkerArgs) == 8 &&
                  sizeof(WorkerKernargs) == sizeof(NodeTable) + sizeof(SparseTable) + sizeof(WorkerArgs),
              "WorkerKernargs must mirror the kernel's argument segment");

// tightly-pack, distribute-evenly, minimal-fragmentation, single-az-tightly-pack, az-aware-tightly-pack
hipError_t worker_blocks_per_cu(gf_algo algo, int* out);
// One launch: 1 + sets * blocks_per_set workgroups of sixteen wavefronts.
hipError_t launch_fit_worker(gf_algo algo, const NodeTable& table, const SparseTable& gpu_view, const WorkerArgs& args,
                             hipStream_t stream);

// FIFO chain (fitEarlierDrivers + final pack) of the plain packers.  One workgroup walks the chain; two kernels:
//   solo (gangfit_fifo_solo.inc) — merged layout, scaled int32 table in LDS, ONE wavefront walking the chain: the fast
//                                  path; when a request of the batch has no scaled form it returns at once
//   v2   (gangfit_kernels.hip)   — any layout, wide (int64) table: the fallback (guarded the other way when both run)
// followed by expand_translate_kernel (run heads -> placement list, slot ids -> node indices).
struct FifoPlan {
    bool narrow;                // launch the solo kernel (merged layout and the table has a narrow form)
    bool wide;                  // launch the wide kernel (alone, or guarded by *d_wide_needed behind the solo kernel)
    uint32_t lds_slots_v2;      // table slots each kernel keeps in LDS
    uint32_t lds_slots_solo;
};
// Checkpoints of a chain (incremental Filter chains, gf_fit_batch): before it stages the application with ABSOLUTE index
// i << shift (i >= 1) the solo kernel dumps its narrow working table (3 * n_slots int32, the layout of NarrowTable) to
// base + (i - 1) * 3 * n_slots.  a_base = absolute index of the first application of this launch (a resumed chain is
// launched on the tail of the queue with the restored table); base == nullptr: no checkpoints.
struct ChainCkpt {
    int32_t* base;
    uint32_t a_base;
    uint32_t shift;
    size_t stride;                          // int32 words between two checkpoints (>= 3 * n_slots; chain_ckpt_stride)
    const unsigned long long* resume_mask;  // solo kernel with a global table tail: the cumulative dirty-chunk mask of the
                                            // checkpoint this launch resumes from (nullptr: from the snapshot)
    // The TIP (LDS chain kernels with the whole table in LDS; nullptr: none): when the chain ends — at the application it aborts at, else at
    // the driver being filtered, behind which nothing is committed — the table it holds is the table BEFORE that application.
    // The epilogue leaves it here (3 * n_slots int32, the layout of a checkpoint), and the next Filter of a queue that agrees with
    // this one up to there resumes from it: the Filter of driver j + 1 evaluates drivers j and j + 1 instead of everything since
    // the last multiple of 2^shift (gangfit_api_fit.cpp, chain_plan).
    int32_t* tip;
};
// Checkpoint layout: cpu | mem | gpu (n_slots int32 each), then — 8-byte aligned — two masks of one bit per 64-slot chunk:
//   cumulative  the chunk differs from the snapshot at this checkpoint,
//   delta       the chunk was touched by a commit since the PREVIOUS checkpoint of the chain.
// Written by the solo kernel when the table has a global tail (the DELTA format): only the delta chunks are dumped — a dump
// costs what the last 2^shift applications touched, not what the chain has touched so far — and a chain that resumes from
// checkpoint i starts from the snapshot with, for every chunk of cumulative(i), the copy in the LATEST checkpoint j <= i whose
// delta names it (chain_prologue_kernel).  Kernels that dump whole tables leave the masks unused.
inline size_t chain_ckpt_mask_words(uint32_t n_chunks) { return 2 * (size_t)((n_chunks + 63u) / 64u); }  // uint32 words of ONE mask
inline size_t chain_ckpt_stride(uint32_t n_slots, uint32_t n_chunks) {
    return 3 * (size_t)n_slots + (n_slots & 1u) + 2 * chain_ckpt_mask_words(n_chunks);
}
// What a chain launcher folds into its first and its last kernel, so that a Filter's chain is three launches instead of
// nine runtime calls (each costs ~7 us of host time alone, several times that when eight threads enqueue eight chains):
//   first kernel (chain_prologue_kernel) — reads the app records from wherever the caller has them (device-mapped pinned
//       host memory, or the device), writes the device copy and the scaled records, presets the run-head slice, copies up
//       to two tables (working table <- snapshot / checkpoint) and lays the dirty chunks of a checkpoint over the first;
//   last kernel (the translate / expand step) — also writes the final results, placements and the abort index to
//       device-mapped host buffers (posted writes, visible when the kernel has completed).
// Everything is optional; a default-constructed ChainIo means "records are in d_apps, nothing to copy, no host outputs".
struct ChainIo {
    const gf_app* apps_src = nullptr;  // device-visible source of the n_apps records (nullptr: d_apps holds them already)
    const uint32_t* copy_src[2] = {nullptr, nullptr};
    uint32_t* copy_dst[2] = {nullptr, nullptr};
    size_t copy_words[2] = {0, 0};
    const int32_t* overlay = nullptr;  // checkpoint 1 of a series in the delta format (chain_ckpt_stride): checkpoints
                                       // 1 .. overlay_count are laid over overlay_dst after the copies, the latest delta of a
                                       // chunk winning
    size_t overlay_stride = 0;         // int32 words between two checkpoints
    uint32_t overlay_count = 0;        // the checkpoint the chain resumes from (1-based)
    int32_t* overlay_dst = nullptr;
    uint32_t overlay_slots = 0, overlay_chunks = 0;
    int32_t* wide_clear = nullptr;     // the flag word the NEXT chain will use (zeroed here: the words alternate)
    gf_result* h_results = nullptr;    // [n_apps] of this launch
    uint32_t* h_exec = nullptr;        // indexed by the records' absolute exec_off
    int32_t* h_failed = nullptr;
};
// What every chain launcher receives: the records of ONE launch — the tail of the queue behind ckpt.a_base — and where its
// answers go (exec_off is absolute: d_exec_nodes, d_scratch and d_zexec are those of the whole queue).
struct ChainBatch {
    uint32_t n_apps = 0;
    const gf_app* d_apps = nullptr;
    NApp* d_napps = nullptr;           // the scaled records (written by the chain's first kernel; LDS chain kernels)
    int32_t* d_wide_needed = nullptr;  // the flag word of this chain: a request has no scaled form
    gf_result* d_results = nullptr;
    uint32_t* d_exec_nodes = nullptr;
    uint32_t* d_scratch = nullptr;  // 2 * half uint32: run heads / survivor lists (plain and generic chains)
    uint32_t* d_zexec = nullptr;    // rows of half uint32: the candidates' placements as slot ids (generic chain: n_zones + 1
                                    // rows), run-list tails beyond the LDS capacity (zoned and minfrag LDS chains: 2 * 16 rows)
    uint64_t half = 0;
    int32_t* d_chain_failed_at = nullptr;
    ChainCkpt ckpt{};
    ChainIo io;
    ScanStats* d_stats = nullptr;  // nullable
    hipStream_t stream = nullptr;
};
// ... and its tables: the wide working table, its scaled twin (LDS chain kernels), the zones and SchedulableResources in slot
// order (zone-aware packers; else empty / nullptr).
struct ChainTables {
    NodeTable table;
    NarrowTable ntable;
    ZoneTable zones;
    const int64_t* d_sched;
    const int64_t* d_frem = nullptr;  // ntable is the floored narrow form: its remainders, [3][n_slots] (nullptr: the exact form)
};
size_t fifo_v2_lds_bytes(uint32_t lds_slots, uint32_t n_chunks);
size_t fifo_solo_lds_bytes(uint32_t lds_slots, uint32_t n_chunks);
// heads_lo: first entry of d_scratch this launch may write run heads to (the placements of a resumed chain start there)
hipError_t launch_fit_fifo(gf_algo algo, const FifoPlan& plan, const ChainTables& tables, const ChainBatch& batch, uint64_t heads_lo);

// Zone-aware packers on an independent batch: one wave per (app, zone) runs SparkBinPack on the zone's view, one wave
// per decision averages the packing efficiencies of [driver] ++ executors in slice order (chooseBestResult,
// single_az.go:75-97), one wave per app keeps the first zone with the strictly highest average and writes the final
// result.  az_aware: apps without a single-zone fit keep the plain tightly-pack answer already in d_results.
struct ZoneBuffers {
    gf_result* zres;      // [n_apps * n_zones]
    double* zavg;         // [n_apps * n_zones][4]
    uint32_t* cnt;        // [n_cnt_waves][n_slots] zero between launches: per-wave executor multiplicity scratch
    uint32_t n_cnt_waves;
};
hipError_t launch_fit_zoned(int inner_algo, bool az_aware, bool reserve_execs, const EffTables& eff, const ZoneBuffers& buf,
                            const FitBatch& batch);

// The same as ONE launch (fit_zoned_fused_kernel): a workgroup per application, a wavefront per candidate view, the choice
// through LDS, the winner's placements written as node indices to d_exec_nodes / d_results — which may be device-mapped host
// memory.  At most 64 views.
hipError_t launch_fit_zoned_fused(int inner_algo, bool az_aware, const FitBatch& batch);

// FIFO chain of the zone-aware and minimal-fragmentation packers: one workgroup, one wavefront per candidate view of the
// current app (each zone, plus the plain pack for az-aware), working table in global memory.  d_zexec needs (n_zones + 1)
// rows, d_cnt (zoned) at least 16 rows of ZoneBuffers::cnt.  Writes final results / placements as node indices.
struct GenericChain {
    int inner_algo;  // the packer of one candidate view
    bool zoned, az_aware;
    uint32_t* d_cnt;          // nullptr when not zoned
    const int32_t* d_run_if;  // nullable: the kernel returns at once unless the word is set (the twin of an LDS chain)
};
hipError_t launch_fit_fifo_generic(const GenericChain& chain, const ChainTables& tables, const ChainBatch& batch);

// LDS-resident chain for the zone-aware tightly-pack packers on the merged layout with a narrow table
// (gangfit_fifo_zoned.inc).  Returns at once when a request of the batch has no scaled form (*d_wide_needed != 0 after
// its own prepare step): the caller then launches launch_fit_fifo_generic with d_run_if = d_wide_needed.
// n_cand = candidate views = zones (+ 1 for az-aware: the plain pack); the workgroup's size follows from it.
size_t fifo_zoned_lds_bytes(uint32_t lds_slots, uint32_t n_chunks, uint32_t n_zones, uint32_t n_cand, uint32_t n_shapes);
hipError_t launch_fit_fifo_zoned_lds(bool az_aware, uint32_t lds_slots /* table slots kept in LDS */, uint32_t n_shapes /* shape-index rows */,
                                     const ChainTables& tables, const ChainBatch& batch);

// LDS-resident, block-cooperative chain for minimal-fragmentation, plain (zoned = false) or single-AZ
// (gangfit_fifo_minfrag.inc); same contract as launch_fit_fifo_zoned_lds.
struct MinfragLdsChain {
    bool zoned;
    uint32_t lds_slots;  // table slots kept in LDS
    uint32_t n_shapes;   // shape ids per role
    uint32_t n_idx;      // ... of which with chunk-index rows in LDS
    int32_t* d_capmat;   // n_shapes x n_slots, nullable
    int32_t* d_hist;     // fifo_minfrag_hist_words, nullable: no histogram path
};
size_t fifo_minfrag_lds_bytes(uint32_t lds_slots, uint32_t n_chunks, uint32_t n_zones, uint32_t n_shapes);
// int32 words of the capacity histograms (one per candidate view and executor shape; gangfit_fifo_minfrag.inc)
size_t fifo_minfrag_hist_words(uint32_t n_zones, uint32_t n_shapes);
hipError_t launch_fit_fifo_minfrag_lds(const MinfragLdsChain& chain, const ChainTables& tables, const ChainBatch& batch);

// ComputeAvgPackingEfficiency over [driver] ++ executors of n_apps finished results whose placements are NODE indices
// (efficiency.go:114-156); d_avg_out: n_apps x 4 doubles {CPU, Memory, GPU, Max}.
hipError_t launch_avg_efficiency(bool reserve_execs, const NodeTable& table, const EffTables& eff, uint32_t* d_cnt,
                                 uint32_t n_cnt_waves, uint32_t n_apps, const gf_app* d_apps,
                                 const gf_result* d_results, const uint32_t* d_exec_nodes, double* d_avg_out,
                                 hipStream_t stream);

// ComputePackingEfficiencies (efficiency.go:66-103) for ONE result: per-node {cpu, memory, gpu} efficiencies in the
// caller's node-index space (eff tables indexed by node), d_reserved: n_nodes x 3 int64 scratch (zeroed here).
hipError_t launch_node_efficiencies(bool reserve_execs, const EffTables& eff_by_node, uint32_t n_nodes, int32_t k,
                                    const gf_app* d_app, const gf_result* d_result, const uint32_t* d_exec_nodes,
                                    int64_t* d_reserved, double* d_eff_out, hipStream_t stream);

// ComputeAvgPackingEfficiency over one PackingEfficiency per metadata key, for ONE result (gangfit_filter_eff.inc;
// gf_filter_efficiency): the sum is a fixed tree over 64-node chunks, spelled out in that file.
struct FilterEffArgs {
    EffTables tab;              // by node index: the snapshot's available quantities, the schedulable quantities
    const int64_t* work;        // nullable: the chain's working table, cpu | mem | gpu by slot; read where a node owns a slot
    const uint32_t* node_slot;  // ... node -> slot, GF_NO_NODE = none (needed with work)
    uint32_t n_slots;
    uint32_t n_nodes;
    uint32_t n_words;           // ceil(n_nodes / 64): chunks, and words of the member row
    uint32_t n_pad;             // n_words rounded up to a multiple of 64: entries per row of part / part_cnt
    const uint64_t* members;    // nullable: every node is a key
    const int64_t* reserved;    // n_nodes x 3, all-zero outside the result's nodes
    double* part;               // [4][n_pad] chunk partials: cpu | memory | gpu | max
    uint32_t* part_cnt;         // [2][n_pad]: keys | keys with a schedulable gpu
};
struct FilterEffOut {
    double avg[4];       // gf_avg_efficiency
    uint32_t counts[2];  // len, nodesWithGPU
};
inline uint32_t filter_eff_pad(uint32_t n_words) { return (uint32_t)((((uint64_t)n_words + 63u) / 64u) * 64u); }
// d_app / d_result / d_exec_nodes: the one record, its result and its placements (exec_off = 0) on the device.  d_reserved is the
// table args.reserved names: all-zero on entry, all-zero again when the launches have run.
hipError_t launch_filter_efficiency(bool reserve_execs, const FilterEffArgs& args, int32_t k, const gf_app* d_app,
                                    const gf_result* d_result, const uint32_t* d_exec_nodes, int64_t* d_reserved,
                                    FilterEffOut* d_out, hipStream_t stream);

// Node-range sharding of an independent batch (gangfit_shard.inc): a GPU owns one or more ranges
// [c_lo, c_hi) of 64-slot chunks of the merged slot order — one per shard it hosts (one shard per device on a real box; a
// repeated device id, the one-GPU stand-in, makes one device host several: its kernels then run ONE launch per step with a
// grid row per hosted shard, one app upload, one gathered table and one placement buffer per device).
constexpr uint32_t kMaxGroupDevices = 16;
struct ShardRange {
    uint32_t c_lo, c_hi;
    uint32_t shard, n_shards;
    uint32_t g_lo, g_hi;  // the range's sub-slots of the sparse gpu view (SparseTable; g_lo == g_hi: none / no view)
};
struct ShardSet {  // the shards one device hosts (grid row q of a step's launch handles entry q)
    uint32_t n, n_shards;
    uint32_t c_lo[kMaxGroupDevices], c_hi[kMaxGroupDevices], shard[kMaxGroupDevices];
    uint32_t g_lo[kMaxGroupDevices], g_hi[kMaxGroupDevices];
};
inline ShardSet shard_set_of(const ShardRange& r) {
    ShardSet s{};
    s.n = 1;
    s.n_shards = r.n_shards;
    s.c_lo[0] = r.c_lo;
    s.c_hi[0] = r.c_hi;
    s.shard[0] = r.shard;
    s.g_lo[0] = r.g_lo;
    s.g_hi[0] = r.g_hi;
    return s;
}
// Exchanges of the in-process multi-device context: up to 16 peer pointers by value.  The producing kernels write their
// 16-byte records straight into row `shard` of EVERY device's gathered table (posted stores over xGMI; dsts.n == 0: into the
// local array d_out instead, row = grid row — the one-process-per-GPU path and the RCCL exchange gather them afterwards).
struct PeerPtrs {
    void* p[kMaxGroupDevices];
    uint32_t n;
};
// The candidate views of the zone-aware tightly-pack packers on the shard steps (single-az-tightly-pack, az-aware-tightly-pack):
// views [0, n_zones) are the zones of the evaluation list (ZoneTable's masks, the compact gpu table's SparseTable::zmask rows),
// view n_zones — az-aware only — the plain order.  A step runs per (application, view); records are laid out
// [n_shards][n_cand][n_apps], and view c's placement is region c of the placement buffer (c * half words in).
struct ShardZones {
    const uint64_t* xmask;  // [n_zones][stride] executor-candidate bits by slot
    const uint64_t* dmask;  // [n_zones][stride] driver-candidate bits by slot (merged layout)
    const uint32_t* span;   // [n_zones][4]: the 64-slot chunks [lo, hi) of the order that hold the zone's candidates, then the
                            // chunks [lo, hi) of the compact gpu table that hold its sub-slots; nullptr: every zone spans everything
    const int64_t* sched;   // [3][n_slots] SchedulableResources in slot order (the averages chooseBestResult compares)
    uint32_t n_zones, stride;
    uint32_t n_cand;        // n_zones (+ 1 for az-aware); 1 <= n_cand <= 64
    uint32_t az_aware;
};
// The packers the shard steps serve, by what a step has to do for them: plain (tightly-pack, distribute-evenly: one record per
// application), zoned (single-az-tightly-pack, az-aware-tightly-pack: a record per candidate view, the finish step chooses) and
// minfrag (minimal-fragmentation, single-az-minimal-fragmentation: a count row next to every record of the first exchange).
enum class ShardFamily { plain, zoned, minfrag };
inline std::optional<ShardFamily> shard_family_of(gf_algo algo) {  // (nothing: no shard step serves the packer)
    switch (algo) {
        case GF_ALGO_TIGHTLY_PACK:
        case GF_ALGO_DISTRIBUTE_EVENLY: return ShardFamily::plain;
        case GF_ALGO_SINGLE_AZ_TIGHTLY_PACK:
        case GF_ALGO_AZ_AWARE_TIGHTLY_PACK: return ShardFamily::zoned;
        case GF_ALGO_MINIMAL_FRAGMENTATION:
        case GF_ALGO_SINGLE_AZ_MINIMAL_FRAGMENTATION: return ShardFamily::minfrag;
        default: return std::nullopt;
    }
}
// A count row of the minimal-fragmentation packers: kShardMfRowBytes per record, laid out like the records ([shard][view][app]).
constexpr uint32_t kShardMfRowBytes = 512;
// What every shard step receives: one device's part of one batch.  A step reads what it needs and leaves the rest alone, so
// an entry point sets only its own pointers.
struct ShardBatch {
    NodeTable table{};
    SparseTable gpu_view{};  // n_x == 0: none; else gangs whose executors need a gpu are summed / emitted from the range's part of it
    ShardSet set{};          // the shards this device hosts
    ShardZones zones{nullptr, nullptr, nullptr, nullptr, 0, 0, 1, 0};  // the candidate views; without zones the one plain view
    bool has_zones = false;  // the packer has zone views (the zoned family, single-az-minimal-fragmentation)
    uint32_t n_apps = 0;
    const gf_app* d_apps = nullptr;
    gf_shard_partial* d_part = nullptr;            // first: this device's records, [hosted shard][view][app] (part_dsts empty)
    const gf_shard_partial* d_all_part = nullptr;  // the gathered records, [shard][view][app]
    gf_shard_driver* d_drv = nullptr;              // drivers: as d_part
    const gf_shard_driver* d_all_drv = nullptr;    // ... and d_all_part
    uint32_t* d_counts = nullptr;                  // first, minimal-fragmentation only (else nullptr): the count rows, as d_part
    const uint32_t* d_all_counts = nullptr;        // ... gathered
    gf_result* d_results = nullptr;  // emit (plain packers, plain minimal-fragmentation) or finish (packers with zone views)
    uint32_t* d_exec2 = nullptr;     // the placement buffer: zeroed by emit, every hosted shard writes its slice of it
    uint64_t half = 0;               // words of one region of it (sum of k + 1)
    uint32_t n_shards = 0;           // finish: shards of the gathered tables
    hipStream_t stream = nullptr;
    // The pushed exchanges of the in-process multi-device context (empty: the one-process-per-GPU path and the RCCL exchange)
    PeerPtrs part_dsts{}, count_dsts{}, drv_dsts{};
};
// first: the capacity sums of the hosted ranges (minimal-fragmentation: and their count rows).
hipError_t launch_shard_first(gf_algo algo, const ShardBatch& batch);
hipError_t launch_shard_drivers(gf_algo algo, const ShardBatch& batch);
// (zeroes d_exec2 first: 2 * half words for the plain packers, a region of half words per view otherwise)
hipError_t launch_shard_emit(gf_algo algo, const ShardBatch& batch);
hipError_t launch_shard_finish(gf_algo algo, const ShardBatch& batch);
// d_dst[i] += sum over srcs of src[i], n uint32 entries (only the first device finishes a batch: the all-reduce is a reduce)
hipError_t launch_shard_reduce_pull(const PeerPtrs& srcs, uint32_t* d_dst, size_t n, hipStream_t stream);

// Placing one executor per request (gangfit_executor.inc): first fit or the minimal-fragmentation choice.
// d_reserved: 3 x n_nodes int64 by node index (row-major, nullable); d_hosts: per request a bit set over node indices.
hipError_t launch_executor_fit(bool minimal_fragmentation, const NodeTable& table, const int64_t* d_reserved, uint32_t n_req,
                               const int64_t* d_exe, const uint32_t* d_hosts, uint32_t hosts_stride, const uint32_t* d_node_zone,
                               const uint32_t* d_req_zone, uint32_t* d_node_out, hipStream_t stream);

// findNodes of the failover reconciler (gangfit_findnodes.inc): n_req requests against the executor order; chained = one
// wavefront walks them in order on `table` (the mutable working copy) and subtracts each request's `reserved` map.
// d_adds_out: n_req x n_nodes (zeroed by the caller) or nullptr.
hipError_t launch_find_nodes(bool chained, const NodeTable& table, uint32_t n_req, const int64_t* d_exe, const int32_t* d_k,
                             const uint64_t* d_exec_off, gf_find_result* d_results, uint32_t* d_exec_nodes,
                             uint32_t* d_adds_out, hipStream_t stream);

// Snapshot construction on the device (gangfit_snapshot.hip): reservation replay, available / schedulable columns,
// zone order, node priority order.  All pointers are device buffers owned by the host layer; columns are SoA
// (cpu | memory | gpu, n_nodes each).  On return (stream order) d_avail / d_sched hold the columns and d_perm_b the
// node indices in priority order.
struct SnapshotBuild {
    uint32_t n_nodes, n_res, n_zones;
    bool usage_resident = false;  // d_usage holds the sums already (gf_usage_apply): neither zeroed nor scattered into
    const int64_t* d_alloc;      // 3 * n_nodes
    const int64_t* d_overhead;   // 3 * n_nodes or nullptr
    const uint32_t* d_res_node;  // n_res
    const int64_t* d_res_req;    // 3 * n_res (cpu | memory | gpu)
    const uint32_t* d_zone;      // n_nodes
    const uint32_t* d_name_rank; // n_nodes, a permutation
    int64_t* d_usage;            // 3 * n_nodes
    int64_t* d_avail;            // 3 * n_nodes
    int64_t* d_sched;            // 3 * n_nodes
    int64_t* d_zone_sum;         // 3 * n_zones (memory, cpu interleaved | population)
    uint32_t* d_zone_order;      // n_zones
    uint32_t* d_zone_rank;       // n_zones
    uint32_t* d_perm_a;          // n_nodes
    uint32_t* d_perm_b;          // n_nodes
    int64_t* d_keys_a;           // n_nodes
    int64_t* d_keys_b;           // n_nodes
    int64_t* d_keys_c;           // n_nodes
    uint32_t* d_perm_c;          // n_nodes
    uint32_t* d_sort_work;       // snapshot_sort_work_words() uint32 (8-byte aligned): count tables, barrier, scalars
    int sort_fault = 0;          // fault injection (tests): 1 = one workgroup of the sort never arrives at the grid barrier and
                                 // the others give up after 2^12 instead of 2^24 probes -> the error word is set
    // what launch_snapshot_finalize accumulates into, cleared by the build's one clearing launch (nullptr: no finalize follows):
    uint32_t* d_zfirst = nullptr;  // n_zones words, set to all ones
    uint32_t* d_zhasx = nullptr;   // the range d_zhasx | d_zeval | d_scalars[0 .. 16), set to zero ...
    size_t zhasx_to_scalars_words = 0;  // ... this many words
    // the label key group (nodesorting.go:161-199; gangfit_label_plan.h decides): one more most-significant group of the same
    // sort, a stable sort by the node's label rank on top of the priority order.  d_label == nullptr or label_width == 0: none,
    // d_perm_b holds the priority order P.  Otherwise d_perm_b holds C (all nodes by (rank, position in P)), d_perm_p holds P
    // and d_ppos[node] = the node's position in P.
    const uint32_t* d_label = nullptr;  // n_nodes: rank of the node's label value, UINT32_MAX = not ranked (behind every ranked one)
    uint32_t label_max = 0;             // largest ranked value: the key is the rank itself, "not ranked" = label_max + 1
    uint32_t label_width = 0;           // bits of label_max + 1
    uint32_t* d_perm_p = nullptr;       // n_nodes
    uint32_t* d_ppos = nullptr;         // n_nodes
};
// The merge check behind a label key group: the reference's list of a role R (driver candidates / executor candidates) is
// stable_sort(filter(P, R), rank_R); it equals filter(C, R) exactly when the pairs (rank_R[n], ppos[n]) of R's candidates are
// strictly increasing along C.  One pass over C; a violation sets *d_fail (never cleared here).  SUFFICIENT, not necessary, for
// the two lists to fit one slot order: lists that merge in an order this construction does not find are flagged too.
constexpr uint32_t kLabelMergeUnits = 1024;  // wavefronts of the pass = rows of d_summary
struct LabelMerge {
    uint32_t n_nodes;
    const uint32_t* d_order;    // C: n_nodes
    const uint32_t* d_flags;    // n_nodes: GF_NODE_*
    const uint32_t* d_ppos;     // n_nodes
    const uint32_t* d_rank[2];  // driver | executor label ranks by node; nullptr = every rank equal
    unsigned long long* d_summary;  // 4 * kLabelMergeUnits words: per wavefront and role, its first and last candidate's pair
    uint32_t* d_fail;
};
hipError_t launch_label_merge_check(const LabelMerge& m, hipStream_t stream);
// usage[node] += sign * entry for n_entries reservation entries (columns cpu | memory | gpu of d_req); entries on nodes
// >= n_nodes are ignored.
// d_count (nullable): n_nodes entry counts, count[node] += sign per entry — "carries a reservation" is a map-key question the
// sums cannot answer (an entry of all zeros still makes the node a key).
// d_negative (nullable): after a removal (sign < 0) bit 0 is set when a touched node's sum or count went below zero.
hipError_t launch_usage_apply(uint32_t n_entries, uint32_t n_nodes, const uint32_t* d_node, const int64_t* d_req, int sign,
                              int64_t* d_usage, uint32_t* d_count, uint32_t* d_negative, hipStream_t stream);
// overhead[d_node[i]] = row i (columns cpu | memory | gpu of d_rows, n_rows each) for n_rows rows of the resident overhead columns
// (d_overhead: 3 * n_nodes).  Every d_node[i] < n_nodes and no node twice (the caller checks): plain stores, stream-ordered
// before any later build.
hipError_t launch_overhead_update(uint32_t n_rows, uint32_t n_nodes, const uint32_t* d_node, const int64_t* d_rows, int64_t* d_overhead,
                                  hipStream_t stream);
// The node side of d_node[i] = row i for n_rows rows of the resident cluster: allocatable (columns cpu | memory | gpu of d_rows,
// n_rows each -> d_alloc: 3 * n_nodes), the flag word (d_row_flags -> d_build_flags and d_default_flags, n_nodes each) and, when
// d_row_zone is not nullptr, the zone id (-> d_zone).  Every d_node[i] < n_nodes and no node twice (the caller checks): plain
// stores, stream-ordered before whatever reads the columns next.
hipError_t launch_cluster_update(uint32_t n_rows, uint32_t n_nodes, const uint32_t* d_node, const int64_t* d_rows, const uint32_t* d_row_flags,
                                 const uint32_t* d_row_zone, int64_t* d_alloc, uint32_t* d_zone, uint32_t* d_build_flags,
                                 uint32_t* d_default_flags, hipStream_t stream);
// The empty-cluster capacity scan (gangfit_scan.inc; gf_cluster_fit_feasible): d_out[a] = HasCapacity of application a on the
// cluster columns in node-index order — available = d_alloc - d_over (d_over nullable: no overhead), driver and executor
// candidates = the nodes with d_select[n] != 0 (nullable: every node), nothing reserved.  zoned: the single-AZ answer (some zone
// fits by itself; d_zone: n_nodes ids below 64) without chooseBestResult's averages — the caller refuses what could make one 0.
// One wavefront per application; reads nothing of the installed snapshot.
// The records below are the kernels' own arguments (taken by value): an entry point fills one, the launcher sets n_words on its copy.
struct ScanArgs {
    const int64_t* alloc;         // 3 * n_nodes: cpu | mem | gpu (gf_cluster_set)
    const int64_t* over;          // 3 * n_nodes, or nullptr: no overhead
    const uint32_t* zone;         // n_nodes zone ids below kScanZones (ZONED only)
    const uint8_t* select;        // n_nodes, or nullptr: every node
    uint32_t n_nodes;
    uint32_t n_apps;
    const gf_app* apps;
    uint8_t* out;                 // n_apps HasCapacity bytes
};
hipError_t launch_cluster_scan(bool zoned, const ScanArgs& args, hipStream_t stream);
// The same scan for applications of many node sets in one launch (gf_cluster_fit_feasible_sets): application a asks the nodes of
// row app_set[a] of set_words — rows of ceil(n_nodes / 64) words, bit (n & 63) of word n >> 6 = node n, no bit at or beyond
// n_nodes, every app_set[a] a row of the matrix (the entry point checks both).  A wavefront reads the columns only of the 64-node
// chunks whose word of its row is not zero.
struct ScanSetsArgs {
    const int64_t* alloc;         // 3 * n_nodes: cpu | mem | gpu (gf_cluster_set)
    const int64_t* over;          // 3 * n_nodes, or nullptr: no overhead
    const uint32_t* zone;         // n_nodes zone ids below kScanZones (ZONED only)
    const uint64_t* set_words;    // n_sets * n_words; no bit at or beyond n_nodes (the entry point checks)
    const uint32_t* app_set;      // n_apps row numbers below n_sets (the entry point checks)
    uint32_t n_nodes;
    uint32_t n_words;             // W = ceil(n_nodes / 64): set by the launcher
    uint32_t n_apps;
    const gf_app* apps;
    uint8_t* out;                 // n_apps HasCapacity bytes
};
hipError_t launch_cluster_scan_sets(bool zoned, const ScanSetsArgs& args, hipStream_t stream);
// The executor Filter on the resident cluster (gangfit_exec_scan.inc; gf_cluster_executor_fit): out[q] = the node the
// installing route (gf_snapshot_build + gf_executor_fit) returns for request q when it is given only the nodes of row req_set[q]
// that pass the zone test — as an order-free minimum over the columns in node-index order.  One workgroup of four wavefronts per
// request; reads nothing of the installed snapshot.
struct ExecScanArgs {
    const int64_t* alloc;         // 3 * n_nodes: cpu | mem | gpu (gf_cluster_set)
    const int64_t* over;          // 3 * n_nodes resident overhead, or nullptr: none
    const int64_t* usage;         // 3 * n_nodes resident usage sums (gf_usage_apply)
    const uint32_t* res_count;    // n_nodes: reservation entries that name the node
    const uint32_t* zone;         // n_nodes cluster zone ids below kExecZones
    const uint32_t* name_rank;    // n_nodes, a permutation
    const uint32_t* flags;        // n_nodes: the cluster's default GF_NODE_* flags
    const uint32_t* node_zone;    // n_nodes ids the zone test compares, or nullptr: the cluster's
    const uint32_t* label_rank;   // n_nodes executor label ranks, or nullptr
    const uint64_t* set_words;    // n_sets * n_words, or nullptr: every node.  No bit at or beyond n_nodes (the entry point checks)
    const uint32_t* req_set;      // n_req rows (with set_words)
    const uint32_t* req_zone;     // n_req, or nullptr: GF_ANY_ZONE
    const uint32_t* hosts;        // n_req * hosts_stride words (32 nodes each), or nullptr
    const int64_t* exe;           // n_req * 3
    uint32_t n_nodes, n_words /* set by the launcher */, n_zones /* <= 64 */, n_req, hosts_stride;
    uint32_t* out;                // n_req node indices
};
hipError_t launch_cluster_executor_fit(bool minimal_fragmentation, const ExecScanArgs& args, hipStream_t stream);
// findNodes of the failover reconciler on the resident cluster (gangfit_find_scan.inc; gf_cluster_find_nodes): request q walks the
// ready, schedulable nodes of its row in ascending create_rank on available = alloc - (usage + over), exactly as find_nodes_kernel
// walks the executor order of an installed snapshot.  The entry point names the rows some request uses (`used rows`: under
// `chained`, rows of equal content are one used row and two used rows share no node) and groups the requests by used row, stable
// in q.  Three launches: prepare (perm, work), order (every used row's list in ord), walk.  Reads nothing of the installed snapshot.
struct FindScanArgs {
    const int64_t* alloc;         // 3 * n_nodes: cpu | mem | gpu (gf_cluster_set)
    const int64_t* over;          // 3 * n_nodes resident overhead, or nullptr: none
    const int64_t* usage;         // 3 * n_nodes resident usage sums (gf_usage_apply)
    const uint32_t* flags;        // n_nodes: the cluster's default GF_NODE_* flags
    const uint32_t* create_rank;  // n_nodes, a permutation (the entry point checks): the position at which a node is visited
    const uint64_t* set_words;    // n_sets * n_words, or nullptr: every node.  No bit at or beyond n_nodes (the entry point checks)
    const uint32_t* row_set;      // n_rows: the row of set_words a used row stands for (with set_words)
    const uint64_t* row_base;     // n_rows: where the used row's list starts in ord; the next base is at least its popcount further
    const uint32_t* row_req;      // n_rows + 1: used row r owns req_list[row_req[r] .. row_req[r + 1])
    const uint32_t* req_list;     // n_req: the requests grouped by used row, ascending q inside a row
    const uint32_t* req_row;      // n_req: request q's used row
    const int64_t* exe;           // n_req * 3
    const int32_t* k;             // n_req counts in [0, GF_MAX_K]
    const uint64_t* exec_off;     // n_req: where request q's placements start in exec_nodes
    uint32_t n_nodes, n_words /* set by the launcher */, n_rows, n_req;
    uint32_t* perm;               // n_nodes: position -> node (written by prepare)
    uint32_t* ord;                // the used rows' lists
    uint32_t* row_len;            // n_rows: the lists' lengths (written by order)
    int64_t* work;                // 3 * n_nodes: the call's working table, cpu | mem | gpu by node; the residual afterwards
    gf_find_result* results;      // n_req
    uint32_t* exec_nodes;         // sum of k
    uint32_t* adds_out;           // n_req * n_nodes (zeroed by the caller), or nullptr
};
hipError_t launch_cluster_find_nodes(bool chained, const FindScanArgs& args, hipStream_t stream);
// The slot tables of the merged layout built from the device-resident snapshot columns (what gf_orders_set builds on the
// host): every node gets the slot of its position in the priority order.
struct SnapshotFinalize {
    uint32_t n_nodes, n_slots, n_chunks, n_zones;
    const int64_t* d_avail;     // 3 * n_nodes, by node
    const int64_t* d_sched;     // 3 * n_nodes, by node
    const uint32_t* d_perm;     // n_nodes: priority order -> node
    const uint32_t* d_zone;     // n_nodes
    const uint32_t* d_flags;    // n_nodes: GF_NODE_*
    int64_t* d_snap;            // 3 * n_slots
    int64_t* d_sched_slot;      // 3 * n_slots
    uint32_t* d_slot_node;      // n_slots
    uint32_t* d_node_slot;      // n_nodes
    uint32_t* d_dslot;          // n_slots (identity)
    uint64_t* d_masks;          // 2 * n_chunks: executor | driver candidate bits
    int64_t* d_cmax;            // 3 * n_chunks
    int64_t* d_node_tab;        // 6 * n_nodes
    unsigned long long* d_gcd_part;  // 6 * n_chunks: chunk gcds, then chunk maxima of the magnitudes
    long long* d_units;         // 3
    uint32_t* d_zfirst;         // n_zones
    uint32_t* d_zhasx;          // n_zones
    uint32_t* d_zeval;          // n_zones: zone -> index in the evaluation list, GF_NO_NODE = not evaluated
    uint32_t* d_scalars;        // 16 words: [0] = zones in the evaluation list, [1] = no narrow form, [2] = negative schedulable
                                // value, [3] = the sort's error word (bit 0) | the label merge check failed (bit 1), [4 .. 16) = d_units as pairs of words
                                // (one read-back)
    uint32_t* h_out = nullptr;  // nullable: the device's address of sixteen pinned host words, ZEROED BY THE HOST before the launch, that
                                // receive d_scalars as the kernels produce it (no read-back copy on the stream)
    uint64_t* d_zmasks;         // 2 * n_zones * n_chunks: executor rows, then (from row n_zones) driver rows
    int32_t* d_nsnap;           // 3 * n_slots
    int32_t* d_ncmax;           // 3 * n_chunks
    int4* d_nquad;              // n_slots records {cpu, mem, gpu, node}: d_nsnap and d_slot_node once more (NodeTable::nquad)
};
hipError_t launch_snapshot_finalize(const SnapshotFinalize& f, const uint32_t* d_sort_error, hipStream_t stream);
struct CopyOut {  // three ranges of 32-bit words, any of them empty
    const uint32_t* src[3];
    uint32_t* dst[3];
    size_t words[3];
};
hipError_t launch_copy_out(const CopyOut& c, hipStream_t stream);
hipError_t launch_stream_copy(const void* src, void* dst, size_t bytes, hipStream_t stream);
hipError_t launch_stream_read(const void* src, size_t bytes, uint32_t* sink, hipStream_t stream);
hipError_t launch_empty(uint32_t* sink, hipStream_t stream);
size_t snapshot_sort_work_words();     // uint32 words of SnapshotBuild::d_sort_work
uint32_t snapshot_sort_error_word();   // index of the word that is non-zero when the sort's grid barrier gave up; the word behind
                                       // it is LabelMerge::d_fail of the same build (launch_snapshot_finalize reads both)
hipError_t launch_snapshot_build(const SnapshotBuild& b, hipStream_t stream);
// A snapshot over a node set of the resident cluster (gf_snapshot_build_resident_set).  Membership is a row of W = ceil(n_nodes / 64)
// words as in ScanSetsArgs (no bit at or beyond n_nodes, n_members = its popcount, at least 1: the entry point checks).  The
// members' columns are gathered into compact ones (member c = the c-th set bit), launch_snapshot_build / launch_snapshot_finalize
// run on those at size n_members exactly as they run on a cluster of the members alone, and launch_snapshot_set_scatter maps what
// the finalize left in member indices back to cluster indices.
struct SnapshotSetGather {
    uint32_t n_nodes, n_words, n_members;
    const uint64_t* d_words;      // W
    uint64_t* d_nbits;            // W, ZERO at launch: receives bit p = "the node of name rank p is a member"
    uint32_t* d_prefix;           // 2 * W: set bits before word w of d_words | of d_nbits
    const int64_t* d_alloc;       // 3 * n_nodes, by cluster index
    const int64_t* d_overhead;    // 3 * n_nodes or nullptr (c_overhead is then not written)
    const int64_t* d_usage;       // 3 * n_nodes
    const uint32_t* d_zone;       // n_nodes
    const uint32_t* d_name_rank;  // n_nodes, a permutation
    const uint32_t* d_flags;      // n_nodes
    int64_t *c_alloc, *c_overhead, *c_usage;  // 3 * n_members each, by member
    uint32_t *c_zone, *c_flags;   // n_members
    uint32_t* c_name_rank;        // n_members: the member's rank among the members' names (a permutation of 0 .. n_members - 1)
    uint32_t* c_node;             // n_members: member -> cluster index
};
hipError_t launch_snapshot_set_gather(const SnapshotSetGather& g, hipStream_t stream);
struct SnapshotSetScatter {
    uint32_t n_nodes, n_members;
    const uint64_t* d_words;      // W
    const uint32_t* d_prefix;     // W: set bits before word w
    const uint32_t* c_node;       // n_members
    const uint32_t* c_node_slot;  // n_members: SnapshotFinalize::d_node_slot of the compact build
    const int64_t* c_node_tab;    // 6 * n_members: its d_node_tab
    uint32_t* d_node_slot;        // n_nodes: the members' slots, GF_NO_NODE for every other node
    int64_t* d_node_tab;          // 6 * n_nodes: the members' rows, 0 for every other node
    const uint32_t* d_status;     // SnapshotFinalize::d_scalars + 3: not zero (the sort gave up, the merge check failed) = nothing
                                  // will be installed from these tables, and nothing is written
    uint32_t* d_slot_node;        // n_members + 1 slots holding member indices: rewritten to cluster indices
    int4* d_nquad;                // ... and the node word of the slot records
};
hipError_t launch_snapshot_set_scatter(const SnapshotSetScatter& s, hipStream_t stream);

// Device self-test of the wave primitives (DPP scan, exact clamped division) against plain reference code.
// Writes the number of mismatching lanes/cases to *d_mismatch.
hipError_t launch_selftest(uint64_t seed, uint32_t n_cases, uint32_t* d_mismatch, hipStream_t stream);

}  // namespace gangfit
