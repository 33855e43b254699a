// gangfit_worker.inc — the resident worker of the independent batch.  Included by gangfit_kernels.hip inside its anonymous
// namespace, behind fit_independent_kernel (same wave-level code: load_group0, wave_decide).
//
// Why: a 1 000-application batch is ~1 000 wavefronts that each walk a short chain of dependent misses; as a launch it pays
// ~2.5 us of dispatch and starts with cold caches, and two launches on one stream never overlap.  The worker is ONE launch
// that stays on the device while batches keep coming: the host posts tickets (where the records are, where the answers go)
// into a ring in pinned memory and rings a doorbell word; a leader wavefront relays new tickets into device memory; `sets`
// groups of wavefronts take the tickets in turn (ticket t belongs to set t % sets), so that many batches are in flight at
// once and none of them pays a dispatch; the last wavefront of a ticket writes its completion word to pinned memory.  The
// snapshot tables are kernel arguments — the library stops the worker before it installs another snapshot — and stay in the
// L2s from one batch to the next.
//
// It cannot hang the device: the leader leaves when no ticket has arrived for `idle_ticks` (100 MHz clock) or when the host
// sets the stop word, and every other wavefront leaves as soon as it has worked off the tickets published before that.
//
// Coherence (MI355X_MICROARCH.md, inter-workgroup visibility): the tables are read through the caches (they do not change
// while the worker lives).  A ticket is six self-validating 8-byte words — every word carries a 16-bit tag of its ticket
// number in bits no pointer or count uses — written by the host, copied by the leader with write-through (sc1) stores and
// read by the pollers with ONE relaxed sc1 load instruction per probe: a probe that finds the right tag in all six words
// has the whole ticket, whatever order the words arrived in; no fence, no second round trip.  App records are read with
// system-scope loads (they may live in pinned host memory).
// Answers leave as write-through (system-scope) stores: the wave-level code writes its placements into a private scratch
// slice, the wavefront copies them out; the 16-byte result goes out as two 8-byte words.  A workgroup drains its stores
// (s_waitcnt vmcnt(0)), adds its share to the ticket's counter, and the workgroup that completes the count writes the
// ticket's completion word to pinned host memory.  (A release fence per workgroup and ticket — an L2 write-back — was
// measured first: it made the groups of wavefronts queue behind each other's write-backs, 5 us per ticket however many
// groups.  And plain stores to pinned host memory stay in the L2 until a write-back: a ticket completed with all-zero
// answers on the host.)

// The per-application pipeline of a wavefront (round 6, each step measured on its own: profiles/r6b_worker_variants.txt — a ticket
// 1.37 -> 1.22 us in a long stream, a window of twenty 54.9 -> 51.2 us):
//   direct     tightly-pack placements leave as write-through stores straight from the run emission (device-resident
//              destinations: no private slice, no read-back of the wavefront's own stores)
//   records    the records of all applications a wavefront serves in a ticket (up to eight) in ONE load instruction —
//              superseded by kRecords below, which requests each record when its application is handed out
//   s_g0       group 0 of the chunk index (the same for every application while the worker lives) read once into LDS
//   kRecords   the applications of a ticket that a workgroup serves are HANDED OUT one by one (an LDS counter per round) instead
//              of belonging to fixed wavefronts: sixteen wavefronts finish a ticket within one application of each other.  The
//              minimal-fragmentation instance, at its register budget, keeps the fixed mapping and reads each record uncached.
// Leaving out the placement and result stores altogether (a measurement build with wrong answers, since retired) was 8 % faster:
// the stores are not what a ticket waits for.
// Measured and removed in the same round (profiles/r6c_worker_lds_table_not_kept.txt): the scaled int32 table resident in LDS
// (145 KB per workgroup, a chunk visit three ds_read_b32) — same answers, 1.64 us per ticket: with sixteen wavefronts per CU the
// bound is the SIMDs' issue slots, not the table's read latency, and the resident table adds instructions.
// Measured and removed (profiles/r6u_worker_record_cache_not_kept.txt): an LDS record cache per workgroup (the records of a round's
// applications 16 .. 47 requested a round ahead) — no difference: the wavefronts of a CU are in different phases and hide each
// other's record latency.

// NARROW (tightly-pack instance; profiles/r7a_worker_narrow_summary.md): an application whose six requests are exact multiples of the
// snapshot's units (scale_record below: one lane-parallel pass, one ballot) is decided on the snapshot's scaled int32 twin — the same
// wave_decide, instantiated over NarrowApp / NarrowView: 12 bytes per slot instead of 24, 32-bit compares, capacities as three
// multiply-highs, four ds_permute per gather instead of seven — and every other application (no scaled form, a gang of gpu executors,
// a snapshot without the twin) on the int64 path by the same wavefront.  Same answers by construction: comparisons, subtractions
// and floor divisions do not change under a common exact factor.  Measured against the int64-only kernel, interleaved on one
// machine: 769.3 k -> 752.7 k instructions per ticket at K = 2 000 (vector -6.7 %, LDS -18 %, scalar +3.6 %), 922-931 M -> 937-983 M
// decisions/s (medians +5.4 %, ranges apart); a window of twenty: unchanged.  94 VGPRs, code 31.9 -> 48.5 KB.
// (The table itself resident in LDS was a different experiment — r6c above — and stays removed.)

// ROUND BOOKKEEPING (profiles/r8a_worker_rounds_summary.md): what a wavefront executes around its decisions.  The round arithmetic
// lives in gangfit_worker_rounds.h (no runtime division: the rotation advances by one and wraps by compare, the one quotient by
// app_stride is a multiplication by a constant of the launch, the workgroup's share of a ticket is a closed form instead of a
// per-lane division and a wave scan); the hand-out word is taken with ONE LDS operation (fetch-and-add first, compare-and-swap only
// on a stale word); what the round's end extracts from the next ticket is carried into the next round instead of being read apart
// again; the narrow path keeps its lane's group 0 in seven registers instead of five LDS reads per application.  Measured against
// the parent, interleaved on one machine: 752.8 k -> 724.9 k instructions per ticket at K = 2 000 (scalar -21.5 k, LDS -4.1 k,
// vector -2.2 k), 968-978 M -> 997-1 016 M decisions/s (medians +4.0 %, ranges apart); a window of twenty: unchanged.  94 -> 98
// VGPRs (92 before group 0 moved into registers; budget 104).
// Measured and dropped: the carried ticket values forced into scalar registers (v_readfirstlane at the round's top) — 735.2 k
// instructions per ticket and 994 M decisions/s against 728.8 k and 1 007 M without: more spilled scalar registers than it saves
// vector compares.

// OPERANDS (profiles/r9a_worker_operands_summary.md): where the launch constants of the tightly-pack instance live.  The instance keeps
// more wave-uniform values alive across its round loop than there are scalar registers; the compiler parks the surplus in lanes of
// spill VGPRs and fetches it back with v_readlane — a VECTOR instruction, on the pipe the kernel is bound by (tools/worker_spills.py
// lists them per basic block).  Two groups of operands that the narrow decision carried through its whole body and seldom reads are
// therefore not held at all but read from the kernel's own argument segment with scalar loads where they are used
// (worker_kernargs_here, gangfit_kernels.hip; the segment lives as long as the launch):
//   argument segment, at use   the wide chunk maxima and the three units of the NARROW view (NarrowView::wide_here: three row pointers
//                              and three 64-bit units before) — read by chunk_may_hold / chunk_maxima, that is for the chunks behind
//                              group 0 (every application of a 10 000-node cluster gets there), and inside group 0 on the general
//                              layout, in the fallback and behind a stale maximum: less often read than the columns, not cold;
//                              the sparse view's size, asked only for a gang of gpu executors (sparse_serves)
//   registers                  everything else: the narrow records (ONE pointer, NodeTable::nquad: {cpu, mem, gpu, node} per slot —
//                              r10a below; three column pointers and slot_node before), xmask, dmask, n_chunks, dslot, n_x, n_d,
//                              dev, sets, leave_after, blocks_per_set, the stride constants, stats, and the operands of the int64
//                              decision (slot_node among them), the sparse table, scratch, host, generation
// Measured on this code, parent and result alternately on one machine, seven runs each: spilled scalar registers 171 -> 112,
// v_readlane on spill lanes inside the loop 510 -> 284; 724.9 k -> 696.5 k instructions per ticket at K = 2 000 (vector -17.6 k,
// scalar -13.6 k, scalar-memory +2.8 k); 1 000-1 016 M -> 1 029-1 045 M decisions/s (medians +3.1 %, ranges apart); a window of
// twenty: 404-428 M -> 431-440 M (no loss).
// Measured and dropped: reading the int64 decision's operands (wide columns, SparseTable, scratch, host, generation) at their use
// as well — that variant had 145 spilled registers and 437 in-loop spill reads, 3.8 k vector and 2.3 k scalar instructions per
// ticket more than the same code without that part, and was no faster; on its own it was 1.2 % slower than the parent.

// RECORDS (profiles/r10a_worker_quad_summary.md): a narrow decision loads about 2.3 chunks of 64 slots and wants a slot's three
// values and its node id together every time; as four columns that was four global_load_dword behind five address computations and
// a staircase of four waits, four base pointers live through the decision, and the slot_node pointer re-read from the argument
// segment at three places.  The snapshot's twin now exists a second time as one 16-byte record per slot (written by both producers
// of the twin in the pass that writes the columns), NarrowView holds that one pointer, and a chunk is one v_lshl_add_u64, one
// global_load_dwordx4 and one wait; the node ids of the driver's chunk and of every scanned chunk — the driver's, the placements' —
// come out of the same load (a driver found by wave_first_fitting_driver / wave_fallback: one more load of its record, behind the
// decision).
// Measured, parent and result alternately on one machine, seven runs each: 1 035-1 041 M -> 1 048-1 063 M decisions/s at K = 2 000
// (medians +1.6 %, ranges apart); a window of twenty 402-420 M -> 405-418 M (medians 408.8 -> 414.9: no loss).  Spilled scalar
// registers 112 -> 107; 97 VGPRs as before.
// COUNTERS ONLY WHERE SOMEBODY READS THEM (same summary): fit_worker_kernel<tightly-pack> has nothing of xvis / dvis compiled in, the
// host launches fit_worker_kernel<kWorkerCounting> while gf_scan_stats is on.  Measured against the tree without it, alternately,
// seven runs each: 1 047-1 059 M -> 1 068-1 081 M decisions/s at K = 2 000 (medians +1.8 %, ranges apart); a window of twenty 411.7 ->
// 417.1 M (medians; no loss).  Measured and dropped: the hand-out's fetch-and-add as ds_add_rtn_u64 in inline assembly under
// `lane == 0` (without the compiler's one-lane reduction around it) — medians +1.1 % on the records alone (1 055-1 068 M against
// 1 047-1 059 M) and +1.2 % on top of the counting split (1 077-1 091 M against 1 068-1 081 M): the ranges overlap both times, so it
// does not pass the project's criterion; it also cost two VGPRs (97 -> 99).

// SHAPE ROWS (profiles/r11a_worker_rows_summary.md; the arithmetic and the proof: gangfit_worker_rows.h): the capacity of a node for
// an executor request does not depend on the application, a real queue asks for a handful of pod sizes, and the snapshot cannot
// change while the worker lives — yet every decision recomputed it: group 0 of the index, ~2.3 chunk loads, the compares, the
// gather, three multiply-highs per lane.  A workgroup now keeps, per scaled executor request it has met kRowSightings times, the
// first 64 slots with room for it {slot, node, capacity} as a row in its LDS (40 rows, a directory probed by 40 lanes at once, no
// eviction), and a wavefront that finds a READY row decides from it: wave_row_driver (the driver step of wave_decide on its own),
// the driver's slot corrected, one wave scan, the run emission; gangs of gpu executors included.  A row that does not cover K, K == 0,
// a driver behind group 0, the general layout: wave_decide on the same record, as before — nothing has been written by then.
// Per workgroup and per launch BY DESIGN: LDS dies with the launch and the worker leaves before every install, so no row outlives
// its snapshot; nothing waits for a row (BUILDING means "not there"); no loop here exits on another wavefront's progress.  Out of
// scope: rows in device memory, rows that survive a launch (that is where a window of twenty could gain).
// The build is inline (a real call gives the kernel a stack); the row state is ONE LDS object addressed through a lane index made
// new at its use (as separate arrays the addresses were hoisted into ten VGPRs: 107; now 104, the whole budget, no scratch).  Not
// looked up at all: the counting instance, a bounded launch of fewer than kRowSightings rounds per set, a wavefront that found the
// directory full before any row was built.  Counters: three LDS words per workgroup, added to WorkerDevCtl::rows when the
// workgroup's last wavefront leaves (gf_worker_row_stats).
// Measured first, as a ceiling: the narrow decision without any pack (wrong answers on purpose) 1 913-1 957 M decisions/s against
// 1 068-1 082 M (+80 %).  The change, parent and result alternately on one machine, seven runs each: 1 068-1 085 M -> 1 389-1 396 M
// decisions/s at K = 2 000 (medians +29.2 %; the result's minimum 304 M above the parent's maximum, whose own range is 17 M wide);
// 673.9 k -> 492.2 k instructions per ticket, 97.8 % of the decisions served from a row (a served decision: about 490 instructions).
// A window of twenty, rows off: 412.9-448.1 M -> 418.7-431.6 M (medians 440.6 -> 429.2, inside the parent's range) — not free:
// 727.5 k -> 772.1 k instructions per ticket there, the register pressure of the code around the row path (97 -> 104 VGPRs, 106 -> 111
// spilled scalar registers).

__device__ __forceinline__ unsigned long long sys_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void sys_store(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The fields of a gf_app from a register that holds the record (lane f < 8 = word f), handed out with v_readlane.
__device__ __forceinline__ App app_from_lanes(unsigned long long w) {
    App r;
    r.drv0 = (int64_t)read_lane((int64_t)w, 0);
    r.drv1 = (int64_t)read_lane((int64_t)w, 1);
    r.drv2 = (int64_t)read_lane((int64_t)w, 2);
    r.exe0 = (int64_t)read_lane((int64_t)w, 3);
    r.exe1 = (int64_t)read_lane((int64_t)w, 4);
    r.exe2 = (int64_t)read_lane((int64_t)w, 5);
    const uint64_t kf = (uint64_t)read_lane((int64_t)w, 6);
    r.k = (int32_t)(uint32_t)kf;
    r.flags = (uint32_t)(kf >> 32);
    r.exec_off = (uint64_t)read_lane((int64_t)w, 7);
    r.rcp0 = r.exe0 > 0 ? fast_rcp((double)r.exe0) : 0.0;
    r.rcp1 = r.exe1 > 0 ? fast_rcp((double)r.exe1) : 0.0;
    r.rcp2 = r.exe2 > 0 ? fast_rcp((double)r.exe2) : 0.0;
    return r;
}

// A gf_app read around the caches: lanes 0..7 fetch one 8-byte word each.
__device__ __forceinline__ App load_app_uncached(const gf_app* apps, uint32_t a, int lane) {
    const unsigned long long* p = reinterpret_cast<const unsigned long long*>(apps + a);
    unsigned long long w = 0;
    if (lane < 8) w = sys_load(p + lane);
    return app_from_lanes(w);
}

// narrow_magic's multiplier 2 * ceil(2^(30 + l) / e), l = ceil(log2 e), per LANE and without a 64-bit division (one of those is
// ~800 cycles of a wavefront): the float64 estimate 2^(30 + l) * (1 / e) is within one of the quotient (fast_rcp: relative error
// below 2^-40, the quotient below 2^31), an exact 64-bit multiply-subtract settles floor and remainder, the remainder the ceiling.
// 0 for e == 0.  gf_selftest compares it with narrow_magic on the device.
__device__ __forceinline__ uint32_t narrow_magic_lane(uint32_t e) {
    const uint32_t d = e != 0u ? e : 1u;
    const uint32_t l = narrow_shift((int32_t)d);
    const uint64_t N = 1ull << (30u + l);
    uint32_t m = (uint32_t)((double)N * fast_rcp((double)d));
    int64_t rem = (int64_t)(N - (uint64_t)m * (uint64_t)d);
    if (rem < 0) {
        m -= 1u;
        rem += (int64_t)d;
    } else if (rem >= (int64_t)d) {
        m += 1u;
        rem -= (int64_t)d;
    }
    m += rem > 0 ? 1u : 0u;
    return e != 0u ? 2u * m : 0u;
}

// One request word per lane, divided by its dimension's unit (unit >= 1, rcp = fast_rcp(unit)): true when the word is a
// non-negative exact multiple of the unit and the quotient q is below 2^30.  The estimate w * rcp is within 2^-10 of an exact
// quotient of that size, so rounding it to the nearest integer gives q, and q * unit == w (exact: the true product is below
// 2^64) is the whole proof — for a word that is no multiple nothing passes it.
__device__ __forceinline__ bool scale_word(unsigned long long w, int64_t unit, double rcp, uint32_t& q) {
    const double qf = (double)(int64_t)w * rcp;
    const bool in = (int64_t)w >= 0 && qf < 1073741823.5;
    q = in ? (uint32_t)__builtin_rint(qf) : 0u;
    return in && (unsigned long long)q * (unsigned long long)unit == w;
}

// The scaled record of the application in lanes 0 .. 7 of w (lanes 0 .. 5 = drv0..2, exe0..2), built lane-parallel: ONE pass
// divides the six requests (lane l by unit_l = the unit of dimension l mod 3) and computes the executor request's multipliers
// in lanes 3 .. 5, one ballot says whether the application has a scaled form, nine v_readlane hand the fields out.  False: the
// caller decides this application on the int64 path (r is then not to be used).
__device__ __forceinline__ bool scale_record(unsigned long long w, int lane, int64_t unit_l, double rcp_l, NarrowApp& r) {
    uint32_t q;
    const bool ok = scale_word(w, unit_l, rcp_l, q) || lane >= 6;
    const uint32_t mag = narrow_magic_lane(q);
    const uint64_t kf = (uint64_t)read_lane((int64_t)w, 6);
    r.k = (int32_t)(uint32_t)kf;
    r.flags = (uint32_t)(kf >> 32);
    r.exec_off = (uint64_t)read_lane((int64_t)w, 7);
    r.drv0 = (int32_t)read_lane(q, 0);
    r.drv1 = (int32_t)read_lane(q, 1);
    r.drv2 = (int32_t)read_lane(q, 2);
    r.exe0 = (int32_t)read_lane(q, 3);
    r.exe1 = (int32_t)read_lane(q, 4);
    r.exe2 = (int32_t)read_lane(q, 5);
    r.mag0 = read_lane(mag, 3);
    r.mag1 = read_lane(mag, 4);
    r.mag2 = read_lane(mag, 5);
    r.sh0 = narrow_shift(r.exe0);
    r.sh1 = narrow_shift(r.exe1);
    r.sh2 = narrow_shift(r.exe2);
    r.un0 = r.exe0 == 0 ? 0xFFFFFFFFu : 0u;
    r.un1 = r.exe1 == 0 ? 0xFFFFFFFFu : 0u;
    r.un2 = r.exe2 == 0 ? 0xFFFFFFFFu : 0u;
    return __ballot(ok) == ~0ull && (uint32_t)r.k <= (uint32_t)GF_MAX_K;
}

// Block 0: the leader (one wavefront).  Blocks 1 ..: set (b - 1) / blocks_per_set, kWorkerWaves wavefronts = applications each.
// Sixteen wavefronts per workgroup: (a) a ticket costs one counter update per workgroup, and those updates — read-modify-writes
// of one word at device scope — queue behind each other (with four-wavefront workgroups, 250 per ticket, they were the floor:
// ~3.5 us per ticket however many groups of wavefronts shared the work); (b) such a workgroup fills a CU's register file, so
// 3 x 64 + 1 workgroups sit on 193 CUs and leave the rest of the device to FIFO chains.
// REGISTER BUDGET: 104 VGPRs, not one more (tools/kernel_resources.py).  Sixteen wavefronts of 104 leave 96 registers per SIMD
// lane on the worker's CUs, and a wavefront of fit_independent_kernel (72) still fits next to them; at 106 — allocated as 112 —
// it does not, and a gf_fit_batch launched next to a resident worker then WAITED FOR THE WORKER TO IDLE OUT (500 ms with
// worker_idle_us = 500 000) although 27 CUs were free: measured twice in round 5 when a change added two registers
// (tools/micro/probe_worker_resident.py; tests/test_gpu_worker.py::test_a_fifo_chain_starts_next_to_a_resident_worker fails on it).
// ZONE-AWARE (single-az-tightly-pack, az-aware-tightly-pack): the ticket protocol is the one above; what a wavefront does with one
// application is wave_decide_zones (gangfit_zones.inc) — its candidate views one after the other, no barrier — on the int64 table
// only.  Placements of candidate views are slot ids and the winner is known behind the last view, so nothing is emitted directly:
// the slot's `priv` and first survivor slice (tightly-pack uses neither survivor list) are the "current" and the "best so far"
// placements, and the copy-out translates slot -> node.  An infeasible record's placements are not touched at all.
template <bool AZ_AWARE>
__device__ __forceinline__ Decision wave_decide_zones(const NodeTable& T, const SparseTable& G, const ZoneTable& Z,
                                                      const int64_t* __restrict__ sched, const GlobalView& plain, const App& app,
                                                      uint32_t* cur, uint32_t* kept, int lane, unsigned long long& xvis,
                                                      unsigned long long& dvis, const uint32_t*& placed);

// SHAPE ROWS (gangfit_worker_rows.h; tightly-pack instance, narrow path): the driver step of wave_decide on its own — the group-0
// test for the driver role, the driver chunk's records, the fit mask, the first fitting lane; the same expressions as
// wave_decide's merged branch (binpack.go:67-71) — so that a decision served from a row touches the node table for its driver
// only.  found == false (no candidate chunk in group 0, or a stale maximum): the caller decides on wave_decide, which searches on.
// The driver's three values stay in lane fl of d0 .. d2.
struct RowDriver {
    bool found;
    uint32_t ds, node;
    int fl;
    int32_t d0, d1, d2;
};
__device__ __forceinline__ RowDriver wave_row_driver(const NarrowView& V, const Orders& O, const NarrowApp& app,
                                                     const Group0T<int32_t>& g0, int lane) {
    RowDriver r{false, 0u, GF_NO_NODE, 0, 0, 0, 0};
    const uint32_t dc = (O.n_d + kWave - 1) / kWave;
    const uint64_t ind_m = low_lanes(dc < V.n_chunks ? dc : V.n_chunks);
    constexpr int kNE = 33;
    const uint64_t md = ge3_mask(g0.m0, g0.m1, g0.m2, app.drv0, app.drv1, app.drv2) & ind_m &
                        __builtin_amdgcn_uicmpl((unsigned long)g0.dcand, 0ul, kNE);
    if (!md) return r;
    const int bd = __ffsll((unsigned long long)md) - 1;
    const uint32_t limit = O.n_d > O.n_x ? O.n_d : O.n_x;
    const uint32_t id = (uint32_t)bd * kWave + lane;
    uint32_t dnode = GF_NO_NODE;
    if (id < limit) V.load(id, r.d0, r.d1, r.d2, dnode);
    const uint64_t cdm = (uint64_t)read_lane((int64_t)g0.dcand, bd);
    const uint64_t fm = ge3_mask(r.d0, r.d1, r.d2, app.drv0, app.drv1, app.drv2) & cdm & low_lanes(chunk_len(O.n_d, (uint32_t)bd * kWave, kWave));
    if (!fm) return r;
    r.fl = __ffsll((unsigned long long)fm) - 1;
    r.ds = (uint32_t)bd * kWave + (uint32_t)r.fl;
    r.node = read_lane(dnode, r.fl);
    r.found = true;
    return r;
}
static_assert(rows::kCapClamp == GF_MAX_K && rows::kRowLen == (uint32_t)kWave && rows::kRows <= (uint32_t)kWave, "lane = entry");

// WHICH: the packer — or kWorkerCounting (tightly-pack with the scan counters).  The slots a decision visits (xvis / dvis, two 64-bit
// wave-uniform accumulators that every chunk visit updates) are summed into W.stats by every instance but fit_worker_kernel<tightly-pack>,
// which has nothing of the accumulation compiled in; the host launches fit_worker_kernel<kWorkerCounting> instead when gf_scan_stats
// is on (launch_fit_worker).  The other packers' instances count whenever W.stats is set, as before.
constexpr int kWorkerCounting = 100 + (int)GF_ALGO_TIGHTLY_PACK;
template <int WHICH>
__global__ __launch_bounds__(kWave* kWorkerWaves, 4) void fit_worker_kernel(NodeTable T, SparseTable G, WorkerArgs W) {
    constexpr int ALGO = WHICH == kWorkerCounting ? (int)GF_ALGO_TIGHTLY_PACK : WHICH;
    constexpr bool COUNT = WHICH != (int)GF_ALGO_TIGHTLY_PACK;
    constexpr bool kZoned = ALGO == GF_ALGO_SINGLE_AZ_TIGHTLY_PACK || ALGO == GF_ALGO_AZ_AWARE_TIGHTLY_PACK;
    constexpr int kInner = kZoned ? (int)GF_ALGO_TIGHTLY_PACK : ALGO;  // the packer of one candidate view
    __shared__ uint32_t s_cnt[8];               // applications the workgroup has finished, per round (recycled every eight rounds)
    __shared__ uint32_t s_round[kWorkerWaves];  // rounds each wavefront has finished
    __shared__ unsigned long long s_next[8];    // (round << 32) | applications of that round handed out so far (kRecords)
    // group 0 of the chunk index: lane l = chunk l (maxima x 3, dcand, xcand)
    __shared__ unsigned long long s_g0[5][kWave];
    // NARROW (tightly-pack): a wavefront decides an application in the snapshot's scaled int32 domain (NarrowView, NarrowApp:
    // 12 bytes per slot, 32-bit compares, capacities by multiplication, a four-dword gather) when the snapshot has that form
    // and the application's requests do (scale_record) — wave-uniform per application; otherwise on the int64 path, as the
    // other instances always do.  Gangs of gpu executors take the int64 path (the compact SparseTable has wide columns only)
    // until their shape has a row: then they are decided from it, on the narrow path, like any other (SHAPE ROWS).
    constexpr bool kNarrow = ALGO == GF_ALGO_TIGHTLY_PACK;
    __shared__ int32_t s_g0n[kNarrow ? 3 : 1][kWave];  // the three maxima of s_g0 in units (upper bounds: rounded up)
    // SHAPE ROWS (gangfit_worker_rows.h): the product instance only — the counting instance keeps the launch path's counters, which
    // a decision served from a row would not add to.  Directory word and key per entry, then the rows as three columns of 64.
    constexpr bool kRowsOn = WHICH == (int)GF_ALGO_TIGHTLY_PACK;
    constexpr uint32_t kRowsN = kRowsOn ? rows::kRows : 1u;
    // (ONE object, and every access below through a lane index made new where it stands — GF_HERE —: a lane's words are one address
    //  register plus immediate offsets, computed at the use; as separate arrays indexed by `lane` their addresses were hoisted out
    //  of the round loop into VGPRs held through every decision: 107 VGPRs against the budget of 104; 104 this way)
    struct RowsLds {
        uint32_t dir[kWave];
        int32_t key[3][kWave];
        uint32_t slot[kRowsN][kWave];
        uint32_t node[kRowsN][kWave];
        int32_t cap[kRowsN][kWave];
    };
    __shared__ RowsLds s_rows[1];
    __shared__ unsigned long long s_row_stat[3];  // rows built, decisions served from a row, decisions that looked up and fell back
    __shared__ uint32_t s_left;                   // wavefronts of the workgroup that have left (the last one flushes s_row_stat)
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (blockIdx.x == 0) {
        // ------------------------------------------------------------------------------------------ the leader
        if (wave != 0) return;
        unsigned long long consumed = W.first_ticket;
        unsigned long long last = wall_clock64();
        if (lane == 0) sys_store(&W.host->state, 1ull);
        for (;;) {
            // the doorbell and the stop word travel together: one round trip over the host link per look, not two
            const unsigned long long posted = sys_load(&W.host->posted);
            const unsigned long long stop = sys_load(&W.host->stop);
            if (posted > consumed) {
                // up to thirty-two tickets per round trip over the host link: lane l copies word l & 7 of tickets
                // consumed + (l >> 3) + 8 q, q = 0..3 — the four requests leave before the first answer is waited for
                while (consumed < posted) {
                    unsigned long long w4[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const unsigned long long t = consumed + (unsigned long long)(lane >> 3) + 8ull * (unsigned long long)q;
                        w4[q] = 0;
                        if (t < posted)
                            w4[q] = sys_load(reinterpret_cast<const unsigned long long*>(&W.host->ring[(uint32_t)(t % kWorkerRing)]) + (lane & 7));
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const unsigned long long t = consumed + (unsigned long long)(lane >> 3) + 8ull * (unsigned long long)q;
                        if (t < posted)
                            __hip_atomic_store(reinterpret_cast<unsigned long long*>(&W.dev->ring[(uint32_t)(t % kWorkerRing)]) + (lane & 7), w4[q],
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    const unsigned long long step = posted - consumed < 32ull ? posted - consumed : 32ull;
                    consumed += step;
                }
                last = wall_clock64();
                continue;
            }
            // leave: on request, when the host said "after ticket N" and N has been relayed (at launch: leave_after; later: the
            // stop word), or for lack of work
            if (stop == 1ull || (stop >= 2ull && consumed >= stop - 2ull) || (W.leave_after != 0ull && consumed >= W.leave_after) ||
                wall_clock64() - last > W.idle_ticks) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every ticket word is out before the quit word
                if (lane == 0) {
                    __hip_atomic_store(&W.dev->quit, W.generation, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    sys_store(&W.host->consumed, consumed);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0) sys_store(&W.host->state, 2ull);
                return;
            }
            __builtin_amdgcn_s_sleep(8);
        }
    }
    // ---------------------------------------------------------------------------------------------- the sets
    // EVERY WAVEFRONT ON ITS OWN (round 6).  Rounds 3-5 ran a workgroup in lock step: wavefront 0 probed for the set's next ticket,
    // a barrier published it, sixteen wavefronts decided their applications, drained their stores and met again — and the
    // instrumented build (profiles/r6e_worker_phases.txt) showed 45 % of a 31.6 k-cycle round outside the decisions: 6.7 k at the
    // barrier behind the slowest wavefront and the probe, 2.3 k for the records' round trip, 2.2 k + 2.2 k for the probe and the
    // drain, all of them with the CU's SIMDs idle because every wavefront was in the same phase.  Now nothing in a round waits for
    // another wavefront: each one reads the ticket itself (lane l < 6 = word l; the words validate themselves), requests the set's
    // NEXT ticket when its round begins and — when that ticket has arrived by the round's end — the next round's records BEFORE it
    // drains its stores, so that one wait covers both; a ticket's completion is counted in an LDS word per round, and the wavefront
    // whose share completes the workgroup's adds it to the ticket's counter in device memory.  Wavefronts of a workgroup drift
    // apart by whole rounds; eight count words are recycled, guarded by the rounds the wavefronts publish.
    const uint32_t b = blockIdx.x - 1u;
    const uint32_t set = b / W.blocks_per_set, bs = b % W.blocks_per_set;
    const uint32_t app_stride = W.blocks_per_set * kWorkerWaves;
    const rounds::StrideDiv sdiv{W.stride_mul, W.stride_shift};  // x / app_stride without a division (gangfit_worker_rounds.h)
    // the first ticket of this set at or behind first_ticket
    unsigned long long t = W.first_ticket + (unsigned long long)((set + W.sets - (uint32_t)(W.first_ticket % W.sets)) % W.sets);
    GlobalView V{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks, T.xmask, T.dmask,
                 T.n_chunks};
    Orders O{T.slot_node, T.dslot, T.n_x, T.n_d, T.d_identity != 0};
    const bool merged = T.d_identity != 0 && kInner != GF_ALGO_MINIMAL_FRAGMENTATION;
    constexpr uint32_t kCountSlots = 8;
    constexpr uint32_t kRoundGone = 0xFFFFFFFFu;  // s_round of a wavefront that has left
    if (threadIdx.x < kCountSlots) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 8) s_next[threadIdx.x] = 0ull;
    if (threadIdx.x < (uint32_t)kWorkerWaves) s_round[threadIdx.x] = 0;
    if constexpr (kRowsOn) {
        if (threadIdx.x < kRowsN) s_rows[0].dir[threadIdx.x] = rows::kEmpty;
        if (threadIdx.x < 3) s_row_stat[threadIdx.x] = 0ull;
        if (threadIdx.x == 0) s_left = 0u;
    }
    const bool narrow_table = kNarrow && T.nquad != nullptr;
    // SHAPE ROWS are looked up by a resident worker and by a bounded stream of at least kRowSightings rounds per set.  A shorter
    // launch shows a workgroup no shape often enough to build a row that pays back — a window of twenty tickets is two rounds — and
    // would pay the probe and the sighting of every decision for nothing (measured: 414.9 against 437.8 M decisions/s, medians of
    // seven, before this condition).  Merged layout only (the driver step of a row decision is the merged one).
    // (per wavefront, and switched off for good by a wavefront that finds the directory full before its workgroup has built any row:
    //  a queue whose shapes do not repeat would otherwise pay the probe for every decision — measured on a stream of 2 000 tickets in
    //  which every record has its own executor request: 960 against 1 032 M decisions/s, medians, before this guard)
    bool rows_live = kRowsOn && merged &&
                           (W.leave_after == 0ull || W.leave_after - W.first_ticket >= (unsigned long long)rows::kRowSightings * W.sets);
    if (wave == 0) {  // the tables do not change while the worker lives
        const Group0 g = load_group0(V, O, lane);
        s_g0[0][lane] = (unsigned long long)g.m0;
        s_g0[1][lane] = (unsigned long long)g.m1;
        s_g0[2][lane] = (unsigned long long)g.m2;
        s_g0[3][lane] = g.dcand;
        s_g0[4][lane] = g.xcand;
        if constexpr (kNarrow) {
            if (narrow_table) {
                s_g0n[0][lane] = NarrowView::scale_max(g.m0, T.nunit[0]);
                s_g0n[1][lane] = NarrowView::scale_max(g.m1, T.nunit[1]);
                s_g0n[2][lane] = NarrowView::scale_max(g.m2, T.nunit[2]);
            }
        }
    }
    // (the wide maxima and the units are no members of the narrow view: OPERANDS above)
    const NarrowView VN(InWorkerKernel{}, T.nquad, T.xmask, T.dmask, T.n_chunks);
    // lane l < 6 scales request word l of a record: dimension l mod 3
    const int64_t unit_l = T.nunit[lane % 3 == 0 ? 0 : (lane % 3 == 1 ? 1 : 2)];
    const double rcp_l = kNarrow ? fast_rcp((double)unit_l) : 0.0;
    __syncthreads();  // the only barrier of the kernel: the LDS words above
    // NARROW: this lane's group 0 in units stays in registers (seven) — it is the same for every application while the worker lives,
    // and reading it back per application put five LDS reads and their wait at the head of every decision.  (The int64 path keeps
    // the LDS words: ten registers more would not fit the budget.)
    constexpr bool kG0Regs = kNarrow;
    Group0T<int32_t> g0n_regs{};
    if constexpr (kG0Regs) {
        if (narrow_table) {
            g0n_regs.m0 = s_g0n[0][lane];
            g0n_regs.m1 = s_g0n[1][lane];
            g0n_regs.m2 = s_g0n[2][lane];
            g0n_regs.dcand = s_g0[3][lane];
            g0n_regs.xcand = s_g0[4][lane];
        }
    }
    typedef __attribute__((address_space(1))) const gf_app glb_app;
    typedef __attribute__((address_space(1))) gf_result glb_result;
    typedef __attribute__((address_space(1))) uint32_t glb_u32w;
    constexpr unsigned long long kPtrMask = 0x0000FFFFFFFFFFFFull;
    constexpr bool kRecords = ALGO != GF_ALGO_MINIMAL_FRAGMENTATION;  // (that instance is at its register budget)
    // the six words of ticket tt as they are now (lane l < 6: word l), and whether they are that ticket's
    auto load_words = [&](unsigned long long tt) {
        const unsigned long long* line = reinterpret_cast<const unsigned long long*>(&W.dev->ring[(uint32_t)(tt % kWorkerRing)]);
        unsigned long long w = 0;
        if (lane < 6) w = __hip_atomic_load(line + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return w;
    };
    auto words_valid = [&](unsigned long long w, unsigned long long tt) {
        const bool ok = lane >= 6 || (lane == 0 ? w == tt + 1ull : (w >> 48) == worker_tag(tt));
        return __ballot(ok) == ~0ull;
    };
    // kRecords: the next application of round r of this workgroup (its i-th: wave-uniform).  The counter word carries the round
    // it counts for: the first wavefront to arrive in a round turns the word over (compare-and-swap), nobody ever resets it.
    // ONE LDS operation on the common path: the fetch-and-add comes first and stands when the word it returns carries round r
    // (the word cannot turn over under a wavefront of round r: nobody is eight rounds ahead).  A word that carries another round
    // is a stale one — of round r - 8 k, or the zero of the start — and the add has left a stray increment in it.  That is
    // harmless: the caller has passed round_guard(r), so every wavefront of the workgroup has left round r - 8 and all before it —
    // nobody reads that count any more —, no wavefront can be in round r + 8 before this one has finished round r, and the
    // turn-over below replaces the whole word, strays included.  A compare-and-swap that fails has lost either to another
    // stray (try again) or to the turn-over (the word is round r's now: add).
    auto grab = [&](uint32_t r) {
        uint32_t got = 0;
        if (lane == 0) {
            unsigned long long* word = (unsigned long long*)&s_next[r % 8u];
            unsigned long long w = __hip_atomic_fetch_add(word, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            got = (uint32_t)w;
            if (__builtin_expect((uint32_t)(w >> 32) != r, 0)) {
                w += 1ull;  // (what this wavefront left there)
                for (;;) {
                    if ((uint32_t)(w >> 32) == r) {
                        w = __hip_atomic_fetch_add(word, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        got = (uint32_t)w;
                        break;
                    }
                    const unsigned long long fresh = ((unsigned long long)r << 32) | 1ull;
                    if (__hip_atomic_compare_exchange_strong(word, &w, fresh, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                        got = 0;
                        break;
                    }
                }
            }
        }
        return (uint32_t)__builtin_amdgcn_readfirstlane(got);
    };
    auto load_record = [&](const gf_app* apps_, uint32_t a) {  // lanes 0..7: the eight words of record a
        unsigned long long r = 0;
        if (lane < 8) r = sys_load(reinterpret_cast<const unsigned long long*>(apps_ + a) + lane);
        return r;
    };
    // every wavefront of the workgroup has left round r - 8 behind (the LDS words of round r are free)
    auto round_guard = [&](uint32_t r) {
        if (r < kCountSlots) return;
        for (;;) {
            const uint32_t x = lane < kWorkerWaves ? __hip_atomic_load(&s_round[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : kRoundGone;
            if (__ballot(x != kRoundGone && x + kCountSlots <= r) == 0ull) break;
            __builtin_amdgcn_s_sleep(4);
        }
    };
    uint32_t i_cur = 0;  // kRecords: the application grabbed for the start of this round (with its record in wrec), if grabbed_cur
    bool grabbed_cur = false;
    unsigned long long w_cur = 0;
    bool have_cur = false;
    {   // the set's first ticket, if the launch brought it along: read from the argument segment HERE, once
        const unsigned long long rel = t - W.first_ticket;
        if (rel < (unsigned long long)W.n_inline) {
            if (lane < 6) w_cur = W.inline_words[rel][lane];
            have_cur = true;
        }
    }
    unsigned long long wrec = 0;  // the record of the application in hand (kRecords)
    uint32_t round = 0;
    // What a round needs of its ticket to hand applications out, extracted ONCE per ticket: by the round before (kRecords, when the
    // ticket had arrived by then: grabbed_cur) or at the round's top (a ticket probed for, brought along by the launch, and every
    // ticket of the minimal-fragmentation instance).  bsr: the workgroup this one acts as in the round — it rotates, see below.
    const gf_app* apps = nullptr;
    uint64_t w5 = 0;    // n_apps | flags << 32
    uint32_t rows = 0;  // rows of the workgroup's first lane (rounds::rows_of)
    uint32_t bsr = bs;
    for (;;) {
        // ---- the ticket: brought along by the launch, requested a round ago, or probed for now
        if (W.leave_after != 0ull && t >= W.leave_after) break;  // a bounded stream: nothing behind its last ticket will come
        if (!have_cur) {
            bool quit_seen = false, gone = false;
            for (;;) {
                w_cur = load_words(t);
                if (words_valid(w_cur, t)) break;
                if (quit_seen) {  // (one more probe after the quit word was seen: the leader left before ticket t)
                    gone = true;
                    break;
                }
                quit_seen = __hip_atomic_load(&W.dev->quit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == W.generation;
                if (!quit_seen) __builtin_amdgcn_s_sleep(16);
            }
            if (gone) break;  // every round this wavefront finished has been counted when it finished
        }
        // (a ticket's pointers name global memory — device or mapped pinned host memory —: said so, or every access through
        //  them is a flat instruction that counts against both wait counters)
        if (!grabbed_cur) {
            apps = (const gf_app*)reinterpret_cast<glb_app*>((uint64_t)read_lane((int64_t)w_cur, 1) & kPtrMask);
            w5 = (uint64_t)read_lane((int64_t)w_cur, 5);
            rows = rounds::rows_of((uint32_t)(w5 & 0xFFFFFFFFull), rounds::first_app(bsr), sdiv);
        }
        gf_result* results = (gf_result*)reinterpret_cast<glb_result*>((uint64_t)read_lane((int64_t)w_cur, 2) & kPtrMask);
        uint32_t* exec_nodes = (uint32_t*)reinterpret_cast<glb_u32w*>((uint64_t)read_lane((int64_t)w_cur, 3) & kPtrMask);
        const unsigned long long half = ((uint64_t)read_lane((int64_t)w_cur, 4) & kPtrMask) + 1ull;
        const uint32_t n_apps = (uint32_t)(w5 & 0xFFFFFFFFull);
        const uint32_t slot = (uint32_t)(t % kWorkerRing);
        // Which applications of the ticket this wavefront takes ROTATES with the ticket: workgroup bs acts as workgroup
        // (bs + round) mod blocks_per_set, wavefront w as wavefront (w + round) mod 16.  A caller that posts the same queue again
        // and again (bench.py does; a scan over instance groups does not) would otherwise hand the same wavefront the heaviest
        // applications every time, and — a ticket is complete when its slowest wavefront is, the ring admits ticket t + 64 when
        // ticket t is complete — the whole stream would run at that wavefront's pace (profiles/r6g_worker_async_phases_static_mapping.txt:
        // rounds of 20 k cycles, then 13 k waiting for the next ticket).  (bsr advances by one per round and wraps by compare.)
        const uint32_t first_app = rounds::first_app(bsr) + rounds::wave_of_round(wave, round);
        // the count words are recycled every kCountSlots rounds: not before every wavefront of the workgroup has left the round
        // that used this one (it practically never waits: the wavefronts serve the same tickets at the same pace)
        round_guard(round);
        // kRecords: the workgroup's applications of this ticket are i = 0 .. total - 1, application (i mod 16) of row (i div 16)
        const uint32_t f0 = rounds::first_app(bsr);
        const uint32_t total = rounds::total_of(rows);
        auto app_index = [&](uint32_t i) { return rounds::app_index(f0, i, app_stride); };
        if constexpr (kRecords) {
            if (!grabbed_cur) {
                i_cur = grab(round);
                if (i_cur < total && app_index(i_cur) < n_apps) wrec = load_record(apps, app_index(i_cur));
            }
        }
        // the set's next ticket, for the end of this round
        // (Measured and removed, profiles/r6i_worker_mailbox_not_kept.txt: ONE wavefront per workgroup asking device memory and
        //  leaving the words in an LDS mailbox for the other fifteen — no faster: sixteen times the probes of rounds 3-5 on the
        //  same lines are not what a stream of tickets waits for.)
        const unsigned long long w_next = load_words(t + W.sets);
        // per slot: the placements as the wave-level code writes (and, distribute-evenly, re-reads) them, then its two
        // survivor lists — all private to this launch; the caller's arrays only see write-through stores
        uint32_t* priv = W.scratch + (size_t)slot * 3 * W.scratch_stride;
        uint32_t* scratch = priv + W.scratch_stride;
        // device-resident destination (gf_worker_submit_dev without GF_WORKER_HOST_OUTPUTS): the run emission itself writes
        // through; a destination in pinned host memory keeps the private slice and the coalesced copy-out (lone dwords over
        // the host link cost more than the read-back)
        const bool direct = ALGO == GF_ALGO_TIGHTLY_PACK && ((w5 >> 32) & 1ull) == 0;
        uint32_t mine = 0;
        for (uint32_t a = kRecords ? app_index(i_cur) : first_app; kRecords ? i_cur < total : a < n_apps;
             a = kRecords ? a : a + app_stride) {
            if constexpr (kRecords) {
                if (a >= n_apps) {  // (the last row is ragged)
                    i_cur = grab(round);
                    a = app_index(i_cur);
                    if (i_cur < total && a < n_apps) wrec = load_record(apps, a);
                    continue;
                }
            }
            unsigned long long xvis = 0, dvis = 0;
            Decision dec;
            int32_t app_k = 0;
            uint64_t app_off = 0;
            bool decided = false;
            int build_row = -1;  // SHAPE ROWS: the directory entry whose row this wavefront builds behind its decision
            const uint32_t* placed = nullptr;  // kZoned: the winner's placement, slot ids
            if constexpr (kNarrow) {
                NarrowApp napp;
                // (gangs of gpu executors are packed from the compact table of gpu nodes: wave_decide's `sparse`, int64 only)
                // (asked in this order, the sparse view's size is wanted only for a gang of gpu executors — and read there, from the
                //  argument segment: OPERANDS)
                auto sparse_serves = [&]() { return worker_kernargs_here()->G.n_x != 0u && O.d_identity; };
                if (narrow_table && scale_record(wrec, lane, unit_l, rcp_l, napp)) {
                if constexpr (kRowsOn) {
                    // SHAPE ROWS: one lane-parallel probe of the directory (lane l = entry l), then by the entry's word — READY: the
                    // row decides, or says nothing and the decision below runs as ever; COUNTING: one sighting, and the wavefront
                    // whose sighting is the kRowSightings-th builds the row behind its own decision; BUILDING: "not there"; no entry:
                    // one attempt to claim an empty one.  Nothing here waits for another wavefront.  Gangs of gpu executors included.
                    if (rows_live && napp.k > 0) {
                        RowsLds& R = s_rows[0];
                        int rl = lane;
                        GF_HERE(rl);
                        uint32_t st = rows::kEmpty;
                        bool same = false;
                        if ((uint32_t)rl < kRowsN) {
                            st = __hip_atomic_load(&R.dir[rl], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                            // (the three key words requested together, compared without short cuts: one LDS wait, not three)
                            const int32_t k0 = R.key[0][rl], k1 = R.key[1][rl], k2 = R.key[2][rl];
                            same = (bool)((int)rows::dir_has_key(st) & (int)(k0 == napp.exe0) & (int)(k1 == napp.exe1) & (int)(k2 == napp.exe2));
                        }
                        const uint64_t hit = __ballot(same);
                        bool served = false;
                        if (hit) {
                            const int e = __ffsll((unsigned long long)hit) - 1;
                            const uint32_t ste = read_lane(st, e);
                            if (rows::dir_ready(ste)) {
                                const RowDriver rd = wave_row_driver(VN, O, napp, g0n_regs, lane);
                                if (rd.found) {
                                    // the driver's slot keeps c_ds for this shape; every other entry is the row's (lanes behind the
                                    // row's count hold capacity 0 and a slot no driver has)
                                    const int32_t c_ds = read_lane(cap3(rd.d0 - napp.drv0, rd.d1 - napp.drv1, rd.d2 - napp.drv2, napp), rd.fl);
                                    const int32_t cp = rows::entry_cap(R.slot[e][rl], R.cap[e][rl], rd.ds, c_ds);
                                    const uint32_t node = R.node[e][rl];
                                    const int32_t incl = wave_inclusive_scan(cp);
                                    if (rows::served((int64_t)read_lane(incl, kWave - 1), napp.k)) {
                                        const int64_t start = (int64_t)(incl - cp);
                                        emit_runs((direct ? exec_nodes : priv) + napp.exec_off, start, rows::run_of(start, cp, napp.k), node,
                                                  lane, direct);
                                        app_k = napp.k;
                                        app_off = napp.exec_off;
                                        dec.feasible = true;
                                        dec.ds = rd.ds;
                                        dec.pass1 = 0;
                                        dec.ds_node = rd.node;
                                        decided = served = true;
                                    }
                                }
                            } else if (rows::dir_counting(ste)) {
                                uint32_t old = 0;
                                if (lane == 0) old = __hip_atomic_fetch_add(&R.dir[e], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                if (rows::dir_sighting_builds((uint32_t)__builtin_amdgcn_readfirstlane(old))) build_row = e;
                            }
                        } else {
                            const uint64_t empty = __ballot((uint32_t)rl < kRowsN && st == rows::kEmpty);
                            // (an entry whose key is still being written may be this very shape's: no second entry beside it —
                            //  the shape is seen again soon enough; so is the shape of a lost race)
                            const uint64_t claimed = __ballot(st == rows::kClaimed);
                            if (empty == 0ull && claimed == 0ull &&
                                __hip_atomic_load(&s_row_stat[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0ull)
                                rows_live = false;
                            if (empty != 0ull && claimed == 0ull && lane == 0) {
                                const int e = __ffsll((unsigned long long)empty) - 1;
                                uint32_t expect = rows::kEmpty;
                                if (__hip_atomic_compare_exchange_strong(&R.dir[e], &expect, rows::kClaimed, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                         __HIP_MEMORY_SCOPE_WORKGROUP)) {
                                    R.key[0][e] = napp.exe0;
                                    R.key[1][e] = napp.exe1;
                                    R.key[2][e] = napp.exe2;
                                    __hip_atomic_store(&R.dir[e], rows::kFirstSighting, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                                }
                            }
                        }
                        if (lane == 0)
                            __hip_atomic_fetch_add(&s_row_stat[served ? 1 : 2], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                if (!decided && !(napp.exe2 > 0 && napp.k > 0 && sparse_serves())) {
                    Group0T<int32_t> g0n = g0n_regs;
                    if constexpr (!kG0Regs) {
                        g0n.m0 = s_g0n[0][lane];
                        g0n.m1 = s_g0n[1][lane];
                        g0n.m2 = s_g0n[2][lane];
                        g0n.dcand = s_g0[3][lane];
                        g0n.xcand = s_g0[4][lane];
                    }
                    app_k = napp.k;
                    app_off = napp.exec_off;
                    dec = wave_decide<ALGO, NarrowView, false>(VN, O, napp, (direct ? exec_nodes : priv) + app_off, scratch + app_off,
                                                               scratch + half + app_off, lane, xvis, dvis, &g0n, nullptr, direct);
                    // (a driver found behind the first chunk: its node id from its record, like every other id of this decision)
                    if (dec.feasible && dec.ds_node == GF_NO_NODE) dec.ds_node = VN.node_of(dec.ds);
                    decided = true;
                }
                }
            }
            if (__builtin_expect(!decided, !kNarrow)) {
                App app{};
                Group0 g0{};
                g0.m0 = (int64_t)s_g0[0][lane];
                g0.m1 = (int64_t)s_g0[1][lane];
                g0.m2 = (int64_t)s_g0[2][lane];
                g0.dcand = s_g0[3][lane];
                g0.xcand = s_g0[4][lane];
                if constexpr (kRecords) {
                    app = app_from_lanes(wrec);
                } else {
                    app = load_app_uncached(apps, a, lane);  // (waits for its load: everything issued before it has returned)
                }
                app_k = app.k;
                app_off = app.exec_off;
                if constexpr (kZoned) {
                    dec = wave_decide_zones<ALGO == GF_ALGO_AZ_AWARE_TIGHTLY_PACK>(T, G, W.zones, W.sched, V, app, priv + app_off,
                                                                                   scratch + app_off, lane, xvis, dvis, placed);
                } else {
                    dec = wave_decide<kInner, GlobalView, false>(V, O, app, (direct ? exec_nodes : priv) + app_off, scratch + app_off,
                                                                 scratch + half + app_off, lane, xvis, dvis, merged ? &g0 : nullptr, &G,
                                                                 direct);
                }
            }
            if constexpr (COUNT) {
                if (W.stats != nullptr && lane == 0) {
                    atomicAdd(&W.stats->exec_slots_visited, xvis);
                    atomicAdd(&W.stats->driver_slots_visited, dvis);
                }
            }
            if (dec.feasible && !direct) {
                // this wavefront's own stores, read back through its CU's L1 / L2 and sent out write-through
                if constexpr (kZoned) {  // (this wavefront's own stores again, as below; slot ids -> node indices; K == 0 writes nothing)
                    for (int32_t i = lane; i < app_k; i += kWave)
                        __hip_atomic_store(exec_nodes + app_off + i, T.slot_node[placed[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                } else {
                    for (int32_t i = lane; i < app_k; i += kWave)
                        __hip_atomic_store(exec_nodes + app_off + i, priv[app_off + i], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
            if (lane < 2) {  // the 16-byte result as two write-through words
                if (dec.feasible && dec.ds_node == GF_NO_NODE) dec.ds_node = T.slot_node[dec.ds];
                const unsigned long long lo = (unsigned long long)(uint32_t)(dec.feasible ? 1 : 0) |
                                              ((unsigned long long)(dec.feasible ? dec.ds_node : GF_NO_NODE) << 32);
                const unsigned long long hi = (unsigned long long)(dec.feasible ? (uint32_t)app_k : 0u) | (1ull << 32);
                __hip_atomic_store(reinterpret_cast<unsigned long long*>(results + a) + lane, lane == 0 ? lo : hi, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
            }
            if constexpr (kRowsOn) {
                if (__builtin_expect(build_row >= 0, 0)) {
                    // BUILD: one scan of the narrow records over the executor order — chunk maxima and candidate words as skips —
                    // for this record's shape (scaled again from the record: nothing of it was kept across the decision), every
                    // qualifying lane writes its entry straight to row[fill + rank]; until 64 entries or the end of the order.
                    // Inline, not a call: a real call gives the kernel a stack (scratch) and the ABI's registers.
                    NarrowApp b;
                    (void)scale_record(wrec, lane, unit_l, rcp_l, b);
                    b.k = rows::kCapClamp;
                    RowsLds& R = s_rows[0];
                    int rl = lane;
                    GF_HERE(rl);
                    R.slot[build_row][rl] = GF_NO_NODE;  // (no driver has this slot; capacity 0)
                    R.node[build_row][rl] = GF_NO_NODE;
                    R.cap[build_row][rl] = 0;
                    const uint32_t xc = (O.n_x + kWave - 1) / kWave;
                    const uint64_t lt_mask = (1ull << lane) - 1ull;
                    uint32_t fill = 0;
                    for (uint32_t g = 0; g * kWave < xc && fill < rows::kRowLen; ++g) {
                        uint64_t cand;
                        uint64_t m = chunk_group_mask<false>(VN, g, xc, b.exe0, b.exe1, b.exe2, lane, cand);
                        while (m != 0ull && fill < rows::kRowLen) {
                            const int bit = __ffsll((unsigned long long)m) - 1;
                            const uint32_t c = g * kWave + (uint32_t)bit;
                            m &= m - 1;
                            const uint32_t j = c * kWave + lane;
                            const uint64_t in_m = (uint64_t)read_lane((int64_t)cand, bit) & low_lanes(chunk_len(O.n_x, c * kWave, kWave));
                            int32_t a0 = 0, a1 = 0, a2 = 0;
                            uint32_t node = 0;
                            if (lane_in(in_m)) VN.load(j, a0, a1, a2, node);
                            const uint64_t fm = ge3_mask(a0, a1, a2, b.exe0, b.exe1, b.exe2) & in_m;
                            const uint32_t pos = fill + (uint32_t)__popcll((unsigned long long)(fm & lt_mask));
                            if (lane_in(fm) && pos < rows::kRowLen) {
                                R.slot[build_row][pos] = j;
                                R.node[build_row][pos] = node;
                                R.cap[build_row][pos] = cap3(a0, a1, a2, b);
                            }
                            fill += (uint32_t)__popcll((unsigned long long)fm);
                        }
                    }
                    // every lane's entries are in LDS before the word says READY (readers: the acquire load of the probe)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    if (lane == 0) {
                        __hip_atomic_fetch_add(&s_row_stat[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_or(&R.dir[build_row], rows::kReadyBit, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
            ++mine;
            if constexpr (kRecords) {  // the next application of this round, whoever's it would have been
                i_cur = grab(round);
                a = app_index(i_cur);
                if (i_cur < total && a < n_apps) wrec = load_record(apps, a);
            }
        }
        // ---- the round's end.  The next ticket's words were requested when the round began: when they are that ticket's, its
        //      records are requested now, so that ONE wait covers them and this round's stores.
        const unsigned long long t_next = t + W.sets;
        const bool have_next = words_valid(w_next, t_next);
        unsigned long long wrec_next = 0;
        uint32_t i_next = 0;
        const uint32_t bsr_n = rounds::next_block(bsr, W.blocks_per_set);
        const gf_app* apps_n = nullptr;
        uint64_t w5_n = 0;
        uint32_t rows_n = 0;
        if (kRecords && have_next) {  // the first application of the next round and its record, before this round's stores are drained
            round_guard(round + 1u);
            // (the next round starts from what is extracted here: it does not read the words apart again)
            const uint32_t f0n = rounds::first_app(bsr_n);
            apps_n = (const gf_app*)reinterpret_cast<glb_app*>((uint64_t)read_lane((int64_t)w_next, 1) & kPtrMask);
            w5_n = (uint64_t)read_lane((int64_t)w_next, 5);
            const uint32_t n_apps_n = (uint32_t)(w5_n & 0xFFFFFFFFull);
            rows_n = rounds::rows_of(n_apps_n, f0n, sdiv);
            i_next = grab(round + 1u);
            const uint32_t a_n = rounds::app_index(f0n, i_next, app_stride);
            if (i_next < rounds::total_of(rows_n) && a_n < n_apps_n) wrec_next = load_record(apps_n, a_n);
        }
        // this round's stores acknowledged (and the next records in registers) before the round is counted
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // ---- completion.  The workgroup's applications of this ticket (lane j: first_j, first_j + stride, ...) in closed form
        {
            const uint32_t share = rounds::share_of(n_apps, f0, app_stride, rows);
            // (a wavefront without an application in this ticket adds nothing: its zero, arriving between the last share and the
            //  reset of the word, would complete the workgroup a second time)
            if (share != 0u && mine != 0u) {
                const uint32_t rs = round % kCountSlots;
                uint32_t old = 0;
                if (lane == 0) old = __hip_atomic_fetch_add(&s_cnt[rs], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                old = __builtin_amdgcn_readfirstlane(old);
                if (old + mine == share) {  // this wavefront's applications complete the workgroup's: the ticket's counter
                    uint32_t before = 0;
                    if (lane == 0) {
                        __hip_atomic_store(&s_cnt[rs], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        before = __hip_atomic_fetch_add(&W.dev->count[slot * kWorkerCountStride], share, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
                        if (before + share == n_apps) {  // ... and the workgroup's complete the ticket: the host is told
                            __hip_atomic_store(&W.dev->count[slot * kWorkerCountStride], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            sys_store(&W.host->done[slot], t + 1ull);
                        }
                    }
                }
            }
        }
        ++round;
        if (lane == 0) __hip_atomic_store(&s_round[wave], round, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (rounds left behind: round_guard)
        t = t_next;
        w_cur = w_next;
        have_cur = have_next;
        wrec = wrec_next;
        i_cur = i_next;
        grabbed_cur = kRecords && have_next;
        bsr = bsr_n;
        apps = apps_n;
        w5 = w5_n;
        rows = rows_n;
    }
    if (lane == 0) __hip_atomic_store(&s_round[wave], kRoundGone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // never in anybody's way
    if constexpr (kRowsOn) {  // the last wavefront to leave adds the workgroup's row counts to the context's totals, once
        uint32_t left = 0;
        if (lane == 0) left = __hip_atomic_fetch_add(&s_left, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((uint32_t)__builtin_amdgcn_readfirstlane(left) == (uint32_t)kWorkerWaves - 1u && lane < 3) {
            const unsigned long long n = __hip_atomic_load(&s_row_stat[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (n != 0ull) __hip_atomic_fetch_add(&W.dev->rows[lane], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

