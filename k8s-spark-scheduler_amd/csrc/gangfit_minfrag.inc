// gangfit_minfrag.inc — minimalFragmentation on one wavefront (included by gangfit_kernels.hip).
//
//   minimalFragmentation / internalMinimalFragmentation   LIB/binpack/minimal_fragmentation.go:59-137
//   GetNodeCapacities / FilterOutNodesWithoutCapacity      LIB/capacity/capacity.go:36-113
//
// Two forms of the same decision: the HISTOGRAM form (wave_minfrag_hist, further down: one pass in the snapshot's scaled int32
// domain counts the capacities, the walk is planned on the counts, one more pass emits the runs of gangs that need several nodes
// — what the independent batch runs where a caller lends LDS) and the WALK described next (a pass per question on the wide table:
// the chains' generic fallback, the resident worker, and whatever the histogram cannot hold).
//
// The reference stable-sorts (node, capacity) pairs by capacity and walks that list with binary searches.  Nothing is
// sorted here: the walk only ever asks three questions of the multiset of capacities, and each is a reduction over the
// executor order (64 slots per step, chunks the maxima index rules out are skipped — their capacity is 0, and
// FilterOutNodesWithoutCapacity drops those):
//   (1) "first node of the sorted list with capacity >= R" (sort.Search, :103-105)  = argmin over (capacity, position)
//       among unconsumed nodes with capacity >= R — the stable sort keeps equal capacities in priority order;
//   (2) "the maximum capacity m and the run of nodes that have it" (:113-116)        = max-reduction, then the nodes with
//       capacity == m in priority order; floor(R / m) of them are drained completely (:119-124);
//   (3) the list that remains (:130) = nodes with capacity below the last completely drained level.
// Levels are visited in descending order, so the state of the walk is two scalars (R executors still to place, the
// exclusive upper bound `lim` of capacities not yet drained) plus, after a partially drained level, the position of
// its first undrained node.  Capacities are exact unclamped 64-bit quotients (the order between two capacities above K
// decides which node receives the gang), math.MaxInt when the executor requests nothing in every dimension.
//
// Success of internalMinimalFragmentation on a list L  <=>  sum of capacities over L >= K  (every step either finishes
// or drains whole nodes, and never places more than K), so feasibility — and with it the O(N) driver choice of
// wave_decide / wave_fallback — is the same predicate as for tightly-pack, and the "avoid mostly empty nodes" attempt
// (:68-78) is decided by one clamped sum over {0 < capacity < target} before anything is emitted.

constexpr int64_t kCapInf = INT64_MAX;  // math.MaxInt on a 64-bit Go build (capacity.go:42-45)

// getCapacityAgainstSingleDimension (capacity.go:36-56) on a = available - reserved: the exact UNCLAMPED quotient.
// rcp = the application's reciprocal of e (App::rcp*: fast_rcp or an IEEE division, relative error below 2^-44 with the
// two int64 -> f64 conversions and the product).  An estimate below 2^40 is therefore within 2^-4 of a / e, its truncation
// within one of floor(a / e), and one exact multiply-subtract settles it — the same argument as cap_dim, without the clamp
// (q * e <= a + e < 2^63: no overflow).  Anything larger (a byte-sized request against terabytes) takes the compiler's 64-bit
// division, ~150 instructions; every pass of minimal-fragmentation over the order used to pay that for every slot and
// dimension.  gf_selftest checks both branches against the plain division on the device.
__device__ __forceinline__ int64_t cap_dim_full(int64_t a, int64_t e, double rcp) {
    if (a < 0) return 0;         // reserved > available
    if (e == 0) return kCapInf;  // wave-uniform
    const double qf = (double)a * rcp;
    if (qf < 1099511627776.0) {  // 2^40
        int64_t q = (int64_t)qf;  // qf >= 0: truncation == floor
        const int64_t rem = a - q * e;
        if (rem < 0)
            q -= 1;
        else if (rem >= e)
            q += 1;
        return q;
    }
    return a / e;  // a >= 0, e > 0: truncation == floor
}

__device__ __forceinline__ int64_t wave_min_i64(int64_t v) { return -wave_max_i64(-v); }  // callers keep v > INT64_MIN

// Sum over the wave of non-negative per-lane values, wave-uniform.  An int32 scan: the TOTAL must stay below 2^31.  The callers
// pass partial sums saturated at K <= 2^20 (64 lanes: below 2^27), how many nodes a part of the order gives (its slots at
// most) and, unsaturated, the capacity sum of a count row (shard_mf_counts_kernel: below 2^24 for the whole wave, possibly all
// of it in one lane).  tests/test_gpu_sharded_minfrag.py::test_range_of_1023_and_1024_chunks holds the largest of each: K = 2^20
// against 130 944 nodes, ranges of 65 472 nodes, and 65 472 x 255.
__device__ __forceinline__ int64_t wave_sum_small(int64_t v) {
    return (int64_t)read_lane(wave_inclusive_scan((int32_t)v), kWave - 1);
}

// GetNodeCapacity of executor-order slot j with the driver reserved on slot ds; 0 for non-candidates.
// From values already loaded: cand = the slot is an executor candidate of the order.
__device__ __forceinline__ int64_t mf_cap_of(bool cand, int64_t a0, int64_t a1, int64_t a2, const App& app, uint32_t ds, uint32_t j) {
    if (!cand) return 0;
    if (j == ds) {
        a0 -= app.drv0;
        a1 -= app.drv1;
        a2 -= app.drv2;
    }
    if (!cap_ge1(a0, a1, a2, app)) return 0;  // capacity 0 without dividing
    const int64_t c = cap_dim_full(a0, app.exe0, app.rcp0), m = cap_dim_full(a1, app.exe1, app.rcp1), g = cap_dim_full(a2, app.exe2, app.rcp2);
    const int64_t cm = c < m ? c : m;
    return cm < g ? cm : g;
}
template <class View>
__device__ __forceinline__ int64_t mf_cap(const View& V, const Orders& O, const App& app, uint32_t ds, uint32_t j) {
    int64_t a0, a1, a2;
    const bool cand = load_with_cand<false>(V, j, O.n_x, a0, a1, a2);
    return mf_cap_of(cand, a0, a1, a2, app, ds, j);
}

// f(j, capacity) for every executor-order slot whose chunk the maxima index cannot rule out, 64 slots per call, in
// priority order.  f returns false (wave-uniformly) to stop the walk.
// A pass is a chain of dependent round trips — candidate word and values of a chunk, then the next chunk —, and a wavefront
// of the one-launch batch spent 19 cycles per instruction waiting for them (profiles/r5c_summary.md: 322 us for 122 M
// instructions).  The walk therefore requests up to kMfAhead candidate chunks at once and hands them to f in order; a walk that
// f stops early has requested at most kMfAhead - 1 chunks it did not need.
constexpr int kMfAhead = 4;  // (8 measured: profiles/r5ar_minfrag_ahead8.txt)
template <class View, class F>
__device__ __forceinline__ void mf_for_each_chunk(const View& V, const Orders& O, const App& app, uint32_t ds, int lane,
                                                  F f) {
    const uint32_t xc = (O.n_x + kWave - 1) / kWave;
    for (uint32_t g = 0; g * kWave < xc; ++g) {
        uint64_t m = chunk_group_mask<false>(V, g, xc, app.exe0, app.exe1, app.exe2, lane);
        while (m) {
            uint32_t j[kMfAhead];
            int64_t a0[kMfAhead], a1[kMfAhead], a2[kMfAhead];
            uint64_t xw[kMfAhead];  // the chunk's candidate word as loaded (its bit is looked at in the work phase: see the scaled walk below)
            int n = 0;  // wave-uniform
#pragma unroll
            for (int t = 0; t < kMfAhead; ++t) {
                j[t] = 0;
                xw[t] = 0;
                a0[t] = a1[t] = a2[t] = 0;
                if (m) {
                    const uint32_t c = g * kWave + (uint32_t)(__ffsll((unsigned long long)m) - 1);
                    m &= m - 1;
                    j[t] = c * kWave + lane;
                    // (not load_with_cand: its register pins would make every request wait for the one before it)
                    V.load(j[t] < O.n_x ? j[t] : O.n_x - 1u, a0[t], a1[t], a2[t]);
                    xw[t] = V.chunk_xmask(c);
                    n = t + 1;
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // all requests first (nothing of the work below is scheduled between them) ...
#pragma unroll
            for (int t = 0; t < kMfAhead; ++t)
                if (t < n) {
                    const bool cand = j[t] < O.n_x && ((xw[t] >> lane) & 1ull);
                    if (!f(j[t], mf_cap_of(cand, a0[t], a1[t], a2[t], app, ds, j[t]))) return;  // ... then the work, in order
                }
        }
    }
}

struct MfProbe {
    int64_t max_cap;   // maximum capacity among the admitted nodes (0: none)
    bool found;        // a node with capacity >= need exists among them
    uint32_t best;     // ... the first of the smallest such capacity, in priority order
};

// One pass over the admitted nodes {0 < capacity, capacity < lim unless !bounded}: questions (1) and (2) at once.
template <class View>
__device__ __forceinline__ MfProbe mf_probe(const View& V, const Orders& O, const App& app, uint32_t ds, int lane,
                                            bool bounded, int64_t lim, int64_t need) {
    int64_t lmax = 0, lbest = kCapInf;
    uint32_t lpos = GF_NO_NODE;
    mf_for_each_chunk(V, O, app, ds, lane, [&](uint32_t j, int64_t c) {
        if (c > 0 && (!bounded || c < lim)) {
            lmax = c > lmax ? c : lmax;
            if (c >= need && (lpos == GF_NO_NODE || c < lbest)) {  // strict <: the earlier position keeps ties
                lbest = c;
                lpos = j;
            }
        }
        return true;
    });
    MfProbe p;
    p.max_cap = wave_max_i64(lmax);
    p.found = __ballot(lpos != GF_NO_NODE) != 0;
    p.best = GF_NO_NODE;
    if (p.found) {
        const int64_t bc = wave_min_i64(lpos != GF_NO_NODE ? lbest : kCapInf);
        const bool mine = lpos != GF_NO_NODE && lbest == bc;
        p.best = (uint32_t)(-wave_max_i64(mine ? -(int64_t)lpos : INT64_MIN + 1));
    }
    return p;
}

// R copies of slot s at out[at, at + R)
template <bool SLOTS>
__device__ __forceinline__ void mf_emit_one(const Orders& O, uint32_t* __restrict__ out, int64_t at, int64_t R,
                                            uint32_t s, int lane) {
    const uint32_t id = SLOTS ? s : O.slot_node[s];
    for (int64_t i = lane; i < R; i += kWave) out[at + i] = id;
}

// ------------------------------------------------------------------------------------------------ histogram form
// The walk below (wave_minfrag) takes a pass over the whole executor order per QUESTION — the sum and the maximum, the "avoid
// mostly empty nodes" subset, every sort.Search, every level — and a pass evaluates three 64-bit quotients per slot: ~200
// instructions per 64-slot chunk, 157 chunks at 10 000 nodes, three passes for a gang that one node takes and one or two more per
// level for a gang that needs several (the slowest application of a 1 000-application batch took ~0.55 ms, and the launch with it).
// Everything those questions ask of the VALUES of the capacities is a question about the multiset of capacities — kept, as in the
// FIFO chain (gangfit_fifo_minfrag.inc), as a histogram: lane l holds bins 4l .. 4l+3 — and "where" is only ever "the first node
// with capacity v" (a second table, filled by the same pass) or "the first q nodes of level m" (ONE emission pass for all levels
// at once: the histogram already says how many nodes every level gives and where its runs start in the output).  So:
//   pass 1   capacity of every candidate slot -> count[c]++, first[c] = min(first[c], slot)          (LDS atomics, wavefront-private)
//   plan     S, the maximum, the subset rule, the first sort.Search; if no node takes the whole gang the level walk of
//            internalMinimalFragmentation (:93-137) on the histogram: per drained level {nodes taken, output offset}, and the node
//            that takes what is left (the first of a lower level, or the first undrained one of the last level)
//   pass 2   (gangs that need several nodes only) every slot of a drained level learns its rank among its level's nodes in priority
//            order (running count per level in LDS + its rank inside the chunk from ballots) and emits its run.
// Both passes run in the snapshot's scaled int32 domain (NodeTable::ncpu ..): a capacity is three multiply-highs (narrow_magic)
// instead of three 64-bit quotients.  Not applicable -> the walk: a request that is not a multiple of the table's units, a
// capacity of kMfHistBins or more somewhere (tiny requests, MaxInt), K = 0, no scaled table, no LDS lent (Orders::mf_hist).
struct MfNarrow {
    int32_t drv0, drv1, drv2, exe0, exe1, exe2;
    uint32_t mag0, mag1, mag2, sh0, sh1, sh2;
    uint32_t un0, un1, un2;  // 0x7FFFFFFF where the request's dimension is zero ("unlimited": math.MaxInt), else 0 — OR-ed into the quotient
};

// The application's requests in the table's units; false (wave-uniform) when one of them has no exact scaled form below 2^30.
__device__ __forceinline__ bool mf_narrow_app(const App& app, const Orders& O, MfNarrow& n) {
    const int64_t u0 = O.nunit0, u1 = O.nunit1, u2 = O.nunit2;
    const int64_t d0 = app.drv0 / u0, d1 = app.drv1 / u1, d2 = app.drv2 / u2;
    const int64_t e0 = app.exe0 / u0, e1 = app.exe1 / u1, e2 = app.exe2 / u2;
    const int64_t top = INT64_C(1) << 30;
    const bool ok = d0 * u0 == app.drv0 && d1 * u1 == app.drv1 && d2 * u2 == app.drv2 && e0 * u0 == app.exe0 && e1 * u1 == app.exe1 &&
                    e2 * u2 == app.exe2 && d0 < top && d1 < top && d2 < top && e0 < top && e1 < top && e2 < top;
    n.drv0 = (int32_t)d0;
    n.drv1 = (int32_t)d1;
    n.drv2 = (int32_t)d2;
    n.exe0 = ok ? (int32_t)e0 : 0;
    n.exe1 = ok ? (int32_t)e1 : 0;
    n.exe2 = ok ? (int32_t)e2 : 0;
    narrow_magic(n.exe0, n.mag0, n.sh0);
    narrow_magic(n.exe1, n.mag1, n.sh1);
    narrow_magic(n.exe2, n.mag2, n.sh2);
    n.un0 = n.exe0 == 0 ? 0x7FFFFFFFu : 0u;  // (narrow_magic leaves multiplier 0 for a zero request: the quotient is 0 | un)
    n.un1 = n.exe1 == 0 ? 0x7FFFFFFFu : 0u;
    n.un2 = n.exe2 == 0 ? 0x7FFFFFFFu : 0u;
    return ok;
}

// getCapacityAgainstSingleDimension (capacity.go:36-56) in the scaled domain: |a| < 2^31, 0 <= e < 2^30; INT32_MAX for math.MaxInt.
// (no branch on e == 0: a conditional block costs the pass two execution-mask hand-overs per dimension and chunk)
__device__ __forceinline__ int32_t mf_ncap_dim(int32_t a, uint32_t un, uint32_t mag, uint32_t sh) {
    const int32_t q = (int32_t)((__umulhi(mag, (uint32_t)a << 1) >> sh) | un);
    return a < 0 ? 0 : q;
}
// GetNodeCapacity of slot j with the driver reserved on ds, from scaled values already loaded; 0 for non-candidates.
__device__ __forceinline__ int32_t mf_ncap_of(bool cand, int32_t a0, int32_t a1, int32_t a2, const MfNarrow& n, uint32_t ds, uint32_t j) {
    if (j == ds) {
        a0 -= n.drv0;
        a1 -= n.drv1;
        a2 -= n.drv2;
    }
    const int32_t c = mf_ncap_dim(a0, n.un0, n.mag0, n.sh0), m = mf_ncap_dim(a1, n.un1, n.mag1, n.sh1),
                  g = mf_ncap_dim(a2, n.un2, n.mag2, n.sh2);
    const int32_t cm = c < m ? c : m;
    return cand ? (cm < g ? cm : g) : 0;
}

constexpr int kMfAheadNarrow = 4;  // chunks of the scaled columns requested together
// mf_for_each_chunk on the scaled columns: f(j, capacity) for every slot of the chunks the maxima index cannot rule out.
// [c_lo, c_hi): the chunks of the order this wavefront walks (a TEAM of wavefronts shares one application: team_minfrag_hist).
template <class View, class F>
__device__ __forceinline__ void mf_for_each_chunk_narrow(const View& V, const Orders& O, const App& app, const MfNarrow& na, uint32_t ds,
                                                         int lane, F f, uint32_t c_lo = 0u, uint32_t c_hi = 0xFFFFFFFFu) {
    const uint32_t xc_all = (O.n_x + kWave - 1) / kWave;
    const uint32_t xc = xc_all < c_hi ? xc_all : c_hi;
    // the three column pointers as LANE values: as scalars they do not fit next to the pass's state and come back from their spill
    // lanes for every chunk (eight v_readlane per chunk request in the listing)
    const int32_t* pcpu = O.ncpu;
    const int32_t* pmem = O.nmem;
    const int32_t* pgpu = O.ngpu;
    GF_HERE(pcpu);
    GF_HERE(pmem);
    GF_HERE(pgpu);
    for (uint32_t g = c_lo / kWave; g * kWave < xc; ++g) {
        uint64_t m = chunk_group_mask<false>(V, g, xc, app.exe0, app.exe1, app.exe2, lane);
        if (g * kWave < c_lo) m &= ~low_lanes(c_lo - g * kWave);  // (the range's first group: chunks before c_lo are somebody else's)
        while (m) {
            uint32_t j[kMfAheadNarrow];
            int32_t a0[kMfAheadNarrow], a1[kMfAheadNarrow], a2[kMfAheadNarrow];
            uint64_t xw[kMfAheadNarrow];  // the chunk's candidate word, as loaded: its bit is looked at with the values, not before —
                                    // turned into a per-lane flag right here it made every chunk's requests wait for its own word
                                    // (s_waitcnt inside the request phase: four dependent round trips per batch instead of one)
            int n = 0;  // wave-uniform
#pragma unroll
            for (int t = 0; t < kMfAheadNarrow; ++t) {
                j[t] = 0;
                xw[t] = 0;
                a0[t] = a1[t] = a2[t] = 0;
                if (m) {
                    const uint32_t c = g * kWave + (uint32_t)(__ffsll((unsigned long long)m) - 1);
                    m &= m - 1;
                    j[t] = c * kWave + lane;
                    const uint32_t jj = j[t] < O.n_x ? j[t] : O.n_x - 1u;  // (no branch around the requests: the last chunk's spare lanes re-read its last slot)
                    a0[t] = pcpu[jj];
                    a1[t] = pmem[jj];
                    a2[t] = pgpu[jj];
                    xw[t] = V.chunk_xmask(c);
                    n = t + 1;
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // all requests first ...
#pragma unroll
            for (int t = 0; t < kMfAheadNarrow; ++t)
                if (t < n) {
                    const bool cand = j[t] < O.n_x && ((xw[t] >> lane) & 1ull);
                    if (!f(j[t], mf_ncap_of(cand, a0[t], a1[t], a2[t], na, ds, j[t]))) return;  // ... then the work, in order
                }
        }
    }
}

// the valid lanes that hold the same value (< 256) as this one: eight ballots
__device__ __forceinline__ uint64_t mf_peers8(uint32_t v, bool valid) {
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (v >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        peers &= bit ? bal : ~bal;
    }
    return peers;
}

// Pass 1's "who speaks for whom" by RUNS: a lane whose capacity differs from its predecessor's speaks for the lanes behind it that
// hold the same one (neighbours in the priority order mostly do) — a shift, a compare, a ballot and the distance to the next head
// instead of mf_peers8's eight ballots with their sixteen selects.  Equal capacities that are not neighbours speak separately (to the
// same bin: served one after the other).  Returns the lanes this one speaks for (0: it does not speak).
// (Counting by value with mf_peers8 for chunks of many short runs measured slower at every threshold: 6 / 12 / 24 runs gave
// 61.0 / 59.5 / 55.8 us per 1 000 applications, always by run 44.8 us — profiles/r6bf_minfrag_run_heads.txt.)
__device__ __forceinline__ uint32_t mf_run_heads(uint32_t v, bool valid, int lane) {
    const uint32_t key = valid ? v : 0x80000000u;
    uint32_t prev = (uint32_t)__shfl_up((int)key, 1, kWave);
    if (lane == 0) prev = ~key;
    const uint64_t heads = __ballot(key != prev);
    const uint64_t speakers = heads & __ballot(valid);
    const uint64_t rest = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
    const uint32_t len = rest ? (uint32_t)__ffsll((unsigned long long)rest) : (uint32_t)(kWave - lane);
    return ((speakers >> lane) & 1ull) ? len : 0u;
}

// Value of bin c (wave-uniform) from the per-lane registers (lane l holds bins 4l .. 4l+3).
__device__ __forceinline__ uint32_t mf_bin(const uint32_t (&v)[4], uint32_t c) {
    const uint32_t k = c & 3u;
    const uint32_t mine = k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3]));
    return read_lane(mine, (int)(c >> 2));
}

// minimalFragmentation in histogram form.  false: not applicable (a capacity of kMfHistBins or more somewhere) — nothing has been
// emitted, the caller takes the walk.  true: S = the clamped capacity total, and for S >= K out[0 .. K) holds the placements.
template <class View, bool SLOTS>
__device__ __forceinline__ bool wave_minfrag_hist(const View& V, const Orders& O, const App& app, const MfNarrow& na, uint32_t ds,
                                                  uint32_t* __restrict__ out, int lane, unsigned long long& visited, int64_t& S) {
    typedef uint32_t mf_u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) mf_u32x4 lds_mf4;
    const int64_t K = app.k;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    lds_u32* const A = O.mf_hist;             // pass 1: count per capacity; plan: nodes a level gives completely
    lds_u32* const B = A + kMfHistBins;       // pass 1: first slot per capacity; plan: where the level's runs start in out[]
    lds_u32* const C = A + 2 * kMfHistBins;   // pass 2: nodes of the level seen so far
    lds_mf4* const A4 = (lds_mf4*)A;
    lds_mf4* const B4 = (lds_mf4*)B;
    lds_mf4* const C4 = (lds_mf4*)C;
    A4[lane] = mf_u32x4{0u, 0u, 0u, 0u};
    B4[lane] = mf_u32x4{GF_NO_NODE, GF_NO_NODE, GF_NO_NODE, GF_NO_NODE};
    // The scaled requests and their multipliers as LANE values for the passes: they are wave-uniform, the compiler keeps them in
    // scalar registers, has none left and reloads every one of them from its spill lane at every use (nineteen v_readlane per
    // chunk of the pass); as vector operands they cost twelve registers and no instruction.
    MfNarrow nv = na;
    GF_HERE(nv.drv0);
    GF_HERE(nv.drv1);
    GF_HERE(nv.drv2);
    GF_HERE(nv.exe0);
    GF_HERE(nv.exe1);
    GF_HERE(nv.exe2);
    GF_HERE(nv.mag0);
    GF_HERE(nv.mag1);
    GF_HERE(nv.mag2);
    GF_HERE(nv.sh0);
    GF_HERE(nv.sh1);
    GF_HERE(nv.sh2);
    GF_HERE(nv.un0);
    GF_HERE(nv.un1);
    GF_HERE(nv.un2);
    int32_t cmax = 0;  // (the largest capacity seen: one comparison behind the pass instead of a branch per chunk)
    mf_for_each_chunk_narrow(V, O, app, nv, ds, lane, [&](uint32_t j, int32_t c) {
        cmax = c > cmax ? c : cmax;
        // the lanes that hold the same capacity speak through their first one (it also holds their smallest slot): neighbours in the
        // priority order have the same capacity more often than not, and same-address LDS atomics are served one lane at a time —
        // two of them per chunk kept the CU's LDS busy for ~120 cycles per chunk of ANY of its wavefronts (5.2 conflicts per active
        // LDS cycle in profiles/pmc_zoned.json): what the pass was bound by once four wavefronts per SIMD hid its latency
        const bool binned = c > 0 && c < kMfHistBins;
        const uint32_t n_run = mf_run_heads((uint32_t)c, binned, lane);
        if (n_run != 0u) {  // (a run's first lane holds its smallest slot)
            __hip_atomic_fetch_add(A + (uint32_t)c, n_run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_min(B + (uint32_t)c, j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        return true;
    });
    const bool big = cmax >= kMfHistBins;
    visited += O.n_x;
    if (__ballot(big) != 0ull) return false;
    const mf_u32x4 cnt4 = A4[lane], pos4 = B4[lane];  // (LDS operations of a wavefront execute in order)
    const uint32_t cn[4] = {cnt4.x, cnt4.y, cnt4.z, cnt4.w};
    const uint32_t fp[4] = {pos4.x, pos4.y, pos4.z, pos4.w};
    // ---- capacities, their clamped sum and maximum (capacity.go:78-113, minimal_fragmentation.go:64-67)
    int64_t lsum = 0, lmax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t c = 4 * lane + i, cc = c < K ? c : K;
        const int64_t add = (int64_t)cn[i] * cc;  // below 2^32 * 2^8
        lsum = lsum + add < K ? lsum + add : K;
        if (cn[i] != 0u) lmax = c;
    }
    S = wave_sum_small(lsum);
    if (S < K) return true;
    const int64_t max_cap = wave_max_i64(lmax);
    // ---- "avoid mostly empty nodes" (:68-78): the nodes below targetCapacity, if they can host the gang by themselves
    int64_t top = kMfHistBins;  // admitted: 0 < capacity < top
    if (K < max_cap) {
        const int64_t target = (K + max_cap) / 2;  // (max_cap < kMfHistBins: nothing wraps)
        int64_t lsub = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t c = 4 * lane + i, cc = c < K ? c : K;
            const int64_t add = c < target ? (int64_t)cn[i] * cc : 0;
            lsub = lsub + add < K ? lsub + add : K;
        }
        if (wave_sum_small(lsub) >= K) top = target;
    }
    // the smallest admitted capacity >= need (kCapInf: none) / the largest admitted capacity (0: none), levels below `below` only
    auto smallest_at_least = [&](int64_t need, int64_t below) {
        int64_t l = kCapInf;
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            const int64_t c = 4 * lane + i;
            if (cn[i] != 0u && c < below && c >= need) l = c;
        }
        return wave_min_i64(l);
    };
    auto largest_below = [&](int64_t below) {
        int64_t l = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t c = 4 * lane + i;
            if (cn[i] != 0u && c < below) l = c;
        }
        return wave_max_i64(l);
    };
    // ---- internalMinimalFragmentation (:93-137) on the admitted list; it succeeds by construction
    int64_t R = K;
    {
        const int64_t cf = smallest_at_least(R, top);  // :103-110 one node takes everything
        if (cf != kCapInf) {
            mf_emit_one<SLOTS>(O, out, 0, K, mf_bin(fp, (uint32_t)cf), lane);
            return true;
        }
    }
    // several nodes: the level walk on the histogram.  A level that is drained gets {nodes taken, output offset}.
    A4[lane] = mf_u32x4{0u, 0u, 0u, 0u};
    C4[lane] = mf_u32x4{0u, 0u, 0u, 0u};
    uint32_t n_runs = 0;       // nodes that emit a complete run of their level
    uint32_t last_pos = GF_NO_NODE;  // the node that takes what is left: known now (the first of its level) ...
    int64_t next_level = -1;         // ... or the first undrained node of this level (found by pass 2)
    uint32_t next_rank = 0;
    for (;;) {
        const int64_t m = largest_below(top);  // :113 (0 < m < R: no admitted node takes R)
        if (m <= 0) return true;               // unreachable when S >= K; guards against a non-terminating walk
        const uint32_t cnt = mf_bin(cn, (uint32_t)m);
        const uint32_t q = (uint32_t)R / (uint32_t)m;  // nodes of this level that can be drained completely (:120)
        const uint32_t drained = cnt < q ? cnt : q;
        A[(uint32_t)m] = drained;  // (every lane stores the same word)
        B[(uint32_t)m] = (uint32_t)(K - R);
        n_runs += drained;
        R -= (int64_t)drained * m;  // :123
        if (R == 0) break;          // :126-128
        if (drained < cnt) {
            // the level was not exhausted, so R < m: the next sort.Search (:103) finds the smallest capacity >= R among the
            // lower levels, else the first undrained node of this level
            const int64_t cf = smallest_at_least(R, m);
            if (cf != kCapInf) {
                last_pos = mf_bin(fp, (uint32_t)cf);
            } else {
                next_level = m;
                next_rank = drained;
            }
            break;
        }
        top = m;  // :130 the drained level leaves the list
        const int64_t cf = smallest_at_least(R, top);
        if (cf != kCapInf) {
            last_pos = mf_bin(fp, (uint32_t)cf);
            break;
        }
    }
    // ---- pass 2: the runs of the drained levels, every node by its rank among its level's nodes in priority order
    uint32_t left = n_runs + (next_level >= 0 ? 1u : 0u);
    if (left != 0u) {
        mf_for_each_chunk_narrow(V, O, app, nv, ds, lane, [&](uint32_t j, int32_t c) {
            const bool binned = c > 0 && c < kMfHistBins;
            // the level's three words requested together, for every lane (bin 0 is nobody's level: its words are zero) — read one
            // after the other, each behind the test of the one before, they were three LDS round trips per chunk
            const uint32_t cb = binned ? (uint32_t)c : 0u;
            const uint32_t take = A[cb], base = B[cb], seen = C[cb];
            const bool act = binned && (take != 0u || (int64_t)c == next_level);
            const uint64_t actm = __ballot(act);
            if (actm == 0ull) return true;
            const uint64_t peers = mf_peers8((uint32_t)c, act);
            const uint32_t rank = seen + (uint32_t)__popcll((unsigned long long)(peers & lt_mask));
            if (act && (peers & lt_mask) == 0ull) C[cb] = seen + (uint32_t)__popcll((unsigned long long)peers);  // the peers' leader
            const bool drain = act && rank < take;
            uint32_t id = j;
            if (!SLOTS && drain) id = O.slot_node[j];
            emit_runs(out, (int64_t)base + (int64_t)rank * c, drain ? c : 0, id, lane);  // :122
            const uint64_t nxt = __ballot(act && (int64_t)c == next_level && rank == next_rank);
            if (nxt) last_pos = read_lane(j, __ffsll((unsigned long long)nxt) - 1);
            left -= (uint32_t)__popcll((unsigned long long)__ballot(drain)) + (nxt ? 1u : 0u);
            return left != 0u;
        });
        visited += O.n_x;
    }
    if (R > 0 && last_pos != GF_NO_NODE) mf_emit_one<SLOTS>(O, out, K - R, R, last_pos, lane);  // (always found when S >= K)
    return true;
}

// The histogram form by a TEAM of wavefronts (round 6; fit_independent_kernel<minimal-fragmentation>: one workgroup = one
// application).  One wavefront per application left every SIMD with ONE wavefront walking 157 chunks of dependent latency
// (~1 100 cycles per chunk for ~50 instructions: profiles/r5bh_minfrag_pass_steps.txt) — the launch lasted as long as its slowest
// application's two passes.  Here every wavefront of the team runs the SAME decision code on the same application (the driver
// search, the plan: identical inputs, identical control flow), and only the two passes over the executor order are shared out:
// wavefront r walks the r-th quarter of the order's chunks,
//   pass 1   into its OWN count / first-slot rows (no atomics between wavefronts); behind ONE barrier everybody adds up the four
//            count rows (lane l = bins 4l .. 4l+3: four 16-byte reads), takes the minimum of the first-slot rows and keeps the sum of
//            the rows of the wavefronts before it — how many nodes of every capacity precede its quarter in priority order;
//   plan     by everybody, in registers, the level walk's {nodes taken, output offset} in its own rows;
//   pass 2   a node's rank among its level's nodes = that prefix + the running count over its own quarter: the quarters emit their
//            runs independently, and each stops when the nodes the plan wants from ITS quarter are out.
// A second barrier frees the rows for the plan (and for the next call: another driver candidate).  What one wavefront emits for
// everybody (a gang one node takes, the node that takes what is left when the plan names it) wavefront 0 emits.
// Bit-identical to wave_minfrag_hist by construction (same multiset, same first slots, same ranks).
template <class View, bool SLOTS>
__device__ __forceinline__ bool team_minfrag_hist(const View& V, const Orders& O, const App& app, const MfNarrow& na, uint32_t ds,
                                                  uint32_t* __restrict__ out, int lane, unsigned long long& visited, int64_t& S) {
    typedef uint32_t mf_u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) mf_u32x4 lds_mf4;
    const int64_t K = app.k;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    const uint32_t team = O.mf_team, rank = O.mf_rank;
    lds_u32* const A = O.mf_hist;             // OWN rows — pass 1: count per capacity; plan: nodes a level gives completely
    lds_u32* const B = A + kMfHistBins;       // pass 1: first slot per capacity; plan: where the level's runs start in out[]
    lds_u32* const C = A + 2 * kMfHistBins;   // pass 2: nodes of the level seen so far (starts at the prefix of the quarters before)
    lds_mf4* const A4 = (lds_mf4*)A;
    lds_mf4* const B4 = (lds_mf4*)B;
    lds_mf4* const C4 = (lds_mf4*)C;
    A4[lane] = mf_u32x4{0u, 0u, 0u, 0u};
    B4[lane] = mf_u32x4{GF_NO_NODE, GF_NO_NODE, GF_NO_NODE, GF_NO_NODE};
    MfNarrow nv = na;  // (as lane values: wave_minfrag_hist)
    GF_HERE(nv.drv0);
    GF_HERE(nv.drv1);
    GF_HERE(nv.drv2);
    GF_HERE(nv.exe0);
    GF_HERE(nv.exe1);
    GF_HERE(nv.exe2);
    GF_HERE(nv.mag0);
    GF_HERE(nv.mag1);
    GF_HERE(nv.mag2);
    GF_HERE(nv.sh0);
    GF_HERE(nv.sh1);
    GF_HERE(nv.sh2);
    GF_HERE(nv.un0);
    GF_HERE(nv.un1);
    GF_HERE(nv.un2);
    const uint32_t xc = (O.n_x + kWave - 1) / kWave;
    const uint32_t per = (xc + team - 1u) / team;
    const uint32_t c_lo = rank * per < xc ? rank * per : xc, c_hi = c_lo + per < xc ? c_lo + per : xc;
    int32_t cmax = 0;
    mf_for_each_chunk_narrow(V, O, app, nv, ds, lane, [&](uint32_t j, int32_t c) {
        cmax = c > cmax ? c : cmax;
        // the lanes that hold the same capacity speak through their first one (it also holds their smallest slot): neighbours in the
        // priority order have the same capacity more often than not, and same-address LDS atomics are served one lane at a time —
        // two of them per chunk kept the CU's LDS busy for ~120 cycles per chunk of ANY of its wavefronts (5.2 conflicts per active
        // LDS cycle in profiles/pmc_zoned.json): what the pass was bound by once four wavefronts per SIMD hid its latency
        const bool binned = c > 0 && c < kMfHistBins;
        const uint32_t n_run = mf_run_heads((uint32_t)c, binned, lane);
        if (n_run != 0u) {  // (a run's first lane holds its smallest slot)
            __hip_atomic_fetch_add(A + (uint32_t)c, n_run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_min(B + (uint32_t)c, j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        return true;
    }, c_lo, c_hi);
    {
        const int32_t wmax = (int32_t)wave_max_i64((int64_t)cmax);
        if (lane == 0) O.mf_words[rank] = (uint32_t)wmax;
    }
    visited += O.n_x;  // (wavefront 0 reports for the team: a pass of the team = one pass over the order)
    lds_barrier();  // every quarter's rows are complete
    uint32_t cn[4] = {0u, 0u, 0u, 0u}, fp[4] = {GF_NO_NODE, GF_NO_NODE, GF_NO_NODE, GF_NO_NODE}, pre[4] = {0u, 0u, 0u, 0u}, own[4] = {0u, 0u, 0u, 0u};
    uint32_t tmax = 0;
#pragma unroll
    for (uint32_t r = 0; r < (uint32_t)kMfTeamMax; ++r) {
        if (r < team) {
            const lds_mf4* Ar = (const lds_mf4*)(O.mf_team_base + (size_t)r * 3 * kMfHistBins);
            const mf_u32x4 c4 = Ar[lane], p4 = Ar[kMfHistBins / 4 + lane];
            const uint32_t cv[4] = {c4.x, c4.y, c4.z, c4.w}, pv[4] = {p4.x, p4.y, p4.z, p4.w};
            const uint32_t wm = O.mf_words[r];
            tmax = wm > tmax ? wm : tmax;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                cn[i] += cv[i];
                fp[i] = pv[i] < fp[i] ? pv[i] : fp[i];
                if (r < rank) pre[i] += cv[i];
                if (r == rank) own[i] = cv[i];
            }
        }
    }
    tmax = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)tmax);
    lds_barrier();  // everybody has read everybody's rows: they may be written again (the plan below, the next call's pass 1)
    if (tmax >= (uint32_t)kMfHistBins) return false;  // a capacity beyond the last bin somewhere: the walk (every wavefront, redundantly)
    // ---- capacities, their clamped sum and maximum (capacity.go:78-113, minimal_fragmentation.go:64-67): as wave_minfrag_hist
    int64_t lsum = 0, lmax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t c = 4 * lane + i, cc = c < K ? c : K;
        const int64_t add = (int64_t)cn[i] * cc;
        lsum = lsum + add < K ? lsum + add : K;
        if (cn[i] != 0u) lmax = c;
    }
    S = wave_sum_small(lsum);
    if (S < K) return true;
    const int64_t max_cap = wave_max_i64(lmax);
    int64_t top = kMfHistBins;
    if (K < max_cap) {
        const int64_t target = (K + max_cap) / 2;
        int64_t lsub = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t c = 4 * lane + i, cc = c < K ? c : K;
            const int64_t add = c < target ? (int64_t)cn[i] * cc : 0;
            lsub = lsub + add < K ? lsub + add : K;
        }
        if (wave_sum_small(lsub) >= K) top = target;
    }
    auto smallest_at_least = [&](int64_t need, int64_t below) {
        int64_t l = kCapInf;
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            const int64_t c = 4 * lane + i;
            if (cn[i] != 0u && c < below && c >= need) l = c;
        }
        return wave_min_i64(l);
    };
    auto largest_below = [&](int64_t below) {
        int64_t l = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t c = 4 * lane + i;
            if (cn[i] != 0u && c < below) l = c;
        }
        return wave_max_i64(l);
    };
    int64_t R = K;
    {
        const int64_t cf = smallest_at_least(R, top);  // :103-110 one node takes everything
        if (cf != kCapInf) {
            if (rank == 0u) mf_emit_one<SLOTS>(O, out, 0, K, mf_bin(fp, (uint32_t)cf), lane);
            return true;
        }
    }
    // several nodes: the level walk on the histogram, by everybody; the quarters' own rows receive {nodes taken, output offset}
    A4[lane] = mf_u32x4{0u, 0u, 0u, 0u};
    C4[lane] = mf_u32x4{pre[0], pre[1], pre[2], pre[3]};
    uint32_t last_pos = GF_NO_NODE;  // the node that takes what is left: known now (the first of its level) ...
    int64_t next_level = -1;         // ... or the first undrained node of this level (found by the quarter that holds it)
    uint32_t next_rank = 0;
    for (;;) {
        const int64_t m = largest_below(top);
        if (m <= 0) return true;
        const uint32_t cnt = mf_bin(cn, (uint32_t)m);
        const uint32_t q = (uint32_t)R / (uint32_t)m;
        const uint32_t drained = cnt < q ? cnt : q;
        A[(uint32_t)m] = drained;  // (every lane stores the same word)
        B[(uint32_t)m] = (uint32_t)(K - R);
        R -= (int64_t)drained * m;
        if (R == 0) break;
        if (drained < cnt) {
            const int64_t cf = smallest_at_least(R, m);
            if (cf != kCapInf) {
                last_pos = mf_bin(fp, (uint32_t)cf);
            } else {
                next_level = m;
                next_rank = drained;
            }
            break;
        }
        top = m;
        const int64_t cf = smallest_at_least(R, top);
        if (cf != kCapInf) {
            last_pos = mf_bin(fp, (uint32_t)cf);
            break;
        }
    }
    const bool last_from_plan = last_pos != GF_NO_NODE;
    // what the plan wants from THIS quarter: of every drained level the nodes with ranks [pre, pre + own) below `taken`, and the
    // next level's node of rank next_rank when it lies in here
    uint32_t left;
    {
        const mf_u32x4 t4 = A4[lane];  // (behind the stores above: LDS operations of a wavefront execute in order)
        const uint32_t tk[4] = {t4.x, t4.y, t4.z, t4.w};
        int64_t want = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t ahead = tk[i] > pre[i] ? tk[i] - pre[i] : 0u;
            want += (int64_t)(ahead < own[i] ? ahead : own[i]);
            if ((int64_t)(4 * lane + i) == next_level && next_rank >= pre[i] && next_rank < pre[i] + own[i]) want += 1;
        }
        left = (uint32_t)wave_sum_small(want);
    }
    if (left != 0u) {
        mf_for_each_chunk_narrow(V, O, app, nv, ds, lane, [&](uint32_t j, int32_t c) {
            const bool binned = c > 0 && c < kMfHistBins;
            const uint32_t cb = binned ? (uint32_t)c : 0u;
            const uint32_t take = A[cb], base = B[cb], seen = C[cb];
            const bool act = binned && (take != 0u || (int64_t)c == next_level);
            const uint64_t actm = __ballot(act);
            if (actm == 0ull) return true;
            const uint64_t peers = mf_peers8((uint32_t)c, act);
            const uint32_t rk = seen + (uint32_t)__popcll((unsigned long long)(peers & lt_mask));
            if (act && (peers & lt_mask) == 0ull) C[cb] = seen + (uint32_t)__popcll((unsigned long long)peers);  // the peers' leader
            const bool drain = act && rk < take;
            uint32_t id = j;
            if (!SLOTS && drain) id = O.slot_node[j];
            emit_runs(out, (int64_t)base + (int64_t)rk * c, drain ? c : 0, id, lane);  // :122
            const uint64_t nxt = __ballot(act && (int64_t)c == next_level && rk == next_rank);
            if (nxt) last_pos = read_lane(j, __ffsll((unsigned long long)nxt) - 1);
            left -= (uint32_t)__popcll((unsigned long long)__ballot(drain)) + (nxt ? 1u : 0u);
            return left != 0u;
        }, c_lo, c_hi);
        visited += O.n_x;
    }
    // what is left goes to the node the plan named (wavefront 0 emits) or to the one this quarter found
    if (R > 0 && last_pos != GF_NO_NODE && (last_from_plan ? rank == 0u : true)) mf_emit_one<SLOTS>(O, out, K - R, R, last_pos, lane);
    return true;
}

// minimalFragmentation with the driver reserved on slot ds.  Returns the sum of capacities clamped at K per node
// (exact when < K; >= K <=> feasible, in which case out[0..K) holds the placements).
template <class View, bool SLOTS>
__device__ __forceinline__ int64_t wave_minfrag(const View& V, const Orders& O, const App& app, uint32_t ds,
                                                uint32_t* __restrict__ out, int lane, unsigned long long& visited) {
    const int64_t K = app.k;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    if (O.mf_lent && O.ncpu != nullptr && K > 0) {  // the histogram form, where it applies (wave-uniform)
        MfNarrow na;
        int64_t S_h = 0;
        if (O.mf_team > 1u) {  // (wave-uniform, and the same in every wavefront of the team: both barriers are met by all)
            if (mf_narrow_app(app, O, na) && team_minfrag_hist<View, SLOTS>(V, O, app, na, ds, out, lane, visited, S_h)) return S_h;
        } else if (mf_narrow_app(app, O, na) && wave_minfrag_hist<View, SLOTS>(V, O, app, na, ds, out, lane, visited, S_h)) {
            return S_h;
        }
    }
    // capacities, their clamped sum and maximum (capacity.go:78-113, minimal_fragmentation.go:64-67)
    int64_t lsum = 0, lmax = 0;
    mf_for_each_chunk(V, O, app, ds, lane, [&](uint32_t, int64_t c) {
        const int64_t cc = c < K ? c : K;
        lsum = lsum + cc < K ? lsum + cc : K;  // saturating: a saturated lane alone proves feasibility
        lmax = c > lmax ? c : lmax;
        return true;
    });
    visited += O.n_x;
    const int64_t S = wave_sum_small(lsum);
    if (S < K) return S;
    const int64_t max_cap = wave_max_i64(lmax);
    // "avoid mostly empty nodes" (:68-78): nodes below targetCapacity, if they can host the gang by themselves
    bool bounded = false;
    int64_t lim = 0;
    if (K < max_cap) {
        const int64_t target = (int64_t)((uint64_t)K + (uint64_t)max_cap) / 2;  // Go int arithmetic wraps (max_cap may be MaxInt)
        int64_t lsub = 0;
        mf_for_each_chunk(V, O, app, ds, lane, [&](uint32_t, int64_t c) {
            if (c > 0 && c < target) {
                const int64_t cc = c < K ? c : K;
                lsub = lsub + cc < K ? lsub + cc : K;
            }
            return true;
        });
        if (wave_sum_small(lsub) >= K) {
            bounded = true;
            lim = target;
        }
    }
    // internalMinimalFragmentation (:93-137) on the admitted list; it succeeds by construction
    int64_t R = K;
    for (;;) {
        const MfProbe p = mf_probe(V, O, app, ds, lane, bounded, lim, R);
        if (p.found) {  // :103-110 one node takes everything that is left
            mf_emit_one<SLOTS>(O, out, K - R, R, p.best, lane);
            return S;
        }
        const int64_t m = p.max_cap;  // :113 (0 < m < R)
        if (m <= 0) return S;         // unreachable when S >= K; guards against a non-terminating walk
        const int64_t q = R / m;      // nodes of this level that can be drained completely (:120)
        int64_t cnt = 0;
        uint32_t lnext = GF_NO_NODE;  // first node of the level that is not drained
        mf_for_each_chunk(V, O, app, ds, lane, [&](uint32_t j, int64_t c) {
            const bool at_level = c == m;
            const uint64_t mask = __ballot(at_level);
            const int64_t rank = cnt + (int64_t)__popcll((unsigned long long)(mask & lt_mask));
            const bool drain = at_level && rank < q;
            if (at_level && rank == q) lnext = j;
            uint32_t id = j;
            if (!SLOTS && drain) id = O.slot_node[j];
            emit_runs(out, (K - R) + rank * m, drain ? (int32_t)m : 0, id, lane);  // :122
            cnt += (int64_t)__popcll((unsigned long long)mask);
            return cnt <= q;  // one node past the drained ones is all that is needed
        });
        const int64_t drained = cnt < q ? cnt : q;
        R -= drained * m;  // :123
        if (R == 0) return S;  // :126-128
        if (drained < cnt) {
            // the level was not exhausted, so R < m: the next sort.Search (:103) finds the smallest capacity >= R among
            // the lower levels, else the first undrained node of this level
            const MfProbe low = mf_probe(V, O, app, ds, lane, true, m, R);
            uint32_t s = low.best;
            if (!low.found) {
                const uint64_t has = __ballot(lnext != GF_NO_NODE);
                s = read_lane(lnext, __ffsll((unsigned long long)has) - 1);
            }
            mf_emit_one<SLOTS>(O, out, K - R, R, s, lane);
            return S;
        }
        bounded = true;  // :130 the drained level leaves the list
        lim = m;
    }
}
