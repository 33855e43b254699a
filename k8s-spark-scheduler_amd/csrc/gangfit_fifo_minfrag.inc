// gangfit_fifo_minfrag.inc — the FIFO chain for minimal-fragmentation (plain and single-AZ), LDS resident and
// block-cooperative (included by gangfit_kernels.hip after gangfit_fifo_zoned.inc, whose views, run lists, shape
// indexes and efficiency sums it shares).
//
//   minimalFragmentation / internalMinimalFragmentation   LIB/binpack/minimal_fragmentation.go:59-137
//   SingleAZMinimalFragmentation                          LIB/binpack/single_az_minimal_fragmentation.go:20, single_az.go:23-97
//   fitEarlierDrivers + final pack                        internal/extender/resource.go:224-262, 309-328
//
// Unlike tightly-pack, minimal-fragmentation cannot stop early: "the smallest capacity >= K" is a minimum over EVERY
// candidate node.  One wavefront per app (gangfit_minfrag.inc inside the generic chain) therefore walks the whole
// executor order several times per app.  Here the 16 wavefronts of the workgroup split the 64-slot chunks of one
// candidate view between them (chunk c belongs to wave c mod 16 — NWV), reduce per wave, and exchange 24 bytes per wave
// through LDS — one barrier per pass.  The walk of the reference over its capacity-sorted list collapses to:
//   pass 1 (always)   S = sum min(cap, K), S_lt = sum of the capacities below K, the maximum capacity, and the first node
//                     with the smallest capacity >= K.
//   - K < max:  target = (K + max) / 2 (Go int arithmetic; max == math.MaxInt wraps and empties the subset);
//               a node with K <= cap < target exists            -> all K executors on the first smallest such node
//               else S_lt >= K (the nodes below K suffice)      -> level walk over {0 < cap < K}
//               else                                            -> all K on the first smallest node with cap >= K
//   - K >= max: a node with cap == K                            -> all K there;  else level walk over {0 < cap < K}
//   level walk (the gang needs several nodes): ONE pass per level — it counts the level's nodes per chunk and keeps their
//   lane masks (a prefix over the chunks then gives every node its rank in priority order and the runs are emitted from
//   the masks), finds the next level below, and the best fit for what a partial drain would leave; one more pass only
//   when a lower node can take everything that is left.
// One workgroup is one CU: a pass over 10 000 slots is bounded by that CU's VALU issue rate, i.e. by the instructions
// spent per slot.  The capacities of a request shape therefore live in a matrix row in global memory (n_shapes x n_slots
// int32, filled when the shape first appears, patched for every shape at the handful of slots a commit touches): a pass
// reads one word per slot instead of three table columns and three divisions.
// Capacities are exact int32 quotients in the scaled domain (both operands below 2^30).  Zone candidates are evaluated
// one after the other (each uses the whole workgroup); chooseBestResult, the winner's expansion and the commit are as
// in gangfit_fifo_zoned.inc, with `reserved` holding the driver only (minimal_fragmentation.go never records its
// placements there).
//
// The histogram path (mf_hist_decide) — what runs unless a shape has a capacity of kMfBins or more somewhere (tiny requests,
// MaxInt; those keep the block-cooperative passes above).  Everything the decision asks of the VALUES of the capacities —
// the maximum, the smallest one >= K, the sum of those below K, the levels of the level walk and how many nodes each gives —
// is a question about the multiset of capacities of one (candidate view, executor shape), and a commit changes that multiset
// at two or three slots.  It is kept as a histogram (kMfBins counts per (view, shape) in global memory, built when the shape's
// matrix row is filled, patched with the matrix at every commit): lane l holds bins 4l .. 4l+3 and every value question is
// a handful of lane-parallel instructions.  Only WHERE — "the first node with capacity v", "the first q nodes of level m" —
// still reads the matrix row, and a second table, a lower bound of the first position of every capacity (lowered by the
// commit's patch, raised to the exact position by every walk that finds it), lets that walk start where the answer is:
// 1.3 batches of 2 048 slots per application instead of passes over the whole table.  Consequences:
//   * one wavefront decides a view alone, without barriers; the zones of single-az-minimal-fragmentation are evaluated
//     concurrently (wavefront c = zone c) and the cost no longer depends on how the zones interleave in the priority order;
//   * the winner's wavefront emits and commits; the matrix / histogram patch (lane = shape, the capacity a slot had is
//     recomputed from what the commit subtracted) is handed to up to four idle helper wavefronts, one touched slot each, and
//     runs next to the next application's staging and driver searches — only a decision on the SAME view waits for it;
//   * every table of a view is read by that view's wavefront only, everything stays inside one workgroup = one CU = one
//     L1: workgroup-scope ordering (waitcnt + barrier / flag) is all that is needed.  Agent-scope fences would write back
//     and invalidate the XCD's L2 once per application.
//   * shape ids (rows of the matrix, 64 per role) no longer need chunk-index rows in LDS: a 100 000-node table with three
//     zones, whose masks alone fill LDS, runs this path for every shape.

// Wavefronts that share the matrix / histogram patch of a commit (touched slot i to helper i mod n); round 4 measured 8 and 12:
// 6.03 / 5.99 ms against 6.05 (single-AZ 7.92 / 7.86 against 7.95) — inside the noise.
constexpr uint32_t kMfHelpers = 4;
// Wavefronts of the workgroup (template parameter NWV of the kernel and of the block-cooperative passes): every wavefront repeats
// the uniform parts of the decision, and with w wavefronts per SIMD each of those instructions costs 4w cycles.  The launch
// bound is also the register budget: sixteen wavefronts = 128 VGPRs per lane (this kernel then spills 22-27 of them to scratch),
// eight = 256 (no spill).  Eight are enough for up to three candidate views + four patch helpers + the emitter
// (fifo_minfrag_waves); more views take sixteen.
constexpr uint32_t kMfNWmax = 16;
static_assert(kMfNWmax == 8 || kMfNWmax == 16, "minimal-fragmentation chain: 8 or 16 wavefronts");
template <int NWV>
__device__ __forceinline__ constexpr uint64_t mf_own_pattern() {
    return NWV == 16 ? 0x0001000100010001ull : (NWV == 8 ? 0x0101010101010101ull : 0x1111111111111111ull);
}
inline uint32_t fifo_minfrag_waves(uint32_t n_cand) { return (n_cand <= 3u && kMfNWmax >= 8u) ? 8u : kMfNWmax; }
constexpr int kMfStage = 16;  // app records staged per refill (LDS is tight next to the per-view masks of a 100k-node table)

struct MfXchg {
    int32_t S, Slt, maxcap, cmin;
    uint32_t cmin_pos;
    int32_t maxlt;
};

struct MfShared {
    MfXchg x[2][16];
    int32_t feas[16];
    uint32_t ds[16];
    uint32_t nruns[16];
    double mx[16];
    int32_t shape_x[kMaxShapes][3];
    int32_t shape_d[kMaxShapes][3];
    // (this struct sits next to the per-view masks of a 100 000-node table with 76 bytes to spare: what it gains it must lose)
    uint32_t shape_xm[kMaxShapes][3];  // narrow_magic multipliers of the executor shapes (the post-shifts follow from the requests)
    uint32_t n_shape_x, n_shape_d;
    int32_t total_cap[16][kMaxShapes];  // per candidate (at most 16 zones)
    uint32_t lvl_total, pnext;
    unsigned long long row_ready;  // bit = executor shape id: its capacity-matrix row has been filled
    unsigned long long row_big;    // ... and holds a capacity >= kMfBins: no histogram for this shape
    // the commit of the histogram path hands its matrix / histogram patch to helper wavefronts (touched slot i to helper
    // i mod n_helpers): the application that must see it (committing app + 1), the view, the touched slots (bit 31: a run's
    // node — it lost one executor request; else the lone driver's node) and the two requests
    uint32_t pl_seq, pl_done, pl_target, pl_view, pl_n;  // pl_done counts finished helpers, pl_target what it must reach
    int32_t pl_req[6];
    uint32_t pl_slot[kZRunMax + 1];
};

inline size_t fifo_minfrag_fixed_lds(uint32_t n_chunks, uint32_t n_views, uint32_t n_shapes /* with index rows */) {
    const uint32_t n_cand = n_views > 1 ? n_views - 1 : 1;  // run lists: one per candidate
    return (size_t)kMfStage * (sizeof(gf_app) + sizeof(NApp)) + ((sizeof(MfShared) + 15) & ~(size_t)15) +
           16 * (size_t)n_chunks * n_views + 12 * (size_t)n_chunks + 2 * 8 * (size_t)kZRunMax * n_cand + 16 * (size_t)n_chunks + 8 +
           2048 * (size_t)n_cand /* histogram + first positions of the row being filled */ +
           2 * 8 * (size_t)n_shapes * n_views * ((n_chunks + 63) / 64) + 64;
}

// getCapacityAgainstSingleDimension (capacity.go:36-56) in the scaled domain; INT32_MAX stands for math.MaxInt.
// floor(a / e) for 0 <= a < 2^30, 0 < e < 2^30 by narrow_magic's multiplication (gangfit_fifo_common.inc).
__device__ __forceinline__ int32_t ncap_full_dim(int32_t a, int32_t e, uint32_t mag, uint32_t sh) {
    if (a < 0) return 0;
    if (e == 0) return INT32_MAX;  // wave-uniform
    return (int32_t)(__umulhi(mag, (uint32_t)a << 1) >> sh);
}

// Unreserved capacity of a slot for the app's executor shape, from the table.
__device__ __forceinline__ int32_t ncap_full3(int32_t a0, int32_t a1, int32_t a2, const NAppR& p) {
    const int32_t c0 = ncap_full_dim(a0, p.exe0, p.mag0, p.msh & 0xFFu), c1 = ncap_full_dim(a1, p.exe1, p.mag1, (p.msh >> 8) & 0xFFu),
                  c2 = ncap_full_dim(a2, p.exe2, p.mag2, p.msh >> 16);
    const int32_t m = c0 < c1 ? c0 : c1;
    return m < c2 ? m : c2;
}

// Capacity of slot j = 64 c + lane with the driver reserved on ds; raw = "takes one executor with nothing reserved".
__device__ __forceinline__ int32_t mf32_cap(const ZView& Z, uint32_t n_x, const NAppR& p, uint32_t ds, uint32_t c, int lane,
                                            int32_t pre, bool& raw) {
    const NarrowHybridView& V = Z.V;
    const uint32_t j = c * kWave + lane;
    raw = false;
    if (!(j < n_x && ((V.xm[c] >> lane) & 1ull))) return 0;
    if (Z.caprow != nullptr) {  // the word of the capacity matrix the walk already fetched (rows are patched by wave 0)
        const int32_t cap0 = pre;
        raw = cap0 > 0;
        if (!raw || j != ds) return cap0;
    }
    int32_t a0, a1, a2;
    V.load32(j, a0, a1, a2);
    raw = nfits_exe(a0, a1, a2, p);
    if (!raw) return 0;
    if (j == ds) {
        a0 -= p.drv0;
        a1 -= p.drv1;
        a2 -= p.drv2;
        if (!nfits_exe(a0, a1, a2, p)) return 0;
    }
    return ncap_full3(a0, a1, a2, p);
}

// f(group, bit, chunk, pre) for the chunks of this wave (chunk mod 16 == wave) that the maxima / shape index cannot rule
// out; pre = the lane's word of the capacity-matrix row for that chunk (0 without a matrix).  A wave owns at most four
// chunks of a 64-chunk group: their matrix words are all requested before the first one is used, so the L2 latency is paid
// once per group instead of once per chunk.
template <int NWV, class F>
__device__ __forceinline__ void mf_block_walk(const ZView& Z, uint32_t n_x, const NAppR& p, uint32_t wave, int lane, F f) {
    const NarrowHybridView& V = Z.V;
    const uint32_t xc = (n_x + kWave - 1) / kWave;
    const uint64_t own = mf_own_pattern<NWV>() << wave;  // 64 is a multiple of the wave count: the pattern repeats in every group
    for (uint32_t g = 0; g * kWave < xc; ++g) {
        uint64_t m;
        if (Z.xrow != nullptr) {
            m = Z.xrow[g] & own;  // the index row is exact up to stale ones: the maxima could only repeat what it says
        } else {
            const uint32_t cl = g * kWave + lane;
            bool ok = false;
            if (cl < xc) {  // four LDS reads in flight together (&& would make them four dependent round trips)
                const int32_t m0 = V.cmax_cpu[cl], m1 = V.cmax_mem[cl], m2 = V.cmax_gpu[cl];
                const uint64_t xmw = V.xm[cl];
                ok = (m0 >= p.exe0) & (m1 >= p.exe1) & (m2 >= p.exe2) & (xmw != 0);
            }
            m = __ballot(ok) & own;
        }
        if (m == 0) continue;
        constexpr int kOwned = 64 / (int)NWV;  // chunks of a group that belong to one wave
        int32_t pre[kOwned];
#pragma unroll
        for (int q = 0; q < kOwned; ++q) pre[q] = 0;
        if (Z.caprow != nullptr) {
#pragma unroll
            for (int q = 0; q < kOwned; ++q) {
                const uint32_t bit = wave + NWV * (uint32_t)q;
                const uint32_t j = (g * kWave + bit) * kWave + (uint32_t)lane;
                if (((m >> bit) & 1ull) && j < n_x)
                    pre[q] = __hip_atomic_load(&Z.caprow[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
#pragma unroll
        for (int q = 0; q < kOwned; ++q) {
            const uint32_t bit = wave + NWV * (uint32_t)q;
            if ((m >> bit) & 1ull) f(g, bit, g * kWave + bit, pre[q]);
        }
    }
}

struct MfStats {
    int32_t S, Slt, maxcap, cmin;
    uint32_t cmin_pos;
    int32_t maxlt;  // the largest admitted capacity below K: the first level of the level walk
};

typedef __attribute__((address_space(3))) MfShared lds_mfshared;

// One cooperative pass over the view: S and S_lt over all nodes, the maximum over the admitted ones (capacity below `lim`
// when bounded), and the first node with the smallest admitted capacity >= need.  Every wave returns the same result.
template <int NWV>
__device__ __forceinline__ MfStats mf_pass(const ZView& Z, uint32_t n_x, const NAppR& p, uint32_t ds, bool bounded,
                                           int32_t lim, int32_t need, uint32_t wave, int lane, lds_mfshared* sh,
                                           uint32_t& xpar) {
    const int32_t K = p.k;
    int32_t lS = 0, lSlt = 0, lmax = 0, lcmin = INT32_MAX, lmaxlt = 0;
    uint32_t lpos = GF_NO_NODE;
    mf_block_walk<NWV>(Z, n_x, p, wave, lane, [&](uint32_t g, uint32_t bit, uint32_t c, int32_t pre) {
        bool raw;
        const int32_t cap = mf32_cap(Z, n_x, p, ds, c, lane, pre, raw);
        if (Z.xrow != nullptr && __ballot(raw) == 0 && lane == 0) Z.xrow[g] &= ~(1ull << bit);  // nothing here, for good
        if (cap > 0) {
            const int32_t cc = cap < K ? cap : K;
            lS = lS + cc < K ? lS + cc : K;
            if (cap < K) {
                lSlt = lSlt + cap < K ? lSlt + cap : K;
                lmaxlt = cap > lmaxlt ? cap : lmaxlt;
            }
            if (!bounded || cap < lim) {
                lmax = cap > lmax ? cap : lmax;
                if (cap >= need && (lpos == GF_NO_NODE || cap < lcmin)) {  // strict: the earlier position keeps ties
                    lcmin = cap;
                    lpos = c * kWave + (uint32_t)lane;
                }
            }
        }
    });
    // wave level
    int32_t wS = read_lane(wave_inclusive_scan(lS), kWave - 1);
    int32_t wSlt = read_lane(wave_inclusive_scan(lSlt), kWave - 1);
    wS = wS < K ? wS : K;
    wSlt = wSlt < K ? wSlt : K;
    const int32_t wmax = (int32_t)wave_max_i64((int64_t)lmax);
    const int32_t wmaxlt = (int32_t)wave_max_i64((int64_t)lmaxlt);
    const int32_t wcmin = (int32_t)wave_min_i64(lpos != GF_NO_NODE ? (int64_t)lcmin : (int64_t)INT32_MAX);
    const bool mine = lpos != GF_NO_NODE && lcmin == wcmin;
    const uint64_t any = __ballot(lpos != GF_NO_NODE);
    const uint32_t wpos = any ? (uint32_t)(-wave_max_i64(mine ? -(int64_t)lpos : INT64_MIN + 1)) : GF_NO_NODE;
    if (lane == 0) {
        sh->x[xpar][wave].S = wS;
        sh->x[xpar][wave].Slt = wSlt;
        sh->x[xpar][wave].maxcap = wmax;
        sh->x[xpar][wave].cmin = wcmin;
        sh->x[xpar][wave].cmin_pos = wpos;
        sh->x[xpar][wave].maxlt = wmaxlt;
    }
    lds_barrier();
    // combine: lane w < 16 holds wave w's entry, then wave-level reductions (all 16 wavefronts execute this redundantly, and
    // with four of them per SIMD every redundant instruction costs 16 cycles — keep it short)
    MfStats r;
    {
        const bool has = lane < (int)NWV;
        const int32_t s = has ? sh->x[xpar][lane & 15].S : 0, sl = has ? sh->x[xpar][lane & 15].Slt : 0;
        const int32_t mx = has ? sh->x[xpar][lane & 15].maxcap : 0, ml = has ? sh->x[xpar][lane & 15].maxlt : 0;
        const int32_t cm = has ? sh->x[xpar][lane & 15].cmin : INT32_MAX;
        const uint32_t ps = has ? sh->x[xpar][lane & 15].cmin_pos : GF_NO_NODE;
        const int32_t tS = read_lane(wave_inclusive_scan(s), kWave - 1), tSl = read_lane(wave_inclusive_scan(sl), kWave - 1);
        r.S = tS < K ? tS : K;
        r.Slt = tSl < K ? tSl : K;
        r.maxcap = (int32_t)wave_max_i64((int64_t)mx);
        r.maxlt = (int32_t)wave_max_i64((int64_t)ml);
        // lexicographic minimum of (capacity, position) over the waves that found a node
        const int64_t key = ps != GF_NO_NODE ? (((int64_t)cm << 32) | (int64_t)ps) : INT64_MAX;
        const int64_t best = wave_min_i64(key);
        r.cmin = best == INT64_MAX ? INT32_MAX : (int32_t)(best >> 32);
        r.cmin_pos = best == INT64_MAX ? GF_NO_NODE : (uint32_t)(best & 0xFFFFFFFFll);
    }
    xpar ^= 1u;  // the next exchange uses the other buffer; this one is overwritten only two barriers from now
    return r;
}

// SparkBinPack with minimalFragmentation on one candidate view, by the whole workgroup.  Returns feasibility (uniform);
// on success R holds the run list (ds_out, nruns_out).
template <int NWV>
__device__ __forceinline__ bool mf_block_decide(const ZView& Z, uint32_t n_d, uint32_t n_x, uint32_t n_chunks, const NAppR& p,
                                                const RunList& R, lds_u32* chunk_cnt, lds_u32* chunk_pre, lds_u64* chunk_msk,
                                                lds_mfshared* sh, uint32_t cand,
                                                uint32_t wave, int lane, uint32_t tid, uint32_t& xpar, uint32_t& ds_out,
                                                uint32_t& nruns_out) {
    const NarrowHybridView& V = Z.V;
    const int32_t K = p.k;
    const bool indexed = p.shape_x != kNoShape;
    nruns_out = 0;
    ds_out = 0;
    if (indexed && K > 0 && sh->total_cap[cand][p.shape_x] < K) return false;
    const int64_t p0 = nwave_first_driver(Z, n_d, p, lane);  // every wave, redundantly: LDS only, no exchange needed
    if (p0 < 0) return false;
    uint32_t ds = (uint32_t)p0;
    ds_out = ds;
    if (K == 0) return true;
    MfStats st = mf_pass<NWV>(Z, n_x, p, ds, false, 0, K, wave, lane, sh, xpar);
    if (st.S < K) {  // the first fitting candidate's node is where the executors were needed (binpack.go:67-85)
        int32_t S0 = st.S;
        if (ds < n_x && V.xcand(ds)) {
            int32_t a0, a1, a2;
            V.load32(ds, a0, a1, a2);
            S0 = st.S + ncap3(a0, a1, a2, p) - ncap3(a0 - p.drv0, a1 - p.drv1, a2 - p.drv2, p);
        }
        if (S0 < K) {
            if (indexed && tid == 0) sh->total_cap[cand][p.shape_x] = S0;
            return false;
        }
        const int64_t p1 = nwave_next_feasible_driver(Z, n_d, n_x, p, ds + 1, (int64_t)S0, lane);
        if (p1 < 0) return false;
        ds = (uint32_t)p1;
        ds_out = ds;
        st = mf_pass<NWV>(Z, n_x, p, ds, false, 0, K, wave, lane, sh, xpar);
        if (st.S < K) return false;  // cannot happen; a logic error would show up as a parity failure
    }
    // ---- minimalFragmentation (:59-91) decided from the statistics of that one pass
    bool single;
    if (K < st.maxcap) {
        const int64_t target = st.maxcap == INT32_MAX ? -1 : ((int64_t)K + (int64_t)st.maxcap) / 2;  // :69 (MaxInt wraps negative)
        if (st.cmin_pos != GF_NO_NODE && (int64_t)st.cmin < target)
            single = true;  // the subset attempt finds it at once (:103-110)
        else
            single = !(target > 0 && st.Slt >= K);  // subset = nodes below K: enough of them? else fall back to all nodes
    } else {
        single = st.cmin_pos != GF_NO_NODE;  // a node with capacity == K
    }
    if (single) {
        if (tid == 0) R.store(0, st.cmin_pos, (uint32_t)K);
        nruns_out = 1;
        return true;
    }
    // ---- internalMinimalFragmentation (:93-137) over {0 < capacity < K}: drain levels from the top.  One walk per level:
    //      it counts the level's nodes per chunk (and keeps their lane masks, so the runs are emitted without a second
    //      look at the table), finds the next level below, and the best fit for what a partial drain would leave.
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    int32_t Rem = K;
    int32_t m = st.maxlt;  // :113 the largest capacity of the list
    uint32_t base = 0;
    for (;;) {
        if (m <= 0) return false;  // unreachable when the capacity sum sufficed; guards against a non-terminating walk
        const uint32_t q = (uint32_t)(Rem / m);        // nodes of this level that can be drained completely (:120)
        const int32_t need1 = Rem - (int32_t)q * m;    // what is left if the level has more than q nodes (< m)
        for (uint32_t i = tid; i < n_chunks; i += kWave * NWV) chunk_cnt[i] = 0u;
        lds_barrier();
        int32_t lcount = 0, lm2 = 0, lbf = INT32_MAX;
        uint32_t lbfpos = GF_NO_NODE;
        mf_block_walk<NWV>(Z, n_x, p, wave, lane, [&](uint32_t, uint32_t, uint32_t c, int32_t pre) {
            bool raw;
            const int32_t cap = mf32_cap(Z, n_x, p, ds, c, lane, pre, raw);
            const uint64_t lm = __ballot(cap == m);
            if (lane == 0 && lm != 0) {
                chunk_cnt[c] = (uint32_t)__popcll((unsigned long long)lm);
                chunk_msk[c] = lm;
            }
            lcount += (cap == m) ? 1 : 0;
            if (cap > 0 && cap < m) {
                lm2 = cap > lm2 ? cap : lm2;
                if (need1 > 0 && cap >= need1 && (lbfpos == GF_NO_NODE || cap < lbf)) {
                    lbf = cap;
                    lbfpos = c * kWave + (uint32_t)lane;
                }
            }
        });
        {
            const int32_t wcount = read_lane(wave_inclusive_scan(lcount), kWave - 1);
            const int32_t wm2 = (int32_t)wave_max_i64((int64_t)lm2);
            const int32_t wbf = (int32_t)wave_min_i64(lbfpos != GF_NO_NODE ? (int64_t)lbf : (int64_t)INT32_MAX);
            const bool mine = lbfpos != GF_NO_NODE && lbf == wbf;
            const uint64_t any = __ballot(lbfpos != GF_NO_NODE);
            const uint32_t wpos = any ? (uint32_t)(-wave_max_i64(mine ? -(int64_t)lbfpos : INT64_MIN + 1)) : GF_NO_NODE;
            if (lane == 0) {
                sh->x[xpar][wave].S = wcount;
                sh->x[xpar][wave].maxcap = wm2;
                sh->x[xpar][wave].cmin = wbf;
                sh->x[xpar][wave].cmin_pos = wpos;
            }
        }
        lds_barrier();
        uint32_t total, bfpos;
        int32_t m2;
        {
            const bool has = lane < (int)NWV;
            const int32_t cnt = has ? sh->x[xpar][lane & 15].S : 0, wm2 = has ? sh->x[xpar][lane & 15].maxcap : 0;
            const int32_t cm = has ? sh->x[xpar][lane & 15].cmin : INT32_MAX;
            const uint32_t ps = has ? sh->x[xpar][lane & 15].cmin_pos : GF_NO_NODE;
            total = (uint32_t)read_lane(wave_inclusive_scan(cnt), kWave - 1);
            m2 = (int32_t)wave_max_i64((int64_t)wm2);
            const int64_t key = ps != GF_NO_NODE ? (((int64_t)cm << 32) | (int64_t)ps) : INT64_MAX;
            const int64_t best = wave_min_i64(key);
            bfpos = best == INT64_MAX ? GF_NO_NODE : (uint32_t)(best & 0xFFFFFFFFll);
        }
        xpar ^= 1u;
        if (wave == 0) {  // exclusive prefix of the per-chunk populations
            uint32_t carry = 0;
            for (uint32_t b = 0; b < n_chunks; b += kWave) {
                const uint32_t i = b + (uint32_t)lane;
                const int32_t v = i < n_chunks ? (int32_t)chunk_cnt[i] : 0;
                const int32_t incl = wave_inclusive_scan(v);
                if (i < n_chunks && v > 0) chunk_pre[i] = carry + (uint32_t)(incl - v);
                carry += (uint32_t)read_lane(incl, kWave - 1);
            }
            if (lane == 0) sh->pnext = GF_NO_NODE;
        }
        lds_barrier();
        // the runs of this level (:119-124), from the masks: chunk c belongs to wave c mod 16
        for (uint32_t c = wave; c < n_chunks; c += NWV) {
            if (chunk_cnt[c] == 0) continue;  // wave-uniform
            const uint64_t lm = chunk_msk[c];
            const bool at = (lm >> lane) & 1ull;
            const uint32_t rank = chunk_pre[c] + (uint32_t)__popcll((unsigned long long)(lm & lt_mask));
            if (at && rank < q) R.store(base + rank, c * kWave + (uint32_t)lane, (uint32_t)m);
            if (at && rank == q) sh->pnext = c * kWave + (uint32_t)lane;  // first undrained node of the level
        }
        const uint32_t drained = q < total ? q : total;
        if (base + drained > kZRunMax) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // spilled runs: global stores
        lds_barrier();
        Rem -= (int32_t)drained * m;
        base += drained;
        if (Rem == 0) {  // :126-128
            nruns_out = base;
            return true;
        }
        if (drained < total) {
            // the level was not exhausted, so Rem == need1 < m: the smallest capacity >= Rem among the lower levels, else
            // the first undrained node of this level (:103-110 on the list that remains)
            const uint32_t node = bfpos != GF_NO_NODE ? bfpos : sh->pnext;
            if (tid == 0) R.store(base, node, (uint32_t)Rem);
            nruns_out = base + 1;
            return true;
        }
        // the level left the list (:130); the next one is m2.  A node that takes everything left exists iff m2 >= Rem
        if (m2 >= Rem) {
            const MfStats low = mf_pass<NWV>(Z, n_x, p, ds, true, m, Rem, wave, lane, sh, xpar);
            if (low.cmin_pos == GF_NO_NODE) return false;  // cannot happen
            if (tid == 0) R.store(base, low.cmin_pos, (uint32_t)Rem);
            nruns_out = base + 1;
            return true;
        }
        m = m2;
    }
}

// ---------------------------------------------------------------------------------------------- the histogram path
constexpr int32_t kMfBins = 256;  // capacities 1 .. 255 are counted; a shape with a larger one somewhere has no histogram
constexpr int32_t kMfNoPos = 0x7F7F7F7F;  // "no slot" in the first-position table

struct MfBins {  // lane l: bins 4 l .. 4 l + 3 of a 256-entry table (bin 0 is never used)
    int32_t h[4];
};
typedef int32_t mf_i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ MfBins mfb_load(const int32_t* row, int lane) {
    const mf_i32x4 w = *reinterpret_cast<const mf_i32x4*>(row + 4 * lane);
    MfBins b;
    b.h[0] = w.x;
    b.h[1] = w.y;
    b.h[2] = w.z;
    b.h[3] = w.w;
    return b;
}
// entry v of the table, wave-uniform
__device__ __forceinline__ int32_t mfb_at(const MfBins& b, int32_t v) {
    const int32_t i = v & 3;
    const int32_t mine = i == 0 ? b.h[0] : (i == 1 ? b.h[1] : (i == 2 ? b.h[2] : b.h[3]));
    return read_lane(mine, v >> 2);
}
// the largest capacity below lim that some node has, 0 = none
__device__ __forceinline__ int32_t mfb_max_below(const MfBins& b, int lane, int32_t lim) {
    int32_t l = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int32_t v = 4 * lane + i;
        if (b.h[i] > 0 && v < lim) l = v;
    }
    return wave_max_i32(l);
}
// the smallest capacity in [lo, hi) that some node has, INT32_MAX = none
__device__ __forceinline__ int32_t mfb_min_in(const MfBins& b, int lane, int32_t lo, int32_t hi) {
    int32_t l = INT32_MAX;
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        const int32_t v = 4 * lane + i;
        if (b.h[i] > 0 && v >= lo && v < hi) l = v;
    }
    return -wave_max_i32(-l);
}
// sum of the capacities below lim (n_slots * 255 stays far below 2^31)
__device__ __forceinline__ int32_t mfb_sum_below(const MfBins& b, int lane, int32_t lim) {
    int32_t l = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int32_t v = 4 * lane + i;
        if (v < lim) l += v * b.h[i];
    }
    return read_lane(wave_inclusive_scan(l), kWave - 1);
}

// The histogram of the view with the driver reserved on ds: the slot's unreserved capacity (what the matrix row and the
// histogram hold) leaves, its capacity next to the driver enters.  cap0 / cap1 = those two (0 when ds is no executor candidate
// of this view).
__device__ __forceinline__ MfBins mfb_with_driver(const MfBins& base, const ZView& Z, uint32_t n_x, const NAppR& p, uint32_t ds,
                                                  int lane, int32_t& cap0, int32_t& cap1) {
    const NarrowHybridView& V = Z.V;
    cap0 = 0;
    cap1 = 0;
    if (ds < n_x && V.xcand(ds)) {
        cap0 = Z.caprow[ds];
        if (cap0 > 0) {
            int32_t a0, a1, a2;
            V.load32(ds, a0, a1, a2);
            a0 -= p.drv0;
            a1 -= p.drv1;
            a2 -= p.drv2;
            if (nfits_exe(a0, a1, a2, p)) cap1 = ncap_full3(a0, a1, a2, p);
        }
    }
    MfBins b = base;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int32_t v = 4 * lane + i;
        if (cap0 > 0 && v == cap0) b.h[i] -= 1;
        if (cap1 > 0 && v == cap1) b.h[i] += 1;
    }
    return b;
}

__device__ __forceinline__ uint32_t mf_match4(const int32_t (&cap)[4], int32_t v) {
    return (cap[0] == v ? 1u : 0u) | (cap[1] == v ? 2u : 0u) | (cap[2] == v ? 4u : 0u) | (cap[3] == v ? 8u : 0u);
}

// One level of the level walk: the first `take` slots at or behind `from`, in priority order, whose capacity (driver
// reserved) is m become runs R[base .. base + take) of m executors each; with want_next the slot behind them is returned in
// next.  The walk: 256 slots ("superchunk") per step — lane l looks at slots 256 sc + 4 l .. + 3, one 16-byte word of the
// matrix row — eight superchunks requested together, because a lone wavefront pays a full L2 round trip per dependent
// request.  Superchunks without an index bit are skipped.  first = the first slot of the level (the caller tightens the
// first-position table with it).  Returns false if the level holds fewer slots than asked for (cannot happen).
__device__ __forceinline__ bool mf_level_from(const ZView& Z, uint32_t n_x, uint32_t ds, int32_t cap1, int lane, int32_t m,
                                              uint32_t take, bool want_next, uint32_t base, uint32_t from, const RunList& R,
                                              uint32_t& first, uint32_t& next, unsigned long long& visited) {
    constexpr int U = 8;
    const NarrowHybridView& V = Z.V;
    const uint32_t n_sc = (n_x + 255u) / 256u;
    const uint32_t sc_from = from / 256u, sc_ds = ds >> 8;
    const uint32_t need = take + (want_next ? 1u : 0u);
    uint32_t cnt = 0, lnext = GF_NO_NODE;
    first = GF_NO_NODE;
    next = GF_NO_NODE;
    for (uint32_t s0 = sc_from & ~(uint32_t)(U - 1); s0 < n_sc && cnt < need; s0 += U) {
        // eight superchunks = 32 chunks = one aligned half of a 64-bit word of the shape's chunk index: ONE uniform LDS read
        const uint32_t c0 = s0 * 4u;
        const uint32_t idx = Z.xrow != nullptr ? (uint32_t)(Z.xrow[c0 >> 6] >> (c0 & 63u)) : 0xFFFFFFFFu;
        if (idx == 0) continue;
        visited += 256u * U;
        // all requests of the batch before anything is used (the matrix is padded by a batch)
        mf_i32x4 w[U];
        uint64_t xm[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t sc = s0 + (uint32_t)u;
            w[u] = *reinterpret_cast<const mf_i32x4*>(Z.caprow + (size_t)sc * 256u + 4u * (uint32_t)lane);
            const uint32_t c = sc * 4u + ((uint32_t)lane >> 4);
            xm[u] = V.xm[c < V.n_chunks ? c : 0u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t sc = s0 + (uint32_t)u;
            if (cnt < need) {
                const uint32_t j0 = sc * 256u + 4u * (uint32_t)lane;
                const uint32_t c = sc * 4u + ((uint32_t)lane >> 4);
                // candidate bits are only ever set for slots of the executor order (j < n_x)
                const uint32_t nib = c < V.n_chunks ? (uint32_t)(xm[u] >> (((uint32_t)lane & 15u) * 4u)) & 0xFu : 0u;
                int32_t cap[4] = {(nib & 1u) ? w[u].x : 0, (nib & 2u) ? w[u].y : 0, (nib & 4u) ? w[u].z : 0, (nib & 8u) ? w[u].w : 0};
                if (sc == sc_ds) {  // wave-uniform: the driver's slot lies in this superchunk
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (j0 + (uint32_t)i == ds && cap[i] != 0) cap[i] = cap1;
                }
                const uint32_t mb = (sc >= sc_from && sc < n_sc) ? mf_match4(cap, m) : 0u;
                const uint64_t lm = __ballot(mb != 0);
                if (lm != 0) {
                    const int32_t mine = (int32_t)__popc(mb);
                    const int32_t incl = wave_inclusive_scan(mine);
                    uint32_t rank = cnt + (uint32_t)(incl - mine);  // of the lane's first slot of the level
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if ((mb >> i) & 1u) {
                            if (rank < take) R.store(base + rank, j0 + (uint32_t)i, (uint32_t)m);
                            if (rank == take) lnext = j0 + (uint32_t)i;
                            ++rank;
                        }
                    }
                    if (first == GF_NO_NODE) {
                        const int L = __ffsll((unsigned long long)lm) - 1;
                        first = sc * 256u + 4u * (uint32_t)L + (uint32_t)(__ffs((int)read_lane(mb, L)) - 1);
                    }
                    cnt += (uint32_t)read_lane(incl, kWave - 1);
                }
            }
        }
    }
    if (want_next) {
        const uint64_t has = __ballot(lnext != GF_NO_NODE);
        if (has) next = read_lane(lnext, __ffsll((unsigned long long)has) - 1);
    }
    return cnt >= need;
}

// The first slot at or behind `from` whose capacity (driver reserved) is v; the same walk as mf_level_from.
__device__ __forceinline__ uint32_t mf_first_from(const ZView& Z, uint32_t n_x, uint32_t ds, int32_t cap1, int lane, int32_t v,
                                                  uint32_t from, unsigned long long& visited) {
    constexpr int U = 8;
    const NarrowHybridView& V = Z.V;
    const uint32_t n_sc = (n_x + 255u) / 256u;
    const uint32_t sc_from = from / 256u, sc_ds = ds >> 8;
    for (uint32_t s0 = sc_from & ~(uint32_t)(U - 1); s0 < n_sc; s0 += U) {
        const uint32_t c0 = s0 * 4u;
        const uint32_t idx = Z.xrow != nullptr ? (uint32_t)(Z.xrow[c0 >> 6] >> (c0 & 63u)) : 0xFFFFFFFFu;
        if (idx == 0) continue;
        visited += 256u * U;
        mf_i32x4 w[U];
        uint64_t xm[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t sc = s0 + (uint32_t)u;
            w[u] = *reinterpret_cast<const mf_i32x4*>(Z.caprow + (size_t)sc * 256u + 4u * (uint32_t)lane);
            const uint32_t c = sc * 4u + ((uint32_t)lane >> 4);
            xm[u] = V.xm[c < V.n_chunks ? c : 0u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t sc = s0 + (uint32_t)u;
            const uint32_t c = sc * 4u + ((uint32_t)lane >> 4);
            const uint32_t nib = c < V.n_chunks ? (uint32_t)(xm[u] >> (((uint32_t)lane & 15u) * 4u)) & 0xFu : 0u;
            // matches among the lane's four slots; the driver's slot shows cap1 instead of the row's value
            uint32_t mb = ((w[u].x == v) ? 1u : 0u) | ((w[u].y == v) ? 2u : 0u) | ((w[u].z == v) ? 4u : 0u) | ((w[u].w == v) ? 8u : 0u);
            mb &= nib;
            if (sc == sc_ds) {  // wave-uniform
                const uint32_t dl = (ds & 255u) >> 2, di = ds & 3u;
                if ((uint32_t)lane == dl) {
                    const int32_t own = di == 0 ? w[u].x : (di == 1 ? w[u].y : (di == 2 ? w[u].z : w[u].w));
                    const bool cand = (nib >> di) & 1u;
                    const bool is = cand && own != 0 && cap1 == v;
                    mb = (mb & ~(1u << di)) | (is ? (1u << di) : 0u);
                }
            }
            const uint64_t lm = __ballot(mb != 0 && sc >= sc_from && sc < n_sc);
            if (lm != 0) {
                const int L = __ffsll((unsigned long long)lm) - 1;
                return sc * 256u + 4u * (uint32_t)L + (uint32_t)(__ffs((int)read_lane(mb, L)) - 1);
            }
        }
    }
    return GF_NO_NODE;
}

// SparkBinPack with minimalFragmentation on one candidate view, by ONE wavefront, from the histogram hrow and the
// first-position table frow of (view, executor shape).  Same decisions as mf_block_decide (which documents the collapse of
// the reference's walk); the shape is indexed and has a matrix row.  Returns feasibility; on success R holds the run list.
__device__ __forceinline__ bool mf_hist_decide(const ZView& Z, const int32_t* hrow, int32_t* frow, uint32_t n_d, uint32_t n_x,
                                               const NAppR& p, const RunList& R, lds_mfshared* sh, uint32_t cand, int lane,
                                               uint32_t& ds_out, uint32_t& nruns_out, unsigned long long& visited,
                                               bool wait_patch) {
    const int32_t K = p.k;
    nruns_out = 0;
    ds_out = 0;
    if (K > 0 && sh->total_cap[cand][p.shape_x] < K) return false;
    const int64_t p0 = nwave_first_driver(Z, n_d, p, lane);
    if (p0 < 0) return false;
    uint32_t ds = (uint32_t)p0;
    ds_out = ds;
    if (K == 0) return true;
    // the previous application committed into this view and the helper wavefront is still patching its tables: the driver
    // search above needed none of them, everything below does
    if (wait_patch) {
        typedef volatile __attribute__((address_space(3))) uint32_t lds_vu32;
        const uint32_t target = sh->pl_target;
        while (*(lds_vu32*)&sh->pl_done != target) __builtin_amdgcn_s_sleep(1);
    }
    // the matrix row, the histogram and the first positions were written by other wavefronts of this workgroup (row fill, the
    // helper's patches, a commit of the block-cooperative path), released at workgroup scope before a barrier / the flag
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const MfBins base = mfb_load(hrow, lane);
    const MfBins fp = mfb_load(frow, lane);
    int32_t cap0, cap1;
    MfBins b = mfb_with_driver(base, Z, n_x, p, ds, lane, cap0, cap1);
    int32_t maxcap = mfb_max_below(b, lane, kMfBins);
    if (maxcap < K) {
        // every capacity is below K, so the clamped sum of mf_pass is the plain sum; it decides feasibility (binpack.go:67-85)
        const int32_t total = mfb_sum_below(b, lane, kMfBins);
        if (total < K) {
            const int32_t S0 = total + (cap0 < K ? cap0 : K) - cap1;  // nothing reserved: a bound for the shape
            if (S0 < K) {
                if (lane == 0) sh->total_cap[cand][p.shape_x] = S0;
                return false;
            }
            const int64_t p1 = nwave_next_feasible_driver(Z, n_d, n_x, p, ds + 1, (int64_t)S0, lane);
            if (p1 < 0) return false;
            ds = (uint32_t)p1;
            ds_out = ds;
            b = mfb_with_driver(base, Z, n_x, p, ds, lane, cap0, cap1);
            maxcap = mfb_max_below(b, lane, kMfBins);
            if (maxcap < K && mfb_sum_below(b, lane, kMfBins) < K) return false;  // cannot happen
        }
    }
    // ---- minimalFragmentation (:59-91), in the value domain first: which levels, how many nodes of each, which last node
    bool single;
    int32_t cmin = K;
    if (K < maxcap) {
        const int32_t target = (K + maxcap) / 2;  // :69
        cmin = mfb_min_in(b, lane, K, kMfBins);   // exists: maxcap > K
        if (cmin < target)
            single = true;
        else
            single = !(target > 0 && mfb_sum_below(b, lane, K) >= K);
    } else {
        single = maxcap == K;
    }
    if (single) {  // all K executors on the first node with capacity cmin
        uint32_t from = (uint32_t)mfb_at(fp, cmin);
        if (cap1 == cmin && ds < from) from = ds;
        if (from >= n_x) from = 0;  // a table entry that was never set: cannot happen for a counted capacity
        const uint32_t pos = mf_first_from(Z, n_x, ds, cap1, lane, cmin, from, visited);
        if (pos == GF_NO_NODE) return false;  // cannot happen; a logic error would show up as a parity failure
        if (lane == 0) {
            if (pos != ds && !(cap0 == cmin && ds < pos)) frow[cmin] = (int32_t)pos;  // see the tightening below
            R.store(0, pos, (uint32_t)K);
        }
        nruns_out = 1;
        return true;
    }
    // ---- internalMinimalFragmentation (:93-137) over {0 < capacity < K}: levels from the top.  The value questions are answered
    //      by the histogram; every level and the last node get their own short walk from that capacity's first position
    auto start_of = [&](int32_t v) {
        uint32_t from = (uint32_t)mfb_at(fp, v);
        if (cap1 == v && ds < from) from = ds;  // the driver's slot shows cap1 here
        return from >= n_x ? 0u : from;         // a table entry that was never set: cannot happen for a counted capacity
    };
    // a find is exact for the UNRESERVED row (what the table bounds) unless the driver's slot is involved
    auto tighten = [&](int32_t v, uint32_t pos) {
        if (lane == 0 && pos != GF_NO_NODE && pos != ds && !(cap0 == v && ds < pos)) frow[v] = (int32_t)pos;
    };
    auto place_rest = [&](int32_t v, uint32_t run, int32_t rest) {  // `rest` executors on the first node with capacity v
        const uint32_t node = mf_first_from(Z, n_x, ds, cap1, lane, v, start_of(v), visited);
        if (node == GF_NO_NODE) return false;  // cannot happen
        tighten(v, node);
        if (lane == 0) R.store(run, node, (uint32_t)rest);
        return true;
    };
    int32_t Rem = K;
    int32_t m = mfb_max_below(b, lane, K);
    uint32_t base_run = 0;
    for (;;) {
        if (m <= 0) return false;  // unreachable when the capacity sum sufficed
        const uint32_t count = (uint32_t)mfb_at(b, m);
        const uint32_t q = (uint32_t)(Rem / m);  // nodes of this level that can be drained completely (:120)
        const uint32_t drained = q < count ? q : count;
        const int32_t rest = Rem - (int32_t)drained * m;
        // the level is not exhausted and something is left (then rest < m): the smallest capacity >= rest among the lower
        // levels takes it, else the first undrained node of this level (:103-110 on the list that remains)
        const bool partial = drained < count && rest > 0;
        const int32_t bf = partial ? mfb_min_in(b, lane, rest, m) : INT32_MAX;
        const bool want_next = partial && bf == INT32_MAX;
        uint32_t first, next;
        if (!mf_level_from(Z, n_x, ds, cap1, lane, m, drained, want_next, base_run, start_of(m), R, first, next, visited))
            return false;  // cannot happen
        tighten(m, first);
        Rem = rest;
        base_run += drained;
        if (Rem == 0) {  // :126-128
            nruns_out = base_run;
            break;
        }
        if (partial) {
            if (bf != INT32_MAX) {
                if (!place_rest(bf, base_run, Rem)) return false;
            } else {
                if (next == GF_NO_NODE) return false;  // cannot happen
                if (lane == 0) R.store(base_run, next, (uint32_t)Rem);
            }
            nruns_out = base_run + 1;
            break;
        }
        // the level left the list (:130); a node that takes everything left exists iff the next level is >= Rem
        const int32_t m2 = mfb_max_below(b, lane, m);
        if (m2 >= Rem) {
            if (!place_rest(mfb_min_in(b, lane, Rem, m), base_run, Rem)) return false;
            nruns_out = base_run + 1;
            break;
        }
        m = m2;
    }
    return true;
}

// The chain kernel, once per narrow form (gangfit_fifo_zoned_chain.inc says why as text)
#define GF_MINFRAG_CHAIN_KERNEL fit_fifo_minfrag_lds_kernel
#define GF_MINFRAG_CHAIN_FLOOR false
#include "gangfit_fifo_minfrag_chain.inc"
#undef GF_MINFRAG_CHAIN_KERNEL
#undef GF_MINFRAG_CHAIN_FLOOR
#define GF_MINFRAG_CHAIN_KERNEL fit_fifo_minfrag_lds_floor_kernel
#define GF_MINFRAG_CHAIN_FLOOR true
#include "gangfit_fifo_minfrag_chain.inc"
#undef GF_MINFRAG_CHAIN_KERNEL
#undef GF_MINFRAG_CHAIN_FLOOR
