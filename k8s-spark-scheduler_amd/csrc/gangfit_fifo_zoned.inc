// gangfit_fifo_zoned.inc — the FIFO chain for the zone-aware tightly-pack packers, LDS resident
// (included by gangfit_kernels.hip).
//
//   fitEarlierDrivers + final pack            internal/extender/resource.go:224-262, 309-328
//   getSingleAZSparkBinFunction               LIB/binpack/single_az.go:23-97   ("single-az-tightly-pack": what production
//   AzAwareTightlyPack                        LIB/binpack/az_aware_pack_tightly.go:27-38        and every reference test selects)
//
// fit_fifo_generic_kernel serves every packer from global memory and pays ~25 dependent L2 round trips per app.  This
// kernel is its fast path for the tightly-pack family on the merged layout when the table has a narrow (scaled int32)
// form: the working table front, the chunk maxima and EVERY candidate view's bit masks live in LDS; one wavefront per
// candidate view (each zone of the evaluation list, plus the plain pack for az-aware) decides concurrently in the SCALED
// domain (all quantities of a dimension divided by the table's unit — capacities and comparisons are scale invariant);
// a tightly-pack placement stays a run list (slot, count) in LDS instead of K expanded entries, so
//   * the averages chooseBestResult compares are summed straight from the runs, in slice order, with the true
//     (unscaled) values — bit-identical to ComputeAvgPackingEfficiency (efficiency.go:114-156);
//   * only the WINNING candidate is expanded to ExecutorNodes (stores only, never read back);
//   * the commit (sparkResourceUsage quirk: one executor request per distinct node, the driver only if it shares no
//     node with an executor) walks the same run list and touches LDS only.
// Per app the only global reads are the schedulable columns of the nodes that were picked.  Barriers order LDS only.
// A candidate with more than kZRunMax distinct nodes spills the tail of its run list to global scratch.
// Tightly-pack drains the FRONT of the priority order, so later apps of a chain would re-scan ever more chunks that can
// no longer host them.  Two monotone shape indexes (capacities only fall during a chain) cut that: per candidate view,
// one row of chunk bits per distinct executor request ("some node of this view in this chunk still takes one
// executor") and per distinct driver request; a scan that finds a chunk empty for its shape clears the bit for every
// later app.  Shapes are deduplicated while the app records are staged (n_shapes per role, as many as LDS allows;
// later shapes scan unindexed).

// (kZRunMax, kZStage, kMaxShapes, ZonedShared and the LDS layout, ZonedLds: gangfit_chain_lds.h)

// wavefronts of the workgroup: one per candidate view plus (while there is room) one that expands the winner's placement
inline int fifo_zoned_waves(uint32_t n_cand) { return n_cand < 4 ? 4 : (n_cand < 8 ? 8 : 16); }

// Run list of one candidate: the first kZRunMax runs in LDS, the rest in global scratch.
struct RunList {
    lds_i32* l_slot;
    lds_i32* l_cnt;
    lds_i32* l_dummy = nullptr;  // two spare words: where the lanes without a run store (nwave_tight_runs), nullptr = masked stores
    uint32_t* g_slot;
    uint32_t* g_cnt;
    __device__ __forceinline__ void store(uint32_t i, uint32_t slot, uint32_t cnt) const {
        if (i < kZRunMax) {
            l_slot[i] = (int32_t)slot;
            l_cnt[i] = (int32_t)cnt;
        } else {
            g_slot[i] = slot;
            g_cnt[i] = cnt;
        }
    }
    __device__ __forceinline__ void load(uint32_t i, uint32_t& slot, uint32_t& cnt) const {
        if (i < kZRunMax) {
            slot = (uint32_t)l_slot[i];
            cnt = (uint32_t)l_cnt[i];
        } else {
            slot = g_slot[i];
            cnt = g_cnt[i];
        }
    }
};

// One candidate view in the scaled int32 domain.
struct ZView {
    NarrowHybridView V;    // table + chunk maxima + THIS view's candidate masks
    lds_u64* xrow;         // shape-index row of the app's executor request, nullptr = not indexed
    lds_u64* drow;         // ... of the driver request
    const int32_t* caprow = nullptr;  // minimal-fragmentation chain: capacities of this executor shape per slot (global)
};

__device__ __forceinline__ bool nfits_drv(int32_t a0, int32_t a1, int32_t a2, const NAppR& p) {
    return p.drv0 <= a0 && p.drv1 <= a1 && p.drv2 <= a2;  // !driverResources.GreaterThan(available), binpack.go:69
}
__device__ __forceinline__ bool nfits_exe(int32_t a0, int32_t a1, int32_t a2, const NAppR& p) {
    return p.exe0 <= a0 && p.exe1 <= a1 && p.exe2 <= a2;  // capacity >= 1
}

// First position of the view's driver candidates that passes the driver-fit check, else -1.
__device__ __forceinline__ int64_t nwave_first_driver(const ZView& Z, uint32_t n_d, const NAppR& p, int lane) {
    const NarrowHybridView& V = Z.V;
    const uint32_t dc = (n_d + kWave - 1) / kWave;
    for (uint32_t g = 0; g * kWave < dc; ++g) {
        uint64_t m;
        if (Z.drow != nullptr) {
            m = uniform64(Z.drow[g]);  // the index row is exact up to stale ones: the maxima could only repeat what it says
        } else {
            const uint32_t cl = g * kWave + lane;
            bool ok = false;
            if (cl < dc) {  // four LDS reads in flight together (&& would make them four dependent round trips)
                const int32_t m0 = V.cmax_cpu[cl], m1 = V.cmax_mem[cl], m2 = V.cmax_gpu[cl];
                const uint64_t dmw = V.dm[cl];
                ok = (m0 >= p.drv0) & (m1 >= p.drv1) & (m2 >= p.drv2) & (dmw != 0);
            }
            m = __ballot(ok);
        }
        while (m) {
            const uint32_t bit = (uint32_t)(__ffsll((unsigned long long)m) - 1);
            const uint32_t c = g * kWave + bit;
            m &= m - 1;
            const uint32_t i = c * kWave + lane;
            // the candidate word and the slot in one round trip; the three compares leave lane masks in scalar registers and
            // meet the (wave-uniform) candidate word there (gangfit_fifo_solo.inc, fit_mask)
            const uint64_t dmw = uniform64(V.dm[c]);
            int32_t a0 = INT32_MIN / 2, a1 = INT32_MIN / 2, a2 = INT32_MIN / 2;
            if (V.resident)  // no masked-out lanes: a lane past the end reads the last slot, and the candidate word holds no bit for it
                V.load32(i < n_d ? i : n_d - 1u, a0, a1, a2);
            else if (i < n_d)
                V.load32(i, a0, a1, a2);
            const uint64_t fm = fit_mask(a0, a1, a2, p.drv0, p.drv1, p.drv2, dmw);
            if (Z.drow != nullptr && fm == 0 && lane == 0) Z.drow[g] &= ~(1ull << bit);  // nothing here, for good
            if (fm) return (int64_t)c * kWave + (__ffsll((unsigned long long)fm) - 1);
        }
    }
    return -1;
}

// wave_next_feasible_driver in the scaled domain (the rare recovery path; not indexed).
__device__ __forceinline__ int64_t nwave_next_feasible_driver(const ZView& Z, uint32_t n_d, uint32_t n_x, const NAppR& p,
                                                              uint32_t from, int64_t S, int lane) {
    const NarrowHybridView& V = Z.V;
    for (uint32_t b = from; b < n_d; b += kWave) {
        const uint32_t i = b + lane;
        bool ok = false;
        if (i < n_d && V.dcand(i)) {
            int32_t a0, a1, a2;
            V.load32(i, a0, a1, a2);
            if (nfits_drv(a0, a1, a2, p)) {
                int64_t total = S;
                if (i < n_x && V.xcand(i))
                    total = S - ncap3(a0, a1, a2, p) + ncap3(a0 - p.drv0, a1 - p.drv1, a2 - p.drv2, p);
                ok = total >= (int64_t)p.k;
            }
        }
        const uint64_t m = __ballot(ok);
        if (m) return (int64_t)b + (__ffsll((unsigned long long)m) - 1);
    }
    return -1;
}

// tightlyPackExecutors with the driver reserved on slot ds, recording runs.  Returns the sum of clamped capacities over
// the visited prefix (>= K <=> feasible).
// on_ds: executors placed on the driver's slot (the averages need it for the driver's element).
__device__ __forceinline__ int64_t nwave_tight_runs(const ZView& Z, uint32_t n_x, const NAppR& p, uint32_t ds,
                                                    const RunList& R, uint32_t& nruns, uint32_t& on_ds, int lane) {
    const NarrowHybridView& V = Z.V;
    const int32_t K = p.k;  // <= 2^20; a visit adds at most 64 K and the walk stops at K: 32-bit sums
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    const uint32_t xc = (n_x + kWave - 1) / kWave;
    const uint32_t dsc = ds >> 6;
    int32_t taken = 0;
    nruns = 0;
    on_ds = 0;
    // operands of ncap3_fit: post-shifts and the "unlimited" masks of zero request dimensions
    const uint32_t sh0 = p.msh & 0xFFu, sh1 = (p.msh >> 8) & 0xFFu, sh2 = p.msh >> 16;
    const uint32_t un0 = p.exe0 == 0 ? 0xFFFFFFFFu : 0u, un1 = p.exe1 == 0 ? 0xFFFFFFFFu : 0u, un2 = p.exe2 == 0 ? 0xFFFFFFFFu : 0u;
    for (uint32_t g = 0; g * kWave < xc; ++g) {
        uint64_t m;
        if (Z.xrow != nullptr) {
            m = uniform64(Z.xrow[g]);
        } else {
            const uint32_t cl = g * kWave + lane;
            bool ok = false;
            if (cl < xc) {
                const int32_t m0 = V.cmax_cpu[cl], m1 = V.cmax_mem[cl], m2 = V.cmax_gpu[cl];
                const uint64_t xmw = V.xm[cl];
                ok = (m0 >= p.exe0) & (m1 >= p.exe1) & (m2 >= p.exe2) & (xmw != 0);
            }
            m = __ballot(ok);
        }
        while (m) {
            const uint32_t bit = (uint32_t)(__ffsll((unsigned long long)m) - 1);
            const uint32_t c = g * kWave + bit;
            m &= m - 1;
            const uint32_t j = c * kWave + lane;
            int32_t cp = 0;
            const uint64_t xmw = uniform64(V.xm[c]);
            int32_t a0 = INT32_MIN / 2, a1 = INT32_MIN / 2, a2 = INT32_MIN / 2;
            if (V.resident)  // (as in nwave_first_driver)
                V.load32(j < n_x ? j : n_x - 1u, a0, a1, a2);
            else if (j < n_x)
                V.load32(j, a0, a1, a2);
            // without the driver reservation: what the index may remember
            uint64_t fm = fit_mask(a0, a1, a2, p.exe0, p.exe1, p.exe2, xmw);
            if (GF_RARE(fm == 0)) {
                if (Z.xrow != nullptr && lane == 0) Z.xrow[g] &= ~(1ull << bit);
                continue;
            }
            if (GF_RARE(c == dsc)) {  // wave-uniform: only the driver's chunk pays for the reservation
                if (j == ds) {
                    a0 -= p.drv0;
                    a1 -= p.drv1;
                    a2 -= p.drv2;
                }
                fm = fit_mask(a0, a1, a2, p.exe0, p.exe1, p.exe2, xmw);
            }
            {  // in every lane, then selected: a conditional block is two execution-mask hand-overs for a lone wavefront
                int32_t cq = ncap3_fit(a0, a1, a2, p, sh0, sh1, sh2, un0, un1, un2);
                GF_HERE(cq);
                cp = lane_bit(fm) ? cq : 0;
            }
            const int32_t incl = wave_inclusive_scan(cp);
            const int32_t tot = read_lane(incl, kWave - 1);
            if (tot > 0) {
                const int32_t start = taken + (incl - cp);
                const int32_t room = K - start;
                const int32_t t = room <= 0 ? 0 : (room < cp ? room : cp);
                const uint64_t tm = (uint64_t)__builtin_amdgcn_sicmp(t, 0, 38);  // lanes with t > 0
                const uint32_t nnew = nruns + (uint32_t)__popcll((unsigned long long)tm);
                const uint32_t idx = nruns + (uint32_t)__popcll((unsigned long long)(tm & lt_mask));
                if (GF_OFTEN(R.l_dummy != nullptr && nnew <= kZRunMax)) {
                    // every lane stores — the lanes without a run to two spare words —: an address select instead of an
                    // execution mask set and restored around two stores
                    lds_i32* ps = lane_bit(tm) ? R.l_slot + idx : R.l_dummy;
                    lds_i32* pc = lane_bit(tm) ? R.l_cnt + idx : R.l_dummy + 1;
                    *ps = (int32_t)j;
                    *pc = t;
                } else if (lane_bit(tm)) {
                    R.store(idx, j, (uint32_t)t);
                }
                nruns = nnew;
                if (GF_RARE(c == dsc) && ((tm >> (ds & 63u)) & 1ull)) on_ds = (uint32_t)read_lane(t, (int)(ds & 63u));
            }
            taken += tot;
            if (taken >= K) return taken;
        }
    }
    return taken;
}

typedef __attribute__((address_space(3))) int32_t lds_shape3[3];

// A shape that has just been registered gets its index rows in every view: bit c <=> the snapshot maxima of chunk c admit
// the request and the view has a candidate in the chunk.  From then on the rows alone steer the scans (bits only go 1 -> 0),
// i.e. the maxima are consulted once per shape instead of once per application and scan.
__device__ __forceinline__ void zshape_rows_init(lds_u64* rows, const lds_u64* lmasks, const lds_i32* lcm, uint32_t nc,
                                                 uint32_t nw, uint32_t n_views, uint32_t n_shapes, uint32_t shape, bool drv,
                                                 int32_t v0, int32_t v1, int32_t v2, int lane) {
    for (uint32_t g = 0; g < nw; ++g) {
        const uint32_t c = g * kWave + (uint32_t)lane;
        bool hold = false;
        if (c < nc) {
            const int32_t m0 = lcm[c], m1 = lcm[nc + c], m2 = lcm[2 * nc + c];
            hold = (m0 >= v0) & (m1 >= v1) & (m2 >= v2);
        }
        for (uint32_t v = 0; v < n_views; ++v) {
            const uint64_t cand = c < nc ? lmasks[(size_t)(2 * v + (drv ? 1u : 0u)) * nc + c] : 0ull;
            const uint64_t word = __ballot(hold & (cand != 0));
            if (lane == 0) rows[((size_t)v * n_shapes + shape) * nw + g] = word;
        }
    }
}

// Shape ids of a batch of staged records (NApp words 0..2 = driver request, 4..6 = executor request, 14 / 15 receive
// {shape_x, shape_d}), by one wavefront.  Everything is read in ONE LDS round trip — lane = record for the requests,
// lane = table entry for the two shape tables — and the loop over the records then works on registers (a lookup per
// record through LDS costs two dependent round trips: ~600 cycles per record, a third of the staging time).  A request
// that is not in its table is appended while there is room; rows_init(is_driver, id, v0, v1, v2) prepares what the
// caller keeps per shape.
template <class RowsInit>
__device__ __forceinline__ void zshapes_assign(lds_u32* recs, uint32_t n_rec, lds_shape3* tab_x, lds_shape3* tab_d, uint32_t& nx,
                                               uint32_t& nd, uint32_t n_max, int lane, RowsInit rows_init) {
    int32_t e0 = 0, e1 = 0, e2 = 0, d0 = 0, d1 = 0, d2 = 0;
    lds_u32* mine = recs + (size_t)lane * (sizeof(NApp) / 4);
    if ((uint32_t)lane < n_rec) {
        d0 = (int32_t)mine[0];
        d1 = (int32_t)mine[1];
        d2 = (int32_t)mine[2];
        e0 = (int32_t)mine[4];
        e1 = (int32_t)mine[5];
        e2 = (int32_t)mine[6];
    }
    int32_t x0 = 0, x1 = 0, x2 = 0, y0 = 0, y1 = 0, y2 = 0;  // this lane's entry of the executor / driver table
    if ((uint32_t)lane < nx) {
        x0 = tab_x[lane][0];
        x1 = tab_x[lane][1];
        x2 = tab_x[lane][2];
    }
    if ((uint32_t)lane < nd) {
        y0 = tab_d[lane][0];
        y1 = tab_d[lane][1];
        y2 = tab_d[lane][2];
    }
    uint32_t my_x = kNoShape, my_d = kNoShape;
    for (uint32_t i = 0; i < n_rec; ++i) {  // in queue order: ids are first-appearance ranks
        {
            const int32_t v0 = read_lane(e0, (int)i), v1 = read_lane(e1, (int)i), v2 = read_lane(e2, (int)i);
            const uint64_t hm = __ballot((uint32_t)lane < nx && x0 == v0 && x1 == v1 && x2 == v2);
            uint32_t id = kNoShape;
            if (hm) {
                id = (uint32_t)(__ffsll((unsigned long long)hm) - 1);
            } else if (nx < n_max) {
                id = nx++;
                if ((uint32_t)lane == id) {
                    x0 = v0;
                    x1 = v1;
                    x2 = v2;
                    tab_x[id][0] = v0;
                    tab_x[id][1] = v1;
                    tab_x[id][2] = v2;
                }
                rows_init(false, id, v0, v1, v2);
            }
            if ((uint32_t)lane == i) my_x = id;
        }
        {
            const int32_t v0 = read_lane(d0, (int)i), v1 = read_lane(d1, (int)i), v2 = read_lane(d2, (int)i);
            const uint64_t hm = __ballot((uint32_t)lane < nd && y0 == v0 && y1 == v1 && y2 == v2);
            uint32_t id = kNoShape;
            if (hm) {
                id = (uint32_t)(__ffsll((unsigned long long)hm) - 1);
            } else if (nd < n_max) {
                id = nd++;
                if ((uint32_t)lane == id) {
                    y0 = v0;
                    y1 = v1;
                    y2 = v2;
                    tab_d[id][0] = v0;
                    tab_d[id][1] = v1;
                    tab_d[id][2] = v2;
                }
                rows_init(true, id, v0, v1, v2);
            }
            if ((uint32_t)lane == i) my_d = id;
        }
    }
    if ((uint32_t)lane < n_rec) {
        mine[14] = my_x;
        mine[15] = my_d;
    }
}

// chooseBestResult (single_az.go:75-97) from the candidates' published (feasible, avg.Max) pairs, lane = candidate: the
// highest maximum wins, strictly ('<'), i.e. the first of equals.  Works on registers — read through LDS one candidate
// after the other this costs two dependent round trips each, on every wavefront, between the barrier and the commit.
__device__ __forceinline__ int32_t zoned_choose_best(int32_t feas, double mx, uint32_t n_zone_cand, int lane) {
    // The reference's loop (best_max starts at 0, a candidate wins on best_max < max) ends on the FIRST candidate that holds
    // the largest maximum, if that is above 0.  Candidates sit in lanes 0..15 = one DPP row: an inclusive max-scan along
    // the row (lanes without a source keep their own value) leaves the largest in lane 15 — straight-line code, one
    // scalar read; the candidate-by-candidate loop paid a VALU -> SGPR -> branch round trip per candidate.
    const bool cand = feas != 0 && (uint32_t)lane < n_zone_cand;
    const double top = bcast_f64(row_max_f64(cand ? mx : -1.0), 15);  // (-1.0: a value that can never win)
    if (!(top > 0.0)) return -1;
    const uint64_t em = __ballot(cand && mx == top);
    return (int32_t)(__ffsll((unsigned long long)em) - 1);
}

// chooseBestResult when every candidate publishes its avg.Max as (value, bound of |value - the reference's value|): the
// winner is certain when its interval lies strictly above every other candidate's and above 0.  Returns the winner, -1 when
// certainly nobody wins, kChooseUndecided when only the exact sums can tell (ties, near-ties, an unbounded candidate).
constexpr int32_t kChooseUndecided = -2;
__device__ __forceinline__ int32_t zoned_choose_bounded(int32_t feas, double mx, double err, uint32_t n_zone_cand, int lane) {
    const bool cand = feas != 0 && (uint32_t)lane < n_zone_cand;
    if (__ballot(cand) == 0) return -1;
    const double top = bcast_f64(row_max_f64(cand ? mx : -1.0), 15);
    const uint64_t em = __ballot(cand && mx == top);
    if (em == 0) return kChooseUndecided;  // (a NaN: cannot happen, divisors are >= 1 — the exact round decides)
    const int w = __ffsll((unsigned long long)em) - 1;
    const double lo = bcast_f64(mx - err, w);  // err = +inf -> -inf
    if (!(lo > 0.0)) {
        // every bounded candidate at 0 is exactly 0 (a sum of non-negative terms): nobody beats the initial best_max = 0
        if (top == 0.0 && __ballot(cand && !(err == 0.0)) == 0) return -1;
        return kChooseUndecided;
    }
    // (two candidates that both publish the slice-order sum itself — bound 0 — are ordered by their values: w is the first
    //  of the largest, exactly the reference's choice)
    const bool w_exact = bcast_f64(err, w) == 0.0;
    if (__ballot(cand && lane != w && !(mx + err < lo) && !(w_exact && err == 0.0))) return kChooseUndecided;
    return (int32_t)w;
}

// carry + (v of lane 0, c of lane 0 times) + (v of lane 1, c of lane 1 times) + ... over the first n lanes, every addition
// performed one after the other in exactly that order (float64 addition does not reassociate; the reference sums a slice).
// A systolic pass instead of a loop over the runs: lane t owns the steps [start_t, start_t + c_t) — start = exclusive prefix
// of the counts —, takes the running sum from lane t - 1 at its first step (one DPP shift) and adds its value at every
// step.  What a lane holds outside its window is never read.  No scalar round trips and no branches per run: the looped
// version (readlane, compare, branch per run and per addition) cost ~200 cycles per run, and the front of a tightly packed
// order yields ~9 runs of mostly one executor per application.  Every count of the first n lanes must be >= 1.
__device__ __forceinline__ double wave_serial_sum_runs(double carry, double v, uint32_t c, int n, int lane) {
    const int32_t incl = wave_inclusive_scan((int32_t)c);  // c = 0 beyond lane n - 1
    const uint32_t steps = (uint32_t)read_lane(incl, kWave - 1);
    const uint32_t start = lane == 0 ? 0xFFFFFFFFu : (uint32_t)incl - c;  // lane 0 starts from the carry it already holds
    double acc = carry;
    auto step = [&](uint32_t q) {
        const double prev = dpp_mov<kDppWaveShr1, 0xf, true>(0.0, acc);
        acc = (start == q ? prev : acc) + v;
    };
    uint32_t q = 0;
    for (; q + 4 <= steps; q += 4) {
        step(q);
        step(q + 1);
        step(q + 2);
        step(q + 3);
    }
    for (; q < steps; ++q) step(q);
    return bcast_f64(acc, n - 1);
}

// ComputeAvgPackingEfficiency over [driver] ++ executors (slice order, duplicates counted) from a run list.  Quantities
// are the true ones: avail = scaled * unit, requests from the wide app record.  Only avg[3] (Max) is compared by
// chooseBestResult.  on_ds = executors the driver's node hosts (only read with RESERVE_EXECS).
// SERIAL = false: the K + 1 additions of the slice-order sum (~1 400 cycles per application and view: float64 addition does
// not reassociate, so they are one dependent chain) are replaced by count x value per run and a tree sum, and *err receives a
// bound of the distance between the two results.  With u = 2^-53 and non-negative terms the slice-order sum is within
// gamma(K) of the real sum, the product-and-tree sum within gamma(7 + blocks), the final division rounds once each:
// (K + blocks + 10) u relative, blocks <= K / 64 + 2.  *err = (4 K + 64) u x the result leaves a factor of more than two for the
// roundings of the chooser's own interval arithmetic.  A negative term (an available quantity above the schedulable one)
// makes *err infinite.  chooseBestResult only COMPARES the averages: zoned_choose_bounded decides from (value, bound) when
// the intervals separate and asks for the slice-order sums (SERIAL = true, one more barrier) when they do not.
// prof (loads | arithmetic | sum, in cycles): no caller passes it any more.  Taking it out changes the code generated for the zone
// kernels — the function is optimised on its own, loop and tests of prof included, before it is inlined — and wants a measurement
// of its own.
// FLOOR: V holds floor(value / unit) and frem ([3][n_slots]) the remainders: avail = scaled * unit + remainder.
template <bool RESERVE_EXECS, bool SERIAL = true, bool FLOOR = false, class View>
__device__ __forceinline__ double wave_runs_avg_max(const View& V, const int64_t unit[3], const int64_t* __restrict__ sched,
                                                    uint32_t n_slots, const gf_app& w, uint32_t ds, const RunList& R,
                                                    uint32_t nruns, uint32_t on_ds, int lane,
                                                    unsigned long long* prof = nullptr, double* err = nullptr,
                                                    const int64_t* __restrict__ frem = nullptr) {
    const int64_t K = w.k;
    double max_sum = 0.0;
    bool unbounded = false;
    if (!SERIAL && nruns < (uint32_t)kWave && prof == nullptr) {
        // The usual case — the driver and at most 63 runs, one lane each — without a masked-out lane anywhere (a conditional
        // block costs a lone wavefront two execution-mask hand-overs; there were five): lanes past the list read the
        // driver's slot like lane 0 and count zero times.
        const uint32_t i = lane > 0 ? (uint32_t)lane - 1u : 0u;
        const bool valid = (uint32_t)lane <= nruns;
        uint32_t s = (uint32_t)R.l_slot[i], c = (uint32_t)R.l_cnt[i];
        s = (lane > 0 && valid) ? s : ds;
        c = valid ? (lane > 0 ? c : 1u) : 0u;
        int32_t b0, b1, b2;
        V.load32(s, b0, b1, b2);
        const int64_t s0 = sched[s], s1 = sched[(size_t)n_slots + s], s2 = sched[2 * (size_t)n_slots + s];
        const uint32_t execs = RESERVE_EXECS ? (lane > 0 ? c : on_ds) : 0u;
        int64_t r0 = (int64_t)execs * w.exe[0], r1 = (int64_t)execs * w.exe[1], r2 = (int64_t)execs * w.exe[2];
        if (s == ds) {
            r0 += w.drv[0];
            r1 += w.drv[1];
            r2 += w.drv[2];
        }
        int64_t a0 = (int64_t)b0 * unit[0], a1 = (int64_t)b1 * unit[1], a2 = (int64_t)b2 * unit[2];
        if constexpr (FLOOR) {
            a0 += frem[s];
            a1 += frem[(size_t)n_slots + s];
            a2 += frem[2 * (size_t)n_slots + s];
        }
        const bool small_cpu = __ballot(((((uint64_t)(s0 - a0 + r0)) | (uint64_t)s0) >> 32) != 0) == 0;
        NodeEff e;
        node_efficiency(a0, a1, a2, s0, s1, s2, r0, r1, r2, e, small_cpu);
        const double m = e.cpu > e.mem ? e.cpu : e.mem;
        const double mx = e.gpu > m ? e.gpu : m;
        if (__ballot(valid && mx < 0.0)) unbounded = true;
        const double avg = wave_sum_f64((double)c * mx) / (double)(K + 1);
        if (err != nullptr) *err = unbounded ? __builtin_inf() : (double)(4 * K + 64) * 0x1p-53 * avg;
        return avg;
    }
    unsigned long long tq = prof ? __builtin_readcyclecounter() : 0ull;
    // element 0 (the driver) is handled as a pseudo run of length 1 in front of the list
    for (int64_t b = -1; b < (int64_t)nruns; b += kWave) {
        const int64_t i = b + lane;
        uint32_t s = ds, c = 1;
        const bool valid = i < (int64_t)nruns;
        if (valid && i >= 0) R.load((uint32_t)i, s, c);
        double mx = 0.0;
        int64_t a0 = 0, a1 = 0, a2 = 0, s0 = 0, s1 = 0, s2 = 0, r0 = 0, r1 = 0, r2 = 0;
        if (valid) {
            int32_t b0, b1, b2;
            V.load32(s, b0, b1, b2);
            // `reserved` holds one executor request per placement on the node — unless the packer is minimalFragmentation,
            // which never records its placements there (minimal_fragmentation.go:59-91)
            const uint32_t execs = RESERVE_EXECS ? ((i < 0) ? on_ds : c) : 0u;
            r0 = (int64_t)execs * w.exe[0];
            r1 = (int64_t)execs * w.exe[1];
            r2 = (int64_t)execs * w.exe[2];
            if (s == ds) {
                r0 += w.drv[0];
                r1 += w.drv[1];
                r2 += w.drv[2];
            }
            a0 = (int64_t)b0 * unit[0];
            a1 = (int64_t)b1 * unit[1];
            a2 = (int64_t)b2 * unit[2];
            if constexpr (FLOOR) {
                a0 += frem[s];
                a1 += frem[(size_t)n_slots + s];
                a2 += frem[2 * (size_t)n_slots + s];
            }
            s0 = sched[s];
            s1 = sched[(size_t)n_slots + s];
            s2 = sched[2 * (size_t)n_slots + s];
        }
        if (prof) {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            GF_TICK(prof, prof, tq, 0)
        }
        // cpu quantities are milli-cpus: below 2^32 on any real cluster, but nothing in the ABI says so
        const bool small_cpu = __ballot(valid && ((((uint64_t)(s0 - a0 + r0)) | (uint64_t)s0) >> 32) != 0) == 0;
        if (valid) {
            NodeEff e;
            node_efficiency(a0, a1, a2, s0, s1, s2, r0, r1, r2, e, small_cpu);
            const double m = e.cpu > e.mem ? e.cpu : e.mem;
            mx = e.gpu > m ? e.gpu : m;
        }
        if (prof) {
            asm volatile("" : "+v"(mx));
            GF_TICK(prof, prof, tq, 1)
        }
        const int n = (int64_t)nruns - b < (int64_t)kWave ? (int)((int64_t)nruns - b) : kWave;
        if (!SERIAL) {
            if (__ballot(valid && mx < 0.0)) unbounded = true;
            max_sum += wave_sum_f64(valid ? (double)c * mx : 0.0);
        } else if (__builtin_expect(__ballot(valid && c == 0u) == 0, 1)) {
            max_sum = wave_serial_sum_runs(max_sum, mx, valid ? c : 0u, n, lane);
        } else {  // a run without executors (no packer records one): the plain loop
            for (int t = 0; t < n; ++t) {  // slice order; t and the repeat count are wave-uniform
                const double v = bcast_f64(mx, t);
                for (uint32_t rep = read_lane(c, t); rep > 0; --rep) max_sum += v;
            }
        }
        if (prof) {
            asm volatile("" : "+v"(max_sum));
            GF_TICK(prof, prof, tq, 2)
        }
    }
    const double avg = max_sum / (double)(K + 1);
    if (!SERIAL && err != nullptr)
        *err = unbounded ? __builtin_inf() : (double)(4 * K + 64) * 0x1p-53 * avg;
    return avg;
}

// The chain kernel, once per narrow form (gangfit_fifo_zoned_chain.inc says why as text)
#define GF_ZONED_CHAIN_KERNEL fit_fifo_zoned_lds_kernel
#define GF_ZONED_CHAIN_FLOOR false
#include "gangfit_fifo_zoned_chain.inc"
#undef GF_ZONED_CHAIN_KERNEL
#undef GF_ZONED_CHAIN_FLOOR
#define GF_ZONED_CHAIN_KERNEL fit_fifo_zoned_lds_floor_kernel
#define GF_ZONED_CHAIN_FLOOR true
#include "gangfit_fifo_zoned_chain.inc"
#undef GF_ZONED_CHAIN_KERNEL
#undef GF_ZONED_CHAIN_FLOOR

// Follow-up of fit_fifo_zoned_lds_kernel: slot ids -> the caller's node indices (results and placements).  One wave per
// app; does nothing when the batch was served by the generic kernel instead (*skip_if != 0).
__global__ __launch_bounds__(kWave* kWavesPerBlock) void zoned_translate_kernel(
    const uint32_t* __restrict__ slot_node, uint32_t n_apps, const gf_app* __restrict__ apps, gf_result* __restrict__ results,
    uint32_t* __restrict__ exec_nodes, const int32_t* __restrict__ skip_if, ChainOut o) {
    if (*skip_if) return;  // (the caller passes host outputs only when no request can lack a scaled form)
    const int lane = lane_id();
    const uint32_t a = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (a >= n_apps) return;
    if (a == 0 && lane == 0 && o.h_failed != nullptr) *o.h_failed = *o.d_failed;
    const gf_result r = results[a];
    gf_result fin = r;
    if (r.evaluated && r.has_capacity) {
        const uint64_t off = apps[a].exec_off;
        uint32_t* out = exec_nodes + off;
        uint32_t* hout = o.h_exec != nullptr ? o.h_exec + off : nullptr;
        for (uint32_t i = lane; i < r.exec_len; i += kWave) {
            const uint32_t node = slot_node[out[i]];
            out[i] = node;
            if (hout != nullptr) hout[i] = node;
        }
        fin.driver_node = slot_node[r.driver_node];
        if (lane == 0) results[a].driver_node = fin.driver_node;
    }
    if (lane == 0 && o.h_results != nullptr) o.h_results[a] = fin;
}
