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
template <bool RESERVE_EXECS, bool SERIAL = true, class View>
__device__ __forceinline__ double wave_runs_avg_max(const View& V, const int64_t unit[3], const int64_t* __restrict__ sched,
                                                    uint32_t n_slots, const gf_app& w, uint32_t ds, const RunList& R,
                                                    uint32_t nruns, uint32_t on_ds, int lane,
                                                    unsigned long long* prof = nullptr, double* err = nullptr) {
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
        const int64_t a0 = (int64_t)b0 * unit[0], a1 = (int64_t)b1 * unit[1], a2 = (int64_t)b2 * unit[2];
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

// RES: the whole table is in LDS (lds_slots >= n_slots, decided by the launcher).
template <bool AZ_AWARE, int NW, bool RES>
__global__ __launch_bounds__(kWave* NW) void fit_fifo_zoned_lds_kernel(
    NodeTable T, NarrowTable NT, ZoneTable Z, const int64_t* __restrict__ sched, uint32_t lds_slots, uint32_t n_apps,
    uint32_t n_shapes, const gf_app* __restrict__ apps, const NApp* __restrict__ napps,
    const int32_t* __restrict__ wide_needed,
    gf_result* __restrict__ results, uint32_t* __restrict__ exec_nodes, uint32_t* __restrict__ spill, uint64_t spill_stride,
    int32_t* __restrict__ chain_failed_at, ChainCkpt ck, ScanStats* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (*wide_needed) return;  // some request has no scaled form: fit_fifo_generic_kernel (guarded the other way) runs
    constexpr uint32_t BLOCK = kWave * NW;
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t nc = T.n_chunks;
    const uint32_t n_zone_cand = Z.n_zones;
    const uint32_t n_cand = n_zone_cand + (AZ_AWARE ? 1u : 0u);  // host guarantees n_cand <= NW
    const uint32_t n_views = n_zone_cand + 1;                     // + the plain view (commit, az-aware candidate)

    // ---- LDS carve (ZonedLds, gangfit_chain_lds.h)
    const chain_lds::ZonedLds L = chain_lds::zoned_lds(lds_slots, nc, n_views, NW, n_shapes);
    lds_u8* stage = (lds_u8*)(smem + L.stage);    // gf_app [kZStage]
    lds_u8* nstage = (lds_u8*)(smem + L.nstage);  // NApp [kZStage]
    typedef __attribute__((address_space(3))) ZonedShared lds_zshared;  // typed: ds_* accesses, no flat/vmcnt waits
    lds_zshared* sh = (lds_zshared*)(smem + L.shared);
    lds_u64* lmasks = (lds_u64*)(smem + L.lmasks);  // [n_views][2][nc]: x then d
    lds_i32* lcm = (lds_i32*)(smem + L.lcm);
    lds_i32* lruns = (lds_i32*)(smem + L.lruns);    // [NW][2 = application parity][2][kZRunMax]: two lists per wavefront
    const uint32_t nw = (nc + 63u) / 64u;           // 64-bit words per shape row
    lds_u64* sbx = (lds_u64*)(smem + L.sbx);        // [n_views][n_shapes][nw] executor-shape index
    lds_u64* sbd = (lds_u64*)(smem + L.sbd);        // [n_views][n_shapes][nw] driver-shape index
    lds_i32* ltab = (lds_i32*)(smem + L.ltab);      // [3][lds_slots]

    // ---- stage tables
    for (uint32_t i = tid; i < nc; i += BLOCK) {
        for (uint32_t v = 0; v < n_zone_cand; ++v) {
            lmasks[(size_t)(2 * v) * nc + i] = Z.xmask[(size_t)v * Z.stride + i];
            lmasks[(size_t)(2 * v + 1) * nc + i] = Z.dmask[(size_t)v * Z.stride + i];
        }
        lmasks[(size_t)(2 * n_zone_cand) * nc + i] = T.xmask[i];
        lmasks[(size_t)(2 * n_zone_cand + 1) * nc + i] = T.dmask[i];
        lcm[i] = NT.cmax[i];
        lcm[nc + i] = NT.cmax[nc + i];
        lcm[2 * nc + i] = NT.cmax[2 * (size_t)nc + i];
    }
    for (uint32_t s = tid; s < lds_slots; s += BLOCK) {
        ltab[s] = NT.cpu[s];
        ltab[lds_slots + s] = NT.mem[s];
        ltab[2 * lds_slots + s] = NT.gpu[s];
    }
    for (uint32_t i = tid; i < n_views * n_shapes * nw; i += BLOCK) {  // every chunk may host every shape until a scan says otherwise
        const uint32_t word = i % nw;
        const uint32_t bits = nc - word * 64u;
        const uint64_t v = bits >= 64u ? ~0ull : ((1ull << bits) - 1ull);
        sbx[i] = v;
        sbd[i] = v;
    }
    for (uint32_t i = tid; i < 17 * kMaxShapes; i += BLOCK) sh->total_cap[i / kMaxShapes][i % kMaxShapes] = INT32_MAX;
    if (tid == 0) {
        sh->n_shape_x = 0;
        sh->n_shape_d = 0;
        sh->commit_done = 0;
    }
    __syncthreads();

    auto view_of = [&](uint32_t v) {
        NarrowHybridView V;
        V.lcpu = ltab;
        V.lmem = ltab + lds_slots;
        V.lgpu = ltab + 2 * lds_slots;
        V.lds_slots = lds_slots;
        V.cpu = (glb_i32*)NT.cpu;
        V.mem = (glb_i32*)NT.mem;
        V.gpu = (glb_i32*)NT.gpu;
        V.cmax_cpu = lcm;
        V.cmax_mem = lcm + nc;
        V.cmax_gpu = lcm + 2 * nc;
        V.xm = lmasks + (size_t)(2 * v) * nc;
        V.dm = lmasks + (size_t)(2 * v + 1) * nc;
        V.n_chunks = nc;
        V.resident = RES;
        return V;
    };
    const NarrowHybridView plain = view_of(n_zone_cand);
    RunList R;
    const int64_t unit[3] = {NT.unit[0], NT.unit[1], NT.unit[2]};
    const bool tail_in_global = lds_slots < T.n_slots;
    // A wavefront without a candidate view expands the winner's runs to ExecutorNodes (stores only, nothing reads them in
    // this kernel) while the other wavefronts commit, stage and decide the next application.  It reads the winner's own
    // list: the lists alternate with the application's parity, so this one is not written again before the barrier of
    // the next application — which the helper only reaches when it is done.
    const uint32_t ew = n_cand < (uint32_t)NW ? n_cand : (uint32_t)NW;  // NW = none: the winner expands its own runs
    // ONE barrier per application for the zone views: every node sits in exactly one zone, so the winner's commit only
    // changes slots that the winner's own wavefront reads (program order), and the other views go straight on to the
    // next application.  The plain view of az-aware reads every slot: its wavefront waits for the helper's commit exactly as
    // the winner's does (commit_done); a second barrier for everybody only publishes the commit where there is no helper
    // (sixteen views) or the table has a global tail.
    const bool kCommitBarrier = AZ_AWARE && (tail_in_global || ew >= (uint32_t)NW);

    int32_t failed_at = -1;
    uint32_t a = 0;
    bool wait_commit = false;  // this wavefront won the previous application and the helper is subtracting its usage
    unsigned long long ph[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long tph = stats != nullptr ? __builtin_readcyclecounter() : 0ull;
    const unsigned long long t0_cycles = tph;
    const unsigned long long t0_real = wall_clock64();
    for (; a < n_apps; ++a) {
        if ((a % kZStage) == 0) {  // refill the staged app records
            // without the commit barrier a wavefront may still be behind the previous application's decision barrier
            // (commit, expansion): nothing of the staging area or the shape rows is rewritten before it is here too
            if (!kCommitBarrier && a != 0) lds_barrier();
            const uint32_t n_stage = (n_apps - a) < (uint32_t)kZStage ? (n_apps - a) : (uint32_t)kZStage;
            const uint32_t words = n_stage * (uint32_t)(sizeof(gf_app) / 4);
            const uint32_t* gw = reinterpret_cast<const uint32_t*>(apps + a);
            const uint32_t* gn = reinterpret_cast<const uint32_t*>(napps + a);
            lds_u32* sw = (lds_u32*)stage;
            lds_u32* sn = (lds_u32*)nstage;
            for (uint32_t i = tid; i < words; i += BLOCK) {
                sw[i] = gw[i];
                sn[i] = gn[i];
            }
            __syncthreads();
            // checkpoint (ChainCkpt): every commit of the applications before `a` has been performed and published (the
            // barriers above), nothing commits before the barrier below — the other wavefronts dump the table meanwhile
            if (chain_ckpt_due(ck, a) && wave != 0) chain_ckpt_dump(plain, T.n_slots, chain_ckpt_slot(ck, a, T.n_slots), tid, BLOCK);
            if (wave == 0) {  // shape ids of the staged requests (NApp words 14 / 15 = {shape_x, shape_d})
                uint32_t nx = sh->n_shape_x, nd = sh->n_shape_d;
                zshapes_assign((lds_u32*)sn, n_stage, sh->shape_x, sh->shape_d, nx, nd, n_shapes, lane,
                               [&](bool drv, uint32_t id, int32_t v0, int32_t v1, int32_t v2) {
                                   zshape_rows_init(drv ? sbd : sbx, lmasks, lcm, nc, nw, n_views, n_shapes, id, drv, v0, v1, v2, lane);
                               });
                if (lane == 0) {
                    sh->n_shape_x = nx;
                    sh->n_shape_d = nd;
                }
            }
            __syncthreads();
        }
        // app records from LDS: the wide one for true quantities, the narrow one for the scaled decision
        gf_app w;
        {
            const lds_i64* rec = (const lds_i64*)(stage + (size_t)(a % kZStage) * sizeof(gf_app));
            w.drv[0] = rec[0];
            w.drv[1] = rec[1];
            w.drv[2] = rec[2];
            w.exe[0] = rec[3];
            w.exe[1] = rec[4];
            w.exe[2] = rec[5];
            const int64_t kf = rec[6];
            w.k = (int32_t)(uint32_t)kf;
            w.flags = (uint32_t)((uint64_t)kf >> 32);
            w.exec_off = (uint64_t)rec[7];
        }
        NAppR app = read_staged_napp((const lds_u4*)(nstage + (size_t)(a % kZStage) * sizeof(NApp)));
        // what steers the control flow as scalars (every lane read the same record): tests on them are scalar compares, not a
        // vector compare handed over to a branch
        app.k = (int32_t)uniform32((uint32_t)app.k);
        app.flags = uniform32(app.flags);
        app.shape_x = uniform32(app.shape_x);
        app.shape_d = uniform32(app.shape_d);
        const int64_t K = app.k;
        const bool last = (a + 1 == n_apps);
        const uint32_t par = a & 1u;
        R.l_slot = lruns + ((size_t)wave * 2 + par) * 2 * kZRunMax;
        R.l_cnt = R.l_slot + kZRunMax;
        R.l_dummy = (lds_i32*)(smem + L.spare_words);  // shared by all views: nobody reads them
        R.g_slot = spill + (size_t)(2 * wave) * spill_stride + app.exec_off;
        R.g_cnt = spill + (size_t)(2 * wave + 1) * spill_stride + app.exec_off;

        GF_TICK(stats != nullptr, ph, tph, 0)
        if (wait_commit) {  // the helper's commit of the previous application ran next to this staging
            while (__hip_atomic_load(&sh->commit_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != a)
                __builtin_amdgcn_s_sleep(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            wait_commit = false;
        }
        // ---- one wavefront per candidate view: SparkBinPack (binpack.go:60-87) with tightly-pack, runs in LDS
        uint32_t my_nruns = 0, my_ds = 0, my_on_ds = 0;
        bool my_feasible = false;
        if (wave < n_cand) {
            const bool zone_view = wave < n_zone_cand;
            ZView ZV;
            ZV.V = zone_view ? view_of(wave) : plain;
            const uint32_t view = zone_view ? wave : n_zone_cand;
            ZV.xrow = app.shape_x != kNoShape ? sbx + ((size_t)view * n_shapes + app.shape_x) * nw : nullptr;
            ZV.drow = app.shape_d != kNoShape ? sbd + ((size_t)view * n_shapes + app.shape_d) * nw : nullptr;
            const NarrowHybridView& V = ZV.V;
            bool feasible = false;
            const bool indexed = app.shape_x != kNoShape;
            const bool hopeless = indexed && K > 0 && (int64_t)sh->total_cap[wave][app.shape_x] < K;
            const int64_t p0 = hopeless ? -1 : nwave_first_driver(ZV, T.n_d, app, lane);
            if (p0 >= 0) {
                my_ds = (uint32_t)p0;
                if (K == 0) {
                    feasible = true;
                } else {
                    const int64_t S_d = nwave_tight_runs(ZV, T.n_x, app, my_ds, R, my_nruns, my_on_ds, lane);
                    if (S_d >= K) {
                        feasible = true;
                    } else {  // the first fitting candidate's node is where the executors were needed (wave_fallback)
                        int64_t S = S_d;
                        if (my_ds < T.n_x && V.xcand(my_ds)) {
                            int32_t a0, a1, a2;
                            V.load32(my_ds, a0, a1, a2);
                            S = S_d + ncap3(a0, a1, a2, app) - ncap3(a0 - app.drv0, a1 - app.drv1, a2 - app.drv2, app);
                        }
                        if (S < K && indexed && lane == 0) sh->total_cap[wave][app.shape_x] = (int32_t)S;
                        if (S >= K) {
                            const int64_t p1 = nwave_next_feasible_driver(ZV, T.n_d, T.n_x, app, (uint32_t)p0 + 1, S, lane);
                            if (p1 >= 0) {
                                my_ds = (uint32_t)p1;
                                feasible = nwave_tight_runs(ZV, T.n_x, app, my_ds, R, my_nruns, my_on_ds, lane) >= K;
                            }
                        }
                    }
                }
            }
            GF_TICK(stats != nullptr, ph, tph, 1)
            double mx = 0.0, me = 0.0;
            my_feasible = feasible;
            if (feasible && zone_view) {
                if (my_nruns > kZRunMax) {  // spilled runs were written by other lanes of this wave
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                }
                mx = wave_runs_avg_max<true, false>(V, unit, sched, T.n_slots, w, my_ds, R, my_nruns, my_on_ds, lane, nullptr, &me);
            }
            if (lane == 0) {
                sh->feas[par][wave] = feasible ? 1 : 0;
                sh->ds[par][wave] = my_ds;
                sh->nruns[par][wave] = my_nruns;
                sh->mx[par][wave] = mx;
                sh->me[par][wave] = me;
            }
            if (feasible && my_nruns > kZRunMax && ew < (uint32_t)NW)  // spilled runs (global): the helper reads them
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        }
        GF_TICK(stats != nullptr, ph, tph, 2)
        lds_barrier();
        GF_TICK(stats != nullptr, ph, tph, 3)
        // ---- chooseBestResult (single_az.go:75-97), evaluated identically by every wave
        int32_t best;
        {
            int32_t f = 0;
            double m = 0.0, e = 0.0;
            if (lane < 16) {
                f = sh->feas[par][lane];
                m = sh->mx[par][lane];
                e = sh->me[par][lane];
            }
            best = zoned_choose_bounded(f, m, e, n_zone_cand, lane);
            if (GF_RARE(best == kChooseUndecided)) {
                // the bounds do not separate the candidates (ties between zones with equal nodes, an unbounded candidate): the
                // reference's own sums, one more barrier — every wavefront reaches the same verdict from the same published values
                if (wave < n_zone_cand && my_feasible) {
                    const NarrowHybridView VZ = view_of(wave);
                    const double mxe = wave_runs_avg_max<true, true>(VZ, unit, sched, T.n_slots, w, my_ds, R, my_nruns, my_on_ds, lane);
                    if (lane == 0) sh->mxe[par][wave] = mxe;
                }
                lds_barrier();
                if (lane < 16) m = sh->mxe[par][lane];  // (only read where f says the candidate is feasible)
                best = zoned_choose_best(f, m, n_zone_cand, lane);
            }
            if (AZ_AWARE && best < 0 && read_lane(f, (int)n_zone_cand)) best = (int32_t)n_zone_cand;  // az_aware_pack_tightly.go:33-37
        }
        const bool feasible = best >= 0;
        bool stop = false;
        if (last) {
            stop = true;
        } else if (!feasible && !(app.flags & GF_APP_SKIPPABLE)) {  // resource.go:249-251
            failed_at = (int32_t)a;
            stop = true;
        }
        const bool defer = feasible && ew < (uint32_t)NW;  // the helper commits, stores the result and expands the runs
        if (wave == (feasible ? (uint32_t)best : 0u)) {
            // (with a helper the winner issues no global store at all: stores are acknowledged ~2 us later and the memory
            //  operations of a wavefront return in order — its next loads would queue behind them)
            if (!defer && lane == 0) {
                gf_result r;
                r.has_capacity = feasible ? 1 : 0;
                r.driver_node = feasible ? my_ds : GF_NO_NODE;  // SLOT id: zoned_translate_kernel maps it
                r.exec_len = feasible ? (uint32_t)K : 0u;
                r.evaluated = 1;
                results[a] = r;
            }
            if (defer) {
                wait_commit = !last;  // the helper commits (below) while this wavefront stages the next application
            } else if (feasible) {
                if (my_nruns > kZRunMax) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                }
                // without a helper: commit the winner's usage (sparkpods.go:139-146) and expand its runs in the same walk
                uint32_t* dst = exec_nodes + app.exec_off;
                int64_t base = 0;
                bool driver_hosts_exec = false;
                for (uint32_t b = 0; b < my_nruns; b += kWave) {
                    const uint32_t i = b + lane;
                    uint32_t s = 0, c = 0;
                    if (i < my_nruns) R.load(i, s, c);
                    const int32_t incl = wave_inclusive_scan((int32_t)c);
                    emit_runs(dst, base + (int64_t)(incl - (int32_t)c), (int32_t)c, s, lane);  // SLOT ids
                    base += read_lane(incl, kWave - 1);
                    if (!last && c > 0) plain.sub32(s, app.exe0, app.exe1, app.exe2);
                    if (__ballot(c > 0 && s == my_ds)) driver_hosts_exec = true;
                }
                if (!last && !driver_hosts_exec && lane == 0) plain.sub32(my_ds, app.drv0, app.drv1, app.drv2);
                if (!kCommitBarrier && tail_in_global) {
                    // slots of the global tail were written by the lanes that hold their runs and are read back by lane
                    // (slot & 63) of this same wavefront in its next scan
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                }
            }
        }
        // az-aware without the second barrier: the plain view reads the winner's slots too, and when the PLAIN placement wins
        // (no single zone fits, az_aware_pack_tightly.go:33-37) its commit touches every zone's slots
        if (AZ_AWARE && !kCommitBarrier && defer && wave < n_cand && (wave == n_zone_cand || best == (int32_t)n_zone_cand))
            wait_commit = !last;
        RunList E;  // the winner's run list as the helper reads it
        uint32_t e_nruns = 0, e_ds = 0;
        if (defer && wave == ew) {
            e_nruns = sh->nruns[par][best];
            e_ds = sh->ds[par][best];
            E.l_slot = lruns + ((size_t)best * 2 + par) * 2 * kZRunMax;
            E.l_cnt = E.l_slot + kZRunMax;
            E.g_slot = spill + (size_t)(2 * best) * spill_stride + app.exec_off;  // the winner's spill area (per app: never reused)
            E.g_cnt = spill + (size_t)(2 * best + 1) * spill_stride + app.exec_off;
            if (e_nruns > kZRunMax) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (!last) {
                // commit the winner's usage (sparkpods.go:139-146): one executor request per distinct node, the driver request
                // only if no executor landed on the driver's node — before anything else, the winner's wavefront waits for it
                if (RES && e_nruns < (uint32_t)kWave) {
                    // The usual case in one pass without a masked-out lane or a read: lane i < e_nruns takes one executor
                    // request off its run's node, lane e_nruns the driver request off the driver's node unless a run sits
                    // there, the others nothing — as LDS atomics without a return value (a plain read-modify-write is a round
                    // trip, and lanes that must not write would have to be masked out).
                    const bool is_run = (uint32_t)lane < e_nruns;
                    const uint32_t i = is_run ? (uint32_t)lane : 0u;
                    uint32_t s2 = (uint32_t)E.l_slot[i];
                    const uint32_t c2 = (uint32_t)E.l_cnt[i];
                    const bool hosts = __ballot(is_run && c2 > 0 && s2 == e_ds) != 0;
                    const bool is_drv = (uint32_t)lane == e_nruns && !hosts;
                    s2 = is_run ? s2 : e_ds;
                    const bool hit = is_run && c2 > 0;
                    const int32_t q0 = hit ? app.exe0 : (is_drv ? app.drv0 : 0), q1 = hit ? app.exe1 : (is_drv ? app.drv1 : 0),
                                  q2 = hit ? app.exe2 : (is_drv ? app.drv2 : 0);
                    __hip_atomic_fetch_add(&plain.lcpu[s2], -q0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&plain.lmem[s2], -q1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&plain.lgpu[s2], -q2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    bool driver_hosts_exec = false;
                    for (uint32_t b = 0; b < e_nruns; b += kWave) {
                        const uint32_t i = b + lane;
                        uint32_t s2 = 0, c2 = 0;
                        if (i < e_nruns) E.load(i, s2, c2);
                        if (c2 > 0) plain.sub32(s2, app.exe0, app.exe1, app.exe2);
                        if (__ballot(c2 > 0 && s2 == e_ds)) driver_hosts_exec = true;
                    }
                    if (!driver_hosts_exec && lane == 0) plain.sub32(e_ds, app.drv0, app.drv1, app.drv2);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (lane == 0) __hip_atomic_store(&sh->commit_done, a + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        GF_TICK(stats != nullptr, ph, tph, 4)
        if (kCommitBarrier) {
            if (tail_in_global)
                __syncthreads();  // commits to the global tail of the table must be visible to the next app's scans
            else
                lds_barrier();
        }
        GF_TICK(stats != nullptr, ph, tph, 5)
        if (defer && wave == ew) {
            if (lane == 0) {
                gf_result r;
                r.has_capacity = 1;
                r.driver_node = e_ds;  // SLOT id: zoned_translate_kernel maps it
                r.exec_len = (uint32_t)K;
                r.evaluated = 1;
                results[a] = r;
            }
            uint32_t* dst = exec_nodes + app.exec_off;
            int64_t base = 0;
            for (uint32_t b = 0; b < e_nruns; b += kWave) {
                const uint32_t i = b + lane;
                uint32_t s2 = 0, c2 = 0;
                if (i < e_nruns) E.load(i, s2, c2);
                const int32_t incl = wave_inclusive_scan((int32_t)c2);
                emit_runs(dst, base + (int64_t)(incl - (int32_t)c2), (int32_t)c2, s2, lane);  // SLOT ids
                base += read_lane(incl, kWave - 1);
            }
        }
        if (stop) {
            ++a;
            break;
        }
    }
    chain_mark_not_evaluated<BLOCK>(results, a, n_apps, tid);
    __syncthreads();
    // residuals back to the wide working table (gf_residual_get reads it): value = scaled value * unit
    const bool tip = RES && ck.tip != nullptr;  // (ChainCkpt::tip: the table this chain ended with, for the next Filter)
    for (uint32_t s = tid; s + 1 < T.n_slots; s += BLOCK) {
        int32_t b0, b1, b2;
        plain.load32(s, b0, b1, b2);
        T.cpu[s] = (int64_t)b0 * unit[0];
        T.mem[s] = (int64_t)b1 * unit[1];
        T.gpu[s] = (int64_t)b2 * unit[2];
        if (tip) chain_tip_store(ck, T.n_slots, s, b0, b1, b2);
    }
    if (tip && tid == 0) {  // the sentinel slot, as the snapshot has it (the loop above leaves it out)
        int32_t b0, b1, b2;
        plain.load32(T.n_slots - 1u, b0, b1, b2);
        chain_tip_store(ck, T.n_slots, T.n_slots - 1u, b0, b1, b2);
    }
    if (tid == 0 && chain_failed_at != nullptr) *chain_failed_at = failed_at;
    // wave 0: stage | decide | efficiency | barrier | select+emit+commit | barrier
    if (tid == 0 && stats != nullptr) chain_write_clocks(stats, t0_cycles, t0_real, ph);
}

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
