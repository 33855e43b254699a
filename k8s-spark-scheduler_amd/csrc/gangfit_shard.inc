// gangfit_shard.inc — node-range sharding of an independent batch across GPUs (included by gangfit_kernels.hip).
//
// SURVEY.md section 8(e): the slot table (the merged priority order) is cut into n_shards contiguous ranges of 64-slot
// chunks; GPU s evaluates EVERY pending app against ITS range only, and three small exchanges stitch the per-range
// answers into the reference's result (LIB/binpack/binpack.go:60-87, pack_tightly.go:34-63, distribute_evenly.go:34-73):
//
//   partials  (kernel 1)  S_s = sum over the range of min(cap(n, 0), K);  C_s = #{n : cap(n, 0) >= 1}
//       -- all-gather [n_shards][n_apps] x 16 B --
//   drivers   (kernel 2)  with S = sum_s S_s: the first driver candidate of the range with fit && S - c0 + c1 >= K
//                         (the O(N) driver choice of SURVEY.md section 8), its position and the deltas c1 - c0,
//                         [c1 >= 1] - [c0 >= 1] that reserving the driver there causes
//       -- all-gather [n_shards][n_apps] x 16 B --
//   emit      (kernel 3)  the winning position is the minimum over shards; shard s knows how many placements the ranges
//                         before it produce (exclusive prefix of S'_t resp. C'_t) and writes ITS slice of ExecutorNodes
//                         (node index + 1; everything else stays 0) — tightly-pack: its runs; distribute-evenly: its
//                         pass-1 nodes, plus their capacities when later passes are needed
//       -- all-reduce(SUM) of the placement buffer: every entry is written by exactly one shard --
//   finish    (kernel 4)  node index + 1 -> node index; distribute-evenly passes >= 2 from the merged survivor list
//                         (< K nodes and their capacities: no table access, identical on every rank)
//
// Gangs whose executors need a gpu (round 6): like fit_independent_kernel they take the compact table of gpu nodes
// (SparseTable) — every node it leaves out has capacity 0 for such a request, so the range's sums and its slice of the
// placement are the same —, cut at the sub-slots of the range (ShardSet::g_lo / g_hi, not chunk aligned: the lanes outside
// are masked).  Without it such a gang visits one or two slots in EVERY chunk of the range, and on a congested cluster
// the launch lasts as long as those gangs.
//
// Sums are allowed to stop early once they reach 2K: every later use only needs them exactly below K, and
// 2K - c0 + c1 >= K keeps the driver test right.  Merged slot layout only (driver position == slot).
//
// The zone-aware tightly-pack packers (the *_zoned kernels; single_az.go:23-97, az_aware_pack_tightly.go:27-38): per zone, single-AZ
// tightly-pack is plain tightly-pack on the zone's candidates, so the same steps run once per (application, candidate view)
// — grid z = view c of ShardZones: the zones of the evaluation list, plus the plain order for az-aware — with the view's
// masks and its records at [shard][c][app].  A zone is usually one stretch of the priority order (the reference sorts it
// AZ-major), so a shard intersects its range with the zone's chunk span first and skips the zone when that is empty.  Emit
// writes view c's slice of its placement (slot + 1) into region c of the buffer; the choice between the zones needs every
// zone's average Max packing efficiency, a float64 sum in slice order that shards cannot split, so the finish step
// (shard_finish_zoned_kernel) computes the averages from the reduced placements — every rank holds the replicated snapshot and
// schedulable columns — with the device functions of fit_zoned_fused_kernel, chooses and writes the result.
//
// The minimal-fragmentation packers (minimal-fragmentation, single-az-minimal-fragmentation) are a family of their own further
// down (the shard_mf_* kernels): their first exchange carries a table of capacity counts next to the 16-byte records.

template <bool DRV, class View>
__device__ __forceinline__ uint64_t range_group_mask(const View& V, uint32_t g, uint32_t c_lo, uint32_t c_hi, int64_t r0,
                                                     int64_t r1, int64_t r2, int lane) {
    const uint32_t c = g * kWave + lane;
    bool ok = false;
    if (c >= c_lo && c < c_hi) {  // maxima and mask in flight together
        const uint64_t cand = DRV ? V.chunk_dmask(c) : V.chunk_xmask(c);
        ok = V.chunk_may_hold(c, r0, r1, r2) & (cand != 0);
    }
    return __ballot(ok);
}

// f(j, in) for the candidate chunks of the slot range [lo, hi) of V's order, 64 slots at a time (j = the lane's slot, in = it
// lies in the range); f returns false to end the scan.
template <class View, class F>
__device__ __forceinline__ void shard_scan_range(const View& V, uint32_t lo, uint32_t hi, int64_t r0, int64_t r1, int64_t r2,
                                                 int lane, F f) {
    const uint32_t c_lo = lo / kWave, c_hi = (hi + kWave - 1) / kWave;
    for (uint32_t g = c_lo / kWave; g * kWave < c_hi; ++g) {
        uint64_t m = range_group_mask<false>(V, g, c_lo, c_hi, r0, r1, r2, lane);
        while (m) {
            const uint32_t c = g * kWave + (uint32_t)(__ffsll((unsigned long long)m) - 1);
            m &= m - 1;
            const uint32_t j = c * kWave + lane;
            if (!f(j, j >= lo && j < hi)) return;
        }
    }
}
// the compact table of gpu nodes as a view of its own (all sub-slots are executor candidates)
__device__ __forceinline__ GlobalView shard_sparse_view(const SparseTable& G) {
    return GlobalView{const_cast<int64_t*>(G.cpu), const_cast<int64_t*>(G.mem), const_cast<int64_t*>(G.gpu), G.cmax,
                      G.cmax + G.n_chunks, G.cmax + 2 * (size_t)G.n_chunks, G.xmask, G.xmask, G.n_chunks};
}

struct ShardSums {
    int64_t before_cap, before_fit, total_fit;
    uint32_t pos;  // winning driver position (slot), GF_NO_NODE when the gang does not fit
};

// Every rank derives the same global picture from the two gathered tables (wave-uniform scalar loops over shards).
// (Row: uint32_t n_apps for the plain packers; the zone-aware views pass size_t n_cand * n_apps — records between two shards' rows —
// with pointers that start at their view's row)
template <class Row>
__device__ __forceinline__ ShardSums shard_sums(const gf_shard_partial* __restrict__ all_part,
                                                const gf_shard_driver* __restrict__ all_drv, Row n_apps, uint32_t a,
                                                uint32_t shard, uint32_t n_shards) {
    ShardSums r;
    r.before_cap = r.before_fit = r.total_fit = 0;
    r.pos = GF_NO_NODE;
    uint32_t owner = 0;
    for (uint32_t t = 0; t < n_shards; ++t) {
        const uint32_t p = all_drv[(size_t)t * n_apps + a].pos;
        if (p < r.pos) {
            r.pos = p;
            owner = t;
        }
    }
    if (r.pos == GF_NO_NODE) return r;
    const gf_shard_driver w = all_drv[(size_t)owner * n_apps + a];
    for (uint32_t t = 0; t < n_shards; ++t) {
        const gf_shard_partial p = all_part[(size_t)t * n_apps + a];
        const int64_t cap = p.cap_sum + (t == owner ? (int64_t)w.d_cap : 0);
        const int64_t fit = p.fit_count + (t == owner ? (int64_t)w.d_fit : 0);
        if (t < shard) {
            r.before_cap += cap;
            r.before_fit += fit;
        }
        r.total_fit += fit;
    }
    return r;
}

// Where a producing kernel's 16-byte record of (shard, application a) goes: row `shard` of every device's gathered table
// (posted peer stores), or row q (the grid row) of the local array.
template <class Rec>
__device__ __forceinline__ void shard_publish(const Rec& r, const PeerPtrs& dsts, Rec* __restrict__ local, uint32_t q,
                                              uint32_t shard, uint32_t n_apps, uint32_t a) {
    if (dsts.n == 0) {
        local[(size_t)q * n_apps + a] = r;
        return;
    }
    for (uint32_t t = 0; t < dsts.n; ++t) reinterpret_cast<Rec*>(dsts.p[t])[(size_t)shard * n_apps + a] = r;
}

template <int ALGO>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void shard_partials_kernel(NodeTable T, SparseTable G, ShardSet SS, uint32_t n_apps,
                                                                              const gf_app* __restrict__ apps,
                                                                              gf_shard_partial* __restrict__ part, PeerPtrs dsts) {
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= n_apps) return;
    const uint32_t q = blockIdx.y, c_lo = SS.c_lo[q], c_hi = SS.c_hi[q];
    const App app = load_app(apps, a);
    const int64_t K = app.k;
    int64_t S = 0, C = 0;
    auto visit = [&](const GlobalView& V, uint32_t n_x, uint32_t j, bool in) {
        int32_t cp = 0;
        int64_t a0, a1, a2;
        if (load_with_cand<false>(V, j, n_x, a0, a1, a2) && in) {
            if (cap_ge1(a0, a1, a2, app)) cp = cap3(a0, a1, a2, app);
        }
        S += read_lane(wave_inclusive_scan(cp), kWave - 1);
        C += (int64_t)__popcll((unsigned long long)__ballot(cp >= 1));
        return !(S >= 2 * K && (ALGO == GF_ALGO_TIGHTLY_PACK || C >= 2 * K));
    };
    if (K != 0) {
        if (G.n_x != 0 && app.exe2 > 0) {  // wave-uniform: the range's part of the compact table of gpu nodes
            const GlobalView VS = shard_sparse_view(G);
            shard_scan_range(VS, SS.g_lo[q], SS.g_hi[q], app.exe0, app.exe1, app.exe2, lane,
                             [&](uint32_t j, bool in) { return visit(VS, G.n_x, j, in); });
        } else {
            const GlobalView V{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks, T.xmask, T.dmask,
                               T.n_chunks};
            shard_scan_range(V, c_lo * kWave, c_hi * kWave, app.exe0, app.exe1, app.exe2, lane,
                             [&](uint32_t j, bool in) { return visit(V, T.n_x, j, in); });
        }
    }
    if (lane == 0) {
        gf_shard_partial p;
        p.cap_sum = S;
        p.fit_count = C;
        shard_publish(p, dsts, part, q, SS.shard[q], n_apps, a);
    }
}

__global__ __launch_bounds__(kWave* kWavesPerBlock) void shard_drivers_kernel(NodeTable T, ShardSet SS, uint32_t n_apps,
                                                                             const gf_app* __restrict__ apps,
                                                                             const gf_shard_partial* __restrict__ all_part,
                                                                             gf_shard_driver* __restrict__ drv_out, PeerPtrs dsts) {
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= n_apps) return;
    const uint32_t q = blockIdx.y, c_lo = SS.c_lo[q], c_hi = SS.c_hi[q], n_shards = SS.n_shards;
    const App app = load_app(apps, a);
    GlobalView V{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks, T.xmask, T.dmask,
                 T.n_chunks};
    const int64_t K = app.k;
    int64_t S = 0;
    for (uint32_t t = 0; t < n_shards; ++t) S += all_part[(size_t)t * n_apps + a].cap_sum;
    gf_shard_driver out;
    out.pos = GF_NO_NODE;
    out.d_cap = 0;
    out.d_fit = 0;
    out.reserved = 0;
    // Reserving a driver never adds capacity (c1 <= c0): with S < K no candidate passes total >= K, and the range need not be
    // searched at all — on a congested cluster that is every gang that does not fit, each a scan of the whole range before.
    bool found = S < K;
    for (uint32_t g = c_lo / kWave; !found && g * kWave < c_hi; ++g) {
        uint64_t m = range_group_mask<true>(V, g, c_lo, c_hi, app.drv0, app.drv1, app.drv2, lane);
        while (m) {
            const uint32_t c = g * kWave + (uint32_t)(__ffsll((unsigned long long)m) - 1);
            m &= m - 1;
            const uint32_t i = c * kWave + lane;
            bool ok = false;
            int32_t dc = 0, df = 0;
            int64_t a0, a1, a2;
            if (load_with_cand<true>(V, i, T.n_d, a0, a1, a2)) {
                if (driver_fits(a0, a1, a2, app)) {  // binpack.go:69
                    int64_t total = S;
                    if (i < T.n_x && V.xcand(i)) {
                        const int32_t c0 = cap3(a0, a1, a2, app);
                        const int32_t c1 = cap3(a0 - app.drv0, a1 - app.drv1, a2 - app.drv2, app);
                        dc = c1 - c0;
                        df = (c1 >= 1 ? 1 : 0) - (c0 >= 1 ? 1 : 0);
                        total = S + dc;
                    }
                    ok = total >= K;
                }
            }
            const uint64_t fm = __ballot(ok);
            if (fm) {
                const int src = __ffsll((unsigned long long)fm) - 1;
                out.pos = c * kWave + (uint32_t)src;
                out.d_cap = read_lane(dc, src);
                out.d_fit = read_lane(df, src);
                found = true;
                break;
            }
        }
    }
    if (lane == 0) shard_publish(out, dsts, drv_out, q, SS.shard[q], n_apps, a);
}

template <int ALGO>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void shard_emit_kernel(
    NodeTable T, SparseTable G, ShardSet SS, uint32_t n_apps, const gf_app* __restrict__ apps,
    const gf_shard_partial* __restrict__ all_part, const gf_shard_driver* __restrict__ all_drv, gf_result* __restrict__ results,
    uint32_t* __restrict__ exec2, uint64_t half) {
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= n_apps) return;
    const uint32_t q = blockIdx.y, c_lo = SS.c_lo[q], c_hi = SS.c_hi[q], shard = SS.shard[q], n_shards = SS.n_shards;
    const App app = load_app(apps, a);
    const int64_t K = app.k;
    const ShardSums GS = shard_sums(all_part, all_drv, n_apps, a, shard, n_shards);
    const bool feasible = GS.pos != GF_NO_NODE;
    if (lane == 0 && q == 0) {  // (every hosted shard derives the same record: the first grid row stores it)
        gf_result r;
        r.has_capacity = feasible ? 1 : 0;
        r.driver_node = feasible ? T.slot_node[GS.pos] : GF_NO_NODE;
        r.exec_len = feasible ? (uint32_t)K : 0u;
        r.evaluated = 1;
        results[a] = r;
    }
    if (!feasible || K == 0) return;
    uint32_t* out = exec2 + app.exec_off;
    uint32_t* caps = exec2 + half + app.exec_off;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    const bool multipass = ALGO == GF_ALGO_DISTRIBUTE_EVENLY && GS.total_fit < K;
    int64_t taken = ALGO == GF_ALGO_TIGHTLY_PACK ? GS.before_cap : GS.before_fit;
    if (taken >= K) return;
    // ds: the driver's slot IN THE ORDER THE VISIT WALKS (GF_NO_NODE: not in it); slot_node: that order's node ids
    auto visit = [&](const GlobalView& V, uint32_t n_x, const uint32_t* __restrict__ slot_node, uint32_t ds, uint32_t j, bool in) {
        int32_t cp = 0;
        int64_t a0, a1, a2;
        if (load_with_cand<false>(V, j, n_x, a0, a1, a2) && in) {
            if (j == ds) {
                a0 -= app.drv0;
                a1 -= app.drv1;
                a2 -= app.drv2;
            }
            if (cap_ge1(a0, a1, a2, app)) cp = (ALGO == GF_ALGO_TIGHTLY_PACK || multipass) ? cap3(a0, a1, a2, app) : 1;
        }
        if (ALGO == GF_ALGO_TIGHTLY_PACK) {  // pack_tightly.go:45-61, continued from the ranges before this one
            const int32_t incl = wave_inclusive_scan(cp);
            const int32_t tot = read_lane(incl, kWave - 1);
            if (tot > 0) {
                const int64_t start = taken + (int64_t)(incl - cp);
                const int64_t room = K - start;
                const int32_t t = room <= 0 ? 0 : (room < (int64_t)cp ? (int32_t)room : cp);
                uint32_t id = 0;
                if (t > 0) id = slot_node[j] + 1u;
                emit_runs(out, start, t, id, lane);
            }
            taken += tot;
        } else {  // distribute_evenly.go:49-71, pass 1
            const bool flag = cp >= 1;
            const uint64_t fm = __ballot(flag);
            const int64_t pos = taken + (int64_t)__popcll((unsigned long long)(fm & lt_mask));
            if (flag && pos < K) {
                out[pos] = slot_node[j] + 1u;
                if (multipass) caps[pos] = (uint32_t)cp;
            }
            taken += (int64_t)__popcll((unsigned long long)fm);
        }
        return taken < K;
    };
    if (G.n_x != 0 && app.exe2 > 0) {  // wave-uniform: the range's part of the compact table of gpu nodes
        const GlobalView VS = shard_sparse_view(G);
        const uint32_t ds_sub = G.sub_of_slot[GS.pos];
        shard_scan_range(VS, SS.g_lo[q], SS.g_hi[q], app.exe0, app.exe1, app.exe2, lane,
                         [&](uint32_t j, bool in) { return visit(VS, G.n_x, G.slot_node, ds_sub, j, in); });
    } else {
        const GlobalView V{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks, T.xmask, T.dmask,
                           T.n_chunks};
        shard_scan_range(V, c_lo * kWave, c_hi * kWave, app.exe0, app.exe1, app.exe2, lane,
                         [&](uint32_t j, bool in) { return visit(V, T.n_x, T.slot_node, GS.pos, j, in); });
    }
}

template <int ALGO>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void shard_finish_kernel(
    uint32_t n_shards, uint32_t n_apps, const gf_app* __restrict__ apps, const gf_shard_partial* __restrict__ all_part,
    const gf_shard_driver* __restrict__ all_drv, const gf_result* __restrict__ results, uint32_t* __restrict__ exec2,
    uint64_t half) {
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= n_apps) return;
    if (!results[a].has_capacity) return;
    const gf_app* p = apps + a;
    const int64_t K = p->k;
    uint32_t* out = exec2 + p->exec_off;
    const uint32_t* caps = exec2 + half + p->exec_off;
    int64_t m1 = K;
    if (ALGO == GF_ALGO_DISTRIBUTE_EVENLY) {
        const ShardSums G = shard_sums(all_part, all_drv, n_apps, a, 0, n_shards);
        if (G.total_fit < K) m1 = G.total_fit;
    }
    for (int64_t i = lane; i < m1; i += kWave) out[i] -= 1u;
    if (m1 >= K) return;
    // distribute-evenly passes r = 2, 3, ... over the survivors of pass 1 (the merged list, in priority order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    int64_t pos = m1;
    for (int32_t r = 2; pos < K; ++r) {
        bool any = false;
        for (int64_t b = 0; b < m1 && pos < K; b += kWave) {
            const int64_t i = b + lane;
            bool flag = false;
            uint32_t node = 0;
            if (i < m1) {
                flag = (int32_t)caps[i] >= r;
                node = out[i];
            }
            const uint64_t m = __ballot(flag);
            const int64_t q = pos + (int64_t)__popcll((unsigned long long)(m & lt_mask));
            if (flag && q < K) out[q] = node;
            pos += (int64_t)__popcll((unsigned long long)m);
            any = any || m != 0;
        }
        if (!any) break;  // cannot happen for a feasible app; guards against a non-terminating loop
    }
}

// ---- the zone-aware tightly-pack packers (the views of ShardZones; see the top of this file)
// Candidate view c of a zone-aware batch on grid row q: its masks, and the shard's ranges intersected with the zone's span
// (chunks of the order in [c_lo, c_hi), sub-slots of the compact gpu table in [g_lo, g_hi)).  The plain view keeps all of them.
struct ShardView {
    const uint64_t* xm;
    const uint64_t* dm;
    const uint64_t* gxm;
    uint32_t c_lo, c_hi, g_lo, g_hi;
};
__device__ __forceinline__ ShardView shard_view(const NodeTable& T, const SparseTable& G, const ShardSet& SS, const ShardZones& SZ,
                                                uint32_t q, uint32_t c) {
    ShardView v{T.xmask, T.dmask, G.xmask, SS.c_lo[q], SS.c_hi[q], SS.g_lo[q], SS.g_hi[q]};
    if (c < SZ.n_zones) {
        v.xm = SZ.xmask + (size_t)c * SZ.stride;
        v.dm = SZ.dmask + (size_t)c * SZ.stride;
        v.gxm = G.zmask + (size_t)c * G.n_chunks;
        if (SZ.span != nullptr) {
            const uint32_t* sp = SZ.span + 4 * (size_t)c;  // (wave-uniform: scalar loads)
            v.c_lo = v.c_lo > sp[0] ? v.c_lo : sp[0];
            v.c_hi = v.c_hi < sp[1] ? v.c_hi : sp[1];
            v.g_lo = v.g_lo > sp[2] * kWave ? v.g_lo : sp[2] * kWave;
            v.g_hi = v.g_hi < sp[3] * kWave ? v.g_hi : sp[3] * kWave;
        }
        if (v.c_hi < v.c_lo) v.c_hi = v.c_lo;  // (an empty range: the scans visit no chunk)
        if (v.g_hi < v.g_lo) v.g_hi = v.g_lo;
    }
    return v;
}


// Partials of view c = blockIdx.z: tightly-pack's capacity sum over the shard's part of the zone (or of the plain order).
__global__ __launch_bounds__(kWave* kWavesPerBlock) void shard_partials_zoned_kernel(NodeTable T, SparseTable G, ShardSet SS, ShardZones SZ,
                                                                                    uint32_t n_apps, const gf_app* __restrict__ apps,
                                                                                    gf_shard_partial* __restrict__ part, PeerPtrs dsts) {
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= n_apps) return;
    const uint32_t q = blockIdx.y, c = blockIdx.z;
    const ShardView zv = shard_view(T, G, SS, SZ, q, c);
    const App app = load_app(apps, a);
    const int64_t K = app.k;
    int64_t S = 0;
    auto visit = [&](const GlobalView& V, uint32_t n_x, uint32_t j, bool in) {
        int32_t cp = 0;
        int64_t a0, a1, a2;
        if (load_with_cand<false>(V, j, n_x, a0, a1, a2) && in) {
            if (cap_ge1(a0, a1, a2, app)) cp = cap3(a0, a1, a2, app);
        }
        S += read_lane(wave_inclusive_scan(cp), kWave - 1);
        return S < 2 * K;
    };
    if (K != 0) {
        if (G.n_x != 0 && app.exe2 > 0) {  // wave-uniform: the range's part of the view's sub-slots of the compact gpu table
            GlobalView VS = shard_sparse_view(G);
            VS.xm = VS.dm = zv.gxm;
            if (zv.g_lo < zv.g_hi)
                shard_scan_range(VS, zv.g_lo, zv.g_hi, app.exe0, app.exe1, app.exe2, lane,
                                 [&](uint32_t j, bool in) { return visit(VS, G.n_x, j, in); });
        } else if (zv.c_lo < zv.c_hi) {
            const GlobalView V{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks, zv.xm, zv.dm,
                               T.n_chunks};
            shard_scan_range(V, zv.c_lo * kWave, zv.c_hi * kWave, app.exe0, app.exe1, app.exe2, lane,
                             [&](uint32_t j, bool in) { return visit(V, T.n_x, j, in); });
        }
    }
    if (lane == 0) {
        gf_shard_partial p;
        p.cap_sum = S;
        p.fit_count = 0;  // (distribute-evenly's count: not used by tightly-pack)
        shard_publish(p, dsts, part, q * SZ.n_cand + c, SS.shard[q] * SZ.n_cand + c, n_apps, a);
    }
}

// Drivers of view c: the first driver candidate of the shard's part of the zone with fit && S - c0 + c1 >= K.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void shard_drivers_zoned_kernel(NodeTable T, ShardSet SS, ShardZones SZ,
                                                                                   uint32_t n_apps, const gf_app* __restrict__ apps,
                                                                                   const gf_shard_partial* __restrict__ all_part,
                                                                                   gf_shard_driver* __restrict__ drv_out, PeerPtrs dsts) {
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= n_apps) return;
    const uint32_t q = blockIdx.y, c = blockIdx.z, n_shards = SS.n_shards;
    const ShardView zv = shard_view(T, SparseTable{}, SS, SZ, q, c);
    const App app = load_app(apps, a);
    const GlobalView V{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks, zv.xm, zv.dm, T.n_chunks};
    const int64_t K = app.k;
    const size_t row = (size_t)SZ.n_cand * n_apps;
    int64_t S = 0;
    for (uint32_t t = 0; t < n_shards; ++t) S += all_part[(size_t)t * row + (size_t)c * n_apps + a].cap_sum;
    gf_shard_driver out;
    out.pos = GF_NO_NODE;
    out.d_cap = 0;
    out.d_fit = 0;
    out.reserved = 0;
    bool found = S < K;  // (as in shard_drivers_kernel: no candidate can pass total >= K)
    for (uint32_t g = zv.c_lo / kWave; !found && zv.c_lo < zv.c_hi && g * kWave < zv.c_hi; ++g) {
        uint64_t m = range_group_mask<true>(V, g, zv.c_lo, zv.c_hi, app.drv0, app.drv1, app.drv2, lane);
        while (m) {
            const uint32_t ch = g * kWave + (uint32_t)(__ffsll((unsigned long long)m) - 1);
            m &= m - 1;
            const uint32_t i = ch * kWave + lane;
            bool ok = false;
            int32_t dc = 0;
            int64_t a0, a1, a2;
            if (load_with_cand<true>(V, i, T.n_d, a0, a1, a2)) {
                if (driver_fits(a0, a1, a2, app)) {  // binpack.go:69
                    int64_t total = S;
                    if (i < T.n_x && V.xcand(i)) {  // the driver's node is an executor candidate of the view
                        dc = cap3(a0 - app.drv0, a1 - app.drv1, a2 - app.drv2, app) - cap3(a0, a1, a2, app);
                        total = S + dc;
                    }
                    ok = total >= K;
                }
            }
            const uint64_t fm = __ballot(ok);
            if (fm) {
                const int src = __ffsll((unsigned long long)fm) - 1;
                out.pos = ch * kWave + (uint32_t)src;
                out.d_cap = read_lane(dc, src);
                found = true;
                break;
            }
        }
    }
    if (lane == 0) shard_publish(out, dsts, drv_out, q * SZ.n_cand + c, SS.shard[q] * SZ.n_cand + c, n_apps, a);
}

// Emit of view c: the shard's slice of the view's tightly-pack placement, as slot + 1, into region c of the buffer (c * half words
// in).  No result record: the finish step chooses.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void shard_emit_zoned_kernel(
    NodeTable T, SparseTable G, ShardSet SS, ShardZones SZ, uint32_t n_apps, const gf_app* __restrict__ apps,
    const gf_shard_partial* __restrict__ all_part, const gf_shard_driver* __restrict__ all_drv, uint32_t* __restrict__ exec2,
    uint64_t half) {
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= n_apps) return;
    const uint32_t q = blockIdx.y, c = blockIdx.z;
    const ShardView zv = shard_view(T, G, SS, SZ, q, c);
    const App app = load_app(apps, a);
    const int64_t K = app.k;
    const ShardSums GS = shard_sums(all_part + (size_t)c * n_apps, all_drv + (size_t)c * n_apps, (size_t)SZ.n_cand * n_apps, a,
                                    SS.shard[q], SS.n_shards);
    if (GS.pos == GF_NO_NODE || K == 0) return;
    uint32_t* out = exec2 + (size_t)c * half + app.exec_off;
    int64_t taken = GS.before_cap;
    if (taken >= K) return;
    // slot_of: sub-slot -> slot (the compact gpu table), nullptr when j is a slot of the full table already
    auto visit = [&](const GlobalView& V, uint32_t n_x, const uint32_t* __restrict__ slot_of, uint32_t ds, uint32_t j, bool in) {
        int32_t cp = 0;
        int64_t a0, a1, a2;
        if (load_with_cand<false>(V, j, n_x, a0, a1, a2) && in) {
            if (j == ds) {
                a0 -= app.drv0;
                a1 -= app.drv1;
                a2 -= app.drv2;
            }
            if (cap_ge1(a0, a1, a2, app)) cp = cap3(a0, a1, a2, app);
        }
        const int32_t incl = wave_inclusive_scan(cp);  // pack_tightly.go:45-61, continued from the ranges before this one
        const int32_t tot = read_lane(incl, kWave - 1);
        if (tot > 0) {
            const int64_t start = taken + (int64_t)(incl - cp);
            const int64_t room = K - start;
            const int32_t t = room <= 0 ? 0 : (room < (int64_t)cp ? (int32_t)room : cp);
            uint32_t id = 0;
            if (t > 0) id = (slot_of != nullptr ? slot_of[j] : j) + 1u;
            emit_runs(out, start, t, id, lane);
        }
        taken += tot;
        return taken < K;
    };
    if (G.n_x != 0 && app.exe2 > 0) {  // wave-uniform: the range's part of the view's sub-slots of the compact gpu table
        GlobalView VS = shard_sparse_view(G);
        VS.xm = VS.dm = zv.gxm;
        const uint32_t ds_sub = G.sub_of_slot[GS.pos];
        if (zv.g_lo < zv.g_hi)
            shard_scan_range(VS, zv.g_lo, zv.g_hi, app.exe0, app.exe1, app.exe2, lane,
                             [&](uint32_t j, bool in) { return visit(VS, G.n_x, G.slot_of_sub, ds_sub, j, in); });
    } else if (zv.c_lo < zv.c_hi) {
        const GlobalView V{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks, zv.xm, zv.dm,
                           T.n_chunks};
        shard_scan_range(V, zv.c_lo * kWave, zv.c_hi * kWave, app.exe0, app.exe1, app.exe2, lane,
                         [&](uint32_t j, bool in) { return visit(V, T.n_x, nullptr, GS.pos, j, in); });
    }
}

// The zone-aware packers' finish, after the all-reduce: a workgroup per application, a wavefront per candidate view (as in
// fit_zoned_fused_kernel).  Each wavefront turns its view's placement back into slots, computes the zone's average Max from
// them with the one-launch kernel's device functions — the same additions in the same order — and leaves its verdict in LDS;
// then chooseBestResult (single_az.go:75-97: strict < from 0.0, the first zone of the evaluation list on a tie), the az-aware
// fallback to the plain view (az_aware_pack_tightly.go:33-37), the result record, and the winner's slots translated to node
// ids into region 0 = [exec_off, exec_off + K) of the buffer (zeros when nothing won).
// (ALGO: the packer that made the views' placements — minimal-fragmentation leaves the executors out of the `reserved` map the
// averages are taken on, minimal_fragmentation.go:59-91)
template <bool AZ_AWARE, int ALGO = GF_ALGO_TIGHTLY_PACK>
__global__ __launch_bounds__(kWave* kFusedWaves) void shard_finish_zoned_kernel(
    NodeTable T, ShardZones SZ, uint32_t n_shards, uint32_t n_apps, const gf_app* __restrict__ apps,
    const gf_shard_partial* __restrict__ all_part, const gf_shard_driver* __restrict__ all_drv, gf_result* __restrict__ results,
    uint32_t* __restrict__ exec2, uint64_t half) {
    __shared__ FusedShared sh;
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t a = blockIdx.x;
    if (a >= n_apps) return;
    const uint32_t n_zone_cand = SZ.n_zones, n_cand = SZ.n_cand;  // (the host guarantees n_cand <= 64)
    const EffView EV{T.cpu, T.mem, T.gpu, SZ.sched, SZ.sched + T.n_slots, SZ.sched + 2 * (size_t)T.n_slots};
    const App app = load_app(apps, a);
    const int64_t K = app.k;
    for (uint32_t c = wave; c < n_cand; c += kFusedWaves) {
        const ShardSums GS = shard_sums(all_part + (size_t)c * n_apps, all_drv + (size_t)c * n_apps, (size_t)n_cand * n_apps, a, 0,
                                        n_shards);
        const bool feasible = GS.pos != GF_NO_NODE;
        // A wrong exchange (what the multi-device context's self-check exists to catch) may leave entries no shard wrote, or a bad
        // driver record: such slots become the sentinel slot, so that the answer is wrong but every table read stays in bounds.
        const uint32_t last = T.n_slots - 1u;
        const uint32_t ds = GS.pos < last ? GS.pos : last;
        double avg[4] = {0.0, 0.0, 0.0, 0.0};
        if (feasible) {
            uint32_t* out = exec2 + (size_t)c * half + app.exec_off;
            for (int64_t i = lane; i < K; i += kWave) {  // slot + 1 -> slot
                const uint32_t s = out[i] - 1u;
                out[i] = s < last ? s : last;
            }
            if (c < n_zone_cand) {
                // out[] was written by other lanes of this wave
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                bool done = false;
                if (ALGO == GF_ALGO_TIGHTLY_PACK && K >= 1 && K <= (int64_t)kRunBlocks * kWave)
                    done = wave_avg_max_tight_runs(EV, app, ds, out, lane, (lds_u32*)&sh.runs[wave][0], avg[3]);
                if (!done) wave_avg_efficiency_runs<ALGO>(EV, app, ds, out, lane, avg);
            }
        }
        if (lane == 0) {
            sh.feas[c] = feasible ? 1 : 0;
            sh.ds[c] = ds;
            sh.mx[c] = avg[3];
        }
    }
    __syncthreads();  // every view's verdict (LDS) and placement (global, same compute unit) is visible to every wavefront
    int32_t best = -1;
    double best_max = 0.0;
    for (uint32_t c = 0; c < n_zone_cand; ++c)
        if (sh.feas[c] && best_max < sh.mx[c]) {
            best = (int32_t)c;
            best_max = sh.mx[c];
        }
    if (AZ_AWARE && best < 0 && sh.feas[n_zone_cand]) best = (int32_t)n_zone_cand;
    const bool feasible = best >= 0;
    uint32_t* dst = exec2 + app.exec_off;
    if (feasible) {
        const uint32_t* src = exec2 + (size_t)best * half + app.exec_off;  // (best == 0: each thread rewrites its own entries)
        for (int64_t i = tid; i < K; i += kWave * kFusedWaves) dst[i] = T.slot_node[src[i]];
    } else {
        for (int64_t i = tid; i < K; i += kWave * kFusedWaves) dst[i] = 0u;
    }
    if (tid == 0) {
        gf_result r;
        r.has_capacity = feasible ? 1 : 0;
        r.driver_node = feasible ? T.slot_node[sh.ds[best]] : GF_NO_NODE;
        r.exec_len = feasible ? (uint32_t)K : 0u;
        r.evaluated = 1;
        results[a] = r;
    }
}

// ---- the minimal-fragmentation packers (minimal_fragmentation.go:59-137; single_az.go:23-97 with it as the inner packer)
// "The smallest capacity >= K" is a minimum over every candidate: the packer cannot stop early, every application walks the
// whole executor order, and that walk divides by the number of shards.  team_minfrag_hist (gangfit_minfrag.inc) already has the
// shape — a quarter of the order per wavefront, per-quarter count rows, one plan from their sum, every quarter emits its runs
// from "how many nodes of every capacity precede my quarter" —; a shard is a quarter whose rows travel through the first exchange
// instead of LDS:
//
//   counts   (kernel 1)  tightly-pack's S_s over the range, with no early stop (feasibility and the driver rule are tightly-pack's:
//                        internalMinimalFragmentation succeeds <=> sum of min(cap, K) >= K), and a COUNT ROW: for every capacity
//                        c in 1 .. 255 the executor candidates of the range with cap(n, nothing reserved) = c, counted in the
//                        snapshot's scaled int32 domain as pass 1 of wave_minfrag_hist does.  kMfRowWords words: uint16 counts,
//                        lane l's bins 4l .. 4l+3 in words 2l, 2l+1.  fit_count of the record = 1 says "no histogram form": a
//                        capacity >= 256 in the range, a request or a snapshot without scaled form, a range of 65 536 slots or more
//       -- all-gather [n_shards][views][n_apps] x (16 B + 512 B) --
//   drivers  (kernel 2)  shard_drivers_kernel / shard_drivers_zoned_kernel as they are
//       -- all-gather x 16 B --
//   emit     (kernel 3)  the winning driver slot d is the minimum over shards; every shard holds the whole table, reads slot d
//                        itself, c0 = cap(d, 0), c1 = cap(d, drv), and patches [c0]--, [c1]++ into the summed rows when d is an
//                        executor candidate of the view — and into its prefix (the rows of the shards before it) when d lies in an
//                        earlier range.  The plan is team_minfrag_hist's; pass 2 runs over the shard's own range with the driver
//                        reserved at d, a node's rank in its level = prefix + running count, and the shard writes only its own
//                        runs (node + 1; slot + 1 for the zone views).  The ONE node that takes everything, or what the drained
//                        levels leave, is named by the plan as (level, rank): the shard whose range holds it emits it.
//                        Applications some shard flagged "no histogram form" are decided by shard  a mod n_shards  alone, over
//                        the FULL order with wave_minfrag's walk and the known driver; the other shards write nothing.
//       -- all-reduce(SUM) of the placement buffer --
//   finish   (kernel 4)  plain: shard_finish_kernel<tightly-pack> (node + 1 -> node); single-AZ: shard_finish_zoned_kernel with
//                        minimal-fragmentation's averages.
// Gangs of gpu executors take the full range (the scaled columns exist for the full table only; the compact gpu view would give
// the same answers).
constexpr uint32_t kMfRowWords = kMfHistBins / 2;    // a count row: kMfHistBins uint16 counts
constexpr uint32_t kMfRowMaxSlots = 65536;           // ... exact below this many slots in the range
static_assert(kMfRowWords * sizeof(uint32_t) == kShardMfRowBytes, "the count row of gf_shard_mf_layout");

// MfNarrow's fields as LANE values for a pass (wave_minfrag_hist says why)
#define GF_MF_PIN(nv)  \
    GF_HERE(nv.drv0);  \
    GF_HERE(nv.drv1);  \
    GF_HERE(nv.drv2);  \
    GF_HERE(nv.exe0);  \
    GF_HERE(nv.exe1);  \
    GF_HERE(nv.exe2);  \
    GF_HERE(nv.mag0);  \
    GF_HERE(nv.mag1);  \
    GF_HERE(nv.mag2);  \
    GF_HERE(nv.sh0);   \
    GF_HERE(nv.sh1);   \
    GF_HERE(nv.sh2);   \
    GF_HERE(nv.un0);   \
    GF_HERE(nv.un1);   \
    GF_HERE(nv.un2)

// Counts of view c = blockIdx.z (the plain packer: the one view): the range's capacity sum and count row.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void shard_mf_counts_kernel(NodeTable T, ShardSet SS, ShardZones SZ, uint32_t n_apps,
                                                                               const gf_app* __restrict__ apps,
                                                                               gf_shard_partial* __restrict__ part,
                                                                               uint32_t* __restrict__ counts, PeerPtrs part_dsts,
                                                                               PeerPtrs cnt_dsts) {
    typedef uint32_t mf_u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) mf_u32x4 lds_mf4;
    __shared__ __attribute__((aligned(16))) uint32_t hist[kWavesPerBlock * kMfHistBins];
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= n_apps) return;
    const uint32_t q = blockIdx.y, c = blockIdx.z;
    const ShardView zv = shard_view(T, SparseTable{}, SS, SZ, q, c);
    const App app = load_app(apps, a);
    const int64_t K = app.k;
    const GlobalView V{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks, zv.xm, zv.dm, T.n_chunks};
    Orders O{T.slot_node, T.dslot, T.n_x, T.n_d, true};
    lds_u32* const A = (lds_u32*)hist + (size_t)wave * kMfHistBins;
    O.lend_minfrag(A, T);
    lds_mf4* const A4 = (lds_mf4*)A;
    A4[lane] = mf_u32x4{0u, 0u, 0u, 0u};
    MfNarrow na;
    // (wave-uniform) the request and the snapshot have a scaled form, and uint16 counts cannot wrap
    bool hist_ok = T.ncpu != nullptr && mf_narrow_app(app, O, na) && (zv.c_hi - zv.c_lo) * (uint32_t)kWave < kMfRowMaxSlots;
    const bool walk = K != 0 && zv.c_lo < zv.c_hi;
    if (hist_ok && walk) {
        MfNarrow nv = na;
        GF_MF_PIN(nv);
        int32_t cmax = 0;
        mf_for_each_chunk_narrow(V, O, app, nv, GF_NO_NODE, lane, [&](uint32_t, int32_t cp) {
            cmax = cp > cmax ? cp : cmax;
            const bool binned = cp > 0 && cp < kMfHistBins;
            const uint32_t n_run = mf_run_heads((uint32_t)cp, binned, lane);  // (pass 1 of wave_minfrag_hist: a run speaks through its first lane)
            if (n_run != 0u) __hip_atomic_fetch_add(A + (uint32_t)cp, n_run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return true;
        }, zv.c_lo, zv.c_hi);
        if (__ballot(cmax >= kMfHistBins) != 0ull) hist_ok = false;
    }
    int64_t S = 0;
    uint32_t cn[4] = {0u, 0u, 0u, 0u};
    if (hist_ok) {
        const mf_u32x4 c4 = A4[lane];  // (LDS operations of a wavefront execute in order)
        cn[0] = c4.x;
        cn[1] = c4.y;
        cn[2] = c4.z;
        cn[3] = c4.w;
        // (the range holds fewer than 2^16 slots of capacity below 2^8: the sum stays below 2^24 — 65 472 x 255 at most, the second
        // range of tests/test_gpu_sharded_minfrag.py::test_range_of_1023_and_1024_chunks[2046-255]; 1024 chunks are flagged: [2047-1])
        int64_t lsum = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t cp = 4 * lane + i;
            lsum += (int64_t)cn[i] * (cp < K ? cp : K);
        }
        S = wave_sum_small(lsum);
    } else if (walk) {  // the wide table, as shard_partials_zoned_kernel
        shard_scan_range(V, zv.c_lo * kWave, zv.c_hi * kWave, app.exe0, app.exe1, app.exe2, lane, [&](uint32_t j, bool in) {
            int32_t cp = 0;
            int64_t a0, a1, a2;
            if (load_with_cand<false>(V, j, T.n_x, a0, a1, a2) && in) {
                if (cap_ge1(a0, a1, a2, app)) cp = cap3(a0, a1, a2, app);
            }
            S += read_lane(wave_inclusive_scan(cp), kWave - 1);
            return S < 2 * K;
        });
    }
    const uint32_t n_cand = gridDim.z;
    const size_t rec_loc = (size_t)(q * n_cand + c) * n_apps + a, rec_all = (size_t)(SS.shard[q] * n_cand + c) * n_apps + a;
    const uint2 w = make_uint2(cn[0] | (cn[1] << 16), cn[2] | (cn[3] << 16));
    if (cnt_dsts.n == 0) {
        reinterpret_cast<uint2*>(counts + rec_loc * kMfRowWords)[lane] = w;
    } else {
        for (uint32_t t = 0; t < cnt_dsts.n; ++t)
            reinterpret_cast<uint2*>(reinterpret_cast<uint32_t*>(cnt_dsts.p[t]) + rec_all * kMfRowWords)[lane] = w;
    }
    if (lane == 0) {
        gf_shard_partial p;
        p.cap_sum = S;
        p.fit_count = hist_ok ? 0 : 1;  // "no histogram form"
        shard_publish(p, part_dsts, part, q * n_cand + c, SS.shard[q] * n_cand + c, n_apps, a);
    }
}

// Emit of view c: the shard's slice of the view's minimal-fragmentation placement into region c of the buffer (node + 1 for the
// plain packer, which also gets its result record here; slot + 1 for the zone views, whose finish step chooses).
template <bool ZONED>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void shard_mf_emit_kernel(
    NodeTable T, ShardSet SS, ShardZones SZ, uint32_t n_apps, const gf_app* __restrict__ apps,
    const gf_shard_partial* __restrict__ all_part, const gf_shard_driver* __restrict__ all_drv,
    const uint32_t* __restrict__ all_cnt, gf_result* __restrict__ results, uint32_t* __restrict__ exec2, uint64_t half) {
    typedef uint32_t mf_u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) mf_u32x4 lds_mf4;
    __shared__ __attribute__((aligned(16))) uint32_t hist[kWavesPerBlock * 3 * kMfHistBins];
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= n_apps) return;
    const uint32_t q = blockIdx.y, c = blockIdx.z, n_cand = gridDim.z, shard = SS.shard[q], n_shards = SS.n_shards;
    const ShardView zv = shard_view(T, SparseTable{}, SS, SZ, q, c);
    const App app = load_app(apps, a);
    const int64_t K = app.k;
    const size_t row = (size_t)n_cand * n_apps, rec = (size_t)c * n_apps + a;  // records between two shards' rows | this view's
    uint32_t pos = GF_NO_NODE;
    bool flagged = false;
    for (uint32_t t = 0; t < n_shards; ++t) {  // (wave-uniform scalar loops over shards, as shard_sums)
        const uint32_t p = all_drv[(size_t)t * row + rec].pos;
        pos = p < pos ? p : pos;
        flagged = flagged || all_part[(size_t)t * row + rec].fit_count != 0;
    }
    const bool feasible = pos < T.n_slots;  // (GF_NO_NODE, or what a wrong exchange left: no table read goes out of bounds)
    if (!ZONED && lane == 0 && q == 0) {  // (every hosted shard derives the same record: the first grid row stores it)
        gf_result r;
        r.has_capacity = feasible ? 1 : 0;
        r.driver_node = feasible ? T.slot_node[pos] : GF_NO_NODE;
        r.exec_len = feasible ? (uint32_t)K : 0u;
        r.evaluated = 1;
        results[a] = r;
    }
    if (!feasible || K == 0) return;
    uint32_t* out = exec2 + (size_t)c * half + app.exec_off;
    const GlobalView V{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks, zv.xm, zv.dm, T.n_chunks};
    Orders O{T.slot_node, T.dslot, T.n_x, T.n_d, true};
    if (flagged) {  // no histogram form in some range: ONE shard decides over the full order with the walk, the others write nothing
        if (shard != a % n_shards) return;
        unsigned long long visited = 0;
        (void)wave_minfrag<GlobalView, true>(V, O, app, pos, out, lane, visited);  // (no LDS lent: the walk) slots into out[0, K)
        // out[] was written by other lanes of this wave
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const uint32_t last = T.n_slots - 1u;
        for (int64_t i = lane; i < K; i += kWave) {
            const uint32_t s = out[i] < last ? out[i] : last;
            out[i] = (ZONED ? s : T.slot_node[s]) + 1u;
        }
        return;
    }
    lds_u32* const A = (lds_u32*)hist + (size_t)wave * 3 * kMfHistBins;  // plan: nodes a level gives completely
    lds_u32* const B = A + kMfHistBins;                                  // plan: where the level's runs start in out[]
    lds_u32* const C = A + 2 * kMfHistBins;                              // pass 2: nodes of the level seen so far (starts at the prefix)
    O.lend_minfrag(A, T);
    MfNarrow na;
    if (T.ncpu == nullptr || !mf_narrow_app(app, O, na)) return;  // (every shard would have flagged it)
    // ---- the driver's node before and after the reservation (every shard holds the whole table)
    const bool d_x = pos < T.n_x && V.xcand(pos);
    int32_t c0 = 0, c1 = 0;
    if (d_x) {
        const int32_t a0 = T.ncpu[pos], a1 = T.nmem[pos], a2 = T.ngpu[pos];
        c0 = mf_ncap_of(true, a0, a1, a2, na, GF_NO_NODE, pos);
        c1 = mf_ncap_of(true, a0, a1, a2, na, pos, pos);
        if (c0 >= kMfHistBins || c1 >= kMfHistBins) return;  // (its range flagged it, unless a wrong exchange lost the flag: see below)
    }
    const uint32_t d_chunk = pos / kWave;
    const bool d_before = d_x && d_chunk < SS.c_lo[q], d_mine = d_x && d_chunk >= SS.c_lo[q] && d_chunk < SS.c_hi[q];
    // ---- the global counts, this range's prefix and its own counts (lane l: bins 4l .. 4l+3), with the driver's node moved
    uint32_t cn[4] = {0u, 0u, 0u, 0u}, pre[4] = {0u, 0u, 0u, 0u}, own[4] = {0u, 0u, 0u, 0u};
    for (uint32_t t = 0; t < n_shards; ++t) {
        const uint2 w = reinterpret_cast<const uint2*>(all_cnt + ((size_t)t * row + rec) * kMfRowWords)[lane];
        const uint32_t cv[4] = {w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            cn[i] += cv[i];
            if (t < shard) pre[i] += cv[i];
            if (t == shard) own[i] = cv[i];
        }
    }
    // (a wrong exchange — what the multi-device context's self-check exists to catch — may leave rows that do not hold the driver's
    // node: the counts then stay at zero instead of wrapping, the answer is wrong, and every store stays inside out[0, K))
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int32_t bin = 4 * lane + i;
        const uint32_t add = (c1 > 0 && bin == c1) ? 1u : 0u, sub = (c0 > 0 && bin == c0) ? 1u : 0u;
        cn[i] += add;
        cn[i] -= sub < cn[i] ? sub : cn[i];
        if (d_before) {
            pre[i] += add;
            pre[i] -= sub < pre[i] ? sub : pre[i];
        }
        if (d_mine) {
            own[i] += add;
            own[i] -= sub < own[i] ? sub : own[i];
        }
    }
    // ---- the plan, by every shard alike: team_minfrag_hist's, on registers
    int64_t lmax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (cn[i] != 0u) lmax = 4 * lane + i;
    const int64_t max_cap = wave_max_i64(lmax);
    int64_t top = kMfHistBins;  // admitted: 0 < capacity < top
    if (K < max_cap) {          // "avoid mostly empty nodes" (:68-78)
        const int64_t target = (K + max_cap) / 2;
        int64_t lsub = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t cp = 4 * lane + i, cc = cp < K ? cp : K;
            const int64_t add = cp < target ? (int64_t)cn[i] * cc : 0;
            lsub = lsub + add < K ? lsub + add : K;
        }
        if (wave_sum_small(lsub) >= K) top = target;
    }
    auto smallest_at_least = [&](int64_t need, int64_t below) {
        int64_t l = kCapInf;
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            const int64_t cp = 4 * lane + i;
            if (cn[i] != 0u && cp < below && cp >= need) l = cp;
        }
        return wave_min_i64(l);
    };
    auto largest_below = [&](int64_t below) {
        int64_t l = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t cp = 4 * lane + i;
            if (cn[i] != 0u && cp < below) l = cp;
        }
        return wave_max_i64(l);
    };
    lds_mf4* const A4 = (lds_mf4*)A;
    lds_mf4* const B4 = (lds_mf4*)B;
    lds_mf4* const C4 = (lds_mf4*)C;
    A4[lane] = mf_u32x4{0u, 0u, 0u, 0u};
    B4[lane] = mf_u32x4{0u, 0u, 0u, 0u};
    C4[lane] = mf_u32x4{pre[0], pre[1], pre[2], pre[3]};
    int64_t R = K;
    // the ONE node that takes everything (:103-110) or what the drained levels leave: the node of rank tgt_rank of level tgt_level
    int64_t tgt_level = -1;
    uint32_t tgt_rank = 0;
    {
        const int64_t cf = smallest_at_least(R, top);
        if (cf != kCapInf) tgt_level = cf;
    }
    while (tgt_level < 0) {  // several nodes: the level walk (:113-130)
        const int64_t m = largest_below(top);
        if (m <= 0) return;  // unreachable for a feasible gang; guards against a non-terminating walk
        const uint32_t cnt = mf_bin(cn, (uint32_t)m);
        const uint32_t qn = (uint32_t)R / (uint32_t)m;
        const uint32_t drained = cnt < qn ? cnt : qn;
        A[(uint32_t)m] = drained;  // (every lane stores the same word)
        B[(uint32_t)m] = (uint32_t)(K - R);
        R -= (int64_t)drained * m;
        if (R == 0) break;
        if (drained < cnt) {  // R < m: the smallest capacity >= R among the lower levels, else the first undrained node of this level
            const int64_t cf = smallest_at_least(R, m);
            tgt_level = cf != kCapInf ? cf : m;
            tgt_rank = cf != kCapInf ? 0u : drained;
            break;
        }
        top = m;  // :130 the drained level leaves the list
        const int64_t cf = smallest_at_least(R, top);
        if (cf != kCapInf) tgt_level = cf;
    }
    // what the plan wants from THIS range: of every drained level the nodes with ranks [pre, pre + own) below `taken`, and the
    // target when its rank lies in here
    uint32_t left;
    {
        const mf_u32x4 t4 = A4[lane];  // (behind the stores above: LDS operations of a wavefront execute in order)
        const uint32_t tk[4] = {t4.x, t4.y, t4.z, t4.w};
        int64_t want = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t ahead = tk[i] > pre[i] ? tk[i] - pre[i] : 0u;
            want += (int64_t)(ahead < own[i] ? ahead : own[i]);
            if ((int64_t)(4 * lane + i) == tgt_level && tgt_rank >= pre[i] && tgt_rank < pre[i] + own[i]) want += 1;
        }
        left = (uint32_t)wave_sum_small(want);
    }
    if (left == 0u || zv.c_lo >= zv.c_hi) return;
    // ---- pass 2 over the own range, the driver reserved at d
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    MfNarrow nv = na;
    GF_MF_PIN(nv);
    mf_for_each_chunk_narrow(V, O, app, nv, pos, lane, [&](uint32_t j, int32_t cp) {
        const bool binned = cp > 0 && cp < kMfHistBins;
        const uint32_t cb = binned ? (uint32_t)cp : 0u;  // (bin 0 is nobody's level: its words are zero)
        const uint32_t take = A[cb], base = B[cb], seen = C[cb];
        const bool act = binned && (take != 0u || (int64_t)cp == tgt_level);
        if (__ballot(act) == 0ull) return true;
        const uint64_t peers = mf_peers8((uint32_t)cp, act);
        const uint32_t rk = seen + (uint32_t)__popcll((unsigned long long)(peers & lt_mask));
        if (act && (peers & lt_mask) == 0ull) C[cb] = seen + (uint32_t)__popcll((unsigned long long)peers);  // the peers' leader
        const bool drain = act && rk < take;
        const bool tgt = act && (int64_t)cp == tgt_level && rk == tgt_rank;
        uint32_t id = 0;
        if (drain || tgt) id = (ZONED ? j : T.slot_node[j]) + 1u;
        emit_runs(out, (int64_t)base + (int64_t)rk * cp, drain ? cp : 0, id, lane);  // :122
        const uint64_t tm = __ballot(tgt);
        if (tm) {  // :106-109 R copies behind the drained levels' runs
            const uint32_t tid = read_lane(id, __ffsll((unsigned long long)tm) - 1);
            for (int64_t i = lane; i < R; i += kWave) out[K - R + i] = tid;
        }
        left -= (uint32_t)__popcll((unsigned long long)__ballot(drain)) + (tm ? 1u : 0u);
        return left != 0u;
    }, zv.c_lo, zv.c_hi);
}
#undef GF_MF_PIN

// ---- the exchanges of the in-process multi-device context (gf_init with n_dev > 1): peer access over xGMI instead of a
// collective library.  The messages are KB-sized, so what matters is the number of round trips, not bandwidth:
//   push   (all-gather)  the producing kernels (partials, drivers) write their 16-byte records straight into row `shard` of
//                        EVERY device's gathered table (shard_publish) — posted stores over the fabric, no reply needed, no
//                        kernel of their own;
//   pull   (reduce)      only shard 0 finishes the batch, so the all-reduce(SUM) of the placement buffer becomes a reduce:
//                        shard 0 reads the other shards' buffers (each over its own xGMI link) and adds them to its own.
// Ordering between devices is by kernel boundaries: HIP events recorded behind the producing kernel, waited for by the
// consuming stream (system-scope release at kernel end / acquire at kernel start).
__global__ __launch_bounds__(256) void shard_reduce_pull_kernel(PeerPtrs srcs, uint32_t* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t acc = dst[i];
        for (uint32_t t = 0; t < srcs.n; ++t) acc += reinterpret_cast<const uint32_t*>(srcs.p[t])[i];
        dst[i] = acc;
    }
}
