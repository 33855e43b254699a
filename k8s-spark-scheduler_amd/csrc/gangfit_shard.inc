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
template <bool AZ_AWARE>
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
                if (K >= 1 && K <= (int64_t)kRunBlocks * kWave)
                    done = wave_avg_max_tight_runs(EV, app, ds, out, lane, (lds_u32*)&sh.runs[wave][0], avg[3]);
                if (!done) wave_avg_efficiency_runs<GF_ALGO_TIGHTLY_PACK>(EV, app, ds, out, lane, avg);
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
