// gangfit_filter_eff.inc — the cluster-wide average packing efficiency of ONE result (included last by gangfit_kernels.hip;
// node_efficiency and reserved_scatter_kernel live in gangfit_zones.inc).  Both kernels are templates and their launcher is the last
// function of gangfit_kernels.hip, so that they are instantiated — and laid out in the code object — behind every other kernel.
//
//   computeAvgPackingEfficiencyForResult   internal/extender/resource.go:372-381
//   ComputeAvgPackingEfficiency            LIB/binpack/efficiency.go:114-156, over one PackingEfficiency per metadata KEY
//
// The reference sums in Go map-range order, which is unspecified; this sum is a FIXED tree, a function of (n_nodes, member row,
// per-node values) alone — not of the grid, not of which workgroup finishes first, no floating-point atomics:
//   level 1  chunk c = nodes 64c .. 64c + 63, lane l owns node 64c + l; a lane whose node is no key (not a member, or past
//            n_nodes) contributes +0.0.  The chunk's partial is wave_sum_f64's balanced binary tree over the 64 lanes
//            (lanes 2i and 2i + 1 first, then pairs of pairs, ... six levels).
//   level 2  the partial of chunk c goes to part[field][c]; the array is padded with +0.0 to a whole number of 64-chunk groups.
//   level 3  one wavefront: lane l adds part[l], part[l + 64], part[l + 128], ... in ascending order onto +0.0, then the same
//            balanced tree over the 64 lanes.
// The four fields (cpu, memory, gpu over the keys with a schedulable gpu, max) share the tree; the two counts are integers.
//
// A workgroup takes a group of 64 chunks (4 096 nodes): every lane loads the member word of chunk 64 g + l — one coalesced
// 512-byte load per wavefront, as in cluster_scan_sets_kernel —, wavefront w visits the chunks 8w .. 8w + 7 of the group whose word
// is not zero (the word reaches the lanes through read_lane64), and lane b keeps the partial of the group's chunk b until the
// group's coalesced store.  A zero word costs nothing beyond its load: a non-member's columns are never read.

constexpr uint32_t kFeWaves = 8;                      // wavefronts per workgroup
constexpr uint32_t kFeChunksPerWave = kWave / kFeWaves;  // chunks of a group each of them visits

// RESIDUAL: the available quantities of a node that owns a slot come from the chain's working table.
template <bool RESIDUAL>
__global__ __launch_bounds__(kWave* kFeWaves) void filter_efficiency_partials_kernel(FilterEffArgs A) {
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n_groups = A.n_pad / kWave;
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const uint32_t c = grp * kWave + (uint32_t)lane;  // this lane's chunk
        uint64_t word = 0ull;
        if (c < A.n_words) {
            word = A.members != nullptr ? A.members[c] : ~0ull;
            word &= low_lanes(A.n_nodes - c * kWave);  // the ragged last chunk (c < n_words: at least one node)
        }
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
        uint32_t p_len = 0, p_gpu = 0;
        uint64_t todo = __ballot(word != 0ull) & (((1ull << kFeChunksPerWave) - 1ull) << (wave * kFeChunksPerWave));
        while (todo != 0ull) {
            const int bit = (int)__ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1ull;
            const uint64_t chunk = read_lane64(word, (uint32_t)bit);
            const uint32_t n = (grp * kWave + (uint32_t)bit) * kWave + (uint32_t)lane;
            NodeEff e;
            e.cpu = e.mem = e.gpu = 0.0;
            double mx = 0.0;
            bool hg = false;
            if ((chunk >> lane) & 1ull) {  // a key: n < n_nodes
                int64_t a0 = A.tab.avail[0][n], a1 = A.tab.avail[1][n], a2 = A.tab.avail[2][n];
                if (RESIDUAL) {  // the chain's residual where the node owns a slot (gf_residual_get's rule)
                    const uint32_t s = A.node_slot[n];
                    if (s != GF_NO_NODE) {
                        a0 = A.work[s];
                        a1 = A.work[(size_t)A.n_slots + s];
                        a2 = A.work[2 * (size_t)A.n_slots + s];
                    }
                }
                const int64_t* r = A.reserved + 3 * (size_t)n;
                hg = node_efficiency(a0, a1, a2, A.tab.sched[0][n], A.tab.sched[1][n], A.tab.sched[2][n], r[0], r[1], r[2], e);
                const double m = e.cpu > e.mem ? e.cpu : e.mem;  // math.Max; no NaN / -0 can occur (divisors >= 1)
                mx = e.gpu > m ? e.gpu : m;
            }
            const double s0 = wave_sum_f64(e.cpu), s1 = wave_sum_f64(e.mem), s2 = wave_sum_f64(e.gpu), s3 = wave_sum_f64(mx);
            const uint64_t hgm = __ballot(hg);
            if (lane == bit) {
                p0 = s0;
                p1 = s1;
                p2 = s2;
                p3 = s3;
                p_len = (uint32_t)__popcll((unsigned long long)chunk);
                p_gpu = (uint32_t)__popcll((unsigned long long)hgm);
            }
        }
        if (((uint32_t)lane / kFeChunksPerWave) == wave) {  // c < n_pad
            A.part[c] = p0;
            A.part[(size_t)A.n_pad + c] = p1;
            A.part[2 * (size_t)A.n_pad + c] = p2;
            A.part[3 * (size_t)A.n_pad + c] = p3;
            A.part_cnt[c] = p_len;
            A.part_cnt[(size_t)A.n_pad + c] = p_gpu;
        }
    }
}

// Level 3 by one wavefront, then the result record; then the entries reserved_scatter_kernel touched are cleared again, so
// the dense `reserved` scratch is all-zero between calls without an O(n_nodes) memset per call.
// RESERVE_EXECS: as in reserved_scatter_kernel.
template <bool RESERVE_EXECS>
__global__ __launch_bounds__(kWave) void filter_efficiency_combine_kernel(FilterEffArgs A, const gf_app* __restrict__ app,
                                                                          const gf_result* __restrict__ res,
                                                                          const uint32_t* __restrict__ exec_nodes,
                                                                          int64_t* __restrict__ reserved,
                                                                          FilterEffOut* __restrict__ out) {
    const int lane = lane_id();
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t n_len = 0, n_gpu = 0;
    for (uint32_t c = (uint32_t)lane; c < A.n_pad; c += kWave) {  // ascending chunk order per lane
        a0 += A.part[c];
        a1 += A.part[(size_t)A.n_pad + c];
        a2 += A.part[2 * (size_t)A.n_pad + c];
        a3 += A.part[3 * (size_t)A.n_pad + c];
        n_len += (int64_t)A.part_cnt[c];
        n_gpu += (int64_t)A.part_cnt[(size_t)A.n_pad + c];
    }
    const double s0 = wave_sum_f64(a0), s1 = wave_sum_f64(a1), s2 = wave_sum_f64(a2), s3 = wave_sum_f64(a3);
    const int64_t len = wave_sum_i64(n_len), with_gpu = wave_sum_i64(n_gpu);
    if (lane == 0) {
        FilterEffOut o;
        if (len == 0) {  // WorstAvgPackingEfficiency (efficiency.go:119-121)
            o.avg[0] = o.avg[1] = o.avg[2] = o.avg[3] = 0.0;
        } else {
            const double l = (double)len;
            o.avg[0] = s0 / l;
            o.avg[1] = s1 / l;
            o.avg[2] = with_gpu == 0 ? 1.0 : s2 / (double)with_gpu;  // :141-145
            o.avg[3] = s3 / l;
        }
        o.counts[0] = (uint32_t)len;
        o.counts[1] = (uint32_t)with_gpu;
        *out = o;
    }
    if (!res->has_capacity) return;
    const uint32_t d = res->driver_node;
    if (lane < 3 && d < A.n_nodes) reserved[3 * (size_t)d + lane] = 0;
    if (RESERVE_EXECS) {
        const int64_t K = app->k;
        for (int64_t i = lane; i < K; i += kWave) {
            const uint32_t n = exec_nodes[app->exec_off + i];
            if (n < A.n_nodes) {
                reserved[3 * (size_t)n] = 0;
                reserved[3 * (size_t)n + 1] = 0;
                reserved[3 * (size_t)n + 2] = 0;
            }
        }
    }
}
