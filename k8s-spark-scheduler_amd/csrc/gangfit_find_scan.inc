// gangfit_find_scan.inc — findNodes of the failover reconciler answered from the resident cluster (gf_cluster_find_nodes;
// included by gangfit_kernels.hip).
//
//   availableResourcesPerInstanceGroup          internal/extender/failover.go:286-323
//   findNodes                                   internal/extender/failover.go:412-436
//   r.availableResources[ig].Sub(reserved)      internal/extender/failover.go:159  (CHAINED)
//
// The reconciler's table is allocatable - (usage + overhead) over the ready, schedulable nodes of an instance group, walked
// newest node first: the columns gf_cluster_set, gf_overhead_update and gf_usage_apply keep on the device, in an order the host
// hands over as one rank per node.  Three launches, none of which reads or writes anything of the installed snapshot:
//   prepare   perm[create_rank[n]] = n, and the call's private working table work[j * N + n] = alloc - (usage + over);
//   order     one wavefront per row some request names: 64 positions of perm a step, member test (row bit, ready, not
//             unschedulable), ballot + lane rank -> ord[base + fill + rank] = node.  A row's candidates become one dense list in
//             visiting order, built once per call; `base` comes from the row's popcount (an upper bound of the list's length);
//   walk      find_nodes_kernel's steps over that list: node ids by one coalesced load, the three values gathered from `work` by
//             node, then find_step.  CHAINED: one wavefront per row takes the row's requests in ascending q (the host groups them)
//             and subtracts each one's `reserved` map from work[node]; rows of two requests are equal (one row here) or disjoint, so
//             two wavefronts never meet on a node.  Not CHAINED: one wavefront per request, `work` is only read.
// The node ids of the NEXT kFindAhead steps are requested together with the gathers of the current ones: a batch costs one
// dependent round trip, not two.  A node is in a row's list once, so a CHAINED store never hits a value requested ahead.

//
// find_step restates the body of find_nodes_kernel's step.  That kernel does not call it: with the call in place its register row
// changed (100 -> 98 SGPRs), so it stays as it was, and tests/test_gpu_cluster_find_nodes.py holds the two kernels to each other
// through the installing route.

constexpr int kFindAhead = 4;

// One step of the walk: lane `lane` holds the available values of one candidate of the order (`cand`; node = its index), `taken`
// executors have been placed on the steps before.  Emits the step's placements and adds, moves `taken` and `last_node` on.
// Returns whether this lane's node was visited; `adds` is then what its `reserved` entry holds in units of exe.
__device__ __forceinline__ bool find_step(int64_t a0, int64_t a1, int64_t a2, bool cand, uint32_t node, const App& app, int64_t K, int lane,
                                          uint32_t* __restrict__ out, uint32_t* __restrict__ adds_row, int64_t& taken,
                                          uint32_t& last_node, int64_t& adds) {
    int32_t cp = 0;
    if (cand && cap_ge1(a0, a1, a2, app)) cp = cap3(a0, a1, a2, app);  // clamped to K
    const int32_t incl = wave_inclusive_scan(cp);
    const int32_t tot = read_lane(incl, kWave - 1);
    const int64_t start = taken + (int64_t)(incl - cp);
    const bool visited = cand && start < K;
    const int64_t room = K - start;
    const int32_t tt = !visited ? 0 : (room < (int64_t)cp ? (int32_t)room : cp);
    emit_runs(out, start, tt, node, lane);
    if (visited) {
        adds = start + (int64_t)cp < K ? (int64_t)cp + 1 : room;
        if (adds_row != nullptr) adds_row[node] = (uint32_t)adds;
    }
    const uint64_t vm = __ballot(visited);
    if (vm) last_node = read_lane(node, 63 - __builtin_clzll((unsigned long long)vm));
    taken += tot;
    return visited;
}

__global__ __launch_bounds__(kWave* kWavesPerBlock) void cluster_find_prepare_kernel(FindScanArgs A) {
    const uint32_t n = blockIdx.x * (uint32_t)(kWave * kWavesPerBlock) + threadIdx.x;
    if (n >= A.n_nodes) return;
    const size_t N = A.n_nodes;
    A.perm[A.create_rank[n]] = n;  // a permutation of 0 .. n_nodes - 1 (the entry point checks)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int64_t o = A.over != nullptr ? A.over[j * N + n] : 0;
        A.work[j * N + n] = A.alloc[j * N + n] - (A.usage[j * N + n] + o);
    }
}

__global__ __launch_bounds__(kWave* kWavesPerBlock) void cluster_find_order_kernel(FindScanArgs A) {
    const int lane = lane_id();
    const uint32_t row = blockIdx.x * kWavesPerBlock + uniform32(threadIdx.x >> 6);
    if (row >= A.n_rows) return;
    const uint64_t* const words = A.set_words != nullptr ? A.set_words + (size_t)uniform32(A.row_set[row]) * A.n_words : nullptr;
    uint32_t* const list = A.ord + uniform64(A.row_base[row]);
    uint32_t fill = 0;
    for (uint32_t p0 = 0; p0 < A.n_nodes; p0 += kWave) {
        const uint32_t p = p0 + (uint32_t)lane;
        bool member = p < A.n_nodes;
        uint32_t node = 0;
        if (member) {
            node = A.perm[p];
            if (words != nullptr) member = ((words[node >> 6] >> (node & 63u)) & 1ull) != 0ull;
        }
        if (member) {  // executor candidates: ready and not unschedulable (failover.go:296-314)
            const uint32_t fl = A.flags[node];
            member = (fl & GF_NODE_READY) != 0u && (fl & GF_NODE_UNSCHEDULABLE) == 0u;
        }
        const uint64_t mm = __ballot(member);
        if (member) list[fill + (uint32_t)__popcll(mm & low_lanes((uint32_t)lane))] = node;
        fill += (uint32_t)__popcll(mm);
    }
    if (lane == 0) A.row_len[row] = fill;
}

template <bool CHAINED>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void cluster_find_nodes_kernel(FindScanArgs A) {
    const int lane = lane_id();
    const uint32_t unit = blockIdx.x * kWavesPerBlock + uniform32(threadIdx.x >> 6);
    if (unit >= (CHAINED ? A.n_rows : A.n_req)) return;
    const uint32_t row = CHAINED ? unit : uniform32(A.req_row[unit]);
    uint32_t i = CHAINED ? uniform32(A.row_req[row]) : unit;
    const uint32_t i_end = CHAINED ? uniform32(A.row_req[row + 1]) : unit + 1u;
    const uint32_t* const list = A.ord + uniform64(A.row_base[row]);
    const uint32_t len = uniform32(A.row_len[row]);
    const uint32_t xc = (len + kWave - 1) / kWave;
    const size_t N = A.n_nodes;
    int64_t* const w0 = A.work;
    int64_t* const w1 = A.work + N;
    int64_t* const w2 = A.work + 2 * N;
    for (; i < i_end; ++i) {
        const uint32_t q = CHAINED ? uniform32(A.req_list[i]) : i;
        App app{};
        app.exe0 = A.exe[3 * (size_t)q];
        app.exe1 = A.exe[3 * (size_t)q + 1];
        app.exe2 = A.exe[3 * (size_t)q + 2];
        app.rcp0 = app.exe0 > 0 ? 1.0 / (double)app.exe0 : 0.0;
        app.rcp1 = app.exe1 > 0 ? 1.0 / (double)app.exe1 : 0.0;
        app.rcp2 = app.exe2 > 0 ? 1.0 / (double)app.exe2 : 0.0;
        app.k = A.k[q];
        const int64_t K = app.k;
        uint32_t* out = A.exec_nodes + A.exec_off[q];
        uint32_t* adds_row = A.adds_out != nullptr ? A.adds_out + (size_t)q * N : nullptr;
        int64_t taken = 0;
        uint32_t last_node = GF_NO_NODE;
        uint32_t bnode[kFindAhead], ahead[kFindAhead];
#pragma unroll
        for (int t = 0; t < kFindAhead; ++t) {
            const uint32_t j = (uint32_t)t * kWave + (uint32_t)lane;
            bnode[t] = j < len ? list[j] : GF_NO_NODE;
        }
        for (uint32_t c0 = 0; c0 < xc && taken < K; c0 += kFindAhead) {
            int64_t b0[kFindAhead], b1[kFindAhead], b2[kFindAhead];
#pragma unroll
            for (int t = 0; t < kFindAhead; ++t) {
                b0[t] = b1[t] = b2[t] = 0;
                if (bnode[t] != GF_NO_NODE) {
                    b0[t] = w0[bnode[t]];
                    b1[t] = w1[bnode[t]];
                    b2[t] = w2[bnode[t]];
                }
                const uint32_t j = (c0 + (uint32_t)(kFindAhead + t)) * kWave + (uint32_t)lane;
                ahead[t] = j < len ? list[j] : GF_NO_NODE;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < kFindAhead; ++t) {
                const uint32_t c = c0 + (uint32_t)t;
                if (c >= xc || taken >= K) break;  // wave-uniform
                const uint32_t node = bnode[t];
                const int64_t a0 = b0[t], a1 = b1[t], a2 = b2[t];
                int64_t adds = 0;
                if (find_step(a0, a1, a2, node != GF_NO_NODE, node, app, K, lane, out, adds_row, taken, last_node, adds)) {
                    if (CHAINED) {  // NodeGroupResources.Sub (LIB/resources/resources.go:119-126)
                        w0[node] = a0 - adds * app.exe0;
                        w1[node] = a1 - adds * app.exe1;
                        w2[node] = a2 - adds * app.exe2;
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < kFindAhead; ++t) bnode[t] = ahead[t];
        }
        if (lane == 0) {
            gf_find_result r;
            r.placed = (uint32_t)(taken < K ? taken : K);
            r.last_node = last_node;
            A.results[q] = r;
        }
        if (CHAINED) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // this request's stores before the next one's loads
    }
}
