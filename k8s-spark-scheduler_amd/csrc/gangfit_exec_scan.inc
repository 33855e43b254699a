// gangfit_exec_scan.inc — the executor Filter answered from the resident cluster (gf_cluster_executor_fit; included by
// gangfit_kernels.hip).
//
//   rescheduleExecutor, first-fit loop                  internal/extender/resource.go:594-673 (:658-662)
//   rescheduleExecutorWithMinimalFragmentation          internal/extender/resource.go:675-703
//   getNodeNamesInPriorityOrder                         internal/sort/nodesorting.go:95-122
//
// The reference builds this Filter's metadata from the request's own node list (getNodes(nodeNames), narrowed by
// filterNodesToZone), so the zone ranks — sums over THAT subset — and with them the executor order differ from the installed
// driver snapshot's.  But the loop's answer needs no order: first-fit over a sorted list is the smallest key among the nodes
// that fit, and the minimal-fragmentation variant only ever replaces `best` strictly, i.e. it returns the lexicographic
// minimum of (not hosting the application, capacity, position).  Both are reductions over the columns gf_cluster_set,
// gf_overhead_update and gf_usage_apply keep on the device, read in NODE-INDEX order: no sort, no slot layout, no install.
//
// One workgroup of four wavefronts per request; wavefront w visits the 64-node steps w, w + 4, ...  S = the nodes of the
// request's set row that pass the zone test.
//   pass 1  the (memory, cpu) sums of available over S per cluster zone, in LDS; lane z then ranks zone z against the others
//           (memory, cpu, zone id: zone_rank_kernel's order).  Zones without a node of S hold zero and rank somewhere between
//           the others, which leaves the order AMONG the zones of S as it is.  Skipped when every node of S shares a rank.
//   pass 2  key(n) = (executor label rank, zone rank, available memory, available cpu, name rank) — what gf_snapshot_build
//           sorts by; name_rank is a permutation, so no two nodes share a key.  Every lane keeps the smallest candidate it has
//           seen, the wavefront reduces field after field with the DPP minimum, the four wavefronts meet in LDS.
// What is subtracted before the fit test (SURVEY.md quirk 5): first-fit — the node's overhead once more when at least one
// reservation entry names the node (`usage.Add(overhead)`, :642); minimal fragmentation — every node's overhead
// (GetNodeCapacities' reservedResources, :682).

constexpr int kExecZones = 64;
constexpr int kExecFields = 6;  // not hosting | capacity | label rank, zone rank | memory | cpu | name rank, node
constexpr int64_t kExecBias = INT64_MIN;  // x ^ kExecBias: unsigned order as signed order

struct ExecScanShared {
    unsigned long long zsum[2][kExecZones];       // memory | cpu of available over S, per cluster zone
    int64_t rec[kWavesPerBlock][kExecFields];     // every wavefront's smallest candidate
    uint32_t have[kWavesPerBlock];
    uint32_t zrank[kWavesPerBlock][kExecZones];   // zone id -> rank, every wavefront's own copy (no barrier between write and read)
};

// The 64 nodes of step c a wavefront must look at: the set row's word (wave-uniform, read once for the step), or every node.
__device__ __forceinline__ uint64_t exec_step_word(const uint64_t* row, uint32_t c, uint32_t n_nodes) {
    if (row != nullptr) return uniform64(row[c]);
    const uint32_t left = n_nodes - c * (uint32_t)kWave;
    return low_lanes(left);
}

template <bool MINFRAG>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void cluster_executor_fit_kernel(ExecScanArgs A) {
    __shared__ ExecScanShared sh;
    const int lane = lane_id();
    const uint32_t wave = uniform32(threadIdx.x >> 6);
    const uint32_t q = blockIdx.x;  // (the grid has n_req workgroups: every wavefront of one reaches every barrier below)
    const size_t N = A.n_nodes;
    App app{};
    app.exe0 = A.exe[3 * (size_t)q];
    app.exe1 = A.exe[3 * (size_t)q + 1];
    app.exe2 = A.exe[3 * (size_t)q + 2];
    app.k = 1;
    app.rcp0 = app.exe0 > 0 ? fast_rcp((double)app.exe0) : 0.0;
    app.rcp1 = app.exe1 > 0 ? fast_rcp((double)app.exe1) : 0.0;
    app.rcp2 = app.exe2 > 0 ? fast_rcp((double)app.exe2) : 0.0;
    const uint64_t* const row = A.set_words != nullptr ? A.set_words + (size_t)uniform32(A.req_set[q]) * A.n_words : nullptr;
    const uint32_t my_zone = A.req_zone != nullptr ? uniform32(A.req_zone[q]) : GF_ANY_ZONE;
    const uint32_t* const test_zone = A.node_zone != nullptr ? A.node_zone : A.zone;  // filterNodesToZone's label
    const uint32_t* const my_hosts = (MINFRAG && A.hosts != nullptr) ? A.hosts + (size_t)q * A.hosts_stride : nullptr;
    // every node of S has the same zone rank: one zone in the cluster, or a request confined to one of the cluster's own zones
    const bool ranked = A.n_zones > 1u && !(my_zone != GF_ANY_ZONE && A.node_zone == nullptr);

    // ---- pass 1: the zone sums of S
    if (ranked) {
        if (threadIdx.x < 2u * kExecZones) (&sh.zsum[0][0])[threadIdx.x] = 0ull;
        lds_barrier();
        for (uint32_t c = wave; c < A.n_words; c += kWavesPerBlock) {
            const uint64_t word = exec_step_word(row, c, A.n_nodes);
            if (word == 0ull) continue;  // none of the step's nodes is in the set: no column is read
            const uint32_t n = c * (uint32_t)kWave + (uint32_t)lane;
            bool in = ((word >> lane) & 1ull) != 0ull && n < A.n_nodes;
            if (in && my_zone != GF_ANY_ZONE) in = test_zone[n] == my_zone;
            int64_t mem = 0, cpu = 0;
            uint32_t z = 0;
            if (in) {
                const int64_t o0 = A.over != nullptr ? A.over[n] : 0, o1 = A.over != nullptr ? A.over[N + n] : 0;
                cpu = A.alloc[n] - (A.usage[n] + o0);
                mem = A.alloc[N + n] - (A.usage[N + n] + o1);
                z = A.zone[n];
            }
            // one pair of LDS atomics per zone present in the step, not per node: the wavefront adds up first
            uint64_t todo = __ballot(in);
            while (todo != 0ull) {
                const uint32_t zz = read_lane(z, (int)__ffsll((unsigned long long)todo) - 1);
                const bool mine = in && z == zz;
                todo &= ~__ballot(mine);
                const int64_t sm = wave_sum_i64(mine ? mem : 0), sc = wave_sum_i64(mine ? cpu : 0);
                if (lane == 0 && zz < (uint32_t)kExecZones) {
                    __hip_atomic_fetch_add((lds_ull*)&sh.zsum[0][zz], (unsigned long long)sm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add((lds_ull*)&sh.zsum[1][zz], (unsigned long long)sc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        lds_barrier();
        // resourcesLessThan over the zones (nodesorting.go:73-80): memory, then cpu, ascending; ties keep the zone-id order
        const int64_t zm = (int64_t)sh.zsum[0][lane], zc = (int64_t)sh.zsum[1][lane];
        uint32_t my_rank = 0;  // lane z: the zones that sort before zone z
        for (int p = 0; p < kExecZones; ++p) {
            const int64_t pm = (int64_t)sh.zsum[0][p], pc = (int64_t)sh.zsum[1][p];
            const bool before = pm != zm ? pm < zm : (pc != zc ? pc < zc : p < lane);
            my_rank += before ? 1u : 0u;
        }
        sh.zrank[wave][lane] = my_rank;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // (the other lanes of this wavefront read these ranks below)
    }

    // ---- pass 2: every lane's smallest candidate
    bool have = false;
    int64_t best[kExecFields];
#pragma unroll
    for (int f = 0; f < kExecFields; ++f) best[f] = INT64_MAX;
    for (uint32_t c = wave; c < A.n_words; c += kWavesPerBlock) {
        const uint64_t word = exec_step_word(row, c, A.n_nodes);
        if (word == 0ull) continue;
        uint64_t hword = 0ull;  // the step's 64 hosting bits, read once
        if (my_hosts != nullptr) {
            const uint32_t lo = uniform32(my_hosts[2 * c]);
            const uint32_t hi = 2 * c + 1 < A.hosts_stride ? uniform32(my_hosts[2 * c + 1]) : 0u;
            hword = ((uint64_t)hi << 32) | lo;
        }
        const uint32_t n = c * (uint32_t)kWave + (uint32_t)lane;
        bool in = ((word >> lane) & 1ull) != 0ull && n < A.n_nodes;
        if (in && my_zone != GF_ANY_ZONE) in = test_zone[n] == my_zone;
        if (in) {  // executor candidates: ready and not unschedulable (nodesorting.go:55-62)
            const uint32_t fl = A.flags[n];
            in = (fl & GF_NODE_READY) != 0u && (fl & GF_NODE_UNSCHEDULABLE) == 0u;
        }
        if (!in) continue;
        const int64_t o0 = A.over != nullptr ? A.over[n] : 0, o1 = A.over != nullptr ? A.over[N + n] : 0,
                      o2 = A.over != nullptr ? A.over[2 * N + n] : 0;
        const int64_t cpu = A.alloc[n] - (A.usage[n] + o0);
        const int64_t mem = A.alloc[N + n] - (A.usage[N + n] + o1);
        const int64_t gpu = A.alloc[2 * N + n] - (A.usage[2 * N + n] + o2);
        const bool twice = MINFRAG || A.res_count[n] != 0u;  // the overhead this path counts a second time
        const int64_t a0 = twice ? cpu - o0 : cpu, a1 = twice ? mem - o1 : mem, a2 = twice ? gpu - o2 : gpu;
        if (!cap_ge1(a0, a1, a2, app)) continue;  // !executorResources.GreaterThan(available)  <=>  capacity >= 1
        int64_t cand[kExecFields];
        cand[0] = 0;
        cand[1] = 0;
        if (MINFRAG) {
            const int64_t c0 = cap_dim_full(a0, app.exe0, app.rcp0), c1 = cap_dim_full(a1, app.exe1, app.rcp1),
                          c2 = cap_dim_full(a2, app.exe2, app.rcp2);
            int64_t cap = c0 < c1 ? c0 : c1;
            cap = cap < c2 ? cap : c2;
            cand[0] = ((hword >> lane) & 1ull) != 0ull ? 0 : 1;
            cand[1] = cap;
        }
        const uint32_t label = A.label_rank != nullptr ? A.label_rank[n] : 0u;
        const uint32_t zr = ranked ? sh.zrank[wave][A.zone[n] & (uint32_t)(kExecZones - 1)] : 0u;
        cand[2] = (int64_t)(((uint64_t)label << 32) | zr) ^ kExecBias;
        cand[3] = mem;
        cand[4] = cpu;
        cand[5] = (int64_t)(((uint64_t)A.name_rank[n] << 32) | n) ^ kExecBias;
        bool less = !have, decided = !have;
#pragma unroll
        for (int f = MINFRAG ? 0 : 2; f < kExecFields; ++f) {
            if (!decided && cand[f] != best[f]) {
                less = cand[f] < best[f];
                decided = true;
            }
        }
        if (less) {
            have = true;
#pragma unroll
            for (int f = 0; f < kExecFields; ++f) best[f] = cand[f];
        }
    }

    // ---- the workgroup's minimum, field after field: DPP inside a wavefront, LDS across the four
    bool alive = have;
    int64_t win[kExecFields];
#pragma unroll
    for (int f = 0; f < kExecFields; ++f) win[f] = 0;
#pragma unroll
    for (int f = MINFRAG ? 0 : 2; f < kExecFields; ++f) {
        win[f] = wave_min_any_i64(alive ? best[f] : INT64_MAX);
        alive = alive && best[f] == win[f];
    }
    const bool wave_has = __ballot(have) != 0ull;
    if (lane == 0) {
        sh.have[wave] = wave_has ? 1u : 0u;
#pragma unroll
        for (int f = 0; f < kExecFields; ++f) sh.rec[wave][f] = win[f];
    }
    lds_barrier();
    if (threadIdx.x == 0) {
        int pick = -1;
        for (int w = 0; w < kWavesPerBlock; ++w) {
            if (sh.have[w] == 0u) continue;
            bool less = pick < 0, decided = pick < 0;
            for (int f = MINFRAG ? 0 : 2; f < kExecFields && !decided; ++f)
                if (sh.rec[w][f] != sh.rec[pick][f]) {
                    less = sh.rec[w][f] < sh.rec[pick][f];
                    decided = true;
                }
            if (less) pick = w;
        }
        A.out[q] = pick < 0 ? GF_NO_NODE : (uint32_t)((uint64_t)(sh.rec[pick][5] ^ kExecBias) & 0xFFFFFFFFull);
    }
}
