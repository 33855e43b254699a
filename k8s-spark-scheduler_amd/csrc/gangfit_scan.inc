// gangfit_scan.inc — the empty-cluster capacity scan (gf_cluster_fit_feasible, gf_cluster_fit_feasible_sets; included by
// gangfit_kernels.hip).
//
//   UnschedulablePodMarker.DoesPodExceedClusterCapacity   internal/extender/unschedulablepods.go:132-166
//
// The marker asks whether an application would fit the cluster if nothing ran on it: zero usage, the non-schedulable overhead,
// every node that matches the driver's required affinity as driver AND executor candidate.  HasCapacity of an independent
// decision does not depend on the priority order (SparkBinPack tries every driver candidate, LIB/binpack/binpack.go:60-87; a
// packer places K executors iff the clamped capacities sum to K — what the node-range shards rest on, DESIGN 4.4):
//     feasible  <=>  some selected node d the driver fits on has  S - cap(d) + cap'(d) >= K,
//     S = sum over the selected nodes of min(cap, K),  cap' = the capacity of d with the driver on it.
// So the scan reads the columns gf_cluster_set keeps on the device in NODE-INDEX order: no sort, no slot layout, no install.
// One wavefront per application, 64 nodes per step; capacities through cap3 — negative available quantities, zero request
// dimensions and K = 0 mean what they mean in every other kernel.
//
// The single-AZ packers (LIB/binpack/single_az.go:23-97) ask the same of every zone by itself: (S_z, best delta_z) per zone id
// in wavefront-private LDS, at most 64 zones.  The caller guarantees what lets chooseBestResult's averages be skipped (available
// equals schedulable and is nowhere negative, the driver asks for cpu or memory: gf_fit_feasible's `surely_positive`).

constexpr int kScanZones = 64;
constexpr int32_t kScanNoDriver = INT32_MIN;  // "no fitting driver candidate seen"

struct ScanShared {
    unsigned long long s[kWavesPerBlock][kScanZones];  // S_z
    int32_t best[kWavesPerBlock][kScanZones];          // the largest cap' - cap over the zone's fitting driver candidates
};

// Sum and maximum over every RUN of lanes that hold the same key (mf_run_heads' runs), left in the run's first lane; `end` = the
// lane behind this lane's run.  Six steps of doubling reach: a lane takes its neighbour `off` ahead while that one is in the run.
__device__ __forceinline__ void scan_run_reduce(int32_t& sum, int32_t& mx, int end, int lane) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int32_t s = __shfl_down(sum, off, kWave);
        const int32_t m = __shfl_down(mx, off, kWave);
        if (lane + off < end) {
            sum += s;
            mx = m > mx ? m : mx;
        }
    }
}

// One step of the scan: lane `lane` holds node n (`in`: n is a node, `sel`: it is one of the question's nodes) and adds it to the
// plain sum and best delta, or to its zone's LDS row.  Returns true (wave-uniform) when the plain answer is already 1.
template <bool ZONED>
__device__ __forceinline__ bool scan_chunk(const int64_t* alloc, const int64_t* over, const uint32_t* zone, size_t N, uint32_t n, bool in,
                                           bool sel, const App& app, int64_t K, int lane, lds_ull* zs, lds_i32* zb, int64_t& S,
                                           int32_t& best) {
    int64_t a0 = -1, a1 = -1, a2 = -1;  // (an unselected lane holds nothing and hosts no driver)
    if (sel) {
        a0 = alloc[n];
        a1 = alloc[N + n];
        a2 = alloc[2 * N + n];
        if (over != nullptr) {
            a0 -= over[n];
            a1 -= over[N + n];
            a2 -= over[2 * N + n];
        }
    }
    const int32_t c0 = sel ? cap3(a0, a1, a2, app) : 0;
    const bool fits = sel && driver_fits(a0, a1, a2, app);
    // the same node with the driver on it (binpack.go:73-74: reserved[driverNode] = driverResources)
    const int32_t delta = fits ? cap3(a0 - app.drv0, a1 - app.drv1, a2 - app.drv2, app) - c0 : kScanNoDriver;
    if (!ZONED) {
        S += (int64_t)read_lane(wave_inclusive_scan(c0), kWave - 1);
        best = delta > best ? delta : best;
        // S only grows: a candidate that passes against the sum so far passes against the whole
        return __ballot(best != kScanNoDriver && S + (int64_t)best >= K) != 0ull;
    }
    // equal zone ids are mostly neighbours: a run's first lane speaks for it (one LDS atomic per run, not 64 on one address)
    const uint32_t z = in ? zone[n] : 0u;
    const uint32_t n_run = mf_run_heads(z, in, lane);
    const uint64_t heads = __ballot(n_run != 0u) | __ballot(!in);
    const uint64_t rest = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
    const int end = rest ? lane + (int)__ffsll((unsigned long long)rest) : kWave;
    int32_t sum = c0, mx = delta;
    scan_run_reduce(sum, mx, end, lane);
    if (n_run != 0u && z < (uint32_t)kScanZones) {
        if (sum != 0) __hip_atomic_fetch_add(zs + z, (unsigned long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (mx != kScanNoDriver) __hip_atomic_fetch_max(zb + z, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return false;
}

// The zone rows of a wavefront, emptied / read back: lane z answers for zone z (LDS operations of a wavefront execute in order).
__device__ __forceinline__ void scan_zones_clear(lds_ull* zs, lds_i32* zb, int lane) {
    zs[lane] = 0ull;
    zb[lane] = kScanNoDriver;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // (the other lanes of this wavefront add to these rows)
}
__device__ __forceinline__ bool scan_zones_answer(lds_ull* zs, lds_i32* zb, int64_t K, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const int64_t sz = (int64_t)zs[lane];
    const int32_t bz = zb[lane];
    return __ballot(bz != kScanNoDriver && sz + (int64_t)bz >= K) != 0ull;
}

template <bool ZONED>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void cluster_scan_kernel(ScanArgs A) {
    __shared__ ScanShared sh;
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= A.n_apps) return;  // (no workgroup barrier below: the LDS rows are private to a wavefront)
    const App app = load_app(A.apps, a);
    const int64_t K = app.k;
    const size_t N = A.n_nodes;
    lds_ull* const zs = (lds_ull*)&sh.s[wave][0];
    lds_i32* const zb = (lds_i32*)&sh.best[wave][0];
    if (ZONED) scan_zones_clear(zs, zb, lane);
    int64_t S = 0;                    // (plain) the clamped capacities so far, wave-uniform
    int32_t best = kScanNoDriver;     // (plain) this lane's best delta so far
    bool feasible = false;
    for (uint32_t base = 0; base < A.n_nodes; base += kWave) {
        const uint32_t n = base + (uint32_t)lane;
        const bool in = n < A.n_nodes;
        const bool sel = in && (A.select == nullptr || A.select[n] != 0);
        if (scan_chunk<ZONED>(A.alloc, A.over, A.zone, N, n, in, sel, app, K, lane, zs, zb, S, best)) {
            feasible = true;
            break;
        }
    }
    if (ZONED) feasible = scan_zones_answer(zs, zb, K, lane);
    if (lane == 0) A.out[a] = feasible ? 1 : 0;
}

// ---- many node sets in one launch (gf_cluster_fit_feasible_sets): application a asks row app_set[a] of a bit matrix, n_sets rows of
// W = ceil(n_nodes / 64) words, bit (n & 63) of word n >> 6 = node n.  A word IS a chunk's selection, so the wavefront walks its row
// 64 words (4 096 nodes) at a time — lane l loads the word of chunk 64 g + l, one coalesced 512-byte load — and visits the chunks
// whose word is not zero, in ascending order; the chunk's word reaches every lane through read_lane.  A zero word costs nothing
// beyond that load: the columns of the other instance groups are never read.

template <bool ZONED>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void cluster_scan_sets_kernel(ScanSetsArgs A) {
    __shared__ ScanShared sh;
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= A.n_apps) return;  // (no workgroup barrier below: the LDS rows are private to a wavefront)
    const App app = load_app(A.apps, a);
    const int64_t K = app.k;
    const size_t N = A.n_nodes;
    const uint32_t W = A.n_words;
    const uint64_t* const row = A.set_words + (size_t)__builtin_amdgcn_readfirstlane(A.app_set[a]) * W;
    lds_ull* const zs = (lds_ull*)&sh.s[wave][0];
    lds_i32* const zb = (lds_i32*)&sh.best[wave][0];
    if (ZONED) scan_zones_clear(zs, zb, lane);
    int64_t S = 0;
    int32_t best = kScanNoDriver;
    bool feasible = false;
    for (uint32_t g = 0; g < W && !feasible; g += kWave) {  // g: the first chunk of the group
        const uint32_t c = g + (uint32_t)lane;
        const uint64_t word = c < W ? row[c] : 0ull;
        uint64_t todo = __ballot(word != 0ull);  // a group of zero words is skipped as a whole
        while (todo != 0ull) {
            const int bit = (int)__ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1ull;
            const uint64_t chunk = (uint64_t)read_lane((int64_t)word, bit);
            const uint32_t n = (g + (uint32_t)bit) * kWave + (uint32_t)lane;
            const bool in = n < A.n_nodes;
            const bool sel = in && ((chunk >> lane) & 1ull) != 0ull;
            if (scan_chunk<ZONED>(A.alloc, A.over, A.zone, N, n, in, sel, app, K, lane, zs, zb, S, best)) {
                feasible = true;
                break;
            }
        }
    }
    if (ZONED) feasible = scan_zones_answer(zs, zb, K, lane);
    if (lane == 0) A.out[a] = feasible ? 1 : 0;
}
