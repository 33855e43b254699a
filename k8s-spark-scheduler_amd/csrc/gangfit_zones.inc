// gangfit_zones.inc — zone-aware packers and packing efficiencies (included by gangfit_kernels.hip).
//
//   getSingleAZSparkBinFunction / chooseBestResult   LIB/binpack/single_az.go:23-97
//   AzAwareTightlyPack                               LIB/binpack/az_aware_pack_tightly.go:27-38
//   ComputePackingEfficiencies / ComputeAvgPackingEfficiency   LIB/binpack/efficiency.go:66-156
//
// A zone's SparkBinPack is the ordinary wave-level decision on the same slot table seen through that zone's candidate
// bit masks (order within a zone = order of the unfiltered priority lists, single_az.go:57-72).  Efficiencies are
// float64 and must match the reference bit for bit because chooseBestResult compares them (strict <): every per-node
// value is one correctly rounded int64->f64 conversion pair and one IEEE division, and the averages are summed in
// slice order [driver, executor-1, ..., executor-K] — a serial left-to-right sum, done uniformly by the wave while
// the per-node values are produced 64 at a time.

// Quantity.Value() of a canonical milli quantity: rounded away from zero to whole units (K8S apimachinery
// quantity.go:731-734, math.go:169-199).
__device__ __forceinline__ int64_t value_of_milli(int64_t v) {
    const int64_t q = v / 1000;  // constant divisor: multiply-high sequence
    const int64_t r = v - q * 1000;
    return r > 0 ? q + 1 : (r < 0 ? q - 1 : q);
}

struct NodeEff {
    double cpu, mem, gpu;
};

// computePackingEfficiency (efficiency.go:79-103): (schedulable - available + reserved).Value() / schedulable.Value(),
// zero schedulable divides by 1 (:105-110), gpu efficiency 0 on nodes without gpus (:91-94).  Returns has_gpu.
// small_cpu (wave-uniform): both cpu quantities of every active lane lie in [0, 2^32) — the rounding to whole cpus and
// the conversions are then 32-bit (a signed 64-bit division by 1000 is ~35 instructions, twice per node); same values.
__device__ __forceinline__ uint32_t value_of_milli_u32(uint32_t v) {
    const uint32_t q = v / 1000u;
    return q + (v - q * 1000u != 0u ? 1u : 0u);
}
__device__ __forceinline__ bool node_efficiency(int64_t a0, int64_t a1, int64_t a2, int64_t s0, int64_t s1, int64_t s2,
                                                int64_t r0, int64_t r1, int64_t r2, NodeEff& e, bool small_cpu = false) {
    if (small_cpu) {
        const uint32_t sv = value_of_milli_u32((uint32_t)s0);
        e.cpu = (double)value_of_milli_u32((uint32_t)(s0 - a0 + r0)) / (double)(sv == 0u ? 1u : sv);
    } else {
        const int64_t sv0 = value_of_milli(s0);
        e.cpu = (double)value_of_milli(s0 - a0 + r0) / (double)(sv0 == 0 ? 1 : sv0);
    }
    e.mem = (double)(s1 - a1 + r1) / (double)(s1 == 0 ? 1 : s1);
    const bool has_gpu = s2 != 0;
    e.gpu = has_gpu ? (double)(s2 - a2 + r2) / (double)s2 : 0.0;
    return has_gpu;
}

struct EffView {  // SoA tables in the id space of the placement list
    const int64_t* a0;
    const int64_t* a1;
    const int64_t* a2;
    const int64_t* s0;
    const int64_t* s1;
    const int64_t* s2;
};

// ComputeAvgPackingEfficiency (efficiency.go:114-156) over nodeNames = [driver] ++ out[0..K) (chooseBestResult,
// single_az.go:83-89), by one wave.  Ids in out[] index the EffView tables and cnt[]; MAP != nullptr translates them
// first (caller's node index -> slot).  cnt[] is all-zero on entry and on exit.
// RESERVE_EXECS: the packer left one executor request per placement in `reserved` (tightly-pack, distribute-evenly);
// false for minimalFragmentation, which never writes its placements there (minimal_fragmentation.go:59-91).
template <bool RESERVE_EXECS>
__device__ __forceinline__ void wave_avg_efficiency(const EffView& E, const App& app, uint32_t driver,
                                                    const uint32_t* __restrict__ out, const uint32_t* __restrict__ map,
                                                    uint32_t* __restrict__ cnt, int lane, double avg[4]) {
    const int64_t K = app.k;
    if (RESERVE_EXECS && K > 0) {
        for (int64_t b = 0; b < K; b += kWave) {
            const int64_t i = b + lane;
            if (i < K) {
                uint32_t s = out[i];
                if (map != nullptr) s = map[s];
                atomicAdd(&cnt[s], 1u);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");  // every lane's increments are performed before the reads
    }
    double cpu_sum = 0.0, mem_sum = 0.0, gpu_sum = 0.0, max_sum = 0.0;
    uint64_t with_gpu = 0;
    for (int64_t b = 0; b <= K; b += kWave) {
        const int64_t i = b + lane;
        NodeEff e;
        e.cpu = e.mem = e.gpu = 0.0;
        double mx = 0.0;
        bool hg = false;
        if (i <= K) {
            uint32_t s = (i == 0) ? driver : out[i - 1];
            if (map != nullptr && i != 0) s = map[s];
            uint32_t c = 0;
            if (RESERVE_EXECS && K > 0) c = __hip_atomic_load(&cnt[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int64_t r0 = (int64_t)c * app.exe0, r1 = (int64_t)c * app.exe1, r2 = (int64_t)c * app.exe2;
            if (s == driver) {
                r0 += app.drv0;
                r1 += app.drv1;
                r2 += app.drv2;
            }
            hg = node_efficiency(E.a0[s], E.a1[s], E.a2[s], E.s0[s], E.s1[s], E.s2[s], r0, r1, r2, e);
            const double m = e.cpu > e.mem ? e.cpu : e.mem;  // math.Max; no NaN / -0 can occur (divisors >= 1)
            mx = e.gpu > m ? e.gpu : m;
        }
        const uint64_t hgm = __ballot(hg);
        const int n = (K + 1 - b) < (int64_t)kWave ? (int)(K + 1 - b) : kWave;
        for (int t = 0; t < n; ++t) {  // slice order; t is wave-uniform
            cpu_sum += bcast_f64(e.cpu, t);
            mem_sum += bcast_f64(e.mem, t);
            if ((hgm >> t) & 1ull) {
                gpu_sum += bcast_f64(e.gpu, t);
                ++with_gpu;
            }
            max_sum += bcast_f64(mx, t);
        }
    }
    const double len = (double)(K + 1);
    avg[0] = cpu_sum / len;
    avg[1] = mem_sum / len;
    avg[2] = with_gpu == 0 ? 1.0 : gpu_sum / (double)with_gpu;
    avg[3] = max_sum / len;
    if (RESERVE_EXECS && K > 0) {
        for (int64_t b = 0; b < K; b += kWave) {
            const int64_t i = b + lane;
            if (i < K) {
                uint32_t s = out[i];
                if (map != nullptr) s = map[s];
                __hip_atomic_store(&cnt[s], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    }
}

// One wave per (app, zone): SparkBinPack on the zone's view.  Placements are SLOT ids (the select kernel translates).
template <int ALGO>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void fit_zoned_kernel(NodeTable T, ZoneTable Z, uint32_t n_apps,
                                                                         const gf_app* __restrict__ apps,
                                                                         gf_result* __restrict__ zres,
                                                                         uint32_t* __restrict__ zexec,
                                                                         uint64_t zexec_stride,
                                                                         uint32_t* __restrict__ scratch,
                                                                         uint64_t scratch_half) {
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t w = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    if (w >= (uint64_t)n_apps * Z.n_zones) return;
    const uint32_t a = (uint32_t)(w / Z.n_zones), zi = (uint32_t)(w % Z.n_zones);
    const App app = load_app(apps, a);
    GlobalView V{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks,
                 Z.xmask + (size_t)zi * Z.stride, Z.dmask + (size_t)zi * Z.stride, T.n_chunks};
    Orders O{T.slot_node, T.dslot, T.n_x, T.n_d, T.d_identity != 0, true};
    unsigned long long xvis = 0, dvis = 0;
    // scratch is only touched by distribute-evenly; the zone packers are tightly-pack shaped, one region per app is enough
    const Decision dec = wave_decide<ALGO, GlobalView, true>(V, O, app, zexec + (size_t)zi * zexec_stride + app.exec_off,
                                                             scratch + app.exec_off,
                                                             scratch + scratch_half + app.exec_off, lane, xvis, dvis);
    if (lane == 0) {
        gf_result r;
        r.has_capacity = dec.feasible ? 1 : 0;
        r.driver_node = dec.feasible ? dec.ds : GF_NO_NODE;  // SLOT id
        r.exec_len = dec.feasible ? (uint32_t)app.k : 0u;
        r.evaluated = 1;
        zres[w] = r;
    }
}

// One wave per decision (persistent: wave g serves decisions g, g + G, ...; cnt row g is its scratch).
// ZONED: decisions are the (app, zone) pairs of fit_zoned_kernel, placements are slot ids in zexec.
// otherwise: decisions are finished results with NODE indices in exec_nodes (gf_avg_packing_efficiency).
template <bool RESERVE_EXECS, bool ZONED>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void avg_efficiency_kernel(
    EffTables E, const uint32_t* __restrict__ node_slot, uint32_t n_slots, uint32_t n_zones, uint32_t n_apps,
    const gf_app* __restrict__ apps, const gf_result* __restrict__ res, const uint32_t* __restrict__ exec,
    uint64_t exec_stride, uint32_t* __restrict__ cnt, uint32_t n_cnt_waves, double* __restrict__ avg_out) {
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t g = blockIdx.x * kWavesPerBlock + wave;
    if (g >= n_cnt_waves) return;
    const EffView V{E.avail[0], E.avail[1], E.avail[2], E.sched[0], E.sched[1], E.sched[2]};
    const uint64_t n_dec = (uint64_t)n_apps * (ZONED ? n_zones : 1u);
    for (uint64_t w = g; w < n_dec; w += n_cnt_waves) {
        const uint32_t a = ZONED ? (uint32_t)(w / n_zones) : (uint32_t)w;
        const uint32_t zi = ZONED ? (uint32_t)(w % n_zones) : 0u;
        const gf_result r = res[w];
        double avg[4] = {0.0, 0.0, 0.0, 0.0};
        if (r.has_capacity) {
            const App app = load_app(apps, a);
            const uint32_t* out = exec + (size_t)zi * exec_stride + app.exec_off;
            const uint32_t driver = ZONED ? r.driver_node : node_slot[r.driver_node];
            wave_avg_efficiency<RESERVE_EXECS>(V, app, driver, out, ZONED ? nullptr : node_slot,
                                               cnt + (size_t)g * n_slots, lane, avg);
        }
        if (lane < 4) avg_out[4 * w + lane] = lane == 0 ? avg[0] : (lane == 1 ? avg[1] : (lane == 2 ? avg[2] : avg[3]));
    }
}

// chooseBestResult (single_az.go:75-97) + result emission, one wave per app: the first zone of the evaluation list
// whose average Max is strictly above the best so far (starting from WorstAvgPackingEfficiency = 0.0) wins; a feasible
// zone result whose average is not > 0 never wins.  Placements are translated slot -> node index.
// KEEP_PLAIN (az-aware-tightly-pack): d_results / exec_nodes already hold the plain TightlyPack answer, which stays
// when no zone won (az_aware_pack_tightly.go:33-37).
template <bool KEEP_PLAIN>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void zone_select_kernel(
    const uint32_t* __restrict__ slot_node, uint32_t n_zones, uint32_t n_apps, const gf_app* __restrict__ apps,
    const gf_result* __restrict__ zres, const uint32_t* __restrict__ zexec, uint64_t zexec_stride,
    const double* __restrict__ zavg, gf_result* __restrict__ results, uint32_t* __restrict__ exec_nodes,
    double* __restrict__ avg_out) {
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t a = blockIdx.x * kWavesPerBlock + wave;
    if (a >= n_apps) return;
    int32_t best = -1;
    double best_max = 0.0;
    for (uint32_t zi = 0; zi < n_zones; ++zi) {
        const uint64_t w = (uint64_t)a * n_zones + zi;
        if (!zres[w].has_capacity) continue;      // single_az.go:44-46
        const double m = zavg[4 * w + 3];
        if (best_max < m) {                       // AvgPackingEfficiency.LessThan, efficiency.go:37-39
            best = (int32_t)zi;
            best_max = m;
        }
    }
    if (best < 0) {
        if (!KEEP_PLAIN && lane == 0) {
            gf_result r;
            r.has_capacity = 0;
            r.driver_node = GF_NO_NODE;
            r.exec_len = 0;
            r.evaluated = 1;
            results[a] = r;
        }
        if (!KEEP_PLAIN && avg_out != nullptr && lane < 4) avg_out[4 * (size_t)a + lane] = 0.0;
        return;
    }
    const uint64_t w = (uint64_t)a * n_zones + (uint32_t)best;
    const gf_app* p = apps + a;
    const int64_t K = p->k;
    const uint32_t* src = zexec + (size_t)best * zexec_stride + p->exec_off;
    uint32_t* dst = exec_nodes + p->exec_off;
    for (int64_t i = lane; i < K; i += kWave) dst[i] = slot_node[src[i]];
    if (lane == 0) {
        gf_result r;
        r.has_capacity = 1;
        r.driver_node = slot_node[zres[w].driver_node];
        r.exec_len = (uint32_t)K;
        r.evaluated = 1;
        results[a] = r;
    }
    if (avg_out != nullptr && lane < 4) avg_out[4 * (size_t)a + lane] = zavg[4 * w + lane];
}

// ------------------------------------------------------------------------------------------------ one launch per batch
// The zone-aware packers on an independent batch as ONE kernel: a workgroup per application, a wavefront per candidate
// view (every zone of the evaluation list, plus the plain pack for az-aware-tightly-pack), chooseBestResult through LDS,
// the winner's placements translated slot -> node index by the whole workgroup and written where the caller wants them
// (device memory or device-mapped host memory) — what the chain kernels do per application, without the chain.  It
// replaces fit_zoned_kernel + avg_efficiency_kernel + zone_select_kernel (+ the copy-out kernel of the host entry point).
//
// The average efficiency needs reserved[n] = (executors placed on n) x exe for every node of the list (efficiency.go:79-103).
// The separate efficiency kernel counts them in a per-wavefront table of n_slots words with atomics and device-scope
// fences; here the wavefront that made the pack recomputes them from what the packer guarantees:
//   tightly-pack        every node of the list is one contiguous run, filled to its capacity (with the driver reserved)
//                       except the LAST node, which holds what was left: K - (index of its first entry)
//                       (pack_tightly.go:45-61: a node is left only when the next executor does not fit, or at K);
//   minimal-fragmentation   never writes its placements into `reserved` (minimal_fragmentation.go:59-91): the driver only.
// Same float64 values, same slice-order sums as wave_avg_efficiency.
template <int ALGO>
__device__ __forceinline__ void wave_avg_efficiency_runs(const EffView& E, const App& app, uint32_t driver,
                                                         const uint32_t* __restrict__ out, int lane, double avg[4]) {
    constexpr bool kReserveExecs = ALGO != GF_ALGO_MINIMAL_FRAGMENTATION;
    const int64_t K = app.k;
    uint32_t last = GF_NO_NODE;  // the last node of the list and where its run starts
    int64_t last_first = 0;
    bool driver_listed = false;
    if (kReserveExecs && K > 0) {
        last = out[K - 1];  // wave-uniform address
        uint32_t first_lo = 0xFFFFFFFFu;  // lowest index holding `last`, over this lane's entries
        for (int64_t b = 0; b < K; b += kWave) {
            const int64_t i = b + lane;
            uint32_t s = GF_NO_NODE;
            if (i < K) s = out[i];
            if (s == last && (uint32_t)i < first_lo && i < K) first_lo = (uint32_t)i;
            if (__ballot(i < K && s == driver)) driver_listed = true;
        }
        // minimum over the lanes: indices fit 31 bits (K <= 2^20); 0x7FFFFFFF when the lane saw none
        int32_t v = first_lo == 0xFFFFFFFFu ? 0x7FFFFFFF : (int32_t)first_lo;
        last_first = -(int64_t)wave_max_i64(-(int64_t)v);
    }
    double cpu_sum = 0.0, mem_sum = 0.0, gpu_sum = 0.0, max_sum = 0.0;
    uint64_t with_gpu = 0;
    for (int64_t b = 0; b <= K; b += kWave) {
        const int64_t i = b + lane;
        NodeEff e;
        e.cpu = e.mem = e.gpu = 0.0;
        double mx = 0.0;
        bool hg = false;
        if (i <= K) {
            const uint32_t s = (i == 0) ? driver : out[i - 1];
            const int64_t a0 = E.a0[s], a1 = E.a1[s], a2 = E.a2[s];
            int64_t c = 0;
            if (kReserveExecs && K > 0 && (i != 0 || driver_listed)) {
                if (s == last) {
                    c = K - last_first;
                } else {
                    const bool dn = s == driver;
                    c = cap3(a0 - (dn ? app.drv0 : 0), a1 - (dn ? app.drv1 : 0), a2 - (dn ? app.drv2 : 0), app);
                }
            }
            int64_t r0 = c * app.exe0, r1 = c * app.exe1, r2 = c * app.exe2;
            if (s == driver) {
                r0 += app.drv0;
                r1 += app.drv1;
                r2 += app.drv2;
            }
            hg = node_efficiency(a0, a1, a2, E.s0[s], E.s1[s], E.s2[s], r0, r1, r2, e);
            const double m = e.cpu > e.mem ? e.cpu : e.mem;  // math.Max; no NaN / -0 can occur (divisors >= 1)
            mx = e.gpu > m ? e.gpu : m;
        }
        const uint64_t hgm = __ballot(hg);
        const int n = (K + 1 - b) < (int64_t)kWave ? (int)(K + 1 - b) : kWave;
        for (int t = 0; t < n; ++t) {  // slice order; t is wave-uniform
            cpu_sum += bcast_f64(e.cpu, t);
            mem_sum += bcast_f64(e.mem, t);
            if ((hgm >> t) & 1ull) {
                gpu_sum += bcast_f64(e.gpu, t);
                ++with_gpu;
            }
            max_sum += bcast_f64(mx, t);
        }
    }
    const double len = (double)(K + 1);
    avg[0] = cpu_sum / len;
    avg[1] = mem_sum / len;
    avg[2] = with_gpu == 0 ? 1.0 : gpu_sum / (double)with_gpu;
    avg[3] = max_sum / len;
}

constexpr int kFusedWaves = 4;  // wavefronts (= candidate views decided at the same time) per application
constexpr int kRunBlocks = 8;   // wave_avg_max_tight_runs: placements of up to kRunBlocks * 64 executors ...
constexpr uint32_t kRunMax = 63;  // ... on up to kRunMax nodes (one lane stays free for a driver that hosts no executor)
struct FusedShared {
    int32_t feas[64];
    uint32_t ds[64];
    double mx[64];
    uint32_t runs[kFusedWaves][2 * kWave];  // per wavefront: slot and first index of every run of its placement
};

// avg.Max of a tightly-pack placement (what chooseBestResult compares, single_az.go:75-97) from the placement's RUNS instead of its
// entries.  wave_avg_efficiency_runs walks the K + 1 entries 64 at a time, and every block of 64 is two dependent global round
// trips (the entries, then the nodes' columns) followed by 64 dependent additions: a gang of 300 executors took ~8 us where one
// executor takes ~2 (tools/probe_zoned_parts.py: the launch waits for these gangs).  Here every block of entries is requested
// before the first is looked at, the run heads (an entry that differs from its predecessor) go through LDS to lane = run, every
// node's efficiency is computed ONCE — with the run's length as the number of executors reserved on it, which is what the
// entry-wise code derives from the capacities (tightly-pack fills every node but the last to its capacity) — and the
// slice-order sum adds a run's value as many times as the run is long, in order: the same additions in the same order, bit for bit.
// Returns false (nothing computed) when the placement has more than kRunMax nodes.  1 <= K <= kRunBlocks * 64.
__device__ __forceinline__ bool wave_avg_max_tight_runs(const EffView& E, const App& app, uint32_t driver,
                                                        const uint32_t* __restrict__ out, int lane, lds_u32* rl, double& avg_max) {
    const uint32_t K = (uint32_t)app.k;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    uint32_t v[kRunBlocks];
#pragma unroll
    for (int b = 0; b < kRunBlocks; ++b) {
        const uint32_t i = (uint32_t)b * kWave + (uint32_t)lane;
        v[b] = GF_NO_NODE;
        if ((uint32_t)b * kWave < K && i < K) v[b] = out[i];
    }
    uint32_t n_runs = 0, prev_last = GF_NO_NODE;
#pragma unroll
    for (int b = 0; b < kRunBlocks; ++b) {
        if ((uint32_t)b * kWave < K) {  // wave-uniform
            const uint32_t i = (uint32_t)b * kWave + (uint32_t)lane;
            uint32_t up = (uint32_t)__shfl_up((int)v[b], 1, kWave);
            if (lane == 0) up = prev_last;
            const bool head = i < K && v[b] != up;  // (entry 0: no slot is GF_NO_NODE)
            const uint64_t hm = __ballot(head);
            const uint32_t idx = n_runs + (uint32_t)__popcll((unsigned long long)(hm & lt_mask));
            if (head && idx < (uint32_t)kWave) {
                rl[idx] = v[b];
                rl[kWave + idx] = i;
            }
            n_runs += (uint32_t)__popcll((unsigned long long)hm);
            prev_last = (uint32_t)read_lane((int32_t)v[b], kWave - 1);
        }
    }
    if (n_runs > kRunMax) return false;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint32_t s = GF_NO_NODE, first = K;
    if ((uint32_t)lane < n_runs) {
        s = rl[lane];
        first = rl[kWave + lane];
    }
    uint32_t next = (uint32_t)__shfl_down((int)first, 1, kWave);
    if ((uint32_t)lane + 1u >= n_runs) next = K;
    const uint32_t len = (uint32_t)lane < n_runs ? next - first : 0u;  // executors on this lane's node
    const uint64_t dmask = __ballot((uint32_t)lane < n_runs && s == driver);
    const bool driver_listed = dmask != 0ull;
    const int dlane = driver_listed ? __ffsll((unsigned long long)dmask) - 1 : (int)n_runs;  // whose value the driver's element has
    if (!driver_listed && (uint32_t)lane == n_runs) s = driver;  // the driver's node hosts no executor: an element of its own
    double mx = 0.0;
    if ((uint32_t)lane < n_runs + (driver_listed ? 0u : 1u)) {
        const int64_t c = (int64_t)len;
        int64_t r0 = c * app.exe0, r1 = c * app.exe1, r2 = c * app.exe2;
        if (s == driver) {
            r0 += app.drv0;
            r1 += app.drv1;
            r2 += app.drv2;
        }
        NodeEff e;
        (void)node_efficiency(E.a0[s], E.a1[s], E.a2[s], E.s0[s], E.s1[s], E.s2[s], r0, r1, r2, e);
        const double m = e.cpu > e.mem ? e.cpu : e.mem;
        mx = e.gpu > m ? e.gpu : m;
    }
    double sum = 0.0;
    sum += bcast_f64(mx, dlane);  // nodeNames = [driver] ++ executor nodes
    for (uint32_t r = 0; r < n_runs; ++r) {  // slice order: a run's value once per executor of the run
        const double val = bcast_f64(mx, (int)r);
        const uint32_t n = (uint32_t)read_lane((int32_t)len, (int)r);
        for (uint32_t q = 0; q < n; ++q) sum += val;
    }
    avg_max = sum / (double)((int64_t)K + 1);
    return true;
}

// A pointer that is the same for every lane, said so to the compiler (two v_readfirstlane): its address then lives in scalar registers.
__device__ __forceinline__ uint32_t* uniform_ptr(uint32_t* p) {
    const uint64_t u = (uint64_t)reinterpret_cast<uintptr_t>(p);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)(u >> 32));
    return reinterpret_cast<uint32_t*>((uintptr_t)(((uint64_t)hi << 32) | lo));
}

// The zone-aware tightly-pack packers by ONE wavefront (the resident worker, gangfit_worker.inc): what fit_zoned_fused_kernel's
// wavefronts decide side by side and choose through LDS behind a barrier, one wavefront walks view after view — every zone of
// the evaluation list in order, then (az-aware, and only when no zone won: az_aware_pack_tightly.go:33-37) the plain order —
// with chooseBestResult's strict '<' from 0.0 applied as it goes (single_az.go:75-97).  Same wave_decide, same candidate
// words, same compact gpu rows and the entry-wise average function of the one-launch kernel: same float64 bits, same answer.
// Placements are SLOT ids and the winner is known only behind the last view: the view being decided writes slice `cur`, the
// best so far stays in `kept`, and the two swap roles on a win — two slices however many zones.  Both are private to the
// wavefront's application (K words each); `placed` names the winner's on return.
template <bool AZ_AWARE>
__device__ __forceinline__ Decision wave_decide_zones(const NodeTable& T, const SparseTable& G, const ZoneTable& Z,
                                                      const int64_t* __restrict__ sched, const GlobalView& plain, const App& app,
                                                      uint32_t* cur, uint32_t* kept, int lane, unsigned long long& xvis,
                                                      unsigned long long& dvis, const uint32_t*& placed) {
    const EffView EV{T.cpu, T.mem, T.gpu, sched, sched + T.n_slots, sched + 2 * (size_t)T.n_slots};
    const int64_t K = app.k;
    // (the two slices are the same for every lane: said so, or their addresses occupy vector registers through every view)
    cur = uniform_ptr(cur);
    kept = uniform_ptr(kept);
    Decision best;
    best.feasible = false;
    best.ds = 0;
    best.pass1 = 0;
    double best_max = 0.0;
    const uint32_t n_zone_cand = Z.n_zones;
    const uint32_t n_cand = n_zone_cand + (AZ_AWARE ? 1u : 0u);  // the host guarantees n_cand <= 64
    for (uint32_t c = 0; c < n_cand; ++c) {
        const bool zone_view = c < n_zone_cand;
        if (AZ_AWARE && !zone_view && best.feasible) break;  // a zone won: the plain order is not asked
        GlobalView V = plain;
        if (zone_view) {
            V.xm = Z.xmask + (size_t)c * Z.stride;
            V.dm = Z.dmask + (size_t)c * Z.stride;
        }
        const Orders O{T.slot_node, T.dslot, T.n_x, T.n_d, T.d_identity != 0, zone_view};
        // gangs of gpu executors: the zone's row of the compact gpu table, exactly as fit_zoned_fused_kernel builds it
        const SparseTable GV{G.cpu, G.mem, G.gpu, G.slot_of_sub, G.cmax, zone_view ? G.zmask + (size_t)c * G.n_chunks : G.xmask,
                             G.sub_of_slot, G.n_x, G.n_chunks, G.zmask, G.slot_of_sub};
        // (tightly-pack uses neither survivor list)
        const Decision dec =
            wave_decide<GF_ALGO_TIGHTLY_PACK, GlobalView, true>(V, O, app, cur, nullptr, nullptr, lane, xvis, dvis, nullptr, &GV);
        if (!dec.feasible) continue;  // single_az.go:44-46
        bool wins = !zone_view;
        if (zone_view) {
            // cur[] was written by other lanes of this wave
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            // the entry-wise form for every K (the same float64 bits as wave_avg_max_tight_runs, DESIGN section 4.3): the run form's
            // eight blocks of entries in registers take this kernel past its register budget (127 VGPRs and scratch against 101)
            double avg[4] = {0.0, 0.0, 0.0, 0.0};
            wave_avg_efficiency_runs<GF_ALGO_TIGHTLY_PACK>(EV, app, dec.ds, cur, lane, avg);
            wins = best_max < avg[3];  // AvgPackingEfficiency.LessThan, efficiency.go:37-39
            if (wins) best_max = avg[3];
        }
        if (wins) {
            best.feasible = true;
            best.ds = dec.ds;
            uint32_t* const t = cur;
            cur = kept;
            kept = t;
        }
    }
    placed = kept;
    return best;
}

// FEAS (gf_fit_feasible; fit_zoned_fused_feasible_kernel): answers.bytes receive HasCapacity through the grid's last workgroup
// and the collection words answers.words (FitOut, feasible_announce / feasible_collect in gangfit_kernels.hip); the winner's
// placement is not expanded — exec_nodes is not read — and no result record is written.
template <int ALGO, bool AZ_AWARE, bool FEAS>
__device__ __forceinline__ void fit_zoned_fused_body(NodeTable T, SparseTable G, ZoneTable Z, const int64_t* sched,
                                                     uint32_t n_apps, const gf_app* apps, const FitOut<FEAS>& answers,
                                                     uint32_t* exec_nodes, uint32_t* zexec, uint64_t zexec_stride, uint32_t* scratch,
                                                     uint64_t scratch_half, uint32_t eff_nonneg) {
    __shared__ FusedShared sh;
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t a = blockIdx.x;
    if constexpr (FEAS)
        if (a == n_apps) {  // the collecting workgroup (launch_fit_zoned_fused appends it)
            if (wave == 0) feasible_collect(answers, n_apps, lane);
            return;
        }
    if (a >= n_apps) return;
    const uint32_t n_zone_cand = Z.n_zones;
    const uint32_t n_cand = n_zone_cand + (AZ_AWARE ? 1u : 0u);  // the launcher guarantees n_cand <= 64
    const GlobalView plain{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks,
                           T.xmask, T.dmask, T.n_chunks};
    const EffView EV{T.cpu, T.mem, T.gpu, sched, sched + T.n_slots, sched + 2 * (size_t)T.n_slots};
    const App app = load_app(apps, a);
    const int64_t K = app.k;
    for (uint32_t c = wave; c < n_cand; c += kFusedWaves) {
        const bool zone_view = c < n_zone_cand;
        GlobalView V = plain;
        if (zone_view) {
            V.xm = Z.xmask + (size_t)c * Z.stride;
            V.dm = Z.dmask + (size_t)c * Z.stride;
        }
        Orders O{T.slot_node, T.dslot, T.n_x, T.n_d, T.d_identity != 0, zone_view};
        if constexpr (ALGO == GF_ALGO_MINIMAL_FRAGMENTATION) {  // the capacity histogram of this wavefront's view
            __shared__ __attribute__((aligned(16))) uint32_t mf_hist[kFusedWaves * 3 * kMfHistBins];
            O.lend_minfrag((lds_u32*)mf_hist + (size_t)wave * 3 * kMfHistBins, T);
        }
        unsigned long long xvis = 0, dvis = 0;
        uint32_t* out = zexec + (size_t)c * zexec_stride + app.exec_off;
        // Gangs of gpu executors are packed from the compact table of gpu nodes, as in the plain kernel (SparseTable; without it
        // such a gang walks 7-20 chunks of the zone's range for a few slots each, and the launch waits for it: 22.3 us against
        // 19.0 without gpu requests, tools/probe_zoned_parts.py): the view's candidate words are the zone's, and its placements
        // name slots of the full table — what the averages below and the copy-out index.
        constexpr bool kSparse = ALGO == GF_ALGO_TIGHTLY_PACK;
        const SparseTable GV{G.cpu, G.mem, G.gpu, G.slot_of_sub, G.cmax, zone_view ? G.zmask + (size_t)c * G.n_chunks : G.xmask,
                             G.sub_of_slot, kSparse ? G.n_x : 0u, G.n_chunks, G.zmask, G.slot_of_sub};
        const Decision dec = wave_decide<ALGO, GlobalView, true>(V, O, app, out, scratch + app.exec_off,
                                                                 scratch + scratch_half + app.exec_off, lane, xvis, dvis, nullptr,
                                                                 kSparse ? &GV : nullptr);
        double avg[4] = {0.0, 0.0, 0.0, 0.0};
        // Feasibility only: chooseBestResult answers "has capacity" iff some zone's placement has an average Max ABOVE 0
        // (single_az.go:75-97 starts from 0 and replaces on '<').  When no node's available quantity exceeds its schedulable one
        // (eff_nonneg: the host checked the snapshot) every node's efficiencies are >= 0 (efficiency.go:79-103: reserved >= 0), and
        // the DRIVER's node alone has a positive one as soon as the driver asks for cpu or memory: the numerator of that
        // dimension is at least the request.  Then a feasible zone counts without its average — no read-back of the placement
        // (behind a store's ~2 us acknowledgement), no schedulable columns, no float64.
        const bool surely_positive = FEAS && eff_nonneg != 0u && (app.drv0 > 0 || app.drv1 > 0);
        if (zone_view && dec.feasible && surely_positive) {
            avg[3] = 1.0;  // (any positive value: only `best >= 0` leaves this kernel)
        } else if (zone_view && dec.feasible) {
            // out[] was written by other lanes of this wave
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            bool done = false;
            if (ALGO == GF_ALGO_TIGHTLY_PACK && K >= 1 && K <= (int64_t)kRunBlocks * kWave)
                done = wave_avg_max_tight_runs(EV, app, dec.ds, out, lane, (lds_u32*)&sh.runs[wave][0], avg[3]);
            if (!done) wave_avg_efficiency_runs<ALGO>(EV, app, dec.ds, out, lane, avg);
        }
        if (lane == 0) {
            sh.feas[c] = dec.feasible ? 1 : 0;
            sh.ds[c] = dec.ds;
            sh.mx[c] = avg[3];
        }
    }
    __syncthreads();  // the candidates' verdicts (LDS) and placements (global, same compute unit) are visible to every wavefront
    // chooseBestResult (single_az.go:75-97), evaluated identically by every thread: the first zone of the evaluation list
    // whose average Max is strictly above the best so far (from WorstAvgPackingEfficiency = 0.0)
    int32_t best = -1;
    double best_max = 0.0;
    for (uint32_t c = 0; c < n_zone_cand; ++c)
        if (sh.feas[c] && best_max < sh.mx[c]) {
            best = (int32_t)c;
            best_max = sh.mx[c];
        }
    if (AZ_AWARE && best < 0 && sh.feas[n_zone_cand]) best = (int32_t)n_zone_cand;  // az_aware_pack_tightly.go:33-37
    const bool feasible = best >= 0;
    if constexpr (FEAS) {
        if (tid == 0) feasible_announce(answers.words, a, feasible);
    } else {
        if (feasible) {
            const uint32_t* src = zexec + (size_t)best * zexec_stride + app.exec_off;
            uint32_t* dst = exec_nodes + app.exec_off;
            for (int64_t i = tid; i < K; i += kWave * kFusedWaves) dst[i] = T.slot_node[src[i]];
        }
        if (tid == 0) {
            gf_result r;
            r.has_capacity = feasible ? 1 : 0;
            r.driver_node = feasible ? T.slot_node[sh.ds[best]] : GF_NO_NODE;
            r.exec_len = feasible ? (uint32_t)K : 0u;
            r.evaluated = 1;
            answers.results[a] = r;
        }
    }
}
// The two parameter lists of that body: the batch proper, and feasibility only.
template <int ALGO, bool AZ_AWARE>
__global__ __launch_bounds__(kWave* kFusedWaves, ALGO == GF_ALGO_MINIMAL_FRAGMENTATION ? 4 : 1) void fit_zoned_fused_kernel(
    NodeTable T, SparseTable G, ZoneTable Z, const int64_t* __restrict__ sched, uint32_t n_apps, const gf_app* __restrict__ apps,
    gf_result* __restrict__ results, uint32_t* __restrict__ exec_nodes, uint32_t* __restrict__ zexec, uint64_t zexec_stride,
    uint32_t* __restrict__ scratch, uint64_t scratch_half) {
    fit_zoned_fused_body<ALGO, AZ_AWARE, false>(T, G, Z, sched, n_apps, apps, {results, nullptr}, exec_nodes, zexec, zexec_stride, scratch, scratch_half, 0u);
}
template <int ALGO, bool AZ_AWARE>
__global__ __launch_bounds__(kWave* kFusedWaves, ALGO == GF_ALGO_MINIMAL_FRAGMENTATION ? 4 : 1) void fit_zoned_fused_feasible_kernel(
    NodeTable T, SparseTable G, ZoneTable Z, const int64_t* __restrict__ sched, uint32_t n_apps, const gf_app* __restrict__ apps,
    uint8_t* __restrict__ bytes, uint32_t* __restrict__ words, uint32_t* __restrict__ zexec, uint64_t zexec_stride,
    uint32_t* __restrict__ scratch, uint64_t scratch_half, uint32_t eff_nonneg) {
    fit_zoned_fused_body<ALGO, AZ_AWARE, true>(T, G, Z, sched, n_apps, apps, {bytes, words}, nullptr, zexec, zexec_stride, scratch, scratch_half, eff_nonneg);
}

// ComputePackingEfficiencies for ONE result in node-index space: phase 1 scatters the `reserved` map, phase 2 (one
// thread per node) divides.  d_reserved is zeroed by the launcher.
template <bool RESERVE_EXECS>
__global__ void reserved_scatter_kernel(const gf_app* __restrict__ app, const gf_result* __restrict__ res,
                                        const uint32_t* __restrict__ exec_nodes, uint32_t n_nodes,
                                        unsigned long long* __restrict__ reserved) {
    if (!res->has_capacity) return;
    const int64_t K = app->k;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && res->driver_node < n_nodes)
        for (int j = 0; j < 3; ++j) atomicAdd(&reserved[3 * (size_t)res->driver_node + j], (unsigned long long)app->drv[j]);
    if (RESERVE_EXECS && (int64_t)i < K) {
        const uint32_t n = exec_nodes[app->exec_off + i];
        if (n < n_nodes)
            for (int j = 0; j < 3; ++j) atomicAdd(&reserved[3 * (size_t)n + j], (unsigned long long)app->exe[j]);
    }
}

__global__ void node_efficiency_kernel(EffTables E, uint32_t n_nodes, const int64_t* __restrict__ reserved,
                                       double* __restrict__ eff_out) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_nodes) return;
    NodeEff e;
    node_efficiency(E.avail[0][n], E.avail[1][n], E.avail[2][n], E.sched[0][n], E.sched[1][n], E.sched[2][n],
                    reserved[3 * (size_t)n], reserved[3 * (size_t)n + 1], reserved[3 * (size_t)n + 2], e);
    eff_out[3 * (size_t)n] = e.cpu;
    eff_out[3 * (size_t)n + 1] = e.mem;
    eff_out[3 * (size_t)n + 2] = e.gpu;
}

// ------------------------------------------------------------------------------------------------ generic FIFO chain
// fitEarlierDrivers + final pack (internal/extender/resource.go:224-262, 309-328) for ANY packer, zone-aware ones
// included: the chain is sequential over apps; within an app the candidates (each zone of the evaluation list, plus
// the plain pack for az-aware-tightly-pack) are decided concurrently, one wavefront each, against the working table
// in global memory (L2-resident; same-CU waves share the vector L1, so a workgroup barrier publishes the commits).
// Slower per app than the specialised plain-packer chain kernels (those keep the table in LDS), but it serves every
// layout and every registered packer with the same wave-level decision code as the independent batch.
struct GenericShared {
    int32_t feas[64];
    uint32_t ds[64];
    int64_t pass1[64];
    double mx[64];
};

template <int ALGO, bool ZONED, bool AZ_AWARE, bool RESERVE_EXECS>
__global__ __launch_bounds__(kWave * 16) void fit_fifo_generic_kernel(
    NodeTable T, ZoneTable Z, const int64_t* __restrict__ sched, uint32_t n_apps, const gf_app* __restrict__ apps,
    gf_result* __restrict__ results, uint32_t* __restrict__ exec_nodes, uint32_t* __restrict__ zexec,
    uint64_t zexec_stride, uint32_t* __restrict__ scratch, uint64_t scratch_half, uint32_t* __restrict__ cnt,
    int32_t* __restrict__ chain_failed_at, const int32_t* __restrict__ run_if) {
    __shared__ GenericShared sh;
    if (run_if != nullptr && *run_if == 0) return;  // the LDS-resident chain (gangfit_fifo_zoned.inc) served this batch
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n_waves = blockDim.x >> 6;
    const uint32_t n_zone_cand = ZONED ? Z.n_zones : 0u;
    const uint32_t n_cand = ZONED ? n_zone_cand + (AZ_AWARE ? 1u : 0u) : 1u;  // host guarantees n_cand <= 64
    const GlobalView plain{T.cpu, T.mem, T.gpu, T.cmax, T.cmax + T.n_chunks, T.cmax + 2 * (size_t)T.n_chunks,
                           T.xmask, T.dmask, T.n_chunks};
    // the chunk-maxima index was taken on the snapshot: still an upper bound while the chain only subtracts
    const EffView EV{T.cpu, T.mem, T.gpu, sched, sched + T.n_slots, sched + 2 * (size_t)T.n_slots};
    int32_t failed_at = -1;
    uint32_t a = 0;
    for (; a < n_apps; ++a) {
        const App app = load_app(apps, a);
        const int64_t K = app.k;
        const bool last = (a + 1 == n_apps);
        for (uint32_t c = wave; c < n_cand; c += n_waves) {
            const bool zone_view = c < n_zone_cand;
            GlobalView V = plain;
            if (zone_view) {
                V.xm = Z.xmask + (size_t)c * Z.stride;
                V.dm = Z.dmask + (size_t)c * Z.stride;
            }
            Orders O{T.slot_node, T.dslot, T.n_x, T.n_d, T.d_identity != 0, zone_view};
            unsigned long long xvis = 0, dvis = 0;
            uint32_t* out = zexec + (size_t)c * zexec_stride + app.exec_off;
            const Decision dec = wave_decide<ALGO, GlobalView, true>(V, O, app, out, scratch + app.exec_off,
                                                                     scratch + scratch_half + app.exec_off, lane, xvis,
                                                                     dvis);
            double avg[4] = {0.0, 0.0, 0.0, 0.0};
            if (ZONED && zone_view && dec.feasible) {
                // out[] was written by other lanes of this wave
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                wave_avg_efficiency<RESERVE_EXECS>(EV, app, dec.ds, out, nullptr, cnt + (size_t)wave * T.n_slots, lane,
                                                   avg);
            }
            if (lane == 0) {
                sh.feas[c] = dec.feasible ? 1 : 0;
                sh.ds[c] = dec.ds;
                sh.pass1[c] = dec.pass1;
                sh.mx[c] = avg[3];
            }
        }
        __syncthreads();
        // chooseBestResult (single_az.go:75-97), evaluated identically by every thread
        int32_t best = -1;
        if (ZONED) {
            double best_max = 0.0;
            for (uint32_t c = 0; c < n_zone_cand; ++c)
                if (sh.feas[c] && best_max < sh.mx[c]) {
                    best = (int32_t)c;
                    best_max = sh.mx[c];
                }
            if (AZ_AWARE && best < 0 && sh.feas[n_zone_cand]) best = (int32_t)n_zone_cand;  // az_aware_pack_tightly.go:33-37
        } else if (sh.feas[0]) {
            best = 0;
        }
        const bool feasible = best >= 0;
        Decision dec;
        dec.feasible = feasible;
        dec.ds = feasible ? sh.ds[best] : 0u;
        dec.pass1 = feasible ? sh.pass1[best] : 0;
        const uint32_t* src = zexec + (size_t)(feasible ? best : 0) * zexec_stride + app.exec_off;
        if (feasible) {
            uint32_t* dst = exec_nodes + app.exec_off;
            for (int64_t i = tid; i < K; i += blockDim.x) dst[i] = T.slot_node[src[i]];
        }
        if (tid == 0) {
            gf_result r;
            r.has_capacity = feasible ? 1 : 0;
            r.driver_node = feasible ? T.slot_node[dec.ds] : GF_NO_NODE;
            r.exec_len = feasible ? (uint32_t)K : 0u;
            r.evaluated = 1;
            results[a] = r;
        }
        bool stop = false;
        if (last) {
            stop = true;  // the driver being filtered: nothing is subtracted after it (resource.go:321-328)
        } else if (!feasible) {
            if (!(app.flags & GF_APP_SKIPPABLE)) {  // resource.go:249-251
                failed_at = (int32_t)a;
                stop = true;
            }
        } else if (wave == 0) {
            // sparkResourceUsage + SubtractUsageIfExists (sparkpods.go:139-146, resources.go:129-135) from the slot list
            wave_commit_from_list<ALGO, GlobalView>(plain, app, dec, src, lane);
        }
        __syncthreads();  // commits visible (and sh reusable) before the next app's scans
        if (stop) {
            ++a;
            break;
        }
    }
    for (uint32_t r = a + tid; r < n_apps; r += blockDim.x) {  // apps behind an abort are reported as not evaluated
        gf_result z;
        z.has_capacity = 0;
        z.driver_node = GF_NO_NODE;
        z.exec_len = 0;
        z.evaluated = 0;
        results[r] = z;
    }
    if (tid == 0 && chain_failed_at != nullptr) *chain_failed_at = failed_at;
}
