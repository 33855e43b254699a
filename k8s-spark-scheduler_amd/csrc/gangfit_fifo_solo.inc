// gangfit_fifo_solo.inc — FIFO chain, narrow domain, ONE controlling wavefront.  Included by gangfit_kernels.hip inside its
// anonymous namespace, after gangfit_fifo_common.inc (app record, capacity arithmetic, shape dedup, run-head contract).
//
// Why: the chain (resource.go:224-262) is sequential in the applications, and with the exact per-shape chunk index of
// gangfit_fifo_narrow.inc an application visits ~1.6 chunks of 64 slots on the headline workload — there is nothing
// left for sixteen wavefronts to share, but every one of them still executes the ~600 instructions of per-app control
// flow, the exchange through LDS and a barrier per scan step (measured with the block-cooperative kernel this one
// replaced: 2 600 cycles per scan step with four wavefronts, 5 800 with sixteen).  Here wavefront 0 walks the chain alone —
// no barrier, no exchange, scalar control flow — and the other wavefronts of the workgroup only fill LDS / build the shape
// index before the chain, dump a CHECKPOINT of the working table every 2^shift applications (ChainCkpt: what lets the next
// Filter of the same queue resume instead of replaying, gangfit_api_fit.cpp) and write the residual table back after it; in
// between they sleep at a barrier and take no issue slots.
//
// Per application (wavefront 0):
//   * bound test: a per-executor-shape upper bound of the cluster's total capacity (learnt from scans that came out
//     short; capacities only fall during a chain) rejects applications that cannot fit without a scan;
//   * driver search: candidate chunks of the driver shape in order, ballot of the driver-fit check (binpack.go:67-71);
//   * executor scan with the driver reserved on that slot (pack_tightly.go:45-61 / distribute_evenly.go pass 1), lazy,
//     candidate chunks of the executor shape only; placements as run heads (tightly-pack) or slot ids;
//   * commit (sparkpods.go:139-146), optimistic: every chunk the scan consumes is committed from the registers it is in
//     (subtract, store); the hit list (chunk, lane mask) in LDS only serves the rollback of a gang that turns out not to fit
//     behind its first driver.  The shape index is maintained lazily (a filled chunk keeps its bits until a scan visits it and
//     clears the shape's whole family) — eagerly only for tables with a global tail;
//   * the rare cases (several distribute-evenly passes, the first fitting driver cannot host the gang) run the generic
//     wave-level code on the scaled table, exactly as in the block-cooperative kernel.
// A slot is always handled by lane (slot & 63), so a global-memory slot (tables larger than the LDS front) is only
// ever touched by one work-item on the fast path; the slow path ends with a workgroup fence.

struct SoloShared {
    uint32_t final_a;   // first application index the chain did not evaluate
    int32_t failed_at;  // chain_failed_at
    uint32_t ckpt_cmd;  // wavefront 0 -> helpers: checkpoint slot to dump the table to, kCkptDone = the chain is over
    uint32_t pad;
};

constexpr uint32_t kCkptDone = 0xFFFFFFFFu;

// LDS layout of the table front: one 784-byte block per 64-slot chunk — cpu[64] | mem[64] | gpu[64] | xmask | dmask — so
// that a chunk visit is ONE address computation, a ds_read2st64_b32 (cpu, mem), a ds_read_b32 (gpu) and a ds_read_b128
// (both candidate masks), all in flight together.
constexpr uint32_t kBlkDwords = 196;
// NApp.flags, bits 8..10 (set by prepare_app, gangfit_fifo_common.inc): executor request dimension j is zero — its capacity term is
// "unlimited unless the slot is overcommitted" and needs no division.
constexpr uint32_t kNAppZeroShift = 8;

// The block-layout table behind the View interface of the generic wave-level code (slow path only).
struct NarrowBlockView {
    lds_i32* blk;
    uint32_t lds_slots;
    glb_i32* cpu;
    glb_i32* mem;
    glb_i32* gpu;
    lds_i32* cmax_cpu;
    lds_i32* cmax_mem;
    lds_i32* cmax_gpu;
    lds_u64* xm;
    lds_u64* dm;
    uint32_t n_chunks;
    lds_u64* dirty;  // one bit per chunk a commit touched since the last checkpoint (tables beyond the LDS front only), else null
    __device__ __forceinline__ void chunk_maxima(uint32_t c, int64_t& m0, int64_t& m1, int64_t& m2) const {
        m0 = cmax_cpu[c];
        m1 = cmax_mem[c];
        m2 = cmax_gpu[c];
    }
    __device__ __forceinline__ bool chunk_may_hold(uint32_t c, int64_t r0, int64_t r1, int64_t r2) const {
        int64_t m0, m1, m2;
        chunk_maxima(c, m0, m1, m2);
        return (bool)((m0 >= r0) & (m1 >= r1) & (m2 >= r2));
    }
    __device__ __forceinline__ uint64_t chunk_xmask(uint32_t c) const { return xm[c]; }
    __device__ __forceinline__ uint64_t chunk_dmask(uint32_t c) const { return dm[c]; }
    __device__ __forceinline__ bool xcand(uint32_t s) const { return (xm[s >> 6] >> (s & 63)) & 1ull; }
    __device__ __forceinline__ bool dcand(uint32_t s) const { return (dm[s >> 6] >> (s & 63)) & 1ull; }
    __device__ __forceinline__ void load32(uint32_t s, int32_t& a0, int32_t& a1, int32_t& a2) const {
        if (s < lds_slots) {
            const lds_i32* p = blk + (size_t)(s >> 6) * kBlkDwords + (s & 63u);
            a0 = p[0];
            a1 = p[64];
            a2 = p[128];
        } else {
            a0 = cpu[s];
            a1 = mem[s];
            a2 = gpu[s];
        }
    }
    __device__ __forceinline__ void load(uint32_t s, int64_t& a0, int64_t& a1, int64_t& a2) const {
        int32_t b0, b1, b2;
        load32(s, b0, b1, b2);
        a0 = b0;
        a1 = b1;
        a2 = b2;
    }
    __device__ __forceinline__ void sub32(uint32_t s, int32_t r0, int32_t r1, int32_t r2) const {
        if (dirty != nullptr) atomicOr((unsigned long long*)&dirty[s >> 12], 1ull << ((s >> 6) & 63u));
        if (s < lds_slots) {
            lds_i32* p = blk + (size_t)(s >> 6) * kBlkDwords + (s & 63u);
            p[0] -= r0;
            p[64] -= r1;
            p[128] -= r2;
        } else {
            cpu[s] -= r0;
            mem[s] -= r1;
            gpu[s] -= r2;
        }
    }
    __device__ __forceinline__ void sub(uint32_t s, int64_t r0, int64_t r1, int64_t r2) const {
        sub32(s, (int32_t)r0, (int32_t)r1, (int32_t)r2);
    }
};

constexpr int kSoloWaves = 16;  // wavefronts of the workgroup (launch bound = VGPR budget: 16 -> 128 per lane, 8 -> 256)

// The staged record: K, the flags and the two shape ids become wave-uniform (SGPRs: they steer the scalar control flow);
// the request vectors, the reciprocals and the placement offset stay in VGPRs (they are only ever VALU operands, and
// sixteen fewer live SGPRs keep the loop free of SGPR spills).
__device__ __forceinline__ NAppR napp_from_words_mixed(const u32x4& w0, const u32x4& w1, const u32x4& w2, const u32x4& w3) {
    NAppR r;
    r.drv0 = (int32_t)w0.x;
    r.drv1 = (int32_t)w0.y;
    r.drv2 = (int32_t)w0.z;
    r.k = (int32_t)uniform32(w0.w);
    r.exe0 = (int32_t)w1.x;
    r.exe1 = (int32_t)w1.y;
    r.exe2 = (int32_t)w1.z;
    r.flags = uniform32(w1.w);
    r.mag0 = w2.x;
    r.mag1 = w2.y;
    r.mag2 = w2.z;
    r.msh = w2.w;
    r.exec_off = ((uint64_t)w3.y << 32) | w3.x;
    r.shape_x = uniform32(w3.z);
    r.shape_d = uniform32(w3.w);
    return r;
}

__device__ __forceinline__ NAppR napp_all_uniform(const NAppR& v) {
    NAppR r;
    r.drv0 = (int32_t)uniform32((uint32_t)v.drv0);
    r.drv1 = (int32_t)uniform32((uint32_t)v.drv1);
    r.drv2 = (int32_t)uniform32((uint32_t)v.drv2);
    r.k = v.k;
    r.exe0 = (int32_t)uniform32((uint32_t)v.exe0);
    r.exe1 = (int32_t)uniform32((uint32_t)v.exe1);
    r.exe2 = (int32_t)uniform32((uint32_t)v.exe2);
    r.flags = v.flags;
    r.mag0 = uniform32(v.mag0);
    r.mag1 = uniform32(v.mag1);
    r.mag2 = uniform32(v.mag2);
    r.msh = uniform32(v.msh);
    r.exec_off = uniform64(v.exec_off);
    r.shape_x = v.shape_x;
    r.shape_d = v.shape_d;
    return r;
}

// "Which lanes hold at least r in every dimension": three compares that leave their lane masks in scalar registers and are
// combined there with the chunk's candidate mask (a wave-uniform 64-bit word: bit l = lane l's slot is a candidate).  The
// same test written on per-lane booleans — (cand >> lane) & 1 & (a0 >= r0) & ... and a __ballot — costs eleven instructions
// instead of six: the compiler turns the combined boolean back into a lane value and compares it again to build the ballot.
// The other direction: "is my lane's bit set in this wave-uniform mask" as the condition of a branch or a select costs nothing
// (the mask becomes the execution mask / the select's condition register); written as (mask >> lane) & 1 it costs three vector
// instructions per use.
__device__ __forceinline__ bool lane_bit(uint64_t uniform_mask) { return __builtin_amdgcn_inverse_ballot_w64(uniform_mask); }

// (cand must already be a scalar value — uniform64 of what the LDS read returned in every lane —, or the AND and everything
//  that branches on the result turn into per-lane code.)
__device__ __forceinline__ uint64_t fit_mask(int32_t a0, int32_t a1, int32_t a2, int32_t r0, int32_t r1, int32_t r2, uint64_t cand) {
    constexpr int kSGE = 39;  // signed >=
    return __builtin_amdgcn_sicmp(a0, r0, kSGE) & __builtin_amdgcn_sicmp(a1, r1, kSGE) & __builtin_amdgcn_sicmp(a2, r2, kSGE) & cand;
}

// The rare cases of one application, out of line: more distribute-evenly passes and / or another driver, on the generic
// wave-level code (scaled values), then the commit from the placement list.  taken = exact capacity total with the driver
// on p0 (tightly-pack) / the number of pass-1 survivors, which are out[0 .. taken) (distribute-evenly).
// Returns the driver slot, kNoPos when the application does not fit.
// A real call on purpose: this code loads from global memory (placement lists, the table tail), and a load the compiler
// cannot prove finished makes it guard every later write of the same VGPR with s_waitcnt vmcnt(0) — which also waits for
// every placement store in flight.  Behind a call boundary all counters are drained once, on this path only.
template <int ALGO>
__device__ __attribute__((noinline)) uint32_t solo_slow_path(const NarrowBlockView& V, const Orders& O, const NAppR app,
                                                             uint32_t p0, int32_t taken, bool last,
                                                             uint32_t* __restrict__ out, uint32_t* __restrict__ sa,
                                                             uint32_t* __restrict__ sb, lds_i32* sbound) {
    const int lane = lane_id();
    const int32_t K = app.k;
    unsigned long long xvis = 0, dvis = 0;
    App wapp;
    wapp.drv0 = app.drv0;
    wapp.drv1 = app.drv1;
    wapp.drv2 = app.drv2;
    wapp.exe0 = app.exe0;
    wapp.exe1 = app.exe1;
    wapp.exe2 = app.exe2;
    wapp.rcp0 = app.exe0 > 0 ? 1.0 / (double)app.exe0 : 0.0;
    wapp.rcp1 = app.exe1 > 0 ? 1.0 / (double)app.exe1 : 0.0;
    wapp.rcp2 = app.exe2 > 0 ? 1.0 / (double)app.exe2 : 0.0;
    wapp.k = app.k;
    wapp.flags = app.flags;
    wapp.exec_off = app.exec_off;
    Decision d2;
    d2.feasible = false;
    d2.ds = p0;
    d2.pass1 = taken;
    int64_t S_d = taken;
    if (ALGO != GF_ALGO_TIGHTLY_PACK) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        for (int32_t i = lane; i < taken; i += kWave) sa[i] = out[i];
        S_d = wave_even_general<NarrowBlockView, true>(V, O, wapp, p0, out, sa, sb, taken, lane);
    }
    if (S_d >= K) {
        d2.feasible = true;
    } else {
        // total capacity without any driver reserved: S = S_d + cap(p0, 0) - cap(p0, drv).  Below K it is exact and
        // unclamped (every term is below K), and capacities only fall during a chain: a bound for the shape.
        int32_t b0, b1, b2;
        V.load32(p0, b0, b1, b2);
        int64_t S = S_d;
        if (V.xcand(p0)) S += ncap3(b0, b1, b2, app) - ncap3(b0 - app.drv0, b1 - app.drv1, b2 - app.drv2, app);
        if (S < K) {
            if (app.shape_x != kNoShape && lane == 0) sbound[app.shape_x] = (int32_t)S;
        } else {
            d2 = wave_fallback<ALGO, NarrowBlockView, true>(V, O, wapp, (int64_t)p0, p0, S_d, out, sa, sb, lane, xvis, dvis);
        }
    }
    if (d2.feasible && !last) wave_commit_from_list<ALGO, NarrowBlockView>(V, wapp, d2, out, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return d2.feasible ? d2.ds : kNoPos;
}

// An application whose request vectors got no shape id (more than kMaxShapes distinct vectors in the batch): the whole
// decision and its commit on the generic wave-level code with the chunk-maxima index (static upper bounds during a
// chain), out of line — the chain loop itself only knows indexed applications.  Returns the driver slot or kNoPos.
template <int ALGO>
__device__ __attribute__((noinline)) uint32_t solo_unindexed_app(const NarrowBlockView& V, const Orders& O, const NAppR app,
                                                                 bool last, uint32_t* __restrict__ out,
                                                                 uint32_t* __restrict__ sa, uint32_t* __restrict__ sb) {
    const int lane = lane_id();
    unsigned long long xvis = 0, dvis = 0;
    App wapp;
    wapp.drv0 = app.drv0;
    wapp.drv1 = app.drv1;
    wapp.drv2 = app.drv2;
    wapp.exe0 = app.exe0;
    wapp.exe1 = app.exe1;
    wapp.exe2 = app.exe2;
    wapp.rcp0 = app.exe0 > 0 ? 1.0 / (double)app.exe0 : 0.0;
    wapp.rcp1 = app.exe1 > 0 ? 1.0 / (double)app.exe1 : 0.0;
    wapp.rcp2 = app.exe2 > 0 ? 1.0 / (double)app.exe2 : 0.0;
    wapp.k = app.k;
    wapp.flags = app.flags;
    wapp.exec_off = app.exec_off;
    const Decision d = wave_decide<ALGO, NarrowBlockView, true>(V, O, wapp, out, sa, sb, lane, xvis, dvis);
    if (d.feasible && !last) wave_commit_from_list<ALGO, NarrowBlockView>(V, wapp, d, out, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return d.feasible ? d.ds : kNoPos;
}

// Everything an application's rare endings need, built at the call site only (the chain loop keeps none of it alive).
struct SoloRare {
    NarrowBlockView V;
    Orders O;
    NAppR app;  // all-uniform copy
    uint32_t a;
    bool last;
    uint32_t p0;      // the first fitting driver candidate (kRareShort)
    int32_t taken;    // what the lazy scan placed behind it (kRareShort)
    uint32_t nhit;    // optimistic commits to take back: hchunk / hmask[0 .. nhit) (kRareShort)
    bool hosts;       // an executor sits on the driver's slot
    bool pc_done;     // the driver's chunk has been committed
    unsigned long long domx, domd;
    lds_u64* sbits;
    uint32_t nwp;
    lds_i32* hchunk;
    lds_u64* hmask;
    lds_i32* sbound;
    uint32_t* out;
    uint32_t* sa;
    uint32_t* sb;
    gf_result* results;
};
enum : int { kSoloOk = 0, kRareUnindexed = 1, kRareBound = 2, kRareNoDriver = 3, kRareShort = 4 };

// The rare endings of one application, ONE real call for all of them: a request without a shape id, the capacity bound, no
// driver candidate, a gang that does not fit behind its first driver (the optimistic commits are taken back, then the generic
// code decides).  Reports the application; returns false when the chain stops here (resource.go:244-251), *failed_at set.
// Keeping these bodies out of the chain loop is what keeps the loop's scalar state in registers: inlined, each of them adds
// its own live ranges and its own edges to the loop's latch (chains of branch-only blocks on the COMMON path).
template <int ALGO, bool OPTIMISTIC>
__device__ __attribute__((noinline)) bool solo_rare_app(const SoloRare& R, int code, int32_t* failed_at) {
    const int lane = lane_id();
    uint32_t ds = kNoPos;
    if (code == kRareUnindexed) {
        ds = uniform32(solo_unindexed_app<ALGO>(R.V, R.O, R.app, R.last, R.out, R.sa, R.sb));
    } else if (code == kRareShort) {
        if (OPTIMISTIC && !R.last) {
            // what the scan subtracted chunk by chunk goes back, and the two shapes' index bits of those chunks are set again
            // (a 1 that should be 0 only costs a visit)
            const uint32_t pc = R.p0 >> 6, pl = R.p0 & 63u;
            for (uint32_t i = 0; i < R.nhit; ++i) {
                const uint32_t c = uniform32((uint32_t)R.hchunk[i]);
                const uint64_t m = uniform64(R.hmask[i]);
                const uint32_t s = c * kWave + (uint32_t)lane;
                const bool h = (m >> lane) & 1ull;
                const bool d = c == pc && (uint32_t)lane == pl && !R.hosts;  // what commit_chunk subtracted there
                if (h || d) R.V.sub32(s, -((h ? R.app.exe0 : 0) + (d ? R.app.drv0 : 0)), -((h ? R.app.exe1 : 0) + (d ? R.app.drv1 : 0)),
                                      -((h ? R.app.exe2 : 0) + (d ? R.app.drv2 : 0)));
                if (((R.domx | R.domd) >> lane) & 1ull)  // (what the optimistic commits cleared: the two shapes' families)
                    atomicOr((unsigned long long*)&R.sbits[(size_t)lane * R.nwp + (c >> 6)], 1ull << (c & 63u));
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        ds = uniform32(solo_slow_path<ALGO>(R.V, R.O, R.app, R.p0, R.taken, R.last, R.out, R.sa, R.sb, R.sbound));
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): nothing of this path's memory traffic is left for the loop to wait for
    const bool feasible = ds != kNoPos;
    if (lane == 0) {
        gf_result r;
        r.has_capacity = feasible ? 1 : 0;
        r.driver_node = feasible ? ds : GF_NO_NODE;  // SLOT id; expand_translate_kernel maps it to the node index
        r.exec_len = feasible ? (uint32_t)R.app.k : 0u;
        r.evaluated = kEvalDone;
        R.results[R.a] = r;
    }
    if (feasible || R.last || (R.app.flags & GF_APP_SKIPPABLE)) return true;
    *failed_at = (int32_t)R.a;
    return false;
}

// A chunk of the table's global tail (tables larger than the LDS front), as REAL calls for the reason given at
// solo_slow_path: inlined, these loads share their destination registers with the LDS path of a chunk visit, and the compiler
// then guards every chunk visit — LDS ones included — with s_waitcnt vmcnt(0), i.e. with a wait for every placement and
// result store in flight (the 100 000-node chain spent more time in those waits than in the work).
struct SoloTriple {
    int32_t v0, v1, v2;
};
__device__ __attribute__((noinline)) SoloTriple solo_tail_load(const glb_i32* cpu, const glb_i32* mem, const glb_i32* gpu,
                                                               uint32_t s, uint32_t n_slots) {
    SoloTriple t{INT32_MIN / 2, INT32_MIN / 2, INT32_MIN / 2};
    if (s < n_slots) {
        t.v0 = cpu[s];
        t.v1 = mem[s];
        t.v2 = gpu[s];
    }
    return t;
}
__device__ __attribute__((noinline)) void solo_tail_store(glb_i32* cpu, glb_i32* mem, glb_i32* gpu, uint32_t s, int32_t a0,
                                                          int32_t a1, int32_t a2) {
    cpu[s] = a0;
    mem[s] = a1;
    gpu[s] = a2;
}

// RESIDENT: the whole table fits the LDS front.  The chain loop then holds no global LOAD at all, which matters because
// placement / result stores count in vmcnt too: a single load in the loop makes the compiler wait for vmcnt(0) — i.e. for
// every store still in flight (~1 us each) — at every chunk visit.
template <int ALGO, int NW, bool PROF, bool RESIDENT>
__global__ __launch_bounds__(kWave* NW) void fit_fifo_solo_kernel(NodeTable T, NarrowTable NT, uint32_t lds_slots,
                                                                 uint32_t n_apps, NApp* __restrict__ napps,
                                                                 const int32_t* __restrict__ wide_needed,
                                                                 gf_result* __restrict__ results,
                                                                 uint32_t* __restrict__ exec_nodes,
                                                                 uint32_t* __restrict__ scratch, uint64_t scratch_half,
                                                                 int32_t* __restrict__ chain_failed_at,
                                                                 ChainCkpt ck, SoloFused F, ScanStats* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t BLOCK = kWave * NW;
    static_assert(NW > 1, "the helpers dump the checkpoints");
    // (F.enabled: the host has proven that every request has a scaled form — the flag is not even computed)
    if (!F.enabled && *wide_needed) return;  // some request of this batch is not representable in the narrow domain
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id();
    const int wave = (int)__builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned long long t0_cycles = __builtin_readcyclecounter();
    const unsigned long long t0_real = wall_clock64();
    const uint32_t nc = T.n_chunks;
    const uint32_t nw = (nc + 63u) / 64u;  // 64-bit words per shape in the shape index = groups of 64 chunks
    const uint32_t nwp = nw < 4u ? 4u : nw;  // row stride of the index: the chain reads the first four words as two b128

    // ---- LDS carve (fifo_solo_lds_bytes mirrors it)
    lds_u4* stage4 = (lds_u4*)smem;
    size_t off = kFusedStage * sizeof(NApp);
    SoloShared* sh = reinterpret_cast<SoloShared*>(smem + off);
    off += sizeof(SoloShared);
    lds_u64* lxm = (lds_u64*)(smem + off);
    off += 8 * (size_t)nc;
    lds_u64* ldm = (lds_u64*)(smem + off);
    off += 8 * (size_t)nc;
    lds_u64* sbits = (lds_u64*)(smem + off);  // [kMaxShapes][nwp]: ONE copy — only wavefront 0 reads it during the chain
    off += 8 * (size_t)kMaxShapes * nwp;
    lds_u64* hmask = (lds_u64*)(smem + off);  // [nc] hit list: lanes of the chunk that host an executor of this app
    off += 8 * (size_t)nc;
    lds_u64* dirty = (lds_u64*)(smem + off);  // [nw] chunks that differ from the snapshot as of the last checkpoint (!RESIDENT)
    off += 8 * (size_t)nw;
    lds_u64* fresh = (lds_u64*)(smem + off);  // [nw] chunks touched by a commit since the last checkpoint: what the next one dumps
    off += 8 * (size_t)nw;
    lds_u64* sdom = (lds_u64*)(smem + off);  // [kMaxShapes] shapes of the same role that need at least as much in every dimension
    off += 8 * (size_t)kMaxShapes;
    off = (off + 15) & ~(size_t)15;
    ShapeEntry* stab = reinterpret_cast<ShapeEntry*>(smem + off);  // [kShapeHashSlots] dedup hash table
    off += sizeof(ShapeEntry) * kShapeHashSlots;
    ShapeEntry* svec = reinterpret_cast<ShapeEntry*>(smem + off);  // [kMaxShapes] dense shape table (tag = role)
    off += sizeof(ShapeEntry) * kMaxShapes;
    lds_i32* sid = (lds_i32*)(smem + off);  // [kShapeHashSlots] hash slot -> dense id
    off += 4 * (size_t)kShapeHashSlots;
    lds_i32* scount = (lds_i32*)(smem + off);
    off += 16;
    lds_i32* sbound = (lds_i32*)(smem + off);  // [kMaxShapes] executor shapes: upper bound of the total capacity
    off += 4 * (size_t)kMaxShapes;
    lds_i32* hchunk = (lds_i32*)(smem + off);  // [nc] hit list: chunk ids
    off += 4 * (size_t)nc;
    lds_i32* lmax = (lds_i32*)(smem + off);  // [3][nc]
    off += 12 * (size_t)nc;
    off = (off + 15) & ~(size_t)15;
    lds_i32* lblk = (lds_i32*)(smem + off);  // [lds_chunks] chunk blocks (kBlkDwords each)
    const uint32_t lds_chunks = lds_slots / kWave;  // lds_slots is a multiple of 64

    // ---- prologue, all wavefronts: table front, maxima, masks, shape dedup + index
    // F.enabled (whole table in LDS, every request proven to have a scaled form): this kernel is also the chain's first one —
    // it takes the records from where the caller has them (pinned host memory or the device), writes the device copy the
    // translate step reads and the scaled records, presets the run heads and fills LDS straight from the snapshot or the
    // checkpoint the chain resumes from, instead of from a working copy another kernel made (chain_prologue_kernel: one
    // launch, one kernel boundary and a 240 KB copy less per Filter)
    const int32_t* src_cpu = NT.cpu;
    const int32_t* src_mem = NT.mem;
    const int32_t* src_gpu = NT.gpu;
    if (F.enabled) {
        if (F.table_src != nullptr) {
            src_cpu = F.table_src;
            src_mem = F.table_src + T.n_slots;
            src_gpu = F.table_src + 2 * (size_t)T.n_slots;
        }
        if (tid == 0 && F.wide_clear != nullptr) *F.wide_clear = 0;
        const int64_t unit[3] = {F.unit[0], F.unit[1], F.unit[2]};
        int32_t never = 0;  // (proven on the host: no request raises the flag)
        for (uint32_t a = tid; a < n_apps; a += BLOCK) {
            gf_app in;
            if (F.apps_src != nullptr) {
                in = F.apps_src[a];
                F.apps_dst[a] = in;
            } else {
                in = F.apps_dst[a];
            }
            prepare_app(in, napps + a, unit, &never);
        }
        for (size_t i = tid; i < F.fill_words; i += BLOCK) F.fill_dst[i] = kHeadEmpty;
        // the scaled records are re-read and the run heads re-written by OTHER wavefronts behind the barriers below: a
        // workgroup-scope release does not wait for stores to leave this wavefront
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    for (uint32_t s = tid; s < lds_slots; s += BLOCK) {
        const bool real = s < T.n_slots;
        lds_i32* p = lblk + (size_t)(s >> 6) * kBlkDwords + (s & 63u);
        p[0] = real ? src_cpu[s] : INT32_MIN / 2;
        p[64] = real ? src_mem[s] : INT32_MIN / 2;
        p[128] = real ? src_gpu[s] : INT32_MIN / 2;
    }
    for (uint32_t c = tid; c < 3 * nc; c += BLOCK) lmax[c] = NT.cmax[c];
    for (uint32_t c = tid; c < nc; c += BLOCK) {
        const uint64_t xm = T.xmask[c], dm = T.dmask[c];
        lxm[c] = xm;
        ldm[c] = dm;
        if (c < lds_chunks) {
            lds_u64* mk = (lds_u64*)(lblk + (size_t)c * kBlkDwords + 192);
            mk[0] = xm;
            mk[1] = dm;
        }
    }
    for (uint32_t i = tid; i < kShapeHashSlots; i += BLOCK) {
        stab[i].tag = 0;
        sid[i] = INT32_MAX;  // during the dedup: the first request (queue order) that names the slot's shape
    }
    for (uint32_t i = tid; i < kMaxShapes * nwp; i += BLOCK) sbits[i] = 0;
    for (uint32_t i = tid; i < kMaxShapes; i += BLOCK) sbound[i] = INT32_MAX;
    // a resumed chain starts from a table that already differs from the snapshot in the chunks its checkpoint names
    for (uint32_t i = tid; i < nw; i += BLOCK) {
        dirty[i] = (!RESIDENT && ck.resume_mask != nullptr) ? ck.resume_mask[i] : 0ull;
        fresh[i] = 0ull;
    }
    if (tid == 0) {
        scount[0] = 0;
        scount[1] = 0;  // hash slots claimed so far
        sh->final_a = n_apps;
        sh->failed_at = -1;
        sh->ckpt_cmd = kCkptDone;
    }
    __syncthreads();
    for (uint32_t v = tid; v < 2 * n_apps; v += BLOCK) {
        const uint32_t role = v & 1u;  // 0 = executor request, 1 = driver request
        const NApp* rec = napps + (v >> 1);
        const int32_t v0 = role ? rec->drv[0] : rec->exe[0], v1 = role ? rec->drv[1] : rec->exe[1],
                      v2 = role ? rec->drv[2] : rec->exe[2];
        const uint32_t tag = shape_tag(v0, v1, v2, role);
        // Linear probing over the WHOLE table.  (Rounds 2-4 gave up after eight probes: a shape whose eight slots had been taken
        // by others got no id and its applications ran on the generic code — and WHICH shape lost that race depended on the order
        // in which the threads arrived.  On BASELINE config 5's queue either a shape with 2 applications or one with 67 was left
        // out: the same chain took 3.3 or 4.3-5.7 ms from one call to the next, profiles/r5c_c5_heads.txt.)
        // Every slot remembers the FIRST request of the queue that names its shape (an atomic minimum over request numbers):
        // the dense ids below follow that order, so which shapes are indexed does not depend on where the hash put them or on
        // which thread arrived first (round 5's ids followed the slot order: with 65 to 128 shapes the 64 indexed ones were the
        // ones in the low slots).  Once every slot is claimed the probing stops early — a queue with more than 128 distinct
        // request vectors would otherwise pay 128 probes per remaining request, twice (which shapes hold the slots is then
        // still a matter of arrival order: such a queue has more shapes than the index can hold either way).
        for (uint32_t i = 0; i < kShapeHashSlots; ++i) {
            const uint32_t slot = ((tag >> 2) + i) & (kShapeHashSlots - 1);
            const uint32_t old = atomicCAS(&stab[slot].tag, 0u, tag);
            if (old == 0) {  // claimed: this thread defines the entry
                stab[slot].v0 = v0;
                stab[slot].v1 = v1;
                stab[slot].v2 = v2;
                __hip_atomic_fetch_add(&scount[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if (old == 0 || old == tag) {
                __hip_atomic_fetch_min(&sid[slot], (int32_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                break;
            }
            if ((i & 15u) == 15u && scount[1] >= (int32_t)kShapeHashSlots) break;  // the table is full
        }
    }
    __syncthreads();
    if (wave == 0) {  // claimed slots get dense ids in the order of their first request
        static_assert(kShapeHashSlots == 2u * (uint32_t)kWave, "two hash slots per lane");
        const bool u0 = stab[lane].tag != 0, u1 = stab[kWave + lane].tag != 0;
        const int32_t f0 = u0 ? sid[lane] : INT32_MAX, f1 = u1 ? sid[kWave + lane] : INT32_MAX;
        int32_t rank0 = 0, rank1 = 0;  // used slots whose first request comes earlier (the firsts of two used slots differ)
        for (int y = 0; y < kWave; ++y) {
            const int32_t g0 = read_lane(f0, y), g1 = read_lane(f1, y);
            rank0 += (g0 < f0 ? 1 : 0) + (g1 < f0 ? 1 : 0);
            rank1 += (g0 < f1 ? 1 : 0) + (g1 < f1 ? 1 : 0);
        }
        const int32_t n_used = (int32_t)__popcll((unsigned long long)__ballot(u0)) + (int32_t)__popcll((unsigned long long)__ballot(u1));
        auto assign = [&](uint32_t slot, bool used, int32_t id) {
            sid[slot] = (used && id < (int32_t)kMaxShapes) ? id : -1;
            if (used && id < (int32_t)kMaxShapes) {
                svec[id].v0 = stab[slot].v0;
                svec[id].v1 = stab[slot].v1;
                svec[id].v2 = stab[slot].v2;
                svec[id].tag = (stab[slot].tag >> 1) & 1u;  // role
            }
        };
        assign((uint32_t)lane, u0, rank0);
        assign((uint32_t)(kWave + lane), u1, rank1);
        if (lane == 0) scount[0] = n_used < (int32_t)kMaxShapes ? n_used : (int32_t)kMaxShapes;
    }
    __syncthreads();
    for (uint32_t v = tid; v < 2 * n_apps; v += BLOCK) {  // every request looks its id up (verifying the vector)
        const uint32_t role = v & 1u;
        NApp* rec = napps + (v >> 1);
        const int32_t v0 = role ? rec->drv[0] : rec->exe[0], v1 = role ? rec->drv[1] : rec->exe[1],
                      v2 = role ? rec->drv[2] : rec->exe[2];
        const uint32_t tag = shape_tag(v0, v1, v2, role);
        uint32_t id = kNoShape;
        for (uint32_t i = 0; i < kShapeHashSlots; ++i) {
            const uint32_t slot = ((tag >> 2) + i) & (kShapeHashSlots - 1);
            const uint32_t t = stab[slot].tag;
            if (t == tag) {
                if (stab[slot].v0 == v0 && stab[slot].v1 == v1 && stab[slot].v2 == v2 && sid[slot] >= 0)
                    id = (uint32_t)sid[slot];
                break;
            }
            if (t == 0) break;
        }
        reinterpret_cast<uint32_t*>(&rec->pad)[role] = id;  // pad = {shape_x, shape_d}
    }
    const uint32_t n_shapes = (uint32_t)scount[0];
    // dominators: when a chunk holds no slot for shape s any more it holds none for a shape of the same role that asks for at
    // least as much in every dimension — their index bits are cleared (and, on a rollback, set) together with s's own, so a
    // filled chunk is discovered once per family of shapes instead of once per shape (a stale visit costs ~600 cycles).  The
    // masks are built below, lane = shape, next to the index (`up`); wavefront 0 leaves them in sdom for the chain.
    {
        // bit c of shape s <=> some candidate slot of chunk c fits s.  Lane = shape id for the shape table (read from LDS once,
        // handed out with v_readlane: a shape per LDS round trip made this loop 4 k cycles per chunk, and a 100 000-node table has
        // 1 563 of them: profiles/r5v_resume_fixed_cost.txt), the verdicts of a chunk are collected in a scalar mask and leave as
        // ONE lane-parallel LDS atomic, and the values of two chunks are requested before the first is tested (the table's
        // tail comes from global memory).
        int32_t sv0 = INT32_MAX, sv1 = INT32_MAX, sv2 = INT32_MAX;
        uint32_t stag = 0;
        if ((uint32_t)lane < n_shapes) {
            const ShapeEntry me = svec[lane];
            sv0 = me.v0;
            sv1 = me.v1;
            sv2 = me.v2;
            stag = me.tag;
        }
        auto values_of = [&](uint32_t c, int32_t& a0, int32_t& a1, int32_t& a2) {
            const uint32_t sl = c * kWave + lane;
            a0 = a1 = a2 = INT32_MIN / 2;
            if (c < nc && sl < T.n_slots) {
                if (sl < lds_slots) {
                    const lds_i32* p = lblk + (size_t)c * kBlkDwords + lane;
                    a0 = p[0];
                    a1 = p[64];
                    a2 = p[128];
                } else {
                    a0 = NT.cpu[sl];
                    a1 = NT.mem[sl];
                    a2 = NT.gpu[sl];
                }
            }
        };
        const uint64_t driver_shapes = __ballot(stag != 0u);  // lane = shape id: the shapes that are driver requests
        const uint64_t all_shapes = low_lanes(n_shapes);
        // lane = shape id: the shapes of my role that ask for at least as much as I do in every dimension (`up`: when I fit nowhere
        // in a chunk, neither do they) and those that ask for at most as much (`down`: where I fit, so do they) — myself in both
        unsigned long long up = 0, down = 0;
        for (uint32_t y = 0; y < n_shapes; ++y) {
            const int32_t y0 = read_lane(sv0, (int)y), y1 = read_lane(sv1, (int)y), y2 = read_lane(sv2, (int)y);
            const bool same = read_lane(stag, (int)y) == stag;
            if (same && y0 >= sv0 && y1 >= sv1 && y2 >= sv2) up |= 1ull << y;
            if (same && y0 <= sv0 && y1 <= sv1 && y2 <= sv2) down |= 1ull << y;
        }
        const uint64_t maximal = __ballot((uint32_t)lane < n_shapes && up == (1ull << lane));  // nobody asks for more than these
        if (wave == 0) sdom[lane] = up;  // (0 for the lanes beyond the last shape)
        // The verdict for ALL shapes from the chunk's maxima over the candidates of a role, lane = shape: a shape that asks for
        // more than the maximum in some dimension fits nowhere in the chunk, and when ONE candidate slot holds all three maxima (an
        // untouched stretch of equal nodes, the rule on a large table) every other shape fits that slot — exact without a look at
        // a single shape.  Only a chunk of unequal crumbs asks the shapes that passed the maxima one by one (the loop over the
        // shape table that used to run for every chunk and shape: 22 instructions of dependent vector -> scalar hand-overs each,
        // 148 k cycles of a 10 000-node prologue and 1.4 M of a 100 000-node one: profiles/r5w_resume_fixed_cost_after.txt).
        auto index_chunk = [&](uint32_t c, int32_t a0, int32_t a1, int32_t a2) {
            const uint64_t cxm = uniform64(lxm[c]), cdm = uniform64(ldm[c]);
            struct RoleMax {
                int32_t m0, m1, m2;
                bool one_slot;  // some candidate slot holds all three maxima
            };
            auto maxima = [&](uint64_t cand) {
                const bool in = lane_bit(cand);
                RoleMax r;
                r.m0 = wave_max_i32(in ? a0 : INT32_MIN);
                r.m1 = wave_max_i32(in ? a1 : INT32_MIN);
                r.m2 = wave_max_i32(in ? a2 : INT32_MIN);
                r.one_slot = (fit_mask(a0, a1, a2, r.m0, r.m1, r.m2, cand) != 0ull);
                return r;
            };
            const RoleMax mx = maxima(cxm);
            const RoleMax md = cdm == cxm ? mx : maxima(cdm);
            const bool drv = stag != 0u;
            const int32_t r0 = drv ? md.m0 : mx.m0, r1 = drv ? md.m1 : mx.m1, r2 = drv ? md.m2 : mx.m2;
            // (shape lanes beyond n_shapes hold INT32_MAX requests: they never pass)
            const uint64_t pass = (uint64_t)(__builtin_amdgcn_sicmp(r0, sv0, 39) & __builtin_amdgcn_sicmp(r1, sv1, 39) &
                                             __builtin_amdgcn_sicmp(r2, sv2, 39)) & all_shapes;
            const uint64_t exact = (mx.one_slot ? ~driver_shapes : 0ull) | (md.one_slot ? driver_shapes : 0ull);
            uint64_t hit = pass & exact;
            uint64_t ask = pass & ~exact;  // passed the maxima, but no single slot vouches for them
            // ... they are asked one by one, the largest requests first: a shape that fits answers for everything it dominates, one
            // that does not for everything that dominates it — a handful of tests per chunk instead of one per shape
            uint64_t first = ask & maximal;
            while (ask) {
                const uint64_t from = first ? first : ask;
                const uint32_t sp = (uint32_t)__ffsll((unsigned long long)from) - 1u;
                first &= ~(1ull << sp);
                const int32_t v0 = read_lane(sv0, (int)sp), v1 = read_lane(sv1, (int)sp), v2 = read_lane(sv2, (int)sp);
                const uint64_t cand = ((driver_shapes >> sp) & 1ull) ? cdm : cxm;
                if (fit_mask(a0, a1, a2, v0, v1, v2, cand) != 0) {
                    const uint64_t d = read_lane64(down, sp);
                    hit |= d;
                    ask &= ~d;
                } else {
                    ask &= ~read_lane64(up, sp);
                }
                first &= ask;
            }
            if (lane_bit(hit)) atomicOr((unsigned long long*)&sbits[(size_t)lane * nwp + (c >> 6)], 1ull << (c & 63u));
        };
        for (uint32_t c = (uint32_t)wave; c < nc; c += 2 * NW) {
            int32_t a0, a1, a2, b0, b1, b2;
            values_of(c, a0, a1, a2);
            values_of(c + NW, b0, b1, b2);
            index_chunk(c, a0, a1, a2);
            if (c + NW < nc) index_chunk(c + NW, b0, b1, b2);
        }
    }
    __threadfence_block();
    __syncthreads();
    {
        const uint32_t n0 = n_apps < (uint32_t)kFusedStage ? n_apps : (uint32_t)kFusedStage;
        const u32x4* src = reinterpret_cast<const u32x4*>(napps);
        for (uint32_t i = tid; i < n0 * 4u; i += BLOCK) stage4[i] = src[i];
    }
    __syncthreads();

    if (wave == 0) {
        // ------------------------------------------------------------------------------------------ the chain
        NarrowBlockView V{lblk, lds_slots, (glb_i32*)NT.cpu, (glb_i32*)NT.mem, (glb_i32*)NT.gpu,
                          lmax, lmax + nc, lmax + 2 * (size_t)nc, lxm, ldm, nc, RESIDENT ? (lds_u64*)nullptr : fresh};
        Orders O{T.slot_node, T.dslot, T.n_x, T.n_d, true};
        glb_i32* gcpu = (glb_i32*)NT.cpu;
        glb_i32* gmem = (glb_i32*)NT.mem;
        glb_i32* ggpu = (glb_i32*)NT.gpu;
        const uint32_t n_slots = T.n_slots;
        const uint64_t lt_mask = (1ull << lane) - 1ull;
        unsigned long long xvis = 0, dvis = 0;
        unsigned long long ph[6] = {0, 0, 0, 0, 0, 0};
        unsigned long long rare_n[5] = {0, 0, 0, 0, 0}, rare_cyc[5] = {0, 0, 0, 0, 0};  // (instrumented variant only)
        constexpr bool prof = PROF;
        unsigned long long tp = prof ? __builtin_readcyclecounter() : 0;
        const unsigned long long t_chain_begin = tp;
        // chunk c (wave-uniform): lane l <-> slot 64 c + l; xm / dm = the chunk's candidate masks (uniform values)
        // MOFF: dword offset of the candidate mask the visit needs inside the block (192 executor candidates, 194 driver
        // candidates); gmask: the same masks per chunk for the table's global tail
#define GF_SOLO_LOAD(c, a0, a1, a2, mk, MOFF, gmask)                             \
    {                                                                            \
        if (RESIDENT || (c) < lds_chunks) {                                      \
            const lds_i32* p_ = lblk + (size_t)(c) * kBlkDwords;                 \
            a0 = p_[lane];                                                       \
            a1 = p_[64 + lane];                                                  \
            a2 = p_[128 + lane];                                                 \
            unsigned long long mk_ = *reinterpret_cast<const lds_u64*>(p_ + (MOFF)); \
            GF_HERE(a0);                                                         \
            GF_HERE(a1);                                                         \
            GF_HERE(a2);                                                         \
            GF_HERE(mk_);                                                        \
            mk = uniform64(mk_);                                                 \
        } else {                                                                 \
            const SoloTriple t_ = solo_tail_load(gcpu, gmem, ggpu, (c) * kWave + (uint32_t)lane, n_slots); \
            a0 = t_.v0;                                                          \
            a1 = t_.v1;                                                          \
            a2 = t_.v2;                                                          \
            mk = uniform64(gmask[c]);                                            \
        }                                                                        \
    }
#define GF_SOLO_STORE(c, a0, a1, a2)                                             \
    {                                                                            \
        if (RESIDENT || (c) < lds_chunks) {                                      \
            lds_i32* p_ = lblk + (size_t)(c) * kBlkDwords;                       \
            p_[lane] = a0;                                                       \
            p_[64 + lane] = a1;                                                  \
            p_[128 + lane] = a2;                                                 \
        } else {                                                                 \
            solo_tail_store(gcpu, gmem, ggpu, (c) * kWave + (uint32_t)lane, a0, a1, a2); \
        }                                                                        \
    }
        int32_t failed_at = -1;
        uint32_t a = 0;
        // Lane = shape id (kMaxShapes = 64 = the wavefront): word 0 of every shape's index row — the first 4 096 slots, where a
        // tightly packed front lives —, its dominator mask and its capacity bound live in REGISTERS for the whole chain.  What an
        // application needs from its two shapes is nine v_readlane with a scalar lane select instead of an LDS round trip behind
        // two multiply-add address computations, and clearing a bit for a whole family of shapes is one masked vector AND
        // instead of a lane-parallel LDS atomic.  Later words of the rows stay in LDS (a scan rarely gets there).  The LDS copy
        // of word 0 is only brought up to date around the rare endings that set bits or learn a bound (solo_rare_app).
        static_assert(kMaxShapes == (uint32_t)kWave, "lane = shape id");
        unsigned long long row0 = sbits[(size_t)lane * nwp];
        const unsigned long long dom_l = sdom[lane];
        int32_t bound_l = sbound[lane];
        // clear bit b of word g (both wave-uniform) in the rows of the shapes named by the wave-uniform mask `family`
        auto clear_family = [&](unsigned long long family, uint32_t g, uint32_t b) {
            if (GF_OFTEN(g == 0)) {
                if (lane_bit(family)) row0 &= ~(1ull << b);
            } else if (lane_bit(family)) {
                atomicAnd((unsigned long long*)&sbits[(size_t)lane * nwp + g], ~(1ull << b));
            }
        };
        // Stores count in vmcnt on gfx9-family ISAs and complete after ~2 us.  Whenever the compiler believes that some VMEM
        // operation issued before the loop (the spilled view structs of the slow path) or behind the call may still own a
        // VGPR, it guards the next write of that VGPR with s_waitcnt vmcnt(N) — which throttles the chain to N placement /
        // result stores in flight (measured: vmcnt(8) => 600 cycles per store).  An explicit drain at these two rare
        // places leaves it nothing to guard inside the loop.
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        for (; a < n_apps; ++a) {
            // ---- app staging: 64 records in LDS, two halves of 32.  Every 32 apps the half that held apps [a-32, a) is
            //      refilled with apps [a+32, a+64), synchronously: a load kept in flight across iterations would put a
            //      vmcnt(0) wait (= a wait for every placement store) at the head of every iteration.
            if (GF_RARE((a & 31u) == 0 && a != 0)) {
                // ---- checkpoint: the table as it is BEFORE application a (absolute index a + a_base), dumped by the helper
                //      wavefronts between two LDS-only barriers while this one refills the staging buffer.  The interval is
                //      a multiple of 32, so a checkpoint always coincides with a refill.
                const bool do_ck = ck.base != nullptr && ((a + ck.a_base) & ((1u << ck.shift) - 1u)) == 0;
                if (do_ck) {
                    if (!RESIDENT) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wavefront's stores to the global tail
                    if (lane == 0) sh->ckpt_cmd = ((a + ck.a_base) >> ck.shift) - 1u;
                    lds_barrier();
                }
                const uint64_t base4 = (uint64_t)(a + 32u) * 4u, lim4 = (uint64_t)n_apps * 4u;
                const u32x4* src = reinterpret_cast<const u32x4*>(napps) + base4;
                lds_u4* dst = stage4 + (size_t)((a + 32u) & 63u) * 4;
                if (base4 + (uint32_t)lane < lim4) dst[lane] = src[lane];
                if (base4 + 64u + (uint32_t)lane < lim4) dst[64 + lane] = src[64 + lane];
                if (do_ck) {
                    lds_barrier();  // the dump has read the table and both masks: the chain may change them again
                    if (!RESIDENT)
                        for (uint32_t i = (uint32_t)lane; i < nw; i += kWave) {
                            dirty[i] |= fresh[i];
                            fresh[i] = 0ull;
                        }
                }
            }
            // (Round 4 measured the record and the shape rows in ONE LDS round trip — shape ids read one application ahead, ten
            //  reads issued as one block —: no faster, the extra scalar address arithmetic and two more spilled scalars cost the
            //  ~130 cycles the second round trip takes.  The chain is bound by the instructions it issues, not by LDS latency.)
            const lds_u4* rec = stage4 + (size_t)(a & 63u) * 4;
            const u32x4 w0 = rec[0], w1 = rec[1], w2 = rec[2], w3 = rec[3];
            const NAppR app = napp_from_words_mixed(w0, w1, w2, w3);
            const int32_t K = app.k;
            const bool last = (a + 1 == n_apps);
            uint32_t* out = exec_nodes + app.exec_off;
            // What the rare endings take over from the common path (solo_rare_app): the first driver candidate, what the lazy scan
            // placed behind it and the optimistic commits it would have to take back.
            uint32_t p0 = kNoPos;
            int32_t taken = 0;
            uint32_t nhit = 0;
            bool hosts = false;    // an executor sits on the driver's slot
            bool pc_done = false;  // the driver's chunk has been committed
            unsigned long long domx = 0, domd = 0;
            // ---- the common path of one application, straight down; every rare ending leaves through a return code
            const int code = [&]() -> int {
                if (GF_RARE(app.shape_x == kNoShape || app.shape_d == kNoShape)) return kRareUnindexed;  // more than kMaxShapes shapes in the batch
                // per-application operands of ncap3_fit, as lane values (the record's words are in vector registers anyway)
                const uint32_t sh0 = w2.w & 0xFFu, sh1 = (w2.w >> 8) & 0xFFu, sh2 = w2.w >> 16;
                const uint32_t un0 = (uint32_t)((int32_t)(w1.w << (31 - kNAppZeroShift)) >> 31),
                               un1 = (uint32_t)((int32_t)(w1.w << (30 - kNAppZeroShift)) >> 31),
                               un2 = (uint32_t)((int32_t)(w1.w << (29 - kNAppZeroShift)) >> 31);
                uint32_t* heads = scratch + app.exec_off;  // tightly-pack: run heads; pre-set to kHeadEmpty by the launcher
                uint32_t* dummy_word = scratch + (scratch_half - 1);  // the spare word behind the first half (half = placements + 1)
                // ---- everything the app needs from its two shapes, in one LDS round trip: word 0 of each index row (the first
                //      4 096 slots, where a tightly packed front lives; a later word is read from LDS if a scan ever gets there — a
                //      four-word register cache selected by an if-cascade cost a dozen instructions and three taken branches per
                //      scan), the executor shape's capacity bound and the two dominator masks.  Reading the executor row before the
                //      driver search is exact: the driver search only clears bits of the DRIVER shape's row.
                const lds_u64* rowd = sbits + (size_t)app.shape_d * nwp;  // (words 1.. of the two rows)
                const lds_u64* rowx = sbits + (size_t)app.shape_x * nwp;
                const uint64_t wd0 = read_lane64(row0, app.shape_d), wx0 = read_lane64(row0, app.shape_x);
                const int32_t bound_v = read_lane(bound_l, (int)app.shape_x);
                domx = read_lane64(dom_l, app.shape_x);
                domd = read_lane64(dom_l, app.shape_d);
                GF_TICK(prof, ph, tp, 0)

                // ---- bound test: the executor shape's total capacity is known to be below K (the bound starts at INT32_MAX)
                if (GF_RARE(K > bound_v)) return kRareBound;
                // ---- driver search (binpack.go:67-71): first candidate slot that passes the driver-fit check
                {
                    uint32_t g = 0;
                    uint64_t w = wd0;
                    if (prof) dvis += kWave;
                    for (;;) {
                        if (GF_RARE(w == 0)) {  // this word of the row is exhausted: the next one, from LDS
                            if (++g >= nw) return kRareNoDriver;
                            w = uniform64(rowd[g]);
                            if (prof) dvis += kWave;
                            continue;
                        }
                        const uint32_t b = (uint32_t)__ffsll((unsigned long long)w) - 1;
                        w &= w - 1;
                        const uint32_t c = g * kWave + b;
                        int32_t d0, d1, d2;
                        uint64_t ddm;
                        GF_SOLO_LOAD(c, d0, d1, d2, ddm, 194, ldm)
                        const uint64_t fm = fit_mask(d0, d1, d2, app.drv0, app.drv1, app.drv2, ddm);
                        if (prof) {
                            dvis += kWave;
                            ph[5] += 1;
                        }
                        if (GF_OFTEN(fm != 0)) {
                            p0 = c * kWave + (uint32_t)__ffsll((unsigned long long)fm) - 1;
                            break;
                        }
                        clear_family(domd, g, b);  // stale bit of the shape and of its dominators (bits only ever go 1 -> 0)
                    }
                }
                GF_TICK(prof, ph, tp, 1)
                const uint32_t pc = p0 >> 6;
                const int pl = (int)(p0 & 63u);
                // commit of one chunk from values in registers (sparkpods.go:139-146): hit lanes lose one executor request, the
                // driver's lane the driver request unless it hosts an executor; the new values are stored.
                // The shape index is maintained LAZILY: a chunk that a commit has just filled for one of the application's two
                // shapes keeps its bits until a scan of that shape (or of a shape it dominates) visits it and finds nothing — that
                // stale visit clears the whole family at once.  Re-testing both shapes on the new values right here (round 3) was
                // exact for successors from the same template, but it put twelve compares and a vector -> scalar -> branch
                // hand-over into EVERY commit to save a visit now and then: measured, the chain is 10 % faster without (tight
                // 1.55 -> 1.38 ms at 2.76 -> 3.18 chunk visits per application).
                auto commit_chunk = [&](uint32_t c, int32_t a0, int32_t a1, int32_t a2, uint64_t m) {
                    // (tables with a global tail: the chunk now differs from the snapshot — the checkpoints dump exactly these)
                    if (!RESIDENT && lane == 0) atomicOr((unsigned long long*)&fresh[c >> 6], 1ull << (c & 63u));
                    if (lane_bit(m)) {
                        a0 -= app.exe0;
                        a1 -= app.exe1;
                        a2 -= app.exe2;
                    }
                    uint64_t sm = m;  // lanes whose values change
                    if (GF_RARE(c == pc)) {  // wave-uniform: only the driver's chunk pays for the driver's lane
                        if (!hosts) {
                            if (lane == pl) {
                                a0 -= app.drv0;
                                a1 -= app.drv1;
                                a2 -= app.drv2;
                            }
                            sm |= 1ull << pl;
                        }
                        pc_done = true;
                    }
                    // (a chunk in LDS is stored back whole — unchanged lanes rewrite what they read, nobody else writes the table
                    //  during the chain —: no execution mask to set and restore)
                    if (RESIDENT || c < lds_chunks) {
                        GF_SOLO_STORE(c, a0, a1, a2)
                    } else if (lane_bit(sm)) {
                        GF_SOLO_STORE(c, a0, a1, a2)
                    }
                    if (!RESIDENT && c >= lds_chunks) {
                        // Tables with a global tail keep the EAGER index: a stale visit out there is a real call and two dependent
                        // memory round trips (cold after a snapshot rebuild), not one LDS read — the first chain on a just-installed
                        // 100 000-node snapshot was 0.23 ms slower with the lazy index although the warm one was faster.  The LDS
                        // front stays lazy like a resident table (re-testing behind every commit, rounds 4-5a: 2.33 against 2.08 ms
                        // per config-5 chain, profiles/r5ac_c5_eager_tail.txt).
                        const uint64_t cxm = uniform64(lxm[c]), cdm = uniform64(ldm[c]);
                        const uint64_t bx = fit_mask(a0, a1, a2, app.exe0, app.exe1, app.exe2, cxm);
                        const uint64_t bd = fit_mask(a0, a1, a2, app.drv0, app.drv1, app.drv2, cdm);
                        if (GF_RARE(bx == 0 || bd == 0)) {  // the chunk has just been filled for one of the two shapes (and its dominators)
                            const unsigned long long gone = (bx == 0 ? domx : 0ull) | (bd == 0 ? domd : 0ull);
                            clear_family(gone, c >> 6, c & 63u);
                        }
                    }
                };
                // ---- executors with the driver reserved on p0 (binpack.go:72-73), candidate chunks in order, lazy
                if (K > 0) {
                    uint32_t g = 0;
                    uint64_t w = wx0;
                    if (prof) xvis += kWave;
                    // (Round 4 measured requesting the NEXT candidate chunk of the row word while this one is worked on — 2.1 executor
                    //  visits per application —: 1.37 -> 1.52 ms.  The loop-carried registers and the extra uniform branch cost more
                    //  than the hidden round trip; LDS returns in order, so the visit's own waits also wait for the prefetch.)
                    for (;;) {
                        if (GF_RARE(w == 0)) {
                            if (++g >= nw) return kRareShort;
                            w = uniform64(rowx[g]);
                            if (prof) xvis += kWave;
                            continue;
                        }
                        const uint32_t b = (uint32_t)__ffsll((unsigned long long)w) - 1;
                        w &= w - 1;
                        const uint32_t c = g * kWave + b;
                        const uint32_t j = c * kWave + (uint32_t)lane;
                        int32_t a0, a1, a2;
                        uint64_t cxm;
                        GF_SOLO_LOAD(c, a0, a1, a2, cxm, 192, lxm)
                        if (prof) {
                            xvis += kWave;
                            ph[5] += 1;
                        }
                        // the shape bit speaks about the table itself (no driver reserved): a chunk without a fit is stale
                        uint64_t fxm = fit_mask(a0, a1, a2, app.exe0, app.exe1, app.exe2, cxm);
                        if (GF_RARE(fxm == 0)) {
                            clear_family(domx, g, b);
                            continue;
                        }
                        int32_t r0 = a0, r1 = a1, r2 = a2;  // ... with the driver reserved
                        if (GF_RARE(c == pc)) {             // wave-uniform: only the driver's chunk pays for the reservation
                            if (lane == pl) {
                                r0 -= app.drv0;
                                r1 -= app.drv1;
                                r2 -= app.drv2;
                            }
                            fxm = fit_mask(r0, r1, r2, app.exe0, app.exe1, app.exe2, cxm);
                        }
                        const bool fx = lane_bit(fxm);
                        uint64_t hm = 0;
                        if (ALGO == GF_ALGO_TIGHTLY_PACK) {
                            // (computed in every lane and selected: a conditional block costs a lone wavefront two execution-mask
                            //  hand-overs, the fourteen instructions cost the same with any mask)
                            int32_t cq = ncap3_fit(r0, r1, r2, app, sh0, sh1, sh2, un0, un1, un2);
                            GF_HERE(cq);
                            const int32_t c0 = fx ? cq : 0;
                            const int32_t incl = wave_inclusive_scan(c0);
                            const int32_t tot = read_lane(incl, kWave - 1);
                            const int32_t start = taken + incl - c0;
                            const int32_t room = K - start;
                            const int32_t t = room <= 0 ? 0 : (room < c0 ? room : c0);
                            // one run head per node (expand_translate_kernel fills the run); lanes without one store to a spare word
                            // instead of being masked out
                            *(t > 0 ? heads + start : dummy_word) = j;
                            hm = __builtin_amdgcn_sicmp(t, 0, 38);  // lanes with t > 0
                            taken += tot;
                        } else {
                            const int32_t pos = taken + (int32_t)__popcll((unsigned long long)(fxm & lt_mask));
                            *((fx && pos < K) ? out + pos : dummy_word) = j;
                            hm = fxm & __builtin_amdgcn_sicmp(pos, K, 40);  // fitting lanes whose position is below K
                            taken += (int32_t)__popcll((unsigned long long)fxm);
                        }
                        if (GF_RARE(c == pc)) hosts = (hm >> pl) & 1ull;
                        // OPTIMISTIC: every consumed chunk is committed while its values are in registers — nearly every gang
                        // that finds a driver fits behind it —, and the hit list (two LDS stores, never waited for) only serves
                        // the rollback of the rare one that does not (the chunk where K is reached needs no entry).  Committing
                        // from the list after the scan cost two dependent LDS round trips and a scalar hand-over per chunk.
                        const bool fin = taken >= K;
                        if (GF_OFTEN(hm != 0)) {
                            if (!last) commit_chunk(c, a0, a1, a2, hm);
                            if (!fin) {  // (every lane writes the same two words)
                                hchunk[nhit] = (int32_t)c;
                                hmask[nhit] = hm;
                                ++nhit;
                            }
                        }
                        if (fin) break;
                    }
                }
                GF_TICK(prof, ph, tp, 2)
                // ---- K == 0 or every executor placed by the lazy scan
                // (every lane stores the same sixteen bytes to the same address: one write, and no execution-mask save / restore
                //  around it — with `lane == 0` the store and its mask hand-overs cost the chain 5 %)
                gf_result r;
                r.has_capacity = 1;
                r.driver_node = p0;  // SLOT id; expand_translate_kernel maps it to the node index
                r.exec_len = (uint32_t)K;
                r.evaluated = (ALGO == GF_ALGO_TIGHTLY_PACK && K > 0) ? kEvalHeads : kEvalDone;
                results[a] = r;
                // ---- the driver sits in a chunk without executors (sparkpods.go:139-146: the driver request only if no executor
                //      landed on the driver's node); nothing is subtracted behind the driver being filtered (resource.go:321-328)
                if (!last && !pc_done) {
                    if (RESIDENT || pc < lds_chunks) {
                        // one LDS atomic per dimension, every lane on its own slot (all but the driver's add zero): nothing of the
                        // driver's chunk has to stay in registers across the executor scan, nothing is masked out
                        lds_i32* p_ = lblk + (size_t)pc * kBlkDwords + lane;
                        const bool me = lane == pl;
                        __hip_atomic_fetch_add(p_, me ? -app.drv0 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_add(p_ + 64, me ? -app.drv1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_add(p_ + 128, me ? -app.drv2 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (!RESIDENT && lane == 0) atomicOr((unsigned long long*)&fresh[pc >> 6], 1ull << (pc & 63u));
                    } else {  // (reload: nothing of the driver's chunk was kept across the executor scan)
                        int32_t e0, e1, e2;
                        uint64_t unused_mask;
                        GF_SOLO_LOAD(pc, e0, e1, e2, unused_mask, 194, ldm)
                        (void)unused_mask;
                        commit_chunk(pc, e0, e1, e2, 0ull);
                    }
                }
                GF_TICK(prof, ph, tp, 4)
                return kSoloOk;
            }();
            if (GF_RARE(code != kSoloOk)) {
                const bool touches = code == kRareShort || code == kRareUnindexed;  // sets index bits (rollback) / learns a bound
                if (touches) sbits[(size_t)lane * nwp] = row0;
                SoloRare R{V, O, napp_all_uniform(app), a, last, p0, taken, nhit, hosts, pc_done, domx, domd, sbits, nwp, hchunk, hmask,
                           sbound, out, scratch + app.exec_off, scratch + scratch_half + app.exec_off, results};
                // (a function's result is a lane value: without the readfirstlane the loop's exit — and with it the loop counter and
                //  everything derived from it — would count as divergent)
                const unsigned long long tr0 = prof ? __builtin_readcyclecounter() : 0;
                const bool goes_on = uniform32((uint32_t)solo_rare_app<ALGO, true>(R, code, &failed_at)) != 0u;
                if (prof) {
#pragma unroll
                    for (int q = 1; q < 5; ++q)
                        if (code == q) {
                            rare_n[q] += 1;
                            rare_cyc[q] += __builtin_readcyclecounter() - tr0;
                        }
                }
                if (touches) {
                    row0 = sbits[(size_t)lane * nwp];
                    bound_l = sbound[lane];
                }
                GF_TICK(prof, ph, tp, 3)
                if (!goes_on) {
                    ++a;
                    break;
                }
            }
        }
#undef GF_SOLO_LOAD
#undef GF_SOLO_STORE
        if (lane == 0) {
            sh->final_a = a;
            sh->failed_at = failed_at;
            sh->ckpt_cmd = kCkptDone;
            if (stats != nullptr) {
                atomicAdd(&stats->exec_slots_visited, xvis);
                atomicAdd(&stats->driver_slots_visited, dvis);
                for (int i = 0; i < 6; ++i) stats->fifo_phase_cycles[i] = ph[i];
                // (index 0 is no rare ending: the cycles from the kernel's start to the chain's first application = the prologue,
                //  and to the chain's end — what follows until fifo_shader_cycles is the epilogue)
                rare_cyc[0] = t_chain_begin - t0_cycles;
                rare_n[0] = __builtin_readcyclecounter() - t0_cycles;
                for (int i = 0; i < 5; ++i) {
                    stats->fifo_rare_count[i] = rare_n[i];
                    stats->fifo_rare_cycles[i] = rare_cyc[i];
                }
                // where the controlling wavefront ran: HW_REG_HW_ID (id 4) and HW_REG_XCC_ID (id 20), 32 bits each
                stats->fifo_hw_id = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                                    ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
            }
        }
        lds_barrier();  // releases the helpers
    } else {
        // ------------------------------------------------------------------------------- the helpers: checkpoint dumps
        // Asleep at the first barrier while wavefront 0 walks the chain; woken with a checkpoint slot (dump the table, meet
        // wavefront 0 at the second barrier) or with kCkptDone.  The table's global tail is read with plain loads: the
        // workgroup shares one L1, and wavefront 0 has drained its stores before the first barrier.
        const uint32_t n_slots = T.n_slots;
        for (;;) {
            lds_barrier();
            const uint32_t cmd = uniform32(sh->ckpt_cmd);
            if (cmd == kCkptDone) break;
            int32_t* dst = ck.base + (size_t)cmd * ck.stride;
            if (RESIDENT) {  // the whole table, from LDS
                for (uint32_t s = tid - kWave; s < n_slots; s += BLOCK - kWave) {
                    const lds_i32* p = lblk + (size_t)(s >> 6) * kBlkDwords + (s & 63u);
                    dst[s] = p[0];
                    dst[(size_t)n_slots + s] = p[64];
                    dst[2 * (size_t)n_slots + s] = p[128];
                }
            } else {
                // tables beyond the LDS front, DELTA format (chain_ckpt_stride): only the chunks a commit has touched since the
                // previous checkpoint are dumped — what the last 2^shift applications touched, not what the chain has touched
                // so far —, with the cumulative and the delta mask; a resumed chain starts from the snapshot with the latest
                // delta of every cumulative chunk laid over it (chain_prologue_kernel).  Loads first, stores behind them: a
                // wavefront's load cannot return before its earlier stores are acknowledged (~2 us, one in-order counter), so a
                // load - store - load - store loop over the chunks costs a store's latency per chunk.
                // The fresh chunks are dealt to the helpers by RANK (the r-th fresh chunk goes to helper r mod (NW - 1)): they sit
                // next to each other at the front of the order, and every helper walks the few mask words itself.  A helper
                // collects up to eight chunk ids in scalar registers (unrolled selects: a dynamically indexed array would live
                // in scratch memory), requests all their values, then stores them.
                constexpr int kBatch = 8;
                uint32_t ids[kBatch];
#pragma unroll
                for (int t = 0; t < kBatch; ++t) ids[t] = 0;
                int nb = 0;
                auto flush = [&]() {
                    int32_t v[kBatch][3];
#pragma unroll
                    for (int t = 0; t < kBatch; ++t) {
                        if (t < nb) {
                            const uint32_t ct = ids[t];
                            const uint32_t s = ct * kWave + (uint32_t)lane;
                            v[t][0] = v[t][1] = v[t][2] = 0;
                            if (ct < lds_chunks) {
                                const lds_i32* p = lblk + (size_t)ct * kBlkDwords + lane;
                                v[t][0] = p[0];
                                v[t][1] = p[64];
                                v[t][2] = p[128];
                            } else if (s < n_slots) {
                                v[t][0] = NT.cpu[s];
                                v[t][1] = NT.mem[s];
                                v[t][2] = NT.gpu[s];
                            }
                        }
                    }
#pragma unroll
                    for (int t = 0; t < kBatch; ++t) {
                        if (t < nb) {
                            const uint32_t s = ids[t] * kWave + (uint32_t)lane;
                            if (s < n_slots) {
                                dst[s] = v[t][0];
                                dst[(size_t)n_slots + s] = v[t][1];
                                dst[2 * (size_t)n_slots + s] = v[t][2];
                            }
                        }
                    }
                    nb = 0;
                };
                uint32_t rank = 0;
                for (uint32_t gi = 0; gi < nw; ++gi) {
                    unsigned long long wbits = uniform64(fresh[gi]);
                    while (wbits) {
                        const uint32_t bit = (uint32_t)__ffsll(wbits) - 1u;
                        wbits &= wbits - 1ull;
                        const bool mine = rank % (uint32_t)(NW - 1) == (uint32_t)wave - 1u;
                        ++rank;
                        if (!mine) continue;
                        const uint32_t cc = gi * 64u + bit;
#pragma unroll
                        for (int t = 0; t < kBatch; ++t)
                            if (nb == t) ids[t] = cc;
                        if (++nb == kBatch) flush();
                    }
                }
                if (nb > 0) flush();
                unsigned long long* mk = reinterpret_cast<unsigned long long*>(dst + 3 * (size_t)n_slots + (n_slots & 1u));
                for (uint32_t i = tid - kWave; i < nw; i += BLOCK - kWave) {
                    const unsigned long long f = fresh[i];
                    mk[i] = dirty[i] | f;  // cumulative: differs from the snapshot at this checkpoint
                    mk[nw + i] = f;        // delta: dumped here
                }
            }
            lds_barrier();
        }
    }
    __syncthreads();  // the helpers' dumps and wavefront 0's stores are done; everybody takes part in the epilogue
    // ---- epilogue, all wavefronts: apps behind an abort are reported as not evaluated; residuals back to the wide table
    const uint32_t a_end = sh->final_a;
    chain_mark_not_evaluated<BLOCK>(results, a_end, n_apps, tid);
    // four slots per thread and trip, every value requested before the first is stored: the tail of a table larger than the LDS
    // front comes from global memory, and a trip that waits for its own three loads made this loop ~0.3 ms at 100 000 nodes
    constexpr int kEpi = 4;
    for (uint32_t s0 = tid; s0 + 1 < T.n_slots; s0 += kEpi * BLOCK) {
        int32_t b[kEpi][3];
#pragma unroll
        for (int u = 0; u < kEpi; ++u) {
            const uint32_t s = s0 + (uint32_t)u * BLOCK;
            b[u][0] = b[u][1] = b[u][2] = 0;
            if (s + 1 < T.n_slots) {
                if (s < lds_slots) {
                    const lds_i32* p = lblk + (size_t)(s >> 6) * kBlkDwords + (s & 63u);
                    b[u][0] = p[0];
                    b[u][1] = p[64];
                    b[u][2] = p[128];
                } else {
                    b[u][0] = NT.cpu[s];
                    b[u][1] = NT.mem[s];
                    b[u][2] = NT.gpu[s];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kEpi; ++u) {
            const uint32_t s = s0 + (uint32_t)u * BLOCK;
            if (s + 1 < T.n_slots) {
                T.cpu[s] = (int64_t)b[u][0] * NT.unit[0];
                T.mem[s] = (int64_t)b[u][1] * NT.unit[1];
                T.gpu[s] = (int64_t)b[u][2] * NT.unit[2];
                if (RESIDENT && ck.tip != nullptr) {  // the tip: the table before the application the chain ended at (ChainCkpt)
                    ck.tip[s] = b[u][0];
                    ck.tip[(size_t)T.n_slots + s] = b[u][1];
                    ck.tip[2 * (size_t)T.n_slots + s] = b[u][2];
                }
            }
        }
    }
    if (RESIDENT && ck.tip != nullptr && tid == 0) {  // the sentinel slot, as the snapshot has it (the loop above leaves it out)
        const uint32_t s = T.n_slots - 1u;
        const lds_i32* p = lblk + (size_t)(s >> 6) * kBlkDwords + (s & 63u);
        ck.tip[s] = p[0];
        ck.tip[(size_t)T.n_slots + s] = p[64];
        ck.tip[2 * (size_t)T.n_slots + s] = p[128];
    }
    if (tid == 0) {
        if (chain_failed_at != nullptr) *chain_failed_at = sh->failed_at;
        if (stats != nullptr) {
            stats->fifo_shader_cycles = __builtin_readcyclecounter() - t0_cycles;
            stats->fifo_realtime_ticks = wall_clock64() - t0_real;
        }
    }
}
