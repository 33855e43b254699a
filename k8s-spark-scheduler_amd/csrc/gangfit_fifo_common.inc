// gangfit_fifo_common.inc — what the LDS-resident FIFO-chain kernels share (gangfit_fifo_solo.inc, gangfit_fifo_zoned.inc,
// gangfit_fifo_minfrag.inc): the narrow (scaled int32) domain, the per-launch app preparation, the request-shape dedup and
// the expansion of run heads.  Included by gangfit_kernels.hip inside its anonymous namespace.
//
// Narrow domain.  The chain is a single workgroup whose speed is the number of instructions on one instruction stream.
// Canonical quantities are int64 (memory in bytes), which gfx950 emulates with 2-4 instructions per compare / subtract and
// ~30 per exact division.  In practice every quantity of a snapshot is a multiple of a per-dimension unit (KiB-granular
// allocatable memory, milli-cores, whole gpus): gf_orders_set computes unit[j] = gcd of the table's dimension j and stores
// value / unit as int32 when every magnitude stays below 2^30.  the chain prologue (prepare_app) checks that each request of the batch
// is a multiple of the units (else the launch falls back to the wide kernel — same results, only slower).  Scaling by a
// common unit preserves every comparison, subtraction and floor division of the reference exactly
// (floor((a u) / (e u)) == floor(a / e)), so results stay bit-identical.

constexpr int kFusedStage = 64;  // app records resident in LDS (two halves of 32)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4 lds_u4;

// (narrow_shift / narrow_magic — floor(a / e) for 0 <= a < 2^30 as a multiplication — live in gangfit_kernels.hip, ahead of
//  gangfit_minfrag.inc, which uses them for the independent batch too)

// gf_app -> NApp (requests divided by the table's units + the multipliers of narrow_magic).  A request that is not a multiple of its unit,
// or whose scaled value does not fit below 2^30, raises *wide_needed: the narrow chain kernel then returns at once and the
// wide one runs.
__device__ __forceinline__ void prepare_app(const gf_app& in, NApp* __restrict__ out, const int64_t (&unit)[3],
                                            int32_t* __restrict__ wide_needed) {
    NApp n;
    bool ok = in.k >= 0 && in.k <= GF_MAX_K;
    for (int j = 0; j < 3; ++j) {
        const int64_t d = in.drv[j] / unit[j], e = in.exe[j] / unit[j];
        ok = ok && d * unit[j] == in.drv[j] && e * unit[j] == in.exe[j] && d >= 0 && e >= 0 && d < (INT64_C(1) << 30) &&
             e < (INT64_C(1) << 30);
        n.drv[j] = (int32_t)d;
        n.exe[j] = (int32_t)e;
    }
    uint32_t sh0 = 0, sh1 = 0, sh2 = 0;
    narrow_magic(ok ? n.exe[0] : 0, n.mag[0], sh0);
    narrow_magic(ok ? n.exe[1] : 0, n.mag[1], sh1);
    narrow_magic(ok ? n.exe[2] : 0, n.mag[2], sh2);
    n.msh = sh0 | (sh1 << 8) | (sh2 << 16);
    n.k = in.k;
    // bits 8..10 (internal; gangfit_fifo_solo.inc): executor request dimension j is zero
    n.flags = (in.flags & 0xFFu) | (n.exe[0] == 0 ? 0x100u : 0u) | (n.exe[1] == 0 ? 0x200u : 0u) | (n.exe[2] == 0 ? 0x400u : 0u);
    n.exec_off = in.exec_off;
    n.pad = ~0ull;  // {shape_x, shape_d}: assigned by the chain kernel's dedup
    *out = n;
    if (!ok) atomicOr(wide_needed, 1);
}

// The first kernel of every chain (ChainIo, gangfit_device.h): app records in (from pinned host memory or the device) ->
// device copy + scaled records; table copies; the dirty chunks of a checkpoint laid over the first copy; the run-head
// preset.  Grid-stride over each range with the SAME thread-to-word mapping for the copy and the overlay, so the overlay of a
// word is program-ordered behind its copy.
struct ChainPrologue {
    uint32_t n_apps;
    const gf_app* apps_src;  // nullptr: apps_dst holds the records already
    gf_app* apps_dst;
    NApp* napps;  // nullable: no scaled form wanted
    int64_t unit[3];
    int32_t* wide_needed;
    int32_t* wide_clear;
    const uint32_t* copy_src[2];
    uint32_t* copy_dst[2];
    size_t copy_words[2];
    const int32_t* overlay;  // checkpoint 1 of a series in the delta format; checkpoints 1 .. overlay_count are laid over the table
    size_t overlay_stride;
    uint32_t overlay_count;
    int32_t* overlay_dst;
    uint32_t overlay_slots, overlay_chunks;
    uint32_t* fill_dst;  // preset to kHeadEmpty (all ones)
    size_t fill_words;
};

__global__ __launch_bounds__(256) void chain_prologue_kernel(ChainPrologue p) {
    const size_t stride = (size_t)gridDim.x * 256u;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t == 0 && p.wide_clear != nullptr) *p.wide_clear = 0;
    for (size_t a = t; a < p.n_apps; a += stride) {
        gf_app in;
        if (p.apps_src != nullptr) {
            in = p.apps_src[a];
            p.apps_dst[a] = in;
        } else {
            in = p.apps_dst[a];
        }
        if (p.napps != nullptr) prepare_app(in, p.napps + a, p.unit, p.wide_needed);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        // tables are 16-byte aligned multiples of four words; anything else takes the word loop
        const bool vec = ((p.copy_words[r] & 3u) | ((uintptr_t)p.copy_src[r] & 15u) | ((uintptr_t)p.copy_dst[r] & 15u)) == 0;
        if (vec) {
            const uint4* src = reinterpret_cast<const uint4*>(p.copy_src[r]);
            uint4* dst = reinterpret_cast<uint4*>(p.copy_dst[r]);
            for (size_t i = t; i < p.copy_words[r] / 4; i += stride) dst[i] = src[i];
        } else {
            for (size_t i = t; i < p.copy_words[r]; i += stride) p.copy_dst[r][i] = p.copy_src[r][i];
        }
    }
    if (p.overlay != nullptr && p.overlay_count > 0) {
        // delta format (chain_ckpt_stride): a chunk named by the cumulative mask of checkpoint `overlay_count` comes from the
        // latest checkpoint at or before it whose delta mask names the chunk
        const size_t n = p.overlay_slots;
        const size_t mask_off = 3 * n + (n & 1u);                       // int32 words to the cumulative mask
        const size_t nwm = ((size_t)p.overlay_chunks + 63u) / 64u;      // 64-bit words per mask
        auto cum_of = [&](uint32_t j) {
            return reinterpret_cast<const unsigned long long*>(p.overlay + (size_t)(j - 1u) * p.overlay_stride + mask_off);
        };
        const unsigned long long* cum = cum_of(p.overlay_count);
        // The source of the chunks a wavefront's words belong to (nullptr: the chunk is the snapshot's), resolved by the WAVEFRONT:
        // for every distinct chunk among its lanes (a handful: sixteen consecutive vectors share one), lane l looks at the delta
        // mask of checkpoint `count - l` — one round trip per 64 checkpoints — and the latest one that names the chunk wins.  (Every
        // lane walking the checkpoints back by itself was one dependent load per step: up to `count` of them — 31 for a
        // 1 000-application queue, 127 for a 4 096-application one — per vector, in the prologue of every resumed chain.)
        const uint32_t lane = threadIdx.x & 63u;
        auto wave_source = [&](bool valid, uint32_t c) -> const int32_t* {
            const bool named = valid && c < p.overlay_chunks && ((cum[c >> 6] >> (c & 63u)) & 1ull);
            const int32_t* mine = nullptr;
            unsigned long long todo = __ballot(named);
            while (todo) {
                const int leader = __ffsll(todo) - 1;
                const uint32_t cc = (uint32_t)__shfl((int)c, leader, 64);
                uint32_t found = 0;  // wave-uniform
                for (uint32_t hi = p.overlay_count; hi >= 1u && found == 0u; hi = hi > 64u ? hi - 64u : 0u) {
                    const uint32_t j = hi > lane ? hi - lane : 0u;
                    const bool bit = j >= 1u && ((cum_of(j)[nwm + (cc >> 6)] >> (cc & 63u)) & 1ull);
                    const unsigned long long m = __ballot(bit);
                    if (m) found = hi - (uint32_t)(__ffsll(m) - 1);
                }
                const bool same = named && c == cc;
                if (same && found != 0u) mine = p.overlay + (size_t)(found - 1u) * p.overlay_stride;  // (a cumulative bit is the OR of the deltas: always found)
                todo &= ~__ballot(same);
            }
            return mine;
        };
        const bool vec = ((p.copy_words[0] & 3u) | ((uintptr_t)p.copy_src[0] & 15u) | ((uintptr_t)p.copy_dst[0] & 15u) |
                          ((p.overlay_stride * sizeof(int32_t)) & 15u) | ((uintptr_t)p.overlay & 15u)) == 0;
        // walk the table exactly as copy 0 did (same thread per word) when copy 0 wrote this table; any mapping otherwise.
        // Whole wavefronts take every trip (a lane beyond the end is only a bystander of the lookups).
        const size_t wave_t = t - lane;
        if (p.copy_dst[0] == reinterpret_cast<uint32_t*>(p.overlay_dst) && p.copy_words[0] == 3 * n && vec) {
            const size_t limit = 3 * n / 4;
            for (size_t base = wave_t; base < limit; base += stride) {
                const size_t i = base + lane;
                const bool valid = i < limit;
                const size_t w = 4 * i;  // 3 n words in whole vectors => n is a multiple of four: the four words share a dimension and a chunk
                const int32_t* src = wave_source(valid, valid ? (uint32_t)((w % n) >> 6) : 0u);
                if (src != nullptr) reinterpret_cast<uint4*>(p.overlay_dst)[i] = reinterpret_cast<const uint4*>(src)[i];
            }
        } else {
            const size_t limit = 3 * n;
            for (size_t base = wave_t; base < limit; base += stride) {
                const size_t w = base + lane;
                const bool valid = w < limit;
                const int32_t* src = wave_source(valid, valid ? (uint32_t)((w % n) >> 6) : 0u);
                if (src != nullptr) p.overlay_dst[w] = src[w];
            }
        }
    }
    for (size_t i = t; i < p.fill_words; i += stride) p.fill_dst[i] = 0xFFFFFFFFu;
}

// The solo chain kernel as the chain's first kernel (fit_fifo_solo_kernel, RESIDENT tables, proven requests).
struct SoloFused {
    int enabled;
    const gf_app* apps_src;    // nullptr: apps_dst holds the records already
    gf_app* apps_dst;
    const int32_t* table_src;  // cpu | mem | gpu of the table the chain starts from (nullptr: NarrowTable's working copy)
    int64_t unit[3];
    uint32_t* fill_dst;        // run heads to preset
    size_t fill_words;
    int32_t* wide_clear;
};

// Host outputs of the last kernel of a chain (ChainIo): nullptr = none.
struct ChainOut {
    gf_result* h_results;
    uint32_t* h_exec;
    const int32_t* d_failed;
    int32_t* h_failed;
};

// min(floor(a / e), k) for one dimension in the narrow domain.  |a| < 2^30, 0 <= e < 2^30, 0 <= k <= 2^20; mag / sh from
// narrow_magic(e); a zero request takes any number of executors (e == 0: mag == 0 and the quotient is replaced by "unlimited").
__device__ __forceinline__ int32_t ncap_dim(int32_t a, int32_t e, uint32_t mag, uint32_t sh, int32_t k) {
    uint32_t q = __umulhi(mag, (uint32_t)a << 1) >> sh;
    q = (e == 0) ? 0xFFFFFFFFu : q;
    q = q < (uint32_t)k ? q : (uint32_t)k;
    return (a < 0) ? 0 : (int32_t)q;
}

struct NAppR {  // app record in registers
    int32_t drv0, drv1, drv2, k;
    int32_t exe0, exe1, exe2;
    uint32_t flags;
    uint32_t mag0, mag1, mag2, msh;  // narrow_magic of the executor request
    uint64_t exec_off;
    uint32_t shape_x, shape_d;  // shape ids of the executor / driver request, kNoShape = none
};

__device__ __forceinline__ int32_t ncap3(int32_t a0, int32_t a1, int32_t a2, const NAppR& p) {
    const int32_t c = ncap_dim(a0, p.exe0, p.mag0, p.msh & 0xFFu, p.k);
    const int32_t m = ncap_dim(a1, p.exe1, p.mag1, (p.msh >> 8) & 0xFFu, p.k);
    const int32_t g = ncap_dim(a2, p.exe2, p.mag2, p.msh >> 16, p.k);
    const int32_t cm = c < m ? c : m;
    return cm < g ? cm : g;
}

// The same for a slot that is known to FIT one executor (a_j >= exe_j >= 0 in every dimension: no negative operand), with
// the per-application operands prepared by the caller: sh_j = the post-shifts, un_j = 0xFFFFFFFF for a zero request
// dimension ("unlimited") and 0 otherwise.  Twelve vector instructions and two minima.
__device__ __forceinline__ int32_t ncap3_fit(int32_t a0, int32_t a1, int32_t a2, const NAppR& p, uint32_t sh0, uint32_t sh1,
                                             uint32_t sh2, uint32_t un0, uint32_t un1, uint32_t un2) {
    const uint32_t q0 = (__umulhi(p.mag0, (uint32_t)a0 << 1) >> sh0) | un0;
    const uint32_t q1 = (__umulhi(p.mag1, (uint32_t)a1 << 1) >> sh1) | un1;
    const uint32_t q2 = (__umulhi(p.mag2, (uint32_t)a2 << 1) >> sh2) | un2;
    uint32_t q = q0 < q1 ? q0 : q1;
    q = q < q2 ? q : q2;
    return (int32_t)(q < (uint32_t)p.k ? q : (uint32_t)p.k);
}

__device__ __forceinline__ NAppR read_staged_napp(const lds_u4* rec) {
    const u32x4 w0 = rec[0], w1 = rec[1], w2 = rec[2], w3 = rec[3];
    NAppR r;
    r.drv0 = (int32_t)w0.x;
    r.drv1 = (int32_t)w0.y;
    r.drv2 = (int32_t)w0.z;
    r.k = (int32_t)w0.w;
    r.exe0 = (int32_t)w1.x;
    r.exe1 = (int32_t)w1.y;
    r.exe2 = (int32_t)w1.z;
    r.flags = w1.w;
    r.mag0 = w2.x;
    r.mag1 = w2.y;
    r.mag2 = w2.z;
    r.msh = w2.w;
    r.exec_off = ((uint64_t)w3.y << 32) | w3.x;
    r.shape_x = w3.z;
    r.shape_d = w3.w;
    return r;
}

// The narrow table seen through the wide View interface: the (rare) slow paths reuse the generic wave-level code of the
// general-layout kernel on scaled values.
struct NarrowHybridView {
    lds_i32* lcpu;
    lds_i32* lmem;
    lds_i32* lgpu;
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
    bool resident = false;  // the WHOLE table sits in LDS (set from a template parameter of the kernel: every helper below is
                            // force-inlined, so the global-memory branch of a slot access — a per-lane branch with its
                            // execution-mask bookkeeping at every access — then compiles away)
    __device__ __forceinline__ bool chunk_may_hold(uint32_t c, int64_t r0, int64_t r1, int64_t r2) const {
        return (int64_t)cmax_cpu[c] >= r0 && (int64_t)cmax_mem[c] >= r1 && (int64_t)cmax_gpu[c] >= r2;
    }
    __device__ __forceinline__ uint64_t chunk_xmask(uint32_t c) const { return xm[c]; }
    __device__ __forceinline__ uint64_t chunk_dmask(uint32_t c) const { return dm[c]; }
    __device__ __forceinline__ bool xcand(uint32_t s) const { return (xm[s >> 6] >> (s & 63)) & 1ull; }
    __device__ __forceinline__ bool dcand(uint32_t s) const { return (dm[s >> 6] >> (s & 63)) & 1ull; }
    __device__ __forceinline__ void load32(uint32_t s, int32_t& a0, int32_t& a1, int32_t& a2) const {
        if (resident || s < lds_slots) {
            a0 = lcpu[s];
            a1 = lmem[s];
            a2 = lgpu[s];
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
        if (resident || s < lds_slots) {
            lcpu[s] -= r0;
            lmem[s] -= r1;
            lgpu[s] -= r2;
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

// Checkpoint of a chain (ChainCkpt, gangfit_device.h): the narrow working table as view V sees it (LDS front + global tail),
// dumped by every wavefront but the first of a workgroup of `block` work-items.  The caller brackets it with workgroup
// barriers: nothing commits while the dump reads.
template <class View>
__device__ __forceinline__ void chain_ckpt_dump(const View& V, uint32_t n_slots, int32_t* __restrict__ dst, uint32_t tid,
                                                uint32_t block) {
    const uint32_t step = block - kWave;
    for (uint32_t s0 = tid - kWave; s0 < n_slots; s0 += 4u * step) {  // four slots in flight per work-item
        int32_t b[4][3];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t s = s0 + (uint32_t)t * step;
            if (s < n_slots) V.load32(s, b[t][0], b[t][1], b[t][2]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t s = s0 + (uint32_t)t * step;
            if (s < n_slots) {
                dst[s] = b[t][0];
                dst[(size_t)n_slots + s] = b[t][1];
                dst[2 * (size_t)n_slots + s] = b[t][2];
            }
        }
    }
}
// The chain's TIP (ChainCkpt::tip), written in the epilogue of a chain kernel whose whole table sits in LDS, next to the wide
// residual table: slot s of the table the chain ended with — the table before the application it ended at.  Layout of a checkpoint.
__device__ __forceinline__ void chain_tip_store(const ChainCkpt& ck, uint32_t n_slots, uint32_t s, int32_t b0, int32_t b1, int32_t b2) {
    ck.tip[s] = b0;
    ck.tip[(size_t)n_slots + s] = b1;
    ck.tip[2 * (size_t)n_slots + s] = b2;
}
__device__ __forceinline__ bool chain_ckpt_due(const ChainCkpt& ck, uint32_t a) {
    return ck.base != nullptr && a != 0 && ((a + ck.a_base) & ((1u << ck.shift) - 1u)) == 0;
}
__device__ __forceinline__ int32_t* chain_ckpt_slot(const ChainCkpt& ck, uint32_t a, uint32_t n_slots) {
    (void)n_slots;
    return ck.base + (size_t)(((a + ck.a_base) >> ck.shift) - 1u) * ck.stride;
}

// Shape index.  Pending applications come from a handful of templates, so a batch holds few DISTINCT request vectors
// ("shapes": an executor request or a driver request, role included).  The kernel prologue dedups them into at most
// kMaxShapes ids and builds, per shape, one bit per 64-slot chunk: "some candidate slot of this chunk fits the shape".
// Unlike the per-dimension chunk maxima this is a JOINT test, so on a depleted table it does not flag chunks where one
// node has the cpu and another one the memory.  Bits only ever go 1 -> 0 (a chain only subtracts): the committing wave
// re-tests the app's own two shapes on the chunks it touched, and any wave that evaluates a flagged chunk and finds no
// fit clears the bit.  A stale 1 therefore costs one cheap chunk test, once; a 0 is always exact.  Apps whose shape did
// not get an id (more than kMaxShapes distinct shapes, hash-tag collision) use the chunk-maxima masks.
// (kMaxShapes and kNoShape: gangfit_chain_lds.h — the zoned chain's LDS layout depends on them)
constexpr uint32_t kShapeHashSlots = 128;

struct ShapeEntry {  // 16 bytes: hash-table entry during dedup
    int32_t v0, v1, v2;
    uint32_t tag;  // 0 = empty; else (hash & ~3) | role << 1 | 1
};

__device__ __forceinline__ uint32_t shape_tag(int32_t v0, int32_t v1, int32_t v2, uint32_t role) {
    uint32_t h = (uint32_t)v0 * 0x9E3779B1u;
    h = (h ^ (h >> 15)) + (uint32_t)v1 * 0x85EBCA77u;
    h = (h ^ (h >> 13)) + (uint32_t)v2 * 0xC2B2AE3Du;
    h ^= h >> 16;
    return (h & ~3u) | (role << 1) | 1u;
}

constexpr uint32_t kHeadEmpty = 0xFFFFFFFFu;  // run-head arrays are pre-set to this by the launcher

// gf_result.evaluated values while the chain kernels and the expansion kernel talk to each other
constexpr uint32_t kEvalDone = 1;   // placements (slot ids) are complete in exec_nodes
constexpr uint32_t kEvalHeads = 3;  // tightly-pack fast path: run heads in the scratch slice, to be expanded

// is the last head at or before i) and maps slot ids to the caller's node indices.  One wave per app.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void expand_translate_kernel(
    const uint32_t* __restrict__ slot_node, uint32_t n_apps, const gf_app* __restrict__ apps,
    gf_result* __restrict__ results, uint32_t* __restrict__ exec_nodes, const uint32_t* __restrict__ scratch, ChainOut o) {
    const int lane = lane_id();
    const uint32_t a = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (a >= n_apps) return;
    if (a == 0 && lane == 0 && o.h_failed != nullptr) *o.h_failed = *o.d_failed;
    const gf_result r = results[a];
    gf_result fin = r;
    if (r.evaluated) {
        fin.evaluated = kEvalDone;
        if (r.has_capacity) {
            const uint64_t off = apps[a].exec_off;
            uint32_t* out = exec_nodes + off;
            uint32_t* hout = o.h_exec != nullptr ? o.h_exec + off : nullptr;
            if (r.evaluated == kEvalHeads) {
                const uint32_t* heads = scratch + off;
                uint32_t carry = kHeadEmpty;  // slot of the run that is open at the chunk boundary
                for (uint32_t b = 0; b < r.exec_len; b += kWave) {
                    const uint32_t i = b + lane;
                    uint32_t h = kHeadEmpty;
                    if (i < r.exec_len) h = heads[i];
                    const uint64_t valid = __ballot(h != kHeadEmpty);
                    const uint64_t upto = valid & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));  // heads at lanes <= mine
                    const int src = upto ? 63 - __clzll((unsigned long long)upto) : lane;
                    const uint32_t v = (uint32_t)__shfl((int)h, src, kWave);
                    const uint32_t slot = upto ? v : carry;
                    if (i < r.exec_len) {
                        const uint32_t node = slot_node[slot];
                        out[i] = node;
                        if (hout != nullptr) hout[i] = node;
                    }
                    carry = (uint32_t)__shfl((int)slot, kWave - 1, kWave);
                }
            } else {
                for (uint32_t i = lane; i < r.exec_len; i += kWave) {
                    const uint32_t node = slot_node[out[i]];
                    out[i] = node;
                    if (hout != nullptr) hout[i] = node;
                }
            }
            fin.driver_node = slot_node[r.driver_node];
        }
        if (lane == 0) results[a] = fin;
    }
    if (lane == 0 && o.h_results != nullptr) o.h_results[a] = fin;
}
