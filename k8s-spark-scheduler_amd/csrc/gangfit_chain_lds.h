// gangfit_chain_lds.h — the dynamic-LDS layout of two single-workgroup FIFO chain kernels as pure functions: no HIP runtime header,
// the same code for the kernel that carves the allocation, for the host that sizes it (fifo_v2_lds_bytes, fifo_zoned_lds_bytes,
// from which gangfit_api_fit.cpp derives routes and lds_slots) and for a CPU test (tests/chain_lds_shim.cpp): WideChainLds
// (fit_fifo_chain_kernel) and ZonedLds (fit_fifo_zoned_lds_kernel).  Every field but `bytes` is the byte offset of one region: the
// kernel takes each region pointer as smem + L.field, the host launches with L.bytes.  Regions follow one another in the order of
// the layout function; one that wants more than the alignment its predecessor leaves starts at an align_up.  `reserve` is the
// unused tail: it keeps `bytes` where the closed formulas this header replaced had it.  The capacities and plain-data shared
// records those two layouts depend on are declared here too.  (fit_fifo_solo_kernel and fit_fifo_minfrag_lds_kernel still carve by
// hand next to a closed host formula: taken from a record they measured slower, profiles/r10a_chain_lds_summary.md.)
#pragma once
#include <cstddef>
#include <cstdint>

#include "gangfit.h"

#if defined(__HIPCC__)
#define GF_LDS_FN __host__ __device__ inline
#else
#define GF_LDS_FN inline
#endif

namespace gangfit {

constexpr int kAppStage = 32;              // wide chain: app records staged into LDS per refill
constexpr int kZStage = 32;                // zoned chain: app records (wide + narrow) staged per refill
constexpr uint32_t kMaxShapes = 64;        // distinct request shapes indexed per role
constexpr uint32_t kNoShape = 0xFFFFFFFFu;
constexpr uint32_t kZRunMax = 64;          // runs per candidate kept in LDS
constexpr size_t kNAppBytes = 64;     // sizeof(NApp) (gangfit_device.h), tied there by a static_assert at the kernels
constexpr size_t kWideAppBytes = 88;  // sizeof(App), the wide chain's record in registers and in FifoShared (gangfit_kernels.hip)
constexpr size_t kFifoSharedBytes = kAppStage * kWideAppBytes + 16;  // sizeof(FifoShared): the staged records + the slow path's verdict

// Workgroup-level exchange of one 32-bit value per wave through LDS.  Two alternating buffers: one barrier per
// exchange is enough (a wave can only be one exchange ahead of the slowest wave).  16 entries regardless of NW (entries
// >= NW hold the identity) so that lanes 0..15 of every wave can combine them with 4 DPP steps instead of a serial loop.
struct Exchange {
    uint32_t first[2][16];
    int32_t tot[2][16];
};

struct ZonedShared {
    // per candidate view, two copies indexed by the application's parity: with one barrier per application (see the
    // chain loop) a fast wavefront publishes application a + 1 while a slow one still reads the results of application a
    int32_t feas[2][16];
    uint32_t ds[2][16];
    uint32_t nruns[2][16];
    double mx[2][16];   // avg.Max of the candidate's placement: the reassociated sum (see wave_runs_avg_max<.., false>) ...
    double me[2][16];   // ... and the bound of its distance from the reference's slice-order sum (+inf: not bounded)
    double mxe[2][16];  // the slice-order sums, published only when the bounds do not separate the candidates
    int32_t shape_x[kMaxShapes][3];  // executor request shapes seen so far (scaled)
    int32_t shape_d[kMaxShapes][3];
    uint32_t n_shape_x, n_shape_d;
    // Upper bound on the total executor capacity of a (candidate view, executor shape): set whenever a full scan came
    // out short (then every node's capacity was below K, so the clamped sum WAS the total); capacities only fall during
    // a chain, so a later gang of that shape with K above the bound is infeasible in that view without any scan.
    int32_t total_cap[17][kMaxShapes];  // always < K <= 2^20 when set; INT32_MAX = unknown
    // commits performed by the helper wavefront: a + 1 once application a's usage has been subtracted (the winner's
    // wavefront waits for it before its next scan; nobody else reads the slots of the winner's zone)
    uint32_t commit_done;
};

namespace chain_lds {

GF_LDS_FN size_t align_up(size_t off, size_t a) { return (off + a - 1) & ~(a - 1); }
GF_LDS_FN size_t index_words(uint32_t n_chunks) { return ((size_t)n_chunks + 63u) / 64u; }  // 64-bit words of one bit per chunk

// ---- fit_fifo_chain_kernel: the wide (int64) table front, any lds_slots
struct WideChainLds {
    size_t lcpu, lmem, lgpu;  // int64 [lds_slots] each
    size_t lmax;              // int64 [3][n_chunks] chunk maxima
    size_t lxm;               // u64 [2][n_chunks] candidate masks, executor then driver
    size_t exchange;          // Exchange
    size_t shared;            // FifoShared
    size_t dirty;             // u8 [n_chunks], rounded up to a multiple of 16 bytes
    size_t reserve, bytes;
};
GF_LDS_FN WideChainLds wide_chain_lds(uint32_t lds_slots, uint32_t n_chunks) {
    WideChainLds L;
    L.lcpu = 0;
    L.lmem = L.lcpu + 8 * (size_t)lds_slots;
    L.lgpu = L.lmem + 8 * (size_t)lds_slots;
    L.lmax = L.lgpu + 8 * (size_t)lds_slots;
    L.lxm = L.lmax + 24 * (size_t)n_chunks;
    L.exchange = L.lxm + 16 * (size_t)n_chunks;
    L.shared = L.exchange + sizeof(Exchange);
    L.dirty = L.shared + kFifoSharedBytes;
    L.reserve = L.dirty + align_up(n_chunks, 16);
    L.bytes = L.reserve + 64;
    return L;
}

// ---- fit_fifo_zoned_lds_kernel: n_views = zones + 1 (the plain view), n_waves = wavefronts of the workgroup (one run-list pair each)
struct ZonedLds {
    size_t stage;    // gf_app [kZStage]
    size_t nstage;   // NApp [kZStage]
    size_t shared;   // ZonedShared
    size_t lmasks;   // u64 [n_views][2][n_chunks]: executor then driver candidates of each view, the plain view last
    size_t lcm;      // i32 [3][n_chunks] chunk maxima
    size_t lruns;    // i32 [n_waves][2 = application parity][2][kZRunMax] run lists (slots, counts)
    size_t sbx;      // u64 [n_views][n_shapes][index_words] executor-shape index
    size_t sbd;      // ... driver-shape index
    size_t ltab;     // i32 [3][lds_slots] table front
    size_t spare_words;  // i32 [2]: where the lanes without a run store (RunList::l_dummy); shared by all views, nobody reads them
    size_t reserve, bytes;
};
GF_LDS_FN ZonedLds zoned_lds(uint32_t lds_slots, uint32_t n_chunks, uint32_t n_views, uint32_t n_waves, uint32_t n_shapes) {
    const size_t rows = 8 * (size_t)n_views * n_shapes * index_words(n_chunks);
    ZonedLds L;
    L.stage = 0;
    L.nstage = L.stage + (size_t)kZStage * sizeof(gf_app);
    L.shared = L.nstage + (size_t)kZStage * kNAppBytes;
    L.lmasks = L.shared + align_up(sizeof(ZonedShared), 16);
    L.lcm = L.lmasks + 16 * (size_t)n_chunks * n_views;
    L.lruns = L.lcm + 12 * (size_t)n_chunks;
    const size_t packed = L.lruns + 2 * 8 * (size_t)kZRunMax * n_waves + 2 * rows;  // the end of sbd without any pad
    L.sbx = align_up(packed - 2 * rows, 8);  // 64-bit words: an odd n_chunks leaves the end of the run lists at 4 mod 8
    L.sbd = L.sbx + rows;
    L.ltab = align_up(L.sbd + rows, 16);
    L.spare_words = L.ltab + 12 * (size_t)lds_slots;
    L.reserve = L.spare_words + 8;
    // Every size above is a multiple of 4, so the two pads together (L.ltab - packed) are 0, 4, 8 or 12 bytes: the 64 spare bytes
    // of the closed formula this replaced pay for them and for spare_words, and `bytes` stays that formula's.
    L.bytes = packed + 12 * (size_t)lds_slots + 64;
    return L;
}

}  // namespace chain_lds
}  // namespace gangfit

#undef GF_LDS_FN
