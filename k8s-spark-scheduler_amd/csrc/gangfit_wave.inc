// gangfit_wave.inc — the wavefront idioms every kernel of gangfit_kernels.hip shares: lane reads, DPP moves and the reductions
// built on them, the LDS-only barrier, register pinning, branch hints, the phase clock (two macros) and the address-space pointer aliases.
// Included first by gangfit_kernels.hip, inside its anonymous namespace (kWave is defined there).  gf_selftest checks the scan
// and every reduction against a serial loop on the device.

// Pointers with explicit address spaces: with generic pointers the compiler folds an LDS arm and a global arm into ONE flat_load
// of a selected address, and every flat access waits on vmcnt(0) — i.e. on all placement stores still in flight.
typedef __attribute__((address_space(3))) int64_t lds_i64;
typedef __attribute__((address_space(3))) uint64_t lds_u64;
typedef __attribute__((address_space(3))) int32_t lds_i32;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) unsigned char lds_u8;
typedef __attribute__((address_space(3))) unsigned long long lds_ull;  // (what atomicAdd takes; uint64_t is unsigned long)
typedef __attribute__((address_space(1))) int64_t glb_i64;
typedef __attribute__((address_space(1))) int32_t glb_i32;

// A taken branch costs a lone wavefront ~30 cycles (tools/micro/probe_f64.hip: 47 cycles per trip of a loop around one
// 8-cycle add), a branch that falls through one issue slot: the rare bodies of the chain loops are laid out out of line.
#define GF_RARE(x) __builtin_expect(!!(x), 0)
#define GF_OFTEN(x) __builtin_expect(!!(x), 1)

// "This value is needed HERE": keeps the compiler from sinking a load below a branch that does not always use it (it would
// then pay one round trip per use instead of one for the whole group of loads issued together).  A macro: as a forceinline
// function taking a reference, the value's address escapes until the inliner has run, and the kernels that pin inside their
// scan loops came out with other instruction orders and register assignments.
#define GF_HERE(x) asm volatile("" : "+v"(x))

__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }
__device__ __forceinline__ uint64_t low_lanes(uint32_t n) { return n >= 64u ? ~0ull : ((1ull << n) - 1ull); }
__device__ __forceinline__ bool lane_in(uint64_t uniform_mask) { return __builtin_amdgcn_inverse_ballot_w64(uniform_mask); }

__device__ __forceinline__ int32_t read_lane(int32_t v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ uint32_t read_lane(uint32_t v, int src) {
    return (uint32_t)__builtin_amdgcn_readlane((int32_t)v, src);
}
__device__ __forceinline__ int64_t read_lane(int64_t v, int src) {
    uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)v, src);
    uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// The 64-bit value lane `src` holds (src wave-uniform): two v_readlane with a scalar lane select.
__device__ __forceinline__ uint64_t read_lane64(unsigned long long v, uint32_t src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)v, (int)src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)(v >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ double bcast_f64(double v, int src) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)u, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)(u >> 32), src);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
// A value every lane holds, as a scalar (tests on it are scalar compares, not a vector compare handed over to a branch).
__device__ __forceinline__ uint32_t uniform32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const uint32_t lo = uniform32((uint32_t)v), hi = uniform32((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for vmcnt(0): with placement stores in
// flight every barrier would stall for a global-memory round trip (measured: ~2 us per app in the FIFO chain).
// Data exchanged through this barrier must live in LDS.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ------------------------------------------------------------------------------------------------ DPP moves

// DPP control words (gfx9 family): row_shr:n = 0x110 + n, wave_shr:1 = 0x138, row_bcast:15 = 0x142, row_bcast:31 = 0x143.
constexpr int dpp_row_shr(int n) { return 0x110 + n; }
constexpr int kDppWaveShr1 = 0x138;
constexpr int kDppRowBcast15 = 0x142;
constexpr int kDppRowBcast31 = 0x143;

// The value of the lane CTRL names; a lane without a source (or outside ROW_MASK) receives `old`, or 0 with BOUND_CTRL.
// 64-bit values (int64_t, uint64_t, double: bit casts, never value conversions) move as two dwords under the same control word.
template <int CTRL, int ROW_MASK, bool BOUND_CTRL = false, class T>
__device__ __forceinline__ T dpp_mov(T old, T src) {
    if constexpr (sizeof(T) == 4) {
        return (T)__builtin_amdgcn_update_dpp((int32_t)old, (int32_t)src, CTRL, ROW_MASK, 0xf, BOUND_CTRL);
    } else {
        static_assert(sizeof(T) == 8, "a DPP move takes one or two dwords");
        const uint64_t o = __builtin_bit_cast(uint64_t, old), s = __builtin_bit_cast(uint64_t, src);
        const uint32_t lo = dpp_mov<CTRL, ROW_MASK, BOUND_CTRL>((uint32_t)o, (uint32_t)s);
        const uint32_t hi = dpp_mov<CTRL, ROW_MASK, BOUND_CTRL>((uint32_t)(o >> 32), (uint32_t)(s >> 32));
        return __builtin_bit_cast(T, ((uint64_t)hi << 32) | lo);
    }
}

// Inclusive prefix sum over the 64 lanes of a wave, 7 DPP adds, no LDS traffic.
__device__ __forceinline__ int32_t wave_inclusive_scan(int32_t v) {
    int32_t x = v;
    x += __builtin_amdgcn_update_dpp(0, v, dpp_row_shr(1), 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, v, dpp_row_shr(2), 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, v, dpp_row_shr(3), 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, dpp_row_shr(4), 0xf, 0xe, false);
    x += __builtin_amdgcn_update_dpp(0, x, dpp_row_shr(8), 0xf, 0xc, false);
    x += __builtin_amdgcn_update_dpp(0, x, kDppRowBcast15, 0xa, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, kDppRowBcast31, 0xc, 0xf, false);
    return x;
}

// ------------------------------------------------------------------------------------------------ reductions

// An operation = how two values combine and what a lane without a source receives (the DPP move's `old` operand).
struct OpMax {  // a lane without a source keeps its own value
    template <class T>
    static __device__ __forceinline__ T old(T v) { return v; }
    template <class T>
    static __device__ __forceinline__ T combine(T t, T v) { return t > v ? t : v; }
};
struct OpMaxF64 : OpMax {  // one v_max_f64 per step (no NaN among the operands)
    static __device__ __forceinline__ double combine(double t, double v) { return __builtin_fmax(t, v); }
};
struct OpSumF64 {
    static __device__ __forceinline__ double old(double) { return 0.0; }
    static __device__ __forceinline__ double combine(double t, double v) { return v + t; }
};
struct OpSumI64 {  // wrapping: two's-complement addition, whatever the order
    static __device__ __forceinline__ int64_t old(int64_t) { return 0; }
    static __device__ __forceinline__ int64_t combine(int64_t t, int64_t v) { return (int64_t)((uint64_t)v + (uint64_t)t); }
};
struct OpMinU32 {
    static __device__ __forceinline__ uint32_t old(uint32_t) { return 0xFFFFFFFFu; }
    static __device__ __forceinline__ uint32_t combine(uint32_t t, uint32_t v) { return t < v ? t : v; }
};

template <class Op, int CTRL, int ROW_MASK, class T>
__device__ __forceinline__ T dpp_reduce_step(T v) {
    return Op::combine(dpp_mov<CTRL, ROW_MASK>(Op::old(v), v), v);
}
// Within each row of 16 lanes: row_shr 1, 2, 4, 8; lane 15 of the row holds the row's result.
template <class Op, class T>
__device__ __forceinline__ T row_reduce(T v) {
    v = dpp_reduce_step<Op, dpp_row_shr(1), 0xf>(v);
    v = dpp_reduce_step<Op, dpp_row_shr(2), 0xf>(v);
    v = dpp_reduce_step<Op, dpp_row_shr(4), 0xf>(v);
    return dpp_reduce_step<Op, dpp_row_shr(8), 0xf>(v);
}
// Over the 64 lanes: the rows, then row_bcast15 / row_bcast31 carry the row results on; lane 63 holds the wave's result.
// ~30 VALU instructions for a 64-bit value, no LDS.
template <class Op, class T>
__device__ __forceinline__ T wave_reduce(T v) {
    v = row_reduce<Op>(v);
    v = dpp_reduce_step<Op, kDppRowBcast15, 0xa>(v);
    return dpp_reduce_step<Op, kDppRowBcast31, 0xc>(v);
}

// Wave-uniform results.  wave_sum_f64 is a tree: every term takes part in at most six additions.
__device__ __forceinline__ int64_t wave_max_i64(int64_t v) { return read_lane(wave_reduce<OpMax>(v), kWave - 1); }
__device__ __forceinline__ int32_t wave_max_i32(int32_t v) { return read_lane(wave_reduce<OpMax>(v), kWave - 1); }
__device__ __forceinline__ double wave_sum_f64(double v) { return bcast_f64(wave_reduce<OpSumF64>(v), kWave - 1); }
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) { return read_lane(wave_reduce<OpSumI64>(v), kWave - 1); }
// The minimum as the complement of a maximum: no value is out of range (negation would lose INT64_MIN).
__device__ __forceinline__ int64_t wave_min_any_i64(int64_t v) { return ~read_lane(wave_reduce<OpMax>(~v), kWave - 1); }
// Per row of 16 lanes, in the row's lane 15.
__device__ __forceinline__ double row_max_f64(double v) { return row_reduce<OpMaxF64>(v); }
__device__ __forceinline__ uint32_t row_min_u32(uint32_t v) { return row_reduce<OpMinU32>(v); }

// ------------------------------------------------------------------------------------------------ phase clock

// Cycle accounting by phase: when `on`, adds the shader cycles since `mark` to ph[i] and moves the mark.  `on` is a template flag
// (the uninstrumented instantiation then holds no cycle-counter read) or a kernel's stats != nullptr; the caller owns ph[] and
// the mark, which it starts as  on ? __builtin_readcyclecounter() : 0.  A macro for the same reason as GF_HERE: a struct with a
// tick() changed the register allocation of every kernel whose switch is a run-time one.
#define GF_TICK(on, ph, mark, i)                                      \
    if (on) {                                                         \
        const unsigned long long now_ = __builtin_readcyclecounter(); \
        (ph)[i] += now_ - (mark);                                     \
        (mark) = now_;                                                \
    }
