// gangfit_worker_rounds.h — the round arithmetic of the resident worker (gangfit_worker.inc) as pure functions: no HIP, no
// context, the same code for the kernel, for the host that launches it and for a CPU test (tests/worker_rounds_shim.cpp).
//
// A ticket of n_apps applications is served by one set of `blocks_per_set` workgroups of sixteen wavefronts.  In round `round`
// (the set's round-th ticket) workgroup bs of the set acts as workgroup bsr = (bs + round) mod blocks_per_set; its applications are
//     f0 + l + row * app_stride,   f0 = 16 bsr,  l = 0 .. 15,  row = 0, 1, ...,  app_stride = 16 blocks_per_set,
// those below n_apps.  They are handed out as positions i = 0 .. total - 1 (position i = lane i mod 16 of row i div 16; only the
// last row is ragged, its positions at or behind n_apps are skipped), and the workgroup has finished the ticket when `share`
// applications are counted.  Nothing here divides at run time: bsr advances by one per round and wraps by compare, and the one
// quotient by app_stride — the rows of the workgroup's first lane — is a multiplication by a constant of the launch (StrideDiv).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GF_ROUNDS_FN __host__ __device__ inline
#else
#define GF_ROUNDS_FN inline
#endif

namespace gangfit {
namespace rounds {

constexpr uint32_t kWaves = 16;  // wavefronts per workgroup (gangfit::kWorkerWaves)

// n / (16 b) for EVERY 32-bit n, b = blocks_per_set >= 1:  n / (16 b) = x / b with x = n >> 4 < 2^28, and with l = ceil(log2 b),
// s = 28 + l, mul = ceil(2^s / b) = (2^s + e) / b, 0 <= e < b:  x * mul / 2^s = x / b + x e / (b 2^s), and x e < 2^28 2^l = 2^s, so the
// excess stays below 1 / b and never carries the floor over.  mul <= 2^29 + 1, the product stays below 2^58.
struct StrideDiv {
    uint32_t mul;
    uint32_t shift;
};

GF_ROUNDS_FN StrideDiv make_stride_div(uint32_t blocks_per_set) {
    const uint32_t b = blocks_per_set != 0u ? blocks_per_set : 1u;
    uint32_t l = 0;
    while (l < 32u && (1ull << l) < (uint64_t)b) ++l;
    const uint32_t s = 28u + l;
    StrideDiv d;
    d.mul = (uint32_t)(((1ull << s) + (uint64_t)b - 1ull) / (uint64_t)b);
    d.shift = s;
    return d;
}

GF_ROUNDS_FN uint32_t div_stride(uint32_t n, StrideDiv d) { return (uint32_t)(((uint64_t)(n >> 4) * (uint64_t)d.mul) >> d.shift); }

// The workgroup that workgroup bs of a set acts as in a round: by definition, and from one round to the next.
GF_ROUNDS_FN uint32_t block_of_round(uint32_t bs, uint32_t round, uint32_t blocks_per_set) {
    return (uint32_t)(((uint64_t)bs + (uint64_t)round) % (uint64_t)blocks_per_set);
}
GF_ROUNDS_FN uint32_t next_block(uint32_t bsr, uint32_t blocks_per_set) { return bsr + 1u >= blocks_per_set ? 0u : bsr + 1u; }
GF_ROUNDS_FN uint32_t wave_of_round(uint32_t wave, uint32_t round) { return (wave + round) & (kWaves - 1u); }

GF_ROUNDS_FN uint32_t first_app(uint32_t bsr) { return bsr * kWaves; }

// Rows of the workgroup's first lane: applications f0, f0 + app_stride, ... below n_apps.
GF_ROUNDS_FN uint32_t rows_of(uint32_t n_apps, uint32_t f0, StrideDiv d) { return f0 < n_apps ? div_stride(n_apps - 1u - f0, d) + 1u : 0u; }

// Hand-out positions of the workgroup in the ticket.
GF_ROUNDS_FN uint32_t total_of(uint32_t rows) { return rows * kWaves; }

// Applications of the workgroup in the ticket: every row but the last is full (app_stride >= 16), the last holds what is left.
GF_ROUNDS_FN uint32_t share_of(uint32_t n_apps, uint32_t f0, uint32_t app_stride, uint32_t rows) {
    if (rows == 0u) return 0u;
    const uint32_t left = n_apps - f0 - (rows - 1u) * app_stride;
    return kWaves * (rows - 1u) + (left < kWaves ? left : kWaves);
}

// The application at hand-out position i.
GF_ROUNDS_FN uint32_t app_index(uint32_t f0, uint32_t i, uint32_t app_stride) {
    return f0 + (i & (kWaves - 1u)) + (i >> 4) * app_stride;
}

}  // namespace rounds
}  // namespace gangfit
