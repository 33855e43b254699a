// gangfit_floor_units.h — the narrow units of one FIFO chain ("Units per batch") as pure host code: no HIP, no
// context.  Two forms of the scaled int32 table exist:
//   exact    every table value is a multiple of the unit (refine_units: the table's own gcds, refined by the requests as far as
//            the scaled magnitudes stay below 2^30) — value = scaled * unit;
//   floored  the unit divides every REQUEST of the queue and the table is floored: A = q * u + r with q = floor(A / u) toward
//            minus infinity and 0 <= r < u.  A chain only subtracts sums of requests, so r stays what it is and every integer
//            decision of every packer is the same on q as on A: rho * u > A <=> rho > q; A - beta * u < 0 <=> q - beta < 0;
//            floor((A - beta * u) / (eps * u)) = floor((q - beta) / eps) whenever q - beta >= 0.  Only the packing efficiencies
//            and the residual table want A = q * u + r back.
// chain_units decides between them.  The exact form wins whenever it is proven (a batch that has it keeps its kernels and its
// units); the floored form is chosen iff -2^30 < floor(A / u) < 2^30 over the real slots, every request is below 2^30 units and
// every k is in range; else the batch has no narrow form and the wide kernels serve.
#pragma once
#include <cstdint>

#include "gangfit.h"

namespace gfapi {

constexpr int64_t kNarrowBound = INT64_C(1) << 30;  // scaled values lie strictly inside (-2^30, 2^30)

// floor(a / u) toward minus infinity, u > 0
inline int64_t floor_div(int64_t a, int64_t u) {
    const int64_t q = a / u;
    return (a % u != 0 && a < 0) ? q - 1 : q;
}

// What a context knows of its installed table, per dimension over the real slots: the exact form's facts (LayoutFacts) and the
// smallest and largest value (tmin > tmax: no real slot).
struct TableFacts {
    bool narrow_ok = false;
    int64_t unit[3] = {1, 1, 1}, nmax[3] = {0, 0, 0};
    int64_t tmin[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, tmax[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
};

struct ChainUnits {
    bool proven = false;   // every request has a scaled form in `unit` and the table has one: an LDS chain kernel serves for certain
    bool floored = false;  // ... the floored one (then factor = 1: the floored snapshot is built in these units)
    int64_t unit[3] = {1, 1, 1};
    int32_t factor[3] = {1, 1, 1};  // exact form: the table's unit / unit, what the int32 snapshot is multiplied by
};

// The exact form: the table's units refined to gcd(table unit, every request of the batch) as long as every scaled magnitude stays
// below 2^30 (`room`), else the table's own.  *proven (nullable): every request is a multiple of the result and below 2^30 units.
inline void refine_units(const int64_t unit[3], const int64_t nmax[3], const gf_app* apps, uint32_t n_apps, int64_t eff[3],
                         int32_t factor[3], bool* proven) {
    for (int j = 0; j < 3; ++j) {
        eff[j] = unit[j];
        factor[j] = 1;
    }
    if (proven) *proven = false;
    if (apps == nullptr) return;
    for (uint32_t a = 0; a < n_apps; ++a)
        for (int j = 0; j < 3; ++j)
            for (const int64_t v : {apps[a].drv[j], apps[a].exe[j]})
                if (v > 0 && v % eff[j] != 0) {
                    int64_t x = eff[j], y = v;
                    while (y) {
                        const int64_t t = x % y;
                        x = y;
                        y = t;
                    }
                    eff[j] = x;
                }
    bool ok = true;
    for (int j = 0; j < 3; ++j) {
        const int64_t f = unit[j] / eff[j];
        const int64_t room = nmax[j] > 0 ? (kNarrowBound - 1) / nmax[j] : kNarrowBound - 1;
        ok = ok && f <= room;
        factor[j] = ok ? (int32_t)f : 1;
    }
    if (!ok)
        for (int j = 0; j < 3; ++j) {
            eff[j] = unit[j];
            factor[j] = 1;
        }
    if (proven) {
        bool all = true;
        for (uint32_t a = 0; a < n_apps && all; ++a)
            for (int j = 0; j < 3; ++j)
                for (const int64_t v : {apps[a].drv[j], apps[a].exe[j]})
                    all = all && v >= 0 && v % eff[j] == 0 && v / eff[j] < kNarrowBound;
        *proven = all;
    }
}

// The shortest prefix of the queue that refine_units does not prove: its length, 0 when the whole queue is proven.  A prefix that
// is not proven stays so however the queue goes on — the refined units only get finer, so a room test that failed fails again and a
// request of 2^30 units or more only grows; and where the refinement falls back to the table's units, the request that made it
// finer is no multiple of them.  So a later queue that begins with this prefix has no exact form either, without a scan (chain_plan).
// One pass: the running gcds and the largest request per dimension decide every prefix.
inline uint32_t exact_fails_at(const int64_t unit[3], const int64_t nmax[3], const gf_app* apps, uint32_t n_apps) {
    int64_t g[3] = {unit[0], unit[1], unit[2]}, top[3] = {0, 0, 0};
    for (uint32_t a = 0; a < n_apps; ++a) {
        for (int j = 0; j < 3; ++j)
            for (const int64_t v : {apps[a].drv[j], apps[a].exe[j]}) {
                if (v < 0) return a + 1;
                top[j] = v > top[j] ? v : top[j];
                int64_t x = g[j], y = v;
                while (y) {
                    const int64_t t = x % y;
                    x = y;
                    y = t;
                }
                g[j] = x;
            }
        for (int j = 0; j < 3; ++j) {
            const int64_t room = nmax[j] > 0 ? (kNarrowBound - 1) / nmax[j] : kNarrowBound - 1;
            if (unit[j] / g[j] > room || top[j] / g[j] >= kNarrowBound) return a + 1;
        }
    }
    return 0;
}

// -2^30 < floor(A / u) < 2^30 for every A of [tmin, tmax] (floor is monotone: the two ends decide; no real slot: nothing to hold)
inline bool floor_range_ok(int64_t tmin, int64_t tmax, int64_t u) {
    if (tmin > tmax) return true;
    return floor_div(tmax, u) < kNarrowBound && floor_div(tmin, u) > -kNarrowBound;
}

// The floored form of a queue: u_j = gcd of its positive drv[j] and exe[j]; a dimension nobody asks for takes the smallest power of
// two that brings its column inside the range.  false: a k outside [0, GF_MAX_K], a negative request, a request of 2^30 units or
// more, or a table value whose floor leaves the range.
inline bool floor_units(const int64_t tmin[3], const int64_t tmax[3], const gf_app* apps, uint32_t n_apps, int64_t unit[3]) {
    if (apps == nullptr) return false;
    uint64_t g[3] = {0, 0, 0};
    int64_t top[3] = {0, 0, 0};  // the largest request
    for (uint32_t a = 0; a < n_apps; ++a) {
        if (apps[a].k < 0 || apps[a].k > GF_MAX_K) return false;
        for (int j = 0; j < 3; ++j)
            for (const int64_t v : {apps[a].drv[j], apps[a].exe[j]}) {
                if (v < 0) return false;
                if (v > top[j]) top[j] = v;
                uint64_t x = g[j], y = (uint64_t)v;
                while (y) {  // (gcd(0, v) = v; v = 0 leaves g)
                    const uint64_t t = x % y;
                    x = y;
                    y = t;
                }
                g[j] = x;
            }
    }
    for (int j = 0; j < 3; ++j) {
        if (g[j] == 0) {
            int64_t u = 1;
            while (!floor_range_ok(tmin[j], tmax[j], u)) u <<= 1;  // (|A| < 2^62: 2^33 at the most)
            unit[j] = u;
            continue;
        }
        unit[j] = (int64_t)g[j];
        if (top[j] / unit[j] >= kNarrowBound || !floor_range_ok(tmin[j], tmax[j], unit[j])) return false;
    }
    return true;
}

// The units of one chain.  The floored form is tried only when the exact one is not proven — the table has none, a request is no
// multiple of the refined units, or the refinement fails its room test; otherwise the answer is refine_units' own.
inline ChainUnits chain_units(const TableFacts& t, const gf_app* apps, uint32_t n_apps, bool allow_floor = true) {
    ChainUnits u;
    if (t.narrow_ok) refine_units(t.unit, t.nmax, apps, n_apps, u.unit, u.factor, &u.proven);
    if (u.proven || !allow_floor) return u;
    int64_t fu[3];
    if (floor_units(t.tmin, t.tmax, apps, n_apps, fu)) {
        u.proven = u.floored = true;
        for (int j = 0; j < 3; ++j) {
            u.unit[j] = fu[j];
            u.factor[j] = 1;
        }
    }
    return u;
}

}  // namespace gfapi
