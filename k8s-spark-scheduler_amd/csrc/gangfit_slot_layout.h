// gangfit_slot_layout.h — the slot layout of an installed snapshot ("Slot space") as pure host code: no HIP, no
// context.  plan_layout cleans and merges the two priority orders and returns the sizes or a refusal; the caller reserves its
// staging memory; fill_layout writes every table gf_orders_set uploads into it.  What the context keeps is LayoutFacts.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "gangfit.h"

namespace gfapi {

constexpr int64_t kSentinelAvail = -(INT64_C(1) << 62);  // "node is not in nodesSchedulingMetadata"
constexpr int32_t kNarrowNever = INT32_MIN / 2;          // int32 twin of an empty / sentinel slot: never fits, never hosts

struct LayoutInput {
    uint32_t n_nodes = 0;
    const int64_t* avail[3] = {nullptr, nullptr, nullptr};
    const int64_t* sched[3] = {nullptr, nullptr, nullptr};  // all NULL: no schedulable columns
    const uint32_t* zone = nullptr;                         // NULL: one zone
    const uint32_t* driver_order = nullptr;
    uint32_t n_d = 0;
    const uint32_t* exec_order = nullptr;
    uint32_t n_x = 0;
    bool force_general_layout = false, sparse_gpu = true;
};

// What a context remembers of its current layout; install_layout (gangfit_api_snapshot.cpp) is the only writer.
struct LayoutFacts {
    uint32_t n_slots = 0, n_x = 0, n_d = 0, n_chunks = 0;  // n_x / n_d: executor slots / driver positions the kernels scan
    bool merged = false, identity = false;                // identity: dslot[i] == i
    bool narrow_ok = false;
    int64_t unit[3] = {1, 1, 1}, nmax[3] = {0, 0, 0};
    uint32_t n_g = 0, n_gpad = 0;  // sparse gpu view: sub-slots, padded to whole chunks; 0 = no view
    std::vector<uint32_t> g_prefix;
    uint32_t n_zones = 0, zstride = 0;
    uint32_t zd_row0 = 0;    // row of the zone masks where the driver rows start
    bool zspan_ok = false;   // the zone spans were built (merged layout with at least one zone, host-built only)
    bool host_stale = false; // node_slot (and the snapshot's host mirrors) still sit on the device: node_slot below is unused
    std::vector<uint32_t> node_slot;
    // the smallest and largest value of each dimension over the real slots (tmin > tmax: none), whatever narrow_ok says: what the
    // floored narrow form of a chain is decided from (gangfit_floor_units.h).  range_known = false (a snapshot built on the device):
    // fetched from the device when a chain first asks
    bool range_known = false;
    int64_t tmin[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, tmax[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
};

// Element counts of the staging regions fill_layout writes (0 = the table does not exist in this layout).
struct LayoutSizes {
    size_t table = 0;   // int64  cpu | mem | gpu, n_slots each
    size_t index = 0;   // uint32 slot_node (n_slots) | dslot (n_d) | node_slot (n_nodes)
    size_t masks = 0;   // uint64 xmask | dmask, n_chunks each
    size_t cmax = 0;    // int64  [3][n_chunks]
    size_t ntable = 0;  // int32  [3][n_slots] | chunk maxima [3][n_chunks]
    size_t nquad = 0;   // int32  [n_slots][4]: the twin again, one record {cpu, mem, gpu, node} per slot (NodeTable::nquad)
    size_t gtab = 0;    // int64  [3][n_gpad] | chunk maxima [3][n_gpad / 64]
    size_t gidx = 0;    // uint32 node of sub-slot (n_gpad) | sub-slot of slot (n_slots) | slot of sub-slot (n_gpad)
    size_t gmask = 0;   // uint64 [1 + n_zones][n_gpad / 64]: every sub-slot, then one row per zone
    size_t sched = 0;   // int64  [3][n_slots]
    size_t zmasks = 0;  // uint64 [2][n_zones][zstride]: executor rows, then driver rows
    size_t zspan = 0;   // uint32 [n_zones + 1][4]
};

struct LayoutTables {
    int64_t* table = nullptr;
    uint32_t* index = nullptr;
    uint64_t* masks = nullptr;
    int64_t* cmax = nullptr;
    int32_t* ntable = nullptr;
    int32_t* nquad = nullptr;  // nullptr: not wanted (the columns alone)
    int64_t* gtab = nullptr;
    uint32_t* gidx = nullptr;
    uint64_t* gmask = nullptr;
    int64_t* sched = nullptr;
    uint64_t* zmasks = nullptr;
    uint32_t* zspan = nullptr;
};

struct LayoutPlan {
    int code = GF_OK;  // GF_ERR_INVALID + error: the orders were refused and nothing below is meaningful
    std::string error;
    LayoutFacts facts;  // sizes and node_slot now; fill_layout completes units, identity, g_prefix and zspan_ok
    LayoutSizes sizes;
    // ---- carried from plan to fill
    std::vector<uint32_t> xs, ds;   // the cleaned orders
    std::vector<uint32_t> merged;   // merged layout: node of slot
    std::vector<uint8_t> mflags;    // ... bit 0: executor candidate, bit 1: driver candidate
    std::vector<uint32_t> eval;     // zone evaluation list
};

namespace layout_detail {

inline void set_bit(uint64_t* words, uint32_t i) { words[i >> 6] |= 1ull << (i & 63); }

inline LayoutPlan& refuse(LayoutPlan& p, const char* fmt, uint32_t arg = 0) {
    char buf[128];
    std::snprintf(buf, sizeof buf, fmt, arg);
    p.code = GF_ERR_INVALID;
    p.error = buf;
    return p;
}

// chunks [lo, hi) of `n_chunks` where row a (or row b, if given) has a bit
inline void chunk_span(const uint64_t* a, const uint64_t* b, uint32_t n_chunks, uint32_t* out) {
    uint32_t lo = n_chunks, hi = 0;
    for (uint32_t c = 0; c < n_chunks; ++c)
        if (a[c] | (b ? b[c] : 0)) {
            lo = c < lo ? c : lo;
            hi = c + 1;
        }
    out[0] = lo < hi ? lo : 0;
    out[1] = hi;
}

// [3][n_chunks] maxima of a [3][n] table in chunks of 64
inline void chunk_maxima(const int64_t* t, size_t n, uint32_t n_chunks, int64_t* out) {
    for (int j = 0; j < 3; ++j)
        for (uint32_t c = 0; c < n_chunks; ++c) {
            int64_t m = INT64_MIN;
            const size_t hi = ((size_t)c + 1) * 64 < n ? ((size_t)c + 1) * 64 : n;
            for (size_t s = (size_t)c * 64; s < hi; ++s) m = t[j * n + s] > m ? t[j * n + s] : m;
            out[(size_t)j * n_chunks + c] = m;
        }
}

// Merged layout: slot s = position s of the common order; per zone of the evaluation list, candidate rows over the same slots and
// the chunks they span (node-range shards skip the zones outside their range: gangfit_shard.inc); then the sparse gpu view
// (gangfit::SparseTable): the executor candidates with a free gpu as a compact table of their own.
inline void fill_merged(const LayoutInput& in, LayoutPlan& p, const LayoutTables& t) {
    LayoutFacts& f = p.facts;
    const uint32_t n_slots = f.n_slots, n_chunks = f.n_chunks, nz = f.n_zones, n_m = (uint32_t)p.merged.size();
    auto zone_of = [&](uint32_t n) { return in.zone ? in.zone[n] : 0u; };
    uint32_t* slot_node = t.index;
    uint32_t* dslot = slot_node + n_slots;
    uint64_t* xmask = t.masks;
    uint64_t* dmask = xmask + n_chunks;
    for (uint32_t s = 0; s < n_m; ++s) {
        dslot[s] = s;
        if (p.mflags[s] & 1) set_bit(xmask, s);
        if (p.mflags[s] & 2) set_bit(dmask, s);
    }
    f.identity = true;
    uint64_t* zx = t.zmasks;
    uint64_t* zd = zx + (size_t)nz * f.zstride;
    for (uint32_t zi = 0; zi < nz; ++zi) {
        uint64_t* rx = zx + (size_t)zi * f.zstride;
        uint64_t* rd = zd + (size_t)zi * f.zstride;
        for (uint32_t s = 0; s < n_m; ++s) {
            if (zone_of(p.merged[s]) != p.eval[zi]) continue;
            if (p.mflags[s] & 1) set_bit(rx, s);
            if (p.mflags[s] & 2) set_bit(rd, s);
        }
        chunk_span(rx, rd, n_chunks, t.zspan + 4 * (size_t)zi);
    }
    f.zspan_ok = nz != 0;
    if (f.n_g == 0) return;
    const uint32_t n_gpad = f.n_gpad, gch = n_gpad / 64u;
    const int64_t* tcpu = t.table;
    const int64_t* tmem = tcpu + n_slots;
    const int64_t* tgpu = tmem + n_slots;
    int64_t* g0 = t.gtab;
    uint32_t* gnode = t.gidx;
    uint32_t* gsub = gnode + n_gpad;
    uint32_t* gslot = gsub + n_slots;  // sub-slot -> slot (SparseTable::slot_of_sub; the padding names the sentinel slot)
    for (size_t i = 0; i < 3 * (size_t)n_gpad; ++i) g0[i] = kSentinelAvail;
    for (uint32_t i = 0; i < n_gpad; ++i) gnode[i] = GF_NO_NODE;
    for (uint32_t i = 0; i < n_gpad; ++i) gslot[i] = n_slots - 1u;
    for (uint32_t s = 0; s < n_slots; ++s) gsub[s] = GF_NO_NODE;
    uint32_t k = 0;
    f.g_prefix.assign((size_t)n_slots / 64u + 2u, f.n_g);
    for (uint32_t s = 0; s < n_m; ++s) {
        if ((s & 63u) == 0u) f.g_prefix[s >> 6] = k;
        if ((p.mflags[s] & 1) && tgpu[s] > 0) {
            g0[k] = tcpu[s];
            g0[n_gpad + k] = tmem[s];
            g0[2 * (size_t)n_gpad + k] = tgpu[s];
            gnode[k] = slot_node[s];
            gslot[k] = s;
            gsub[s] = k++;
        }
    }
    chunk_maxima(g0, n_gpad, gch, g0 + 3 * (size_t)n_gpad);
    // SparseTable::xmask (row 0: every sub-slot) and ::zmask (row 1 + zi: the sub-slots of zone eval[zi]), and each zone's span there
    for (size_t i = 0; i < p.sizes.gmask; ++i) t.gmask[i] = 0;
    for (uint32_t i = 0; i < f.n_g; ++i) {
        set_bit(t.gmask, i);
        for (uint32_t zi = 0; zi < nz; ++zi)
            if (p.eval[zi] == zone_of(gnode[i])) set_bit(t.gmask + (size_t)gch * (1u + zi), i);
    }
    for (uint32_t zi = 0; zi < nz; ++zi) chunk_span(t.gmask + (size_t)gch * (1u + zi), nullptr, gch, t.zspan + 4 * (size_t)zi + 2);
}

// General layout: the executor order with its unknown names (which stay empty slots), then the driver-only nodes; dslot[] maps
// driver positions (unknown names to the sentinel) and the zone driver rows go by driver POSITION (Orders::dpos_mask).
inline void fill_general(const LayoutInput& in, LayoutPlan& p, const LayoutTables& t) {
    LayoutFacts& f = p.facts;
    auto zone_of = [&](uint32_t n) { return in.zone ? in.zone[n] : 0u; };
    uint32_t* dslot = t.index + f.n_slots;
    uint64_t* xmask = t.masks;
    uint64_t* dmask = xmask + f.n_chunks;
    for (uint32_t i = 0; i < in.n_d; ++i) {
        const uint32_t n = in.driver_order[i];
        dslot[i] = n < in.n_nodes ? f.node_slot[n] : f.n_slots - 1;
    }
    f.identity = false;
    for (uint32_t i = 0; i < in.n_x; ++i)
        if (in.exec_order[i] < in.n_nodes) set_bit(xmask, i);
    for (uint32_t c = 0; c < f.n_chunks; ++c) dmask[c] = ~0ull;  // not consulted: positions go through dslot[]
    uint64_t* zx = t.zmasks;
    uint64_t* zd = zx + (size_t)f.n_zones * f.zstride;
    for (uint32_t zi = 0; zi < f.n_zones; ++zi) {
        const uint32_t z = p.eval[zi];
        for (uint32_t i = 0; i < in.n_x; ++i)
            if (in.exec_order[i] < in.n_nodes && zone_of(in.exec_order[i]) == z) set_bit(zx + (size_t)zi * f.zstride, i);
        for (uint32_t i = 0; i < in.n_d; ++i)
            if (in.driver_order[i] < in.n_nodes && zone_of(in.driver_order[i]) == z) set_bit(zd + (size_t)zi * f.zstride, i);
    }
}

// narrow form: unit[j] = gcd of dimension j over the real slots; scaled magnitudes must stay below 2^30.  nq (nullable): the same
// values once more as one 16-byte record per slot, {cpu, mem, gpu, slot_node}, written in the pass that writes the columns.
inline void fill_narrow(LayoutFacts& f, const int64_t* table, const uint32_t* slot_node, int32_t* nt, int32_t* nq = nullptr) {
    const uint32_t n_slots = f.n_slots, n_chunks = f.n_chunks;
    for (int j = 0; j < 3; ++j) {
        const int64_t* col = table + (size_t)j * n_slots;
        uint64_t g = 0;
        for (uint32_t s = 0; s + 1 < n_slots; ++s) {
            if (slot_node[s] == GF_NO_NODE) continue;
            uint64_t v = (uint64_t)(col[s] < 0 ? -col[s] : col[s]);
            while (v) {  // Euclid
                const uint64_t r = g % v;
                g = v;
                v = r;
            }
            if (g == 1) break;
        }
        f.unit[j] = g ? (int64_t)g : 1;
    }
    int32_t* ncm = nt + 3 * (size_t)n_slots;
    f.narrow_ok = true;
    for (int j = 0; j < 3; ++j) {
        const int64_t* col = table + (size_t)j * n_slots;
        f.nmax[j] = 0;
        for (uint32_t c = 0; c < n_chunks; ++c) ncm[(size_t)j * n_chunks + c] = INT32_MIN;
        for (uint32_t s = 0; s < n_slots; ++s) {
            int32_t v32 = kNarrowNever;
            if (s + 1 < n_slots && slot_node[s] != GF_NO_NODE) {
                const int64_t q = col[s] / f.unit[j];
                if (q >= (INT64_C(1) << 30) || q <= -(INT64_C(1) << 30)) {
                    f.narrow_ok = false;  // no narrow form: the int32 table is not uploaded
                    return;
                }
                v32 = (int32_t)q;
                const int64_t mag = q < 0 ? -q : q;
                if (mag > f.nmax[j]) f.nmax[j] = mag;
            }
            nt[(size_t)j * n_slots + s] = v32;
            if (nq != nullptr) {
                nq[4 * (size_t)s + j] = v32;
                if (j == 0) nq[4 * (size_t)s + 3] = (int32_t)slot_node[s];
            }
            int32_t& m = ncm[(size_t)j * n_chunks + (s >> 6)];
            m = v32 > m ? v32 : m;
        }
    }
}

// tmin / tmax of the facts: every real slot of every dimension (fill_narrow stops at the first value without a scaled form).
inline void fill_range(LayoutFacts& f, const int64_t* table, const uint32_t* slot_node) {
    for (int j = 0; j < 3; ++j) {
        const int64_t* col = table + (size_t)j * f.n_slots;
        int64_t lo = INT64_MAX, hi = INT64_MIN;
        for (uint32_t s = 0; s + 1 < f.n_slots; ++s) {
            if (slot_node[s] == GF_NO_NODE) continue;
            lo = col[s] < lo ? col[s] : lo;
            hi = col[s] > hi ? col[s] : hi;
        }
        f.tmin[j] = lo;
        f.tmax[j] = hi;
    }
    f.range_known = true;
}

}  // namespace layout_detail

// Step 1.  Positions of the known nodes in the two orders: unknown names (index >= n_nodes) never host anything (binpack.go:68,
// pack_tightly.go:51, distribute_evenly.go:59) and a repeated driver candidate can only repeat the failure of its first
// occurrence, so both are dropped from the slot space without changing any result.  Then the merged layout — one order that has
// both cleaned orders as subsequences — if it exists, else the general one; and the zone evaluation list (single_az.go:23-72):
// zones in order of first appearance in the driver order that own at least one executor candidate.
inline LayoutPlan plan_layout(const LayoutInput& in) {
    using namespace layout_detail;
    LayoutPlan p;
    LayoutFacts& f = p.facts;
    const uint32_t n_nodes = in.n_nodes;
    std::vector<uint32_t> xpos(n_nodes, GF_NO_NODE), dpos(n_nodes, GF_NO_NODE);
    p.xs.reserve(in.n_x);
    p.ds.reserve(in.n_d);
    uint32_t x_gpu = 0;  // executor candidates with a free gpu
    for (uint32_t i = 0; i < in.n_x; ++i) {
        const uint32_t n = in.exec_order[i];
        if (n >= n_nodes) continue;
        if (xpos[n] != GF_NO_NODE) return refuse(p, "node %u appears twice in the executor priority order", n);
        xpos[n] = (uint32_t)p.xs.size();
        p.xs.push_back(n);
        if (in.avail[2][n] > 0) ++x_gpu;
    }
    for (uint32_t i = 0; i < in.n_d; ++i) {
        const uint32_t n = in.driver_order[i];
        if (n >= n_nodes || dpos[n] != GF_NO_NODE) continue;
        dpos[n] = (uint32_t)p.ds.size();
        p.ds.push_back(n);
    }
    const std::vector<uint32_t>& xs = p.xs;
    const std::vector<uint32_t>& ds = p.ds;
    f.merged = !in.force_general_layout;
    if (f.merged) {
        p.merged.reserve(xs.size() + ds.size());
        size_t i = 0, j = 0;
        while (i < ds.size() || j < xs.size()) {
            if (i < ds.size() && j < xs.size() && ds[i] == xs[j]) {
                p.merged.push_back(ds[i]);
                p.mflags.push_back(3);
                ++i;
                ++j;
            } else if (i < ds.size() && xpos[ds[i]] == GF_NO_NODE) {
                p.merged.push_back(ds[i++]);
                p.mflags.push_back(2);
            } else if (j < xs.size() && dpos[xs[j]] == GF_NO_NODE) {
                p.merged.push_back(xs[j++]);
                p.mflags.push_back(1);
            } else {  // two nodes present in both orders, in opposite relative order
                f.merged = false;
                break;
            }
        }
    }
    f.node_slot.assign(n_nodes, GF_NO_NODE);
    uint64_t n_slots64;
    if (f.merged) {
        f.n_x = f.n_d = (uint32_t)p.merged.size();
        n_slots64 = (uint64_t)p.merged.size() + 1;
        for (uint32_t s = 0; s < p.merged.size(); ++s) f.node_slot[p.merged[s]] = s;
        if (in.sparse_gpu && x_gpu > 0 && (uint64_t)x_gpu * 4 <= p.merged.size()) {  // a minority of the order: the view exists
            f.n_g = x_gpu;
            f.n_gpad = (x_gpu + 63u) / 64u * 64u;
        }
    } else {
        for (uint32_t i = 0; i < in.n_x; ++i)
            if (in.exec_order[i] < n_nodes) f.node_slot[in.exec_order[i]] = i;
        uint32_t extra = 0;
        for (uint32_t i = 0; i < in.n_d; ++i) {
            const uint32_t n = in.driver_order[i];
            if (n < n_nodes && f.node_slot[n] == GF_NO_NODE) f.node_slot[n] = in.n_x + extra++;
        }
        n_slots64 = (uint64_t)in.n_x + extra + 1;
        f.n_x = in.n_x;
        f.n_d = in.n_d;
    }
    if (n_slots64 >= GF_NO_NODE) return refuse(p, "order vectors too long");
    f.n_slots = (uint32_t)n_slots64;
    f.n_chunks = (f.n_slots + 63) / 64;
    auto zone_of = [&](uint32_t n) { return in.zone ? in.zone[n] : 0u; };
    std::vector<uint32_t> zlist;
    for (uint32_t n : ds) {
        const uint32_t z = zone_of(n);
        bool seen = false;
        for (uint32_t q : zlist) seen = seen || q == z;
        if (!seen) zlist.push_back(z);
    }
    for (uint32_t z : zlist) {
        bool has_x = false;
        for (uint32_t n : xs)
            if (zone_of(n) == z) {
                has_x = true;
                break;
            }
        if (has_x) p.eval.push_back(z);
    }
    const uint32_t d_words = (f.n_d + 63) / 64;
    f.n_zones = f.zd_row0 = (uint32_t)p.eval.size();
    f.zstride = f.n_chunks > d_words ? f.n_chunks : d_words;
    LayoutSizes& z = p.sizes;
    const size_t S = f.n_slots, C = f.n_chunks, G = f.n_gpad;
    z.table = 3 * S;
    z.index = S + f.n_d + n_nodes;
    z.masks = 2 * C;
    z.cmax = 3 * C;
    z.ntable = 3 * S + 3 * C;
    z.nquad = 4 * S;
    if (f.n_g) {
        z.gtab = 3 * G + 3 * (G / 64);
        z.gidx = 2 * G + S;
        z.gmask = (G / 64) * (1 + (size_t)f.n_zones);
    }
    if (in.sched[0]) z.sched = 3 * S;
    z.zmasks = 2 * (size_t)f.n_zones * f.zstride;
    if (f.merged && f.n_zones) z.zspan = 4 * (size_t)f.n_zones + 4;
    return p;
}

// Step 2.  Every table of an accepted plan, into memory of at least p.sizes elements each; completes p.facts.
inline void fill_layout(const LayoutInput& in, LayoutPlan& p, const LayoutTables& t) {
    using namespace layout_detail;
    LayoutFacts& f = p.facts;
    const uint32_t n_slots = f.n_slots;
    uint32_t* slot_node = t.index;
    uint32_t* nslot = slot_node + n_slots + f.n_d;
    for (size_t i = 0; i < p.sizes.table; ++i) t.table[i] = kSentinelAvail;
    for (uint32_t s = 0; s < n_slots; ++s) slot_node[s] = GF_NO_NODE;
    for (size_t i = 0; i < p.sizes.masks; ++i) t.masks[i] = 0;
    for (size_t i = 0; i < p.sizes.zmasks; ++i) t.zmasks[i] = 0;
    for (size_t i = 0; i < p.sizes.zspan; ++i) t.zspan[i] = 0;
    for (uint32_t n = 0; n < in.n_nodes; ++n) {
        const uint32_t s = f.node_slot[n];
        nslot[n] = s;
        if (s == GF_NO_NODE) continue;
        slot_node[s] = n;
        for (int j = 0; j < 3; ++j) t.table[(size_t)j * n_slots + s] = in.avail[j][n];
    }
    if (f.merged)
        fill_merged(in, p, t);
    else
        fill_general(in, p, t);
    chunk_maxima(t.table, n_slots, f.n_chunks, t.cmax);  // chunk-maxima index over all slots (see NodeTable::cmax)
    fill_narrow(f, t.table, slot_node, t.ntable, t.nquad);
    fill_range(f, t.table, slot_node);
    if (p.sizes.sched)  // SchedulableResources in slot order (efficiencies); empty slots read 0
        for (int j = 0; j < 3; ++j)
            for (uint32_t s = 0; s < n_slots; ++s)
                t.sched[(size_t)j * n_slots + s] = slot_node[s] == GF_NO_NODE ? 0 : in.sched[j][slot_node[s]];
}

}  // namespace gfapi
