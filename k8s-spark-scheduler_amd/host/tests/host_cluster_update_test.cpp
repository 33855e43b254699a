// host_cluster_update_test.cpp — node rows of the resident cluster changed in place (FlatCluster::BuildWithSpare / Rebuild ->
// gf_cluster_update through SparkSchedulerExtender::syncResident).
// `host_cluster_update_test cpu` needs no GPU: Rebuild against a brute-force restatement — stable indices over join, leave and
// rejoin sequences, ranks a permutation in name order, rows_out, the carried-entry rule for index reuse, spare exhaustion, a changed
// set of zone labels;
// `host_cluster_update_test gpu` drives the device through the C ABI: group Filters, a marker scan, an executor Filter and a
// reconcile across node join, leave, cordon and resize — every answer equals that of a fresh extender (on a context of its own)
// given a fresh Build of the same nodes, with one gf_cluster_set and one usage replay while the reservation list's version stands.
// Exit code 0 = all passed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

#define HOST_TEST_SEED 0xC1057E2
#include "failover.hpp"
#include "host_test_common.hpp"

static const char* kZones[] = {"az-a", "az-b", "az-c"};

static Node NewNode(const std::string& name, const char* zone, int64_t cpu, int64_t mem_gi) {
    Node nd;
    nd.Name = name;
    nd.labels[kLabelZoneFailureDomain] = zone;
    nd.labels[kLabelTopologyZone] = zone;
    nd.Allocatable = {{kResourceCPU, Quantity::FromInt(cpu)}, {kResourceMemory, Quantity::FromInt(mem_gi * Gi)}, {kResourceNvidiaGPU, Quantity::FromInt(0)}};
    nd.Ready = true;
    return nd;
}
static Node RandomNode(const std::string& name) { return NewNode(name, kZones[next() % 3], 16 + 16 * (int64_t)(next() % 3), 64 + 64 * (int64_t)(next() % 3)); }

// ------------------------------------------------------------------------------------------------ the restatement
// A row as the brute force sees it: a name ("" = absent) and the three things gf_cluster_update carries.
struct Row {
    std::string name;
    int64_t alloc[3] = {0, 0, 0};
    uint32_t flags = 0, zone = 0;
    bool sameColumns(const Row& o) const {
        return alloc[0] == o.alloc[0] && alloc[1] == o.alloc[1] && alloc[2] == o.alloc[2] && flags == o.flags && zone == o.zone;
    }
};

static std::vector<Row> RowsOf(const FlatCluster& c) {
    std::vector<Row> rows(c.names.size());
    for (size_t i = 0; i < rows.size(); ++i) {
        rows[i].name = c.names[i];
        for (int j = 0; j < 3; ++j) rows[i].alloc[j] = c.alloc[j][i];
        rows[i].flags = c.base_flags[i];
        rows[i].zone = c.zone[i];
    }
    return rows;
}

static Row RowOfNode(const Node& nd, const std::vector<std::string>& zone_labels) {
    Row r;
    r.name = nd.Name;
    // (every quantity of this program is a whole number of cores / bytes)
    int64_t v[3];
    Resources a = Resources::Zero();
    a.CPU = nd.Allocatable.at(kResourceCPU);
    a.Memory = nd.Allocatable.at(kResourceMemory);
    a.NvidiaGPU = nd.Allocatable.at(kResourceNvidiaGPU);
    (void)a.canonical(v);
    for (int j = 0; j < 3; ++j) r.alloc[j] = v[j];
    r.flags = (nd.Unschedulable ? GF_NODE_UNSCHEDULABLE : 0u) | (nd.Ready ? GF_NODE_READY : 0u);
    const std::string& label = nd.labels.at(kLabelZoneFailureDomain);
    r.zone = (uint32_t)(std::find(zone_labels.begin(), zone_labels.end(), label) - zone_labels.begin());
    return r;
}

// The rule, restated slot by slot: names keep their index, the departed become absent (allocatable 0, flags 0, the zone stays), a
// newcomer — in the order of `nodes` — takes the lowest absent index no carried entry names.  false: a newcomer found no row.
static bool Restated(const std::vector<Row>& prev, const std::vector<Node>& nodes, const std::set<uint32_t>& carried,
                     const std::vector<std::string>& zone_labels, std::vector<Row>* out) {
    std::vector<Row> rows = prev;
    for (Row& r : rows) {
        bool listed = false;
        for (const Node& nd : nodes) listed = listed || nd.Name == r.name;
        if (!r.name.empty() && !listed) {
            r.name.clear();
            r.alloc[0] = r.alloc[1] = r.alloc[2] = 0;
            r.flags = 0;
        }
    }
    for (const Node& nd : nodes) {
        size_t at = rows.size();
        for (size_t i = 0; i < rows.size(); ++i)
            if (rows[i].name == nd.Name) at = i;
        for (size_t i = 0; at == rows.size() && i < rows.size(); ++i)
            if (rows[i].name.empty() && carried.count((uint32_t)i) == 0) at = i;
        if (at == rows.size()) return false;
        rows[at] = RowOfNode(nd, zone_labels);
    }
    *out = rows;
    return true;
}

// name_rank as the contract words it: the present names in lexicographic order, then the absent rows in index order
static std::vector<uint32_t> RestatedRanks(const std::vector<Row>& rows) {
    std::vector<uint32_t> rank(rows.size());
    uint32_t present = 0;
    for (const Row& r : rows) present += r.name.empty() ? 0u : 1u;
    uint32_t absent_seen = 0;
    for (size_t i = 0; i < rows.size(); ++i) {
        if (rows[i].name.empty()) {
            rank[i] = present + absent_seen++;
            continue;
        }
        uint32_t before = 0;
        for (const Row& o : rows) before += (!o.name.empty() && o.name < rows[i].name) ? 1u : 0u;
        rank[i] = before;
    }
    return rank;
}

static void CheckAgainstRestatement(const FlatCluster& prev, const FlatCluster& got, const std::vector<uint32_t>& rows_out,
                                    const std::vector<Row>& want) {
    const std::vector<Row> have = RowsOf(got), before = RowsOf(prev);
    CHECK(have.size() == want.size() && have.size() == before.size());
    bool same = true;
    std::vector<uint32_t> changed;
    for (size_t i = 0; i < want.size(); ++i) {
        same = same && have[i].name == want[i].name && have[i].sameColumns(want[i]);
        if (!want[i].sameColumns(before[i])) changed.push_back((uint32_t)i);
        // the index: exactly the present names, each at its row
        const bool indexed = !want[i].name.empty() && got.index.count(want[i].name) != 0 && got.index.at(want[i].name) == i;
        same = same && (want[i].name.empty() || indexed) && got.isAbsent((uint32_t)i) == want[i].name.empty();
    }
    CHECK(same);
    size_t present = 0;
    for (const Row& r : want) present += r.name.empty() ? 0 : 1;
    CHECK(got.index.size() == present);
    CHECK(rows_out == changed && got.changed_rows == changed);
    const std::vector<uint32_t> ranks = RestatedRanks(want);
    CHECK(got.name_rank == ranks);
    std::vector<uint32_t> sorted = got.name_rank;
    std::sort(sorted.begin(), sorted.end());
    bool permutation = true;
    for (size_t i = 0; i < sorted.size(); ++i) permutation = permutation && sorted[i] == i;
    CHECK(permutation);
    CHECK(got.ranks_changed == (got.name_rank != prev.name_rank));
    CHECK(got.derived_from == prev.version && got.version != prev.version && got.version != 0);
    CHECK(got.zone_labels == prev.zone_labels);
    CHECK(got.present.empty() == (present == want.size()));
}

// ------------------------------------------------------------------------------------------------ no device
static void TestBuildWithSpare() {
    std::vector<Node> nodes;
    for (int i = 0; i < 70; ++i) nodes.push_back(RandomNode("n" + std::to_string(next() % 1000) + "-" + std::to_string(i)));
    FlatCluster plain, spare, none;
    std::string err;
    CHECK(FlatCluster::Build(nodes, &plain, &err));
    CHECK(FlatCluster::BuildWithSpare(nodes, 9, &spare, &err));
    CHECK(FlatCluster::BuildWithSpare(nodes, 0, &none, &err));
    CHECK(none.names == plain.names && none.name_rank == plain.name_rank && none.present.empty() && none.derived_from == 0);
    CHECK(spare.names.size() == 79 && spare.index.size() == 70 && spare.zone_labels == plain.zone_labels && spare.derived_from == 0);
    bool same = true;
    for (uint32_t i = 0; i < 70; ++i)
        same = same && spare.names[i] == plain.names[i] && spare.name_rank[i] == plain.name_rank[i] && spare.zone[i] == plain.zone[i] &&
               spare.base_flags[i] == plain.base_flags[i] && spare.alloc[1][i] == plain.alloc[1][i] && !spare.isAbsent(i);
    for (uint32_t i = 70; i < 79; ++i)
        same = same && spare.names[i].empty() && spare.name_rank[i] == i && spare.zone[i] == spare.zone[0] && spare.base_flags[i] == 0 &&
               spare.alloc[0][i] == 0 && spare.alloc[1][i] == 0 && spare.alloc[2][i] == 0 && spare.isAbsent(i);
    CHECK(same);
    CHECK(spare.present.size() == 2 && spare.present[0] == ~UINT64_C(0) && spare.present[1] == (UINT64_C(1) << 6) - 1);
}

static void TestJoinLeaveRejoinSequences() {
    std::vector<Node> pool;  // every name that ever exists; the zone of a name never changes, so the label set can stand
    for (int i = 0; i < 60; ++i) pool.push_back(RandomNode("node-" + std::to_string(next() % 500) + "-" + std::to_string(i)));
    for (int z = 0; z < 3; ++z) pool.push_back(NewNode(std::string("anchor-") + kZones[z], kZones[z], 32, 128));  // never leave
    std::set<size_t> live = {60, 61, 62};
    for (size_t i = 0; i < 25; ++i) live.insert(i);
    auto listed = [&](bool shuffled) {
        std::vector<Node> nodes;
        for (size_t i : live) nodes.push_back(pool[i]);
        if (shuffled)
            for (size_t i = nodes.size(); i > 1; --i) std::swap(nodes[i - 1], nodes[next() % i]);
        return nodes;
    };
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::BuildWithSpare(listed(false), 20, &cluster, &err));
    std::map<std::string, uint32_t> first_index;  // a name's index while it stays
    int rebuilt = 0, joined = 0, left = 0, rejoined = 0;
    std::set<size_t> ever_left;
    for (int step = 0; step < 80; ++step) {
        // leave, join (a name that left may come back), and change what stays: resize, cordon, readiness
        for (size_t i = 0; i < 60; ++i) {
            const uint64_t dice = next() % 16;
            if (live.count(i) && dice == 0) {
                live.erase(i);
                ever_left.insert(i);
                ++left;
            } else if (!live.count(i) && dice <= 1 && live.size() < 40) {
                live.insert(i);
                ++joined;
                rejoined += ever_left.count(i) ? 1 : 0;
            } else if (live.count(i) && dice == 2) {
                pool[i].Allocatable[kResourceCPU] = Quantity::FromInt(8 + 8 * (int64_t)(next() % 6));
            } else if (live.count(i) && dice == 3) {
                pool[i].Unschedulable = !pool[i].Unschedulable;
            } else if (live.count(i) && dice == 4) {
                pool[i].Ready = !pool[i].Ready;
            }
        }
        const std::vector<Node> nodes = listed(true);
        std::set<uint32_t> carried_rows;
        FlatReservations carried;
        for (uint32_t i = 0; i < cluster.names.size(); ++i)
            if (next() % 5 == 0) {  // entries on present and on absent rows alike
                carried_rows.insert(i);
                carried.node.push_back(i);
                for (int j = 0; j < 3; ++j) carried.req[j].push_back(1);
            }
        carried.node.push_back((uint32_t)cluster.names.size() + 3);  // (an entry outside the cluster names no row)
        for (int j = 0; j < 3; ++j) carried.req[j].push_back(1);
        std::vector<Row> want;
        const bool fits = Restated(RowsOf(cluster), nodes, carried_rows, cluster.zone_labels, &want);
        FlatCluster next_cluster;
        std::vector<uint32_t> rows_out = {12345};
        const bool ok = FlatCluster::Rebuild(cluster, nodes, &carried, &next_cluster, &rows_out, &err);
        CHECK(ok == fits);
        if (!ok) {  // (the carried rows took every free one: the caller's fallback)
            CHECK(FlatCluster::BuildWithSpare(nodes, 20, &cluster, &err));
            first_index.clear();
            continue;
        }
        ++rebuilt;
        CheckAgainstRestatement(cluster, next_cluster, rows_out, want);
        bool stable = true;
        for (const auto& [name, at] : next_cluster.index) {
            auto it = first_index.find(name);
            if (cluster.index.count(name) && it != first_index.end()) stable = stable && it->second == at && cluster.index.at(name) == at;
            if (!cluster.index.count(name) || it == first_index.end()) first_index[name] = at;
        }
        CHECK(stable);
        cluster = next_cluster;
    }
    CHECK(rebuilt >= 60 && joined >= 20 && left >= 20 && rejoined >= 5);
}

static void TestCarriedEntriesKeepARowFromANewcomer() {
    std::vector<Node> nodes = {NewNode("a", "az-a", 16, 64), NewNode("b", "az-a", 16, 64), NewNode("c", "az-a", 16, 64)};
    FlatCluster c0, c1, with, without;
    std::string err;
    std::vector<uint32_t> rows;
    CHECK(FlatCluster::BuildWithSpare(nodes, 2, &c0, &err));
    const uint32_t b = c0.index.at("b");
    FlatReservations carried;  // "b" carries a reservation
    carried.node = {b};
    for (int j = 0; j < 3; ++j) carried.req[j] = {1000};
    nodes.erase(nodes.begin() + 1);  // b leaves
    CHECK(FlatCluster::Rebuild(c0, nodes, &carried, &c1, &rows, &err));
    CHECK(c1.isAbsent(b) && c1.index.count("b") == 0 && rows == std::vector<uint32_t>{b} && c1.alloc[0][b] == 0 && c1.base_flags[b] == 0);
    CHECK(c1.ranks_changed);  // (c moves up a rank)
    nodes.push_back(NewNode("d", "az-a", 32, 128));  // d joins: b's row is the lowest absent one, and the stale entry still names it
    CHECK(FlatCluster::Rebuild(c1, nodes, &carried, &with, &rows, &err));
    CHECK(with.index.at("d") == 3 && with.isAbsent(b) && rows == std::vector<uint32_t>{3});
    CHECK(FlatCluster::Rebuild(c1, nodes, nullptr, &without, &rows, &err));  // the list was rebuilt since: nothing names the row
    CHECK(without.index.at("d") == b && rows == std::vector<uint32_t>{b});
    // b comes back while its row still stands empty: it is a newcomer like any other (the lowest free row)
    nodes.push_back(NewNode("b", "az-a", 16, 64));
    FlatCluster back;
    CHECK(FlatCluster::Rebuild(with, nodes, nullptr, &back, &rows, &err));
    CHECK(back.index.at("b") == b && back.index.at("d") == 3 && back.present.size() == 1 && back.present[0] == 0xF);
}

static void TestWhatRebuildRefuses() {
    std::vector<Node> nodes = {NewNode("a", "az-a", 16, 64), NewNode("b", "az-b", 16, 64)};
    FlatCluster c0, out;
    std::string err;
    std::vector<uint32_t> rows;
    CHECK(FlatCluster::BuildWithSpare(nodes, 1, &c0, &err));
    out.version = 777;
    // ---- spare exhaustion: two newcomers, one absent row
    std::vector<Node> two_more = nodes;
    two_more.push_back(NewNode("c", "az-a", 16, 64));
    two_more.push_back(NewNode("d", "az-b", 16, 64));
    CHECK(!FlatCluster::Rebuild(c0, two_more, nullptr, &out, &rows, &err) && err.find("no absent row is free") != std::string::npos);
    // ... and one newcomer whose only row a carried entry names
    two_more.pop_back();
    FlatReservations carried;
    carried.node = {2};
    for (int j = 0; j < 3; ++j) carried.req[j] = {0};
    CHECK(!FlatCluster::Rebuild(c0, two_more, &carried, &out, &rows, &err) && err.find("no absent row is free") != std::string::npos);
    CHECK(FlatCluster::Rebuild(c0, two_more, nullptr, &out, &rows, &err) && out.present.empty());
    out = FlatCluster();
    out.version = 777;
    // ---- a changed set of zone labels: a new label, and a label whose last node left
    std::vector<Node> new_label = nodes;
    new_label.push_back(NewNode("c", "az-c", 16, 64));
    CHECK(!FlatCluster::Rebuild(c0, new_label, nullptr, &out, &rows, &err) && err.find("zone labels") != std::string::npos);
    const std::vector<Node> one_label = {nodes[0]};
    CHECK(!FlatCluster::Rebuild(c0, one_label, nullptr, &out, &rows, &err) && err.find("zone labels") != std::string::npos);
    std::vector<Node> swapped = {nodes[0], NewNode("b", "az-c", 16, 64)};  // as many labels, another set
    CHECK(!FlatCluster::Rebuild(c0, swapped, nullptr, &out, &rows, &err));
    // ---- a quantity that is not exactly representable, a duplicate name
    std::vector<Node> micro = nodes;
    micro[1].Allocatable[kResourceCPU] = Quantity::FromNano(1500);
    CHECK(!FlatCluster::Rebuild(c0, micro, nullptr, &out, &rows, &err) && err.find("not exactly representable") != std::string::npos);
    std::vector<Node> twice = nodes;
    twice.push_back(nodes[0]);
    CHECK(!FlatCluster::Rebuild(c0, twice, nullptr, &out, &rows, &err));
    CHECK(out.version == 777 && out.names.empty());  // a refusal leaves *out alone
    // ---- nothing changed: no row, the ranks stand
    CHECK(FlatCluster::Rebuild(c0, nodes, nullptr, &out, &rows, &err) && rows.empty() && !out.ranks_changed && out.derived_from == c0.version);
}

// ------------------------------------------------------------------------------------------------ through the device
static Pod Driver(const std::string& app, const std::string& group, int k, const char* emem, const char* ecpu, int64_t created_s) {
    Pod p;
    p.Name = app + "-spark-driver";
    p.Namespace = "namespace";
    p.labels = {{common::SparkRoleLabel, common::Driver}, {common::SparkAppIDLabel, app}};
    p.Annotations = {{"spark-driver-cpu", "1"},    {"spark-driver-mem", "2Gi"}, {"spark-executor-cpu", ecpu},
                     {"spark-executor-mem", emem}, {"spark-executor-count", std::to_string(k)}};
    p.SchedulerName = common::SparkSchedulerName;
    p.InstanceGroup = group;
    p.CreationTimestampNanos = created_s * 1000000000;
    return p;
}

static Pod Executor(const std::string& app, int i) {
    Pod p;
    p.Name = app + "-spark-exec-" + std::to_string(i);
    p.Namespace = "namespace";
    p.labels = {{common::SparkRoleLabel, common::Executor}, {common::SparkAppIDLabel, app}};
    p.SchedulerName = common::SparkSchedulerName;
    p.Phase = "Pending";
    return p;
}

static bool SameAnswer(const SelectNodeResult& got, const SelectNodeResult& w) {
    bool same = got.served && w.served && got.outcome == w.outcome && got.node == w.node && got.created.has_value() == w.created.has_value();
    if (same && got.created) {
        same = got.created->Reservations.size() == w.created->Reservations.size();
        for (const auto& [name, res] : w.created->Reservations)
            same = same && got.created->Reservations.count(name) && got.created->Reservations.at(name).Node == res.Node;
    }
    // the efficiency averages over every metadata key: an absent row that became one would move it (the sums run over the keys in
    // index order, which differs between the two clusters: equal up to the rounding of a sum of doubles)
    same = same && got.has_efficiency == w.has_efficiency;
    if (same && got.has_efficiency)
        same = std::fabs(got.efficiency.CPU - w.efficiency.CPU) < 1e-9 && std::fabs(got.efficiency.Memory - w.efficiency.Memory) < 1e-9 &&
               std::fabs(got.efficiency.Max - w.efficiency.Max) < 1e-9;
    return same;
}

// The cluster state both extenders are given, and what the groups are.
struct World {
    std::vector<Node> nodes;
    std::map<std::string, std::string> group_of;  // node name -> instance group
    std::map<std::string, std::vector<Node>> groupNodes() const {
        std::map<std::string, std::vector<Node>> out;
        for (const Node& nd : nodes) out[group_of.at(nd.Name)].push_back(nd);
        return out;
    }
};

static void TestFiltersScansAndReconcilesAcrossNodeChanges() {
    const char* group_names[] = {"group-a", "group-b", "group-c"};
    gf_ctx* fresh_ctx = nullptr;
    CHECK(gf_init(nullptr, 0, &fresh_ctx) == GF_OK);
    if (fresh_ctx == nullptr) return;
    for (const char* packer : {"tightly-pack", "single-az-tightly-pack"}) {
        World w;
        SparkSchedulerExtender ext(SelectBinpacker(packer, g_ctx), NodeSorter(), true, FifoConfig{});
        int serial = 0;
        auto add_node = [&](const char* group) {
            Node nd = RandomNode("n" + std::to_string(next() % 100000) + "-" + std::to_string(serial));
            nd.CreationTimestamp = 1000 + (int64_t)(next() % 500);
            ++serial;
            w.group_of[nd.Name] = group;
            w.nodes.push_back(nd);
            ext.overhead[nd.Name] = Resources{Quantity::FromMilli(100 + 50 * (int64_t)(next() % 20)),
                                              Quantity::FromInt((int64_t)(256 + 128 * (next() % 16)) * Mi), Quantity()};
            return nd.Name;
        };
        for (int i = 0; i < 150; ++i) add_node(i < 50 ? group_names[0] : (i % 4 == 0 ? group_names[2] : group_names[1]));
        for (int r = 0; r < 30; ++r) {  // running applications, spread over every group
            ResourceReservation rr;
            rr.Name = "running-" + std::to_string(r);
            rr.Namespace = "namespace";
            const int k = 1 + (int)(next() % 10);
            for (int e = 0; e <= k; ++e) {
                Reservation res;
                res.Node = w.nodes[next() % w.nodes.size()].Name;
                res.Resources = {{kResourceCPU, Quantity::FromInt(1 + (int64_t)(next() % 2))},
                                 {kResourceMemory, Quantity::FromInt((int64_t)(2 + next() % 6) * Gi)},
                                 {kResourceNvidiaGPU, Quantity::FromInt(0)}};
                rr.Reservations[e == 0 ? "driver" : executorReservationName(e - 1)] = res;
            }
            ext.reservations.push_back(rr);
        }
        const char* ecpu[] = {"1", "2", "4"};
        const char* emem[] = {"4Gi", "8Gi", "16Gi"};
        const int n_pending = 18;
        for (int p = 0; p < n_pending; ++p) {
            Pod pod = Driver("pending-" + std::to_string(p), group_names[p % 3], 1 + (int)(next() % 30), emem[next() % 3], ecpu[next() % 3], p + 1);
            pod.UID = "uid-" + std::to_string(p);
            pod.ResourceVersion = 100 + (uint64_t)p;
            ext.pods.push_back(pod);
        }
        ext.nowNanos = (int64_t)(n_pending + 700) * 1000000000;
        NodeGroupResources nonSchedulable;
        for (size_t i = 0; i < w.nodes.size(); i += 3) nonSchedulable[w.nodes[i].Name] = ext.overhead[w.nodes[i].Name];
        // the node that will leave while it carries a reservation, and the reservation list whose version must stand
        const std::string leaver = ext.reservations[0].Reservations.at("driver").Node;
        ext.nodes = w.nodes;
        FlatCluster cluster;
        FlatReservations flat;
        std::string err;
        CHECK(FlatCluster::BuildWithSpare(w.nodes, 16, &cluster, &err));
        CHECK(FlatReservations::Build(ext.reservations, ext.softReservationUsage, cluster, &flat, &err));
        const uint64_t flat_version = flat.version;
        const uint32_t leaver_row = cluster.index.at(leaver);

        // every question of one stage, asked of the resident extender on `cluster` and of a fresh extender on a fresh Build
        auto stage = [&](const char* what) {
            ext.nodes = w.nodes;
            const auto groups = w.groupNodes();
            std::map<std::string, std::vector<std::string>> group_node_names;
            for (const auto& [g, nodes] : groups)
                for (const Node& nd : nodes) group_node_names[g].push_back(nd.Name);
            FlatOverhead over;
            CHECK(FlatOverhead::Build(ext.overhead, cluster, &over, &err));
            SparkSchedulerExtender fresh(SelectBinpacker(packer, fresh_ctx), NodeSorter(), true, FifoConfig{});
            fresh.nodes = w.nodes;
            fresh.pods = ext.pods;
            fresh.reservations = ext.reservations;
            fresh.overhead = ext.overhead;
            fresh.nowNanos = ext.nowNanos;
            FlatCluster fcluster;
            FlatReservations fflat;
            FlatOverhead fover;
            CHECK(FlatCluster::Build(w.nodes, &fcluster, &err));
            CHECK(FlatReservations::Build(fresh.reservations, fresh.softReservationUsage, fcluster, &fflat, &err));
            CHECK(FlatOverhead::Build(fresh.overhead, fcluster, &fover, &err));
            // ---- group Filters, the groups alternating
            int placed = 0;
            for (int p = n_pending - 1; p >= n_pending - 6; --p) {
                const Pod& d = ext.pods[(size_t)p];
                const std::string& g = d.InstanceGroup;
                const SelectNodeResult got = ext.selectDriverNodeFlatGroup(g, d, group_node_names[g], cluster, groups.at(g), &flat, &over);
                const SelectNodeResult want = fresh.selectDriverNodeFlatGroup(g, d, group_node_names[g], fcluster, groups.at(g), &fflat, &fover);
                if (!SameAnswer(got, want))
                    std::printf("   %s %s %s: resident (%d %s %s %s) fresh (%d %s %s)\n", packer, what, d.Name.c_str(), (int)got.served,
                                got.outcome.c_str(), got.node.c_str(), got.error.c_str(), (int)want.served, want.outcome.c_str(), want.node.c_str());
                CHECK(SameAnswer(got, want));
                placed += got.node.empty() ? 0 : 1;
            }
            CHECK(placed >= 1);
            // ---- the marker's scan of every group
            bool served = false, resident = false, fserved = false, fresident = false;
            const auto scan = ext.scanForUnschedulablePodsAllGroups(ext.pods, 600ll * 1000000000, cluster, groups, nonSchedulable, &served, &err, &resident);
            const auto fscan = fresh.scanForUnschedulablePodsAllGroups(fresh.pods, 600ll * 1000000000, fcluster, groups, nonSchedulable, &fserved,
                                                                      &err, &fresident);
            CHECK(served && resident && fserved && fresident && scan.size() == ext.pods.size() && scan == fscan);
            // ---- an executor Filter, offered group-b's nodes
            Pod xdriver = Driver("dyn", "group-b", 0, "8Gi", "2", 1);
            xdriver.Annotations.erase("spark-executor-count");
            xdriver.Annotations["spark-dynamic-allocation-enabled"] = "true";
            xdriver.Annotations["spark-dynamic-allocation-min-executor-count"] = "0";
            xdriver.Annotations["spark-dynamic-allocation-max-executor-count"] = "4";
            xdriver.NodeName = group_node_names["group-b"][3];
            xdriver.Phase = "Running";
            bool took = false, ftook = false;
            const SelectNodeResult x = ext.rescheduleExecutorFlat(Executor("dyn", 0), xdriver, {xdriver}, group_node_names["group-b"], {}, true, cluster,
                                                                  &flat, &over, &took);
            const SelectNodeResult fx = fresh.rescheduleExecutorFlat(Executor("dyn", 0), xdriver, {xdriver}, group_node_names["group-b"], {}, true,
                                                                     fcluster, &fflat, &fover, &ftook);
            CHECK(took && ftook && x.served && !x.node.empty() && x.node == fx.node && x.outcome == fx.outcome);
            // ---- the reconciler's findNodes for every group (an absent row belongs to no group and was never created)
            auto reconcile = [&](gf_ctx* ctx, const FlatCluster& c, bool* route) {
                std::vector<std::string> node_group(c.names.size());
                std::vector<int64_t> created(c.names.size(), 0);
                for (const Node& nd : w.nodes) {
                    node_group[c.index.at(nd.Name)] = w.group_of.at(nd.Name);
                    created[c.index.at(nd.Name)] = nd.CreationTimestamp;
                }
                std::vector<FindNodesRequest> requests;
                std::vector<std::string> request_group;
                for (int q = 0; q < 9; ++q) {
                    requests.push_back({2 + 3 * q, Resources{Quantity::FromInt(1 + q % 3), Quantity::FromInt((int64_t)(2 + q) * Gi), Quantity()}});
                    request_group.push_back(group_names[q % 3]);
                }
                std::map<std::string, NodeGroupResources> available;
                return findNodesForStaleApplicationsResident(ctx, c, node_group, created, request_group, requests, &available, route);
            };
            bool rroute = false, froute = false;
            const std::vector<FindNodesResult> rec = reconcile(g_ctx, cluster, &rroute), frec = reconcile(fresh_ctx, fcluster, &froute);
            CHECK(rroute && froute && rec.size() == frec.size());
            bool same = rec.size() == frec.size();
            size_t names = 0;
            for (size_t q = 0; same && q < rec.size(); ++q) {
                same = rec[q].served && frec[q].served && rec[q].executorNodeNames == frec[q].executorNodeNames &&
                       rec[q].reserved.size() == frec[q].reserved.size();
                for (const auto& [node, res] : frec[q].reserved) same = same && rec[q].reserved.count(node) && rec[q].reserved.at(node).Eq(res);
                names += rec[q].executorNodeNames.size();
            }
            CHECK(same && names > 0);
            // ---- and what the resident extender sent so far: one full set, one replay of the reservation list
            CHECK(flat.version == flat_version);
            CHECK(ext.clusterSetCalls() == 1 && ext.usageReplayCalls() == 1);
        };
        auto rebuild = [&](size_t rows_expected_at_least) {
            FlatCluster next_cluster;
            std::vector<uint32_t> rows;
            CHECK(FlatCluster::Rebuild(cluster, w.nodes, &flat, &next_cluster, &rows, &err));
            CHECK(rows.size() >= rows_expected_at_least && rows.size() <= 8);
            cluster = next_cluster;
        };
        auto node_named = [&](const std::string& name) -> Node& {
            for (Node& nd : w.nodes)
                if (nd.Name == name) return nd;
            std::abort();
        };

        stage("as installed");
        CHECK(ext.clusterUpdateCalls() == 0);
        // ---- join: three nodes, one per group
        for (const char* g : group_names) add_node(g);
        rebuild(3);
        stage("three nodes joined");
        CHECK(ext.clusterUpdateCalls() == 1 && ext.clusterRowsSent() == 3);
        // ---- leave: a node that carries a reservation (the list keeps naming its row) and another one
        uint64_t updates = ext.clusterUpdateCalls();
        for (const std::string& gone : {leaver, w.nodes[70].Name == leaver ? w.nodes[71].Name : w.nodes[70].Name}) {
            w.nodes.erase(std::find_if(w.nodes.begin(), w.nodes.end(), [&](const Node& nd) { return nd.Name == gone; }));
            ext.overhead.erase(gone);
        }
        rebuild(2);
        CHECK(cluster.isAbsent(leaver_row));
        stage("two nodes left");
        CHECK(ext.clusterUpdateCalls() == updates + 1);
        // ---- a newcomer must not land on the row the stale reservation names
        const std::string newcomer = add_node("group-a");
        rebuild(1);
        CHECK(cluster.isAbsent(leaver_row) && cluster.index.at(newcomer) != leaver_row);
        stage("a node joined behind a leaver");
        // ---- cordon and NotReady
        updates = ext.clusterUpdateCalls();
        node_named(w.nodes[5].Name).Unschedulable = true;
        node_named(w.nodes[60].Name).Unschedulable = true;
        node_named(w.nodes[90].Name).Ready = false;
        rebuild(3);
        stage("two nodes cordoned, one NotReady");
        CHECK(ext.clusterUpdateCalls() == updates + 1);
        // ---- resize: up, down
        node_named(w.nodes[7].Name).Allocatable[kResourceMemory] = Quantity::FromInt(512 * Gi);
        node_named(w.nodes[61].Name).Allocatable[kResourceCPU] = Quantity::FromInt(4);
        node_named(w.nodes[91].Name).Allocatable[kResourceMemory] = Quantity::FromInt(8 * Gi);
        rebuild(3);
        stage("three nodes resized");
        // ---- nothing changed but the version: no row travels, nothing is set again
        updates = ext.clusterRowsSent();
        rebuild(0);
        stage("a rebuild that changed nothing");
        CHECK(ext.clusterRowsSent() == updates);
        // ---- most of the cluster changes: the full set is cheaper, and the usage replays behind it
        for (size_t i = 0; i < w.nodes.size(); ++i)
            if (i % 3 != 0) w.nodes[i].Allocatable[kResourceCPU] = Quantity::FromInt(24 + (int64_t)(i % 5));
        FlatCluster most;
        std::vector<uint32_t> rows;
        CHECK(FlatCluster::Rebuild(cluster, w.nodes, &flat, &most, &rows, &err) && rows.size() > cluster.names.size() / 2);
        cluster = most;
        ext.nodes = w.nodes;
        const auto groups = w.groupNodes();
        std::vector<std::string> a_names;
        for (const Node& nd : groups.at("group-a")) a_names.push_back(nd.Name);
        FlatOverhead over;
        CHECK(FlatOverhead::Build(ext.overhead, cluster, &over, &err));
        CHECK(ext.selectDriverNodeFlatGroup("group-a", ext.pods[0], a_names, cluster, groups.at("group-a"), &flat, &over).served);
        CHECK(ext.clusterSetCalls() == 2 && ext.usageReplayCalls() == 2);
    }
    gf_destroy(fresh_ctx);
}

static void CpuHalf() {
    TestBuildWithSpare();
    TestJoinLeaveRejoinSequences();
    TestCarriedEntriesKeepARowFromANewcomer();
    TestWhatRebuildRefuses();
}

static void GpuHalf() { TestFiltersScansAndReconcilesAcrossNodeChanges(); }

int main(int argc, char** argv) { return RunHostTests(argc, argv, CpuHalf, GpuHalf); }
