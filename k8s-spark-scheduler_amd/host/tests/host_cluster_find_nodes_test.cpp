// host_cluster_find_nodes_test.cpp — the failover reconciler's findNodes for every instance group from the resident cluster
// (findNodesForStaleApplicationsResident -> gf_cluster_find_nodes): the same names, `reserved` maps and availableResources
// afterwards as one findNodesForStaleApplications per group (which installs) and as a literal map-keyed findNodes written here from
// failover.go:412-436; a refused call falls back; the driver Filter behind a resident reconcile resumes its chain.
// `host_cluster_find_nodes_test cpu` needs no GPU (the rows and create_rank the mirror builds for a three-group cluster);
// `host_cluster_find_nodes_test gpu` drives the device through the C ABI.  Exit code 0 = all passed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#define HOST_TEST_SEED 0xF1AD
#include "failover.hpp"
#include "host_test_common.hpp"

static const char* kGroups[] = {"group-a", "group-b", "group-c"};

// ---- the literal: findNodes (failover.go:412-436) and the loop around it (:132-160), on the reference's map shapes
static std::pair<std::vector<std::string>, NodeGroupResources> LiteralFindNodes(int executorCount, const Resources& executorResources,
                                                                                 const NodeGroupResources& availableResources,
                                                                                 const std::vector<Node>& orderedNodes) {
    std::vector<std::string> executorNodeNames;
    NodeGroupResources reserved;
    for (const Node& n : orderedNodes) {
        if (!reserved.count(n.Name)) reserved[n.Name] = Resources::Zero();
        for (;;) {
            reserved[n.Name].Add(executorResources);
            if (reserved[n.Name].GreaterThan(availableResources.at(n.Name))) break;  // (the add is not taken back)
            executorNodeNames.push_back(n.Name);
            if ((int)executorNodeNames.size() == executorCount) return {executorNodeNames, reserved};
        }
    }
    return {executorNodeNames, reserved};
}

// availableResourcesPerInstanceGroup's node lists (failover.go:286-314): newest first, ready and schedulable, by instance group
static std::map<std::string, std::vector<Node>> LiteralOrderedNodes(std::vector<Node> nodes, const std::map<std::string, std::string>& group_of) {
    std::stable_sort(nodes.begin(), nodes.end(), [](const Node& a, const Node& b) { return a.CreationTimestamp > b.CreationTimestamp; });
    std::map<std::string, std::vector<Node>> out;
    for (const Node& n : nodes)
        if (!n.Unschedulable && n.Ready) out[group_of.at(n.Name)].push_back(n);
    return out;
}

struct Cluster {
    std::vector<Node> nodes;
    std::map<std::string, std::string> group_of;
    std::vector<std::string> node_group;  // by node index
    std::vector<int64_t> created;
};

static Cluster ThreeGroups(int n) {
    Cluster c;
    const char* zones[] = {"az-a", "az-b", "az-c"};
    for (int i = 0; i < n; ++i) {
        Node nd;
        nd.Name = "n" + std::to_string(next() % 100000) + "-" + std::to_string(i);
        nd.labels[kLabelZoneFailureDomain] = zones[next() % 3];
        nd.Allocatable = {{kResourceCPU, Quantity::FromInt(8 + 8 * (int64_t)(next() % 3))},
                          {kResourceMemory, Quantity::FromInt((int64_t)(32 + 32 * (next() % 3)) * Gi)},
                          {kResourceNvidiaGPU, Quantity::FromInt(next() % 6 == 0 ? 2 : 0)}};
        nd.Ready = next() % 15 != 0;
        nd.Unschedulable = next() % 20 == 0;
        nd.CreationTimestamp = 1000 + (int64_t)(next() % 40);  // many ties: the input order breaks them
        // a contiguous third, and two dealt node by node; group-c is the smallest
        const char* g = i < n / 3 ? kGroups[0] : (i % 4 == 0 ? kGroups[2] : kGroups[1]);
        c.group_of[nd.Name] = g;
        c.node_group.push_back(g);
        c.created.push_back(nd.CreationTimestamp);
        c.nodes.push_back(nd);
    }
    return c;
}

struct Stale {
    std::vector<FindNodesRequest> requests;
    std::vector<std::string> group;
};

static Stale StaleApplications(int per_group) {
    Stale s;
    const int64_t cpu[] = {1, 2, 4}, mem[] = {2, 8, 16};
    for (int i = 0; i < 3 * per_group; ++i) {  // the groups interleaved
        FindNodesRequest r;
        r.executorCount = 1 + (int)(next() % 40);
        r.executorResources = Resources::Create(cpu[next() % 3], mem[next() % 3] * Gi, next() % 7 == 0 ? 1 : 0);
        s.requests.push_back(r);
        s.group.push_back(kGroups[i % 3]);
    }
    s.requests[0].executorCount = 100000;  // more than its group holds: a partial answer
    s.requests.push_back({3, Resources::Create(1, Gi, 0)});
    s.group.push_back("group-nobody");  // a group without a node
    return s;
}

static bool SameMap(const NodeGroupResources& a, const NodeGroupResources& b) {
    if (a.size() != b.size()) return false;
    for (const auto& [name, r] : a)
        if (!b.count(name) || !b.at(name).Eq(r)) return false;
    return true;
}

// the literal reconcile: every request on its group's table, in order; the tables afterwards in *available
static std::vector<FindNodesResult> LiteralReconcile(const Cluster& c, const Stale& s, std::map<std::string, NodeGroupResources>* available) {
    const std::map<std::string, std::vector<Node>> ordered = LiteralOrderedNodes(c.nodes, c.group_of);
    std::vector<FindNodesResult> out(s.requests.size());
    for (size_t q = 0; q < s.requests.size(); ++q) {
        const std::vector<Node> none;
        const auto it = ordered.find(s.group[q]);
        auto [names, reserved] = LiteralFindNodes(s.requests[q].executorCount, s.requests[q].executorResources, (*available)[s.group[q]],
                                                  it == ordered.end() ? none : it->second);
        for (const auto& [node, r] : reserved) (*available)[s.group[q]][node].Sub(r);
        out[q].executorNodeNames = names;
        out[q].reserved = reserved;
    }
    return out;
}

static int Differences(const std::vector<FindNodesResult>& got, const std::vector<FindNodesResult>& want, const char* what) {
    int bad = got.size() == want.size() ? 0 : 1;
    for (size_t q = 0; q < got.size() && q < want.size(); ++q)
        if (!got[q].served || got[q].executorNodeNames != want[q].executorNodeNames || !SameMap(got[q].reserved, want[q].reserved)) {
            ++bad;
            std::printf("   %s: request %zu differs (served %d, %zu names against %zu, %zu entries against %zu) %s\n", what, q,
                        (int)got[q].served, got[q].executorNodeNames.size(), want[q].executorNodeNames.size(), got[q].reserved.size(),
                        want[q].reserved.size(), got[q].error.c_str());
        }
    return bad;
}

static bool SameTables(const std::map<std::string, NodeGroupResources>& a, const std::map<std::string, NodeGroupResources>& b) {
    for (const char* g : kGroups)
        if (!a.count(g) || !b.count(g) || !SameMap(a.at(g), b.at(g))) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------ no device
static void TestTheRowsAndTheRanksOfThreeGroups() {
    const int n = 150;  // three words per row, 22 bits used in the last
    const Cluster c = ThreeGroups(n);
    const Stale s = StaleApplications(4);
    const ReconcileRows rows = buildReconcileRows(c.node_group, c.created, s.group);
    CHECK(rows.groups.size() == 4 && rows.groups[0] == "group-a" && rows.groups[3] == "group-nobody");
    CHECK(rows.words_per_row == 3 && rows.words.size() == 12 && rows.create_rank.size() == (size_t)n && rows.req_set.size() == s.group.size());
    // every node in exactly its group's row, nothing at or beyond n, the request-only group's row empty
    int wrong = 0;
    for (size_t r = 0; r < rows.groups.size(); ++r)
        for (int i = 0; i < 192; ++i) {
            const bool bit = (rows.words[r * 3 + (size_t)i / 64] >> (i % 64)) & 1u;
            wrong += bit != (i < n && c.node_group[(size_t)i] == rows.groups[r]) ? 1 : 0;
        }
    CHECK(wrong == 0);
    for (size_t q = 0; q < s.group.size(); ++q) CHECK(rows.groups[rows.req_set[q]] == s.group[q]);
    // the visiting order is a permutation, newest first, ties in input order; create_rank is its inverse
    std::vector<int> seen((size_t)n, 0);
    for (int p = 0; p < n; ++p) {
        const uint32_t node = rows.visit[(size_t)p];
        CHECK(node < (uint32_t)n && rows.create_rank[node] == (uint32_t)p);
        if (node < (uint32_t)n) ++seen[node];
        if (p > 0) {
            const uint32_t before = rows.visit[(size_t)p - 1];
            CHECK(c.created[before] > c.created[node] || (c.created[before] == c.created[node] && before < node));
        }
    }
    CHECK(std::count(seen.begin(), seen.end(), 1) == n);
    // the rows and ranks name the reference's lists: a row's ready, schedulable members in visiting order are
    // availableResourcesPerInstanceGroup's schedulableNodes[instanceGroup]
    const std::map<std::string, std::vector<Node>> ordered = LiteralOrderedNodes(c.nodes, c.group_of);
    for (size_t r = 0; r < 3; ++r) {
        std::vector<std::string> mine, theirs;
        for (const uint32_t node : rows.visit)
            if (((rows.words[r * 3 + node / 64] >> (node % 64)) & 1u) && c.nodes[node].Ready && !c.nodes[node].Unschedulable)
                mine.push_back(c.nodes[node].Name);
        for (const Node& nd : ordered.at(rows.groups[r])) theirs.push_back(nd.Name);
        CHECK(mine == theirs && !mine.empty());
    }
    // ... and the literal findNodes keeps the failing add: 2 executors of 3 cpu on a node of 4, then the next node
    NodeGroupResources avail = {{"x", Resources::Create(4, 10 * Gi, 0)}, {"y", Resources::Create(8, 10 * Gi, 0)}};
    Node x, y;
    x.Name = "x";
    y.Name = "y";
    auto [names, reserved] = LiteralFindNodes(2, Resources::Create(3, Gi, 0), avail, {x, y});
    CHECK(names == (std::vector<std::string>{"x", "y"}));
    CHECK(reserved.at("x").Eq(Resources::Create(6, 2 * Gi, 0)) && reserved.at("y").Eq(Resources::Create(3, Gi, 0)));
}

// ------------------------------------------------------------------------------------------------ through the device
static std::map<std::string, NodeGroupResources> AvailablePerGroup(const SparkSchedulerExtender& ext, const Cluster& c) {
    // availableResourcesPerInstanceGroup (failover.go:315-321): allocatable - (reservation usage + overhead + soft reservations)
    NodeGroupResources usage = UsageForNodes(ext.reservations);
    for (const auto& [node, r] : ext.softReservationUsage) usage[node].Add(r);
    const NodeGroupSchedulingMetadata meta = NodeSchedulingMetadataForNodes(ext.nodes, usage, ext.overhead);
    std::map<std::string, NodeGroupResources> out;
    for (const char* g : kGroups) out[g];
    for (const Node& nd : ext.nodes)
        if (nd.Ready && !nd.Unschedulable) out[c.group_of.at(nd.Name)][nd.Name] = meta.at(nd.Name).AvailableResources;
    return out;
}

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

static void TestTheResidentReconcileOfThreeGroups() {
    const int n = 300, n_pending = 24;
    const Cluster c = ThreeGroups(n);
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", g_ctx), NodeSorter(), true, FifoConfig{});
    ext.nodes = c.nodes;
    std::map<std::string, std::vector<Node>> groups;
    std::map<std::string, std::vector<std::string>> group_node_names;
    for (const Node& nd : c.nodes) {
        groups[c.group_of.at(nd.Name)].push_back(nd);
        group_node_names[c.group_of.at(nd.Name)].push_back(nd.Name);
        if (next() % 4 != 0)
            ext.overhead[nd.Name] = Resources{Quantity::FromMilli(100 + 250 * (int64_t)(next() % 20)),
                                              Quantity::FromInt((int64_t)(256 + 1024 * (next() % 16)) * Mi), Quantity()};
    }
    for (int r = 0; r < 60; ++r) {
        ResourceReservation rr;
        rr.Name = "running-" + std::to_string(r);
        rr.Namespace = "namespace";
        const int k = 1 + (int)(next() % 12);
        for (int e = 0; e <= k; ++e) {
            Reservation res;
            res.Node = ext.nodes[next() % n].Name;
            res.Resources = {{kResourceCPU, Quantity::FromInt(1 + (int64_t)(next() % 3))},
                             {kResourceMemory, Quantity::FromInt((int64_t)(2 + next() % 14) * Gi)},
                             {kResourceNvidiaGPU, Quantity::FromInt(0)}};
            rr.Reservations[e == 0 ? "driver" : executorReservationName(e - 1)] = res;
        }
        ext.reservations.push_back(rr);
    }
    ext.softReservationUsage[ext.nodes[7].Name] = Resources::Create(1, 2 * Gi, 0);
    for (int p = 0; p < n_pending; ++p) {
        Pod pod = Driver("pending-" + std::to_string(p), "group-b", 1 + (int)(next() % 30), "8Gi", "2", p + 1);
        pod.UID = "uid-" + std::to_string(p);
        pod.ResourceVersion = 100 + (uint64_t)p;
        ext.pods.push_back(pod);
    }
    ext.nowNanos = (int64_t)(n_pending + 700) * 1000000000;
    FlatCluster cluster;
    FlatReservations flat;
    FlatOverhead over;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    CHECK(FlatReservations::Build(ext.reservations, ext.softReservationUsage, cluster, &flat, &err));
    CHECK(FlatOverhead::Build(ext.overhead, cluster, &over, &err));
    const Stale s = StaleApplications(8);
    const std::map<std::string, NodeGroupResources> start = AvailablePerGroup(ext, c);

    // ---- a refused call falls back: nothing is resident on this context yet (GF_ERR_STATE), the per-group route answers
    std::map<std::string, NodeGroupResources> lit_tables = start;
    const std::vector<FindNodesResult> literal = LiteralReconcile(c, s, &lit_tables);
    {
        std::map<std::string, NodeGroupResources> tables = start;
        bool took = true;
        const std::vector<FindNodesResult> got = findNodesForStaleApplicationsResident(g_ctx, cluster, c.node_group, c.created, s.group,
                                                                                       s.requests, &tables, &took);
        CHECK(!took);
        CHECK(Differences(got, literal, "fallback") == 0);
        CHECK(SameTables(tables, lit_tables));
    }
    // the comparison sees a full answer, a partial one, an over-add and a node gone negative
    bool full = false, partial = false, over_add = false;
    for (size_t q = 0; q < literal.size(); ++q) {
        full = full || (int)literal[q].executorNodeNames.size() == s.requests[q].executorCount;
        partial = partial || (int)literal[q].executorNodeNames.size() < s.requests[q].executorCount;
        over_add = over_add || literal[q].reserved.size() > 1;
    }
    bool negative = false;
    for (const auto& [name, r] : lit_tables.at("group-a")) negative = negative || Resources::Zero().GreaterThan(r);
    CHECK(full && partial && over_add && negative);

    // ---- the warm driver Filter: twice, the second resumes
    const Pod& last = ext.pods.back();
    const SelectNodeResult first = ext.selectDriverNodeFlatGroup("group-b", last, group_node_names["group-b"], cluster, groups["group-b"], &flat, &over);
    CHECK(first.served);
    const SelectNodeResult second = ext.selectDriverNodeFlatGroup("group-b", last, group_node_names["group-b"], cluster, groups["group-b"], &flat, &over);
    CHECK(second.served && second.outcome == first.outcome && second.node == first.node);
    uint64_t gen0[3], gen1[3], st[4];
    CHECK(gf_generation(g_ctx, gen0) == GF_OK);

    // ---- the resident reconcile of the three groups in front of it: one call, the literal's answers, nothing moved
    std::map<std::string, NodeGroupResources> res_tables = start;
    bool took = false;
    const std::vector<FindNodesResult> resident = findNodesForStaleApplicationsResident(g_ctx, cluster, c.node_group, c.created, s.group,
                                                                                        s.requests, &res_tables, &took);
    CHECK(took);
    CHECK(Differences(resident, literal, "resident") == 0);
    CHECK(SameTables(res_tables, lit_tables));
    CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0] && gen1[1] == gen0[1] && gen1[2] == gen0[2]);
    CHECK(gf_chain_cache_stats(g_ctx, 1, st) == GF_OK);
    const SelectNodeResult third = ext.selectDriverNodeFlatGroup("group-b", last, group_node_names["group-b"], cluster, groups["group-b"], &flat, &over);
    CHECK(third.served && third.outcome == first.outcome && third.node == first.node);
    CHECK(gf_chain_cache_stats(g_ctx, 0, st) == GF_OK);
    CHECK(st[0] == 1 && st[1] == 1);
    if (!(st[0] == 1 && st[1] == 1))
        std::printf("   chains %llu resumed %llu evaluated %llu skipped %llu\n", (unsigned long long)st[0], (unsigned long long)st[1],
                    (unsigned long long)st[2], (unsigned long long)st[3]);
    CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0]);

    // ---- the per-group route gives the same names, `reserved` and tables — and installs: the snapshot epoch moves
    std::map<std::string, NodeGroupResources> grp_tables = start;
    const std::map<std::string, std::vector<Node>> ordered = LiteralOrderedNodes(c.nodes, c.group_of);
    std::vector<FindNodesResult> per_group(s.requests.size());
    for (const char* g : kGroups) {
        std::vector<FindNodesRequest> mine;
        std::vector<size_t> at;
        for (size_t q = 0; q < s.requests.size(); ++q)
            if (s.group[q] == g) {
                mine.push_back(s.requests[q]);
                at.push_back(q);
            }
        const std::vector<FindNodesResult> got = findNodesForStaleApplications(g_ctx, mine, &grp_tables[g], ordered.at(g));
        for (size_t i = 0; i < at.size(); ++i) per_group[at[i]] = got[i];
    }
    int bad = 0;
    for (size_t q = 0; q + 1 < s.requests.size(); ++q)  // (the last request's group has no node: the per-group route is never asked)
        bad += per_group[q].served && per_group[q].executorNodeNames == resident[q].executorNodeNames &&
                       SameMap(per_group[q].reserved, resident[q].reserved)
                   ? 0
                   : 1;
    CHECK(bad == 0);
    CHECK(resident.back().served && resident.back().executorNodeNames.empty() && resident.back().reserved.empty());
    CHECK(SameTables(grp_tables, res_tables));
    CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] > gen0[0]);
}

static void CpuHalf() { TestTheRowsAndTheRanksOfThreeGroups(); }

static void GpuHalf() { TestTheResidentReconcileOfThreeGroups(); }

int main(int argc, char** argv) { return RunHostTests(argc, argv, CpuHalf, GpuHalf); }
