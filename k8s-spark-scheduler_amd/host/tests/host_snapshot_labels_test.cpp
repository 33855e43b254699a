// host_snapshot_labels_test.cpp — gf_snapshot_build with a prioritized node label (executor-prioritized-node-label: "spot" before
// "on-demand", nodes without the label last) on the cluster of host_test's device check, against the string-keyed host mirror of
// NodeSorter.PotentialNodes, and the route the build reports (gf_snapshot_build_info):
//   - the request's NodeNames drawn independently of the label: whichever route the build took, the reference's two orders;
//   - drivers confined to the on-demand nodes: the slot tables are built on the device, nothing of the cluster's size returns.
// `host_snapshot_labels_test cpu` needs no GPU (the mirror alone: the confined lists share one order); `... gpu` drives the device
// through the C ABI.  Exit code 0 = all passed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <optional>
#include <set>
#include <string>
#include <vector>

#include "host_test_common.hpp"

struct Cluster {
    std::vector<Node> nodes;
    std::vector<std::string> requested;
    std::vector<ResourceReservation> rrs;
    NodeGroupResources overhead;
};

// host_test's cluster (TestDeviceSnapshotBuildAgainstHostMirror), same generator and seed; confined: the request names exactly
// the on-demand nodes
static Cluster MakeCluster(bool confined) {
    const int n = 300;
    uint64_t rng = 0x5EED;
    auto next = [&]() {
        rng += 0x9E3779B97F4A7C15ull;
        uint64_t z = rng;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    const char* zones[] = {"az-a", "az-b", "az-c"};  // ids in label order
    Cluster c;
    for (int i = 0; i < n; ++i) {
        Node nd;
        nd.Name = "node-" + std::to_string(next() % 100000) + "-" + std::to_string(i);
        nd.labels[kLabelZoneFailureDomain] = zones[next() % 3];
        const uint64_t p = next() % 3;
        if (p < 2) nd.labels["pool"] = p == 0 ? "spot" : "on-demand";
        nd.Allocatable = {{kResourceCPU, Quantity::FromInt(8 + 8 * (int64_t)(next() % 3))},
                          {kResourceMemory, Quantity::FromInt((int64_t)(16 + 16 * (next() % 4)) * Gi)},
                          {kResourceNvidiaGPU, Quantity::FromInt(next() % 10 == 0 ? 4 : 0)}};
        nd.Unschedulable = next() % 20 == 0;
        nd.Ready = next() % 20 != 0;
        const bool drawn = next() % 5 != 0;
        if (confined ? p == 1 : drawn) c.requested.push_back(nd.Name);
        c.nodes.push_back(nd);
    }
    for (int r = 0; r < 120; ++r) {
        ResourceReservation rr;
        rr.Name = "app-" + std::to_string(r);
        const int k = 1 + (int)(next() % 9);
        for (int e = 0; e <= k; ++e) {
            Reservation res;
            res.Node = c.nodes[next() % n].Name;
            res.Resources = {{kResourceCPU, Quantity::FromMilli(500 * (int64_t)(1 + next() % 8))},
                             {kResourceMemory, Quantity::FromInt((int64_t)(1 + next() % 8) * Gi)},
                             {kResourceNvidiaGPU, Quantity::FromInt(next() % 30 == 0 ? 1 : 0)}};
            rr.Reservations[e == 0 ? "driver" : executorReservationName(e - 1)] = res;
        }
        c.rrs.push_back(rr);
    }
    for (int i = 0; i < n; i += 3) c.overhead[c.nodes[i].Name] = Resources{Quantity::FromMilli(250), Quantity::FromInt(Gi / 2), Quantity()};
    return c;
}

static std::pair<std::vector<std::string>, std::vector<std::string>> MirrorOrders(const Cluster& c) {
    const LabelPriorityOrder pool{"pool", {"spot", "on-demand"}};
    NodeGroupResources usage = UsageForNodes(c.rrs);
    NodeGroupSchedulingMetadata md = NodeSchedulingMetadataForNodes(c.nodes, usage, c.overhead);
    NodeSorter sorter(std::nullopt, pool);
    return sorter.PotentialNodes(md, c.requested);
}

// the nodes both lists name come in the same relative order
static bool ShareOneOrder(const std::vector<std::string>& D, const std::vector<std::string>& X) {
    const std::set<std::string> d(D.begin(), D.end()), x(X.begin(), X.end());
    std::vector<std::string> cd, cx;
    for (const auto& v : D)
        if (x.count(v)) cd.push_back(v);
    for (const auto& v : X)
        if (d.count(v)) cx.push_back(v);
    return cd == cx;
}

static void TestMirrorConfinedListsShareOneOrder() {
    const Cluster c = MakeCluster(true);
    auto [D, X] = MirrorOrders(c);
    CHECK(!D.empty() && !X.empty());
    CHECK(ShareOneOrder(D, X));
}

static void BuildAndCompare(bool confined) {
    const Cluster c = MakeCluster(confined);
    const int n = (int)c.nodes.size();
    auto [wantD, wantX] = MirrorOrders(c);
    std::vector<std::string> sorted_names;
    for (const Node& nd : c.nodes) sorted_names.push_back(nd.Name);
    std::sort(sorted_names.begin(), sorted_names.end());
    std::map<std::string, uint32_t> index, rank;
    for (int i = 0; i < n; ++i) index[c.nodes[i].Name] = (uint32_t)i;
    for (int i = 0; i < n; ++i) rank[sorted_names[i]] = (uint32_t)i;
    const std::set<std::string> req(c.requested.begin(), c.requested.end());
    std::vector<int64_t> alloc[3], over[3], rreq[3];
    std::vector<uint32_t> flags, zone, name_rank, exec_label, rnode;
    for (const Node& nd : c.nodes) {
        Resources a{nd.Allocatable.at(kResourceCPU), nd.Allocatable.at(kResourceMemory), nd.Allocatable.at(kResourceNvidiaGPU)};
        int64_t v[3], o[3] = {0, 0, 0};
        a.canonical(v);
        if (c.overhead.count(nd.Name)) c.overhead.at(nd.Name).canonical(o);
        for (int j = 0; j < 3; ++j) {
            alloc[j].push_back(v[j]);
            over[j].push_back(o[j]);
        }
        flags.push_back((nd.Unschedulable ? GF_NODE_UNSCHEDULABLE : 0u) | (nd.Ready ? GF_NODE_READY : 0u) |
                        (req.count(nd.Name) ? GF_NODE_DRIVER_CANDIDATE : 0u));
        const std::string& z = nd.labels.at(kLabelZoneFailureDomain);
        zone.push_back(z == "az-a" ? 0u : (z == "az-b" ? 1u : 2u));
        name_rank.push_back(rank.at(nd.Name));
        auto l = nd.labels.find("pool");
        exec_label.push_back(l == nd.labels.end() ? 0xFFFFFFFFu : (l->second == "spot" ? 0u : 1u));
    }
    for (const auto& rr : c.rrs)
        for (const auto& [name, res] : rr.Reservations) {
            rnode.push_back(index.at(res.Node));
            Resources r{res.Resources.at(kResourceCPU), res.Resources.at(kResourceMemory), res.Resources.at(kResourceNvidiaGPU)};
            int64_t v[3];
            r.canonical(v);
            for (int j = 0; j < 3; ++j) rreq[j].push_back(v[j]);
        }
    std::vector<uint32_t> D(n), X(n);
    uint32_t nd = 0, nx = 0;
    const int rc = gf_snapshot_build(g_ctx, n, alloc[0].data(), alloc[1].data(), alloc[2].data(), over[0].data(), over[1].data(),
                                     over[2].data(), (uint32_t)rnode.size(), rnode.data(), rreq[0].data(), rreq[1].data(),
                                     rreq[2].data(), flags.data(), zone.data(), 3, name_rank.data(), nullptr, exec_label.data(),
                                     D.data(), &nd, X.data(), &nx);
    CHECK(rc == GF_OK);
    if (rc != GF_OK) {
        std::printf("   %s\n", gf_last_error(g_ctx));
        return;
    }
    std::vector<std::string> gotD, gotX;
    for (uint32_t i = 0; i < nd; ++i) gotD.push_back(c.nodes[D[i]].Name);
    for (uint32_t i = 0; i < nx; ++i) gotX.push_back(c.nodes[X[i]].Name);
    CHECK(gotD == wantD);
    CHECK(gotX == wantX);
    uint32_t info[4] = {9, 9, 9, 9};
    CHECK(gf_snapshot_build_info(g_ctx, info) == GF_OK);
    CHECK(gf_snapshot_build_info(g_ctx, nullptr) == GF_ERR_INVALID && gf_snapshot_build_info(nullptr, info) == GF_ERR_INVALID);
    std::printf("   %s: route %u, label group %u, fell back %u, %u bytes device -> host\n", confined ? "confined drivers" : "drawn drivers",
                info[0], info[1], info[2], info[3]);
    CHECK(info[1] == 1);  // the label re-sorts something: the sort ran its label group
    CHECK((info[0] == 1 && info[2] == 0) || (info[0] == 2 && info[2] == 1));
    if (!ShareOneOrder(wantD, wantX)) CHECK(info[0] == 2);  // lists that conflict cannot come from one slot order
    if (confined) {
        CHECK(info[0] == 1);
        CHECK(info[3] <= 512);
    } else {
        CHECK((info[0] == 1) == (info[3] <= 512));
    }
    // and a decision on the built snapshot equals the one through the string interface
    NodeGroupResources usage = UsageForNodes(c.rrs);
    NodeGroupSchedulingMetadata md = NodeSchedulingMetadataForNodes(c.nodes, usage, c.overhead);
    Binpacker bp = SelectBinpacker("single-az-tightly-pack", g_ctx);
    gf_app app{};
    Resources::Create(1, 2 * Gi, 0).canonical(app.drv);
    Resources::Create(2, 4 * Gi, 0).canonical(app.exe);
    app.k = 40;
    gf_result res{};
    std::vector<uint32_t> exec(41);
    CHECK(gf_spark_binpack(g_ctx, bp.Algo, &app, &res, exec.data(), 40) == GF_OK);
    PackingResult want = bp.BinpackFunc(Resources::Create(1, 2 * Gi, 0), Resources::Create(2, 4 * Gi, 0), 40, wantD, wantX, md);
    CHECK(want.served && want.HasCapacity == (res.has_capacity != 0));
    if (want.HasCapacity && res.has_capacity) {
        CHECK(c.nodes[res.driver_node].Name == want.DriverNode);
        bool same_exec = true;
        for (int i = 0; i < 40; ++i) same_exec = same_exec && c.nodes[exec[i]].Name == want.ExecutorNodes[i];
        CHECK(same_exec);
    }
}

static void CpuHalf() {
    TestMirrorConfinedListsShareOneOrder();
}

static void GpuHalf() {
    BuildAndCompare(false);
    BuildAndCompare(true);
}

int main(int argc, char** argv) { return RunHostTests(argc, argv, CpuHalf, GpuHalf); }
