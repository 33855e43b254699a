// host_group_filter_test.cpp — driver Filters of several instance groups on ONE resident cluster
// (SparkSchedulerExtender::selectDriverNodeFlatGroup -> gf_snapshot_build_resident_set): a three-group cluster with overhead on
// every node; Filters of the three groups alternate, a scanForUnschedulablePodsAllGroups and a rescheduleExecutorFlat run in
// between; every Filter equals selectDriverNode (the string-map route) on that group's nodes, gf_cluster_set is sent once, and
// the same group's Filter twice in a row does not rebuild.
// `host_group_filter_test cpu` needs no GPU (what the route hands to selectDriverNode before it touches a device, and what the
// three driver Filters refuse before they do);
// `host_group_filter_test gpu` drives the device through the C ABI.  Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#define HOST_TEST_SEED 0x6709
#include "host_test_common.hpp"

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
    return same;
}

static Node NewNode(const std::string& name, const char* zone) {
    Node nd;
    nd.Name = name;
    nd.labels[kLabelZoneFailureDomain] = zone;
    nd.Allocatable = {{kResourceCPU, Quantity::FromInt(16 + 16 * (int64_t)(next() % 3))},
                      {kResourceMemory, Quantity::FromInt((int64_t)(64 + 64 * (next() % 3)) * Gi)},
                      {kResourceNvidiaGPU, Quantity::FromInt(0)}};
    nd.Ready = true;
    return nd;
}

// ------------------------------------------------------------------------------------------------ no device
static void TestWhatNeedsNoDevice() {
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", nullptr), NodeSorter(), true, FifoConfig{});
    ext.nodes = {NewNode("node1", "az-a"), NewNode("node2", "az-b")};
    ext.nowNanos = 1000ll * 1000000000;
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    // a driver whose reservation exists is answered from it, before any device call, by both routes alike
    Pod bound = Driver("bound", "group-a", 2, "1Gi", "1", 1);
    ResourceReservation rr;
    rr.Name = "bound";
    rr.Namespace = "namespace";
    Reservation res;
    res.Node = "node2";
    rr.Reservations["driver"] = res;
    ext.reservations.push_back(rr);
    const std::vector<Node> group = {ext.nodes[1]};
    const SelectNodeResult got = ext.selectDriverNodeFlatGroup("group-a", bound, {"node1", "node2"}, cluster, group);
    const SelectNodeResult want = ext.selectDriverNode("group-a", bound, {"node1", "node2"}, group);
    CHECK(got.served && got.node == "node2" && got.outcome == std::string(outcome::success));
    CHECK(got.node == want.node && got.outcome == want.outcome);
    CHECK(ext.clusterSetCalls() == 0);
}

// What the three driver Filters answer before any device call, each case with the same expectation for selectDriverNode,
// selectDriverNodeFlat and selectDriverNodeFlatGroup.
static void TestRefusalsOfTheDriverFilters() {
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", nullptr), NodeSorter(), true, FifoConfig{});
    ext.nodes = {NewNode("node1", "az-a"), NewNode("node2", "az-b")};
    ext.nowNanos = 1000ll * 1000000000;
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    const std::vector<std::string> names = {"node1", "node2"};
    auto all_three = [&](const Pod& d, auto expected) {
        CHECK(expected(ext.selectDriverNode("group-a", d, names, ext.nodes)));
        CHECK(expected(ext.selectDriverNodeFlat("group-a", d, names, cluster)));
        CHECK(expected(ext.selectDriverNodeFlatGroup("group-a", d, names, cluster, ext.nodes)));
    };
    // ---- an existing reservation answers with the reserved node; one without a "driver" entry with no node
    const Pod reserved = Driver("reserved", "group-a", 2, "1Gi", "1", 5);
    ResourceReservation rr;
    rr.Name = "reserved";
    rr.Namespace = "namespace";
    rr.Reservations["driver"].Node = "node2";
    ext.reservations = {rr};
    all_three(reserved, [](const SelectNodeResult& r) {
        return r.served && r.outcome == std::string(outcome::success) && r.node == "node2" && r.error.empty() && !r.created;
    });
    rr.Reservations.clear();
    rr.Reservations[executorReservationName(0)].Node = "node1";
    ext.reservations = {rr};
    all_three(reserved, [](const SelectNodeResult& r) { return r.served && r.outcome == std::string(outcome::success) && r.node.empty(); });
    ext.reservations.clear();
    // ---- an unparsable current driver: failure-internal with the parse error behind its prefix, and served
    Pod unparsable = Driver("unparsable", "group-a", 2, "1Gi", "1", 5);
    unparsable.Annotations["spark-executor-count"] = "many";
    std::string parse_err;
    CHECK(!sparkResources(unparsable, &parse_err) && !parse_err.empty());
    all_three(unparsable, [&](const SelectNodeResult& r) {
        return r.served && r.node.empty() && r.outcome == std::string(outcome::failureInternal) &&
               r.error == "failed to get spark resources: " + parse_err;
    });
    // ---- an unrepresentable current driver is not served
    const Pod micro = Driver("micro", "group-a", 2, "1Gi", "1500u", 5);
    all_three(micro, [](const SelectNodeResult& r) {
        return !r.served && r.node.empty() && r.error == "application resources are not exactly representable";
    });
    // ---- an unrepresentable earlier driver (FIFO on) is not served either, and is named
    const Pod current = Driver("current", "group-a", 2, "1Gi", "1", 5);
    ext.pods = {Driver("earlier", "group-a", 2, "1Gi", "1500u", 1), current};
    all_three(current, [](const SelectNodeResult& r) {
        return !r.served && r.node.empty() && r.error == "earlier driver earlier-spark-driver is not exactly representable";
    });
    // (the earlier driver is looked at first: the same answer when the current one is unrepresentable too)
    ext.pods.push_back(micro);
    all_three(micro, [](const SelectNodeResult& r) {
        return !r.served && r.error == "earlier driver earlier-spark-driver is not exactly representable";
    });
    CHECK(ext.clusterSetCalls() == 0);
}

// ------------------------------------------------------------------------------------------------ through the device
// "failed to get driver resources, skipping driver" (resource.go:231-237): an earlier driver that cannot be parsed is left out of
// the FIFO replay by the string route and by the flat route alike.  Two nodes, two pods.
static void TestAnUnparsableEarlierDriverIsSkipped() {
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", g_ctx), NodeSorter(), true, FifoConfig{});
    ext.nodes = {NewNode("node1", "az-a"), NewNode("node2", "az-b")};
    ext.nowNanos = 1000ll * 1000000000;
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    const std::vector<std::string> names = {"node1", "node2"};
    Pod earlier = Driver("earlier", "group-a", 2, "1Gi", "1", 1);
    earlier.Annotations["spark-executor-count"] = "many";
    const Pod current = Driver("current", "group-a", 2, "1Gi", "1", 5);
    ext.pods = {earlier, current};
    const SelectNodeResult flat = ext.selectDriverNodeFlat("group-a", current, names, cluster);
    const SelectNodeResult map = ext.selectDriverNode("group-a", current, names, ext.nodes);
    CHECK(map.served && map.outcome == std::string(outcome::success) && !map.node.empty() && map.created.has_value());
    CHECK(SameAnswer(flat, map));
    // alone in the queue the driver gets the same answer: the unparsable one took nothing
    ext.pods = {current};
    CHECK(SameAnswer(ext.selectDriverNode("group-a", current, names, ext.nodes), map));
}

static void TestThreeGroupsOnOneResidentCluster() {
    const int n = 300, n_pending = 36;
    const char* group_names[] = {"group-a", "group-b", "group-c"};
    const char* zones[] = {"az-a", "az-b", "az-c"};
    for (const char* packer : {"tightly-pack", "single-az-tightly-pack"}) {
        SparkSchedulerExtender ext(SelectBinpacker(packer, g_ctx), NodeSorter(), true, FifoConfig{});
        std::vector<std::string> names;
        std::map<std::string, std::vector<Node>> groups;
        std::map<std::string, std::vector<std::string>> group_node_names;
        NodeGroupResources nonSchedulable;
        for (int i = 0; i < n; ++i) {
            Node nd = NewNode("n" + std::to_string(next() % 100000) + "-" + std::to_string(i), zones[next() % 3]);
            names.push_back(nd.Name);
            ext.nodes.push_back(nd);
            // the groups: a contiguous third, and two dealt node by node; group-c is the smallest
            const char* g = i < n / 3 ? group_names[0] : (i % 4 == 0 ? group_names[2] : group_names[1]);
            groups[g].push_back(nd);
            group_node_names[g].push_back(nd.Name);
            ext.overhead[nd.Name] = Resources{Quantity::FromMilli(100 + 50 * (int64_t)(next() % 20)),
                                              Quantity::FromInt((int64_t)(256 + 128 * (next() % 16)) * Mi), Quantity()};  // on EVERY node
            if (next() % 3 == 0) nonSchedulable[nd.Name] = ext.overhead[nd.Name];
        }
        for (int r = 0; r < 40; ++r) {  // running applications, spread over every group
            ResourceReservation rr;
            rr.Name = "running-" + std::to_string(r);
            rr.Namespace = "namespace";
            const int k = 1 + (int)(next() % 12);
            for (int e = 0; e <= k; ++e) {
                Reservation res;
                res.Node = ext.nodes[next() % n].Name;
                res.Resources = {{kResourceCPU, Quantity::FromInt(1 + (int64_t)(next() % 2))},
                                 {kResourceMemory, Quantity::FromInt((int64_t)(2 + next() % 6) * Gi)},
                                 {kResourceNvidiaGPU, Quantity::FromInt(0)}};
                rr.Reservations[e == 0 ? "driver" : executorReservationName(e - 1)] = res;
            }
            ext.reservations.push_back(rr);
        }
        const char* ecpu[] = {"1", "2", "4"};
        const char* emem[] = {"4Gi", "8Gi", "16Gi"};
        for (int p = 0; p < n_pending; ++p) {  // pending drivers, the groups interleaved
            Pod pod = Driver("pending-" + std::to_string(p), group_names[p % 3], 1 + (int)(next() % 30), emem[next() % 3], ecpu[next() % 3], p + 1);
            pod.UID = "uid-" + std::to_string(p);
            pod.ResourceVersion = 100 + (uint64_t)p;
            ext.pods.push_back(pod);
        }
        ext.nowNanos = (int64_t)(n_pending + 700) * 1000000000;
        FlatCluster cluster;  // EVERY group: what the all-groups scan and the executor Filter want resident
        FlatReservations flat;
        FlatOverhead over;
        std::string err;
        CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
        CHECK(FlatReservations::Build(ext.reservations, ext.softReservationUsage, cluster, &flat, &err));
        CHECK(FlatOverhead::Build(ext.overhead, cluster, &over, &err));
        // the string-map route on an extender of its own (it installs its own snapshots): this one's record stays the flat route's
        auto filter = [&](const Pod& d) {
            const std::string& g = d.InstanceGroup;
            const SelectNodeResult got = ext.selectDriverNodeFlatGroup(g, d, group_node_names[g], cluster, groups[g], &flat, &over);
            SparkSchedulerExtender maps = ext;
            const SelectNodeResult want = maps.selectDriverNode(g, d, group_node_names[g], groups[g]);
            if (!SameAnswer(got, want))
                std::printf("   %s %s: group (%d %s %s %s) map (%d %s %s)\n", packer, d.Name.c_str(), (int)got.served, got.outcome.c_str(),
                            got.node.c_str(), got.error.c_str(), (int)want.served, want.outcome.c_str(), want.node.c_str());
            return SameAnswer(got, want);
        };
        uint64_t gen0[3], gen1[3];
        uint32_t info[4];
        int placed = 0;
        // ---- the Filters of the three groups alternate: the last pending drivers of each, newest first
        for (int p = n_pending - 1; p >= n_pending - 9; --p) CHECK(filter(ext.pods[(size_t)p]));
        CHECK(ext.clusterSetCalls() == 1);
        // ---- the layout of a group Filter: the group's members and one sentinel, not the cluster's
        for (const char* g : group_names) {
            const Pod* d = nullptr;
            for (const Pod& p : ext.pods)
                if (p.InstanceGroup == g) d = &p;
            const SelectNodeResult r = ext.selectDriverNodeFlatGroup(g, *d, group_node_names[g], cluster, groups[g], &flat, &over);
            CHECK(r.served);
            placed += r.node.empty() ? 0 : 1;
            CHECK(gf_snapshot_set_info(g_ctx, info) == GF_OK && info[0] == 1 && info[1] == groups[g].size() && info[2] == groups[g].size() + 1);
            // the same group's Filter again: nothing is rebuilt, nothing is sent
            CHECK(gf_generation(g_ctx, gen0) == GF_OK);
            const SelectNodeResult again = ext.selectDriverNodeFlatGroup(g, *d, group_node_names[g], cluster, groups[g], &flat, &over);
            CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0] && gen1[1] == gen0[1] && gen1[2] == gen0[2]);
            CHECK(again.served && again.outcome == r.outcome && again.node == r.node);
        }
        CHECK(placed >= 1);
        CHECK(ext.clusterSetCalls() == 1);
        // ---- another group's Filter rebuilds (the snapshot epoch moves) from the same resident columns and usage sums
        CHECK(gf_generation(g_ctx, gen0) == GF_OK);
        const Pod& a_driver = ext.pods[(size_t)n_pending - 3];  // group-a; group-c was installed last
        CHECK(a_driver.InstanceGroup == "group-a");
        const SelectNodeResult a1 = ext.selectDriverNodeFlatGroup("group-a", a_driver, group_node_names["group-a"], cluster, groups["group-a"], &flat, &over);
        CHECK(a1.served);
        CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] > gen0[0] && gen1[1] == gen0[1] && gen1[2] == gen0[2]);
        // ---- the all-groups scan next to it: the resident route answers and leaves everything where it is
        bool served = false, resident = false;
        CHECK(gf_generation(g_ctx, gen0) == GF_OK);
        const auto scan = ext.scanForUnschedulablePodsAllGroups(ext.pods, 600ll * 1000000000, cluster, groups, nonSchedulable, &served, &err, &resident);
        CHECK(served && resident && scan.size() == ext.pods.size());
        CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0] && gen1[1] == gen0[1] && gen1[2] == gen0[2]);
        // ---- an executor Filter on the same resident cluster, offered group-b's nodes
        Pod xdriver = Driver("dyn-warm", "group-b", 0, "8Gi", "2", 1);
        xdriver.Annotations.erase("spark-executor-count");
        xdriver.Annotations["spark-dynamic-allocation-enabled"] = "true";
        xdriver.Annotations["spark-dynamic-allocation-min-executor-count"] = "0";
        xdriver.Annotations["spark-dynamic-allocation-max-executor-count"] = "4";
        xdriver.NodeName = group_node_names["group-b"][3];
        xdriver.Phase = "Running";
        bool took = false;
        const SelectNodeResult x = ext.rescheduleExecutorFlat(Executor("dyn-warm", 0), xdriver, {xdriver}, group_node_names["group-b"], {}, true,
                                                              cluster, &flat, &over, &took);
        CHECK(took && x.served && !x.node.empty());
        CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0] && gen1[1] == gen0[1] && gen1[2] == gen0[2]);
        {
            SparkSchedulerExtender maps = ext;
            const SelectNodeResult y = maps.rescheduleExecutor(Executor("dyn-warm", 0), xdriver, {xdriver}, group_node_names["group-b"], {}, true);
            CHECK(x.node == y.node && x.outcome == y.outcome);
        }
        // ---- and the Filters go on alternating; still one gf_cluster_set
        for (int p = n_pending - 10; p >= n_pending - 15; --p) CHECK(filter(ext.pods[(size_t)p]));
        CHECK(ext.clusterSetCalls() == 1);
        // ---- an overhead row changes: one gf_overhead_update, no gf_cluster_set, and the group Filter sees it
        ext.overhead[group_node_names["group-b"][0]] = Resources{Quantity::FromInt(9), Quantity::FromInt(40 * Gi), Quantity()};
        CHECK(FlatOverhead::Build(ext.overhead, cluster, &over, &err));
        const uint64_t updates = ext.overheadUpdateCalls();
        CHECK(filter(ext.pods[(size_t)n_pending - 2]));  // group-b
        CHECK(ext.pods[(size_t)n_pending - 2].InstanceGroup == "group-b");
        CHECK(ext.overheadUpdateCalls() == updates + 1 && ext.clusterSetCalls() == 1);
        // ---- a group node the cluster does not know: selectDriverNode answers
        std::vector<Node> with_a_stranger = groups["group-c"];
        Node stranger = NewNode("not-in-the-cluster", "az-a");
        with_a_stranger.push_back(stranger);
        std::vector<std::string> stranger_names = group_node_names["group-c"];
        stranger_names.push_back(stranger.Name);
        const Pod& c_driver = ext.pods[(size_t)n_pending - 1];
        CHECK(c_driver.InstanceGroup == "group-c");
        SparkSchedulerExtender maps = ext;
        maps.nodes.push_back(stranger);
        SparkSchedulerExtender falls = ext;
        falls.nodes.push_back(stranger);
        const SelectNodeResult fell = falls.selectDriverNodeFlatGroup("group-c", c_driver, stranger_names, cluster, with_a_stranger, &flat, &over);
        const SelectNodeResult want = maps.selectDriverNode("group-c", c_driver, stranger_names, with_a_stranger);
        CHECK(SameAnswer(fell, want));
    }
}

static void CpuHalf() {
    TestWhatNeedsNoDevice();
    TestRefusalsOfTheDriverFilters();
}

static void GpuHalf() {
    TestThreeGroupsOnOneResidentCluster();
    TestAnUnparsableEarlierDriverIsSkipped();
}

int main(int argc, char** argv) { return RunHostTests(argc, argv, CpuHalf, GpuHalf); }
