// host_group_filter_test.cpp — driver Filters of several instance groups on ONE resident cluster
// (SparkSchedulerExtender::selectDriverNodeFlatGroup -> gf_snapshot_build_resident_set): a three-group cluster with overhead on
// every node; Filters of the three groups alternate, a scanForUnschedulablePodsAllGroups and a rescheduleExecutorFlat run in
// between; every Filter equals selectDriverNode (the string-map route) on that group's nodes, gf_cluster_set is sent once, and
// the same group's Filter twice in a row does not rebuild.
// `host_group_filter_test cpu` needs no GPU (what the route hands to selectDriverNode before it touches a device);
// `host_group_filter_test gpu` drives the device through the C ABI.  Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "extender.hpp"

using namespace gangfit::host;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        ++g_checked;                                                           \
        if (!(cond)) {                                                         \
            ++g_failed;                                                        \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);        \
        }                                                                      \
    } while (0)

static const int64_t Mi = 1024 * 1024, Gi = 1024 * Mi;
static gf_ctx* g_ctx = nullptr;

static uint64_t g_rng = 0x6709;
static uint64_t next() {
    g_rng += 0x9E3779B97F4A7C15ull;
    uint64_t z = g_rng;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
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

// ------------------------------------------------------------------------------------------------ through the device
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

int main(int argc, char** argv) {
    (void)setenv("GPU_MAX_HW_QUEUES", "16", 0);  // the deployment's part ("Deployment")
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "cpu" || mode == "all") TestWhatNeedsNoDevice();
    if (mode == "gpu" || mode == "all") {
        if (gf_init(nullptr, 0, &g_ctx) != GF_OK) {
            std::printf("FAIL gf_init: no gfx950 device (there is no CPU fallback)\n");
            return 2;
        }
        TestThreeGroupsOnOneResidentCluster();
        gf_destroy(g_ctx);
    }
    std::printf("%s: %d checks, %d failed\n", mode.c_str(), g_checked, g_failed);
    return g_failed == 0 ? 0 : 1;
}
