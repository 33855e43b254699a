// host_cluster_scan_test.cpp — the UnschedulablePodMarker's scan next to the Filter's installed snapshot
// (SparkSchedulerExtender::scanForUnschedulablePodsResident -> gf_cluster_fit_feasible): the same (pod, exceeds) list as
// scanForUnschedulablePods, which installs the empty-cluster snapshot, on the scenarios of the reference's
// unschedulablepods_test.go (the gpu scenario included) and on a cluster with zones, overhead and a node selection; the Filter
// after the scan resumes its chain; a question the entry point refuses falls back to the installing route.
// `host_cluster_scan_test cpu` needs no GPU (the node selection of a flat cluster, the listing filter and the refusals of
// the scans); `host_cluster_scan_test gpu` drives the device through the C ABI.  Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#define HOST_TEST_SEED 0x5CA9
#include "host_test_common.hpp"

static Node NewNode(const std::string& name, const char* zone) {  // extendertest.NewNode (extender_test_utils.go:239-271)
    Node n;
    n.Name = name;
    n.labels = {{"resource_channel", "batch-medium-priority"},
                {"com.palantir.rubix/instance-group", "batch-medium-priority"},
                {"test", "something"},
                {"topology.kubernetes.io/zone", zone}};
    n.Allocatable = {{kResourceCPU, Quantity::FromInt(8)}, {kResourceMemory, Quantity::FromInt(8 * Gi)},
                     {kResourceNvidiaGPU, Quantity::FromInt(1)}};
    n.Ready = true;
    return n;
}

static Pod Driver(const std::string& app, std::map<std::string, std::string> annotations, int64_t created_s) {
    Pod p;
    p.Name = app + "-spark-driver";
    p.Namespace = "namespace";
    p.labels = {{common::SparkRoleLabel, common::Driver}, {common::SparkAppIDLabel, app}};
    p.Annotations = std::move(annotations);
    p.SchedulerName = common::SparkSchedulerName;
    p.InstanceGroup = "batch-medium-priority";
    p.CreationTimestampNanos = created_s * 1000000000;
    return p;
}

// extendertest.StaticAllocationSparkPods / ...WithExecutorGPUs (extender_test_utils.go)
static std::map<std::string, std::string> StaticAnnotations(int numExecutors, const char* driverMem = "1", const char* driverCPU = "1",
                                                            const char* executorMem = "1", const char* executorCPU = "1",
                                                            bool executorGpu = false) {
    std::map<std::string, std::string> a = {{"spark-driver-cpu", driverCPU},     {"spark-driver-mem", driverMem},
                                            {"spark-driver-nvidia.com/gpu", "1"}, {"spark-executor-cpu", executorCPU},
                                            {"spark-executor-mem", executorMem},
                                            {"spark-executor-count", std::to_string(numExecutors)}};
    if (executorGpu) a["spark-executor-nvidia.com/gpu"] = "1";
    return a;
}

typedef std::vector<std::pair<std::string, bool>> ScanResult;

// ------------------------------------------------------------------------------------------------ no device
static void TestNodesOutsideTheClusterTakeTheOtherRoute() {
    // a node the flat cluster does not know cannot be selected: the resident scan must not answer (it hands over before it
    // touches the context — there is none here)
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", nullptr), NodeSorter(), true, FifoConfig{});
    ext.nodes = {NewNode("node1", "zone1")};
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    CHECK(cluster.index.count("node1") == 1 && cluster.index.count("node2") == 0);
    bool served = false, resident = true;
    const ScanResult r = ext.scanForUnschedulablePodsResident({}, 0, cluster, {NewNode("node2", "zone1")}, {}, &served, &err, &resident);
    CHECK(r.empty() && !resident);  // (no pending driver: the installing route returns before it needs a device)
}

// What each scan does with a stale pod it cannot take, decided before any device call: an unparsable pod ends the listing with
// the parse error, an unrepresentable one is not served; the resident scan hands both to the installing scan.
static void TestRefusalsOfTheScans() {
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", nullptr), NodeSorter(), true, FifoConfig{});
    ext.nodes = {NewNode("node1", "zone1")};
    ext.nowNanos = 10000ll * 1000000000;
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    Pod unparsable = Driver("unparsable", StaticAnnotations(2), 1);
    unparsable.Annotations["spark-executor-count"] = "many";
    Pod unrepresentable = Driver("unrepresentable", StaticAnnotations(2), 1);
    unrepresentable.Annotations["spark-executor-cpu"] = "1500u";
    const Pod behind = Driver("behind", StaticAnnotations(2), 2);
    std::string parse_err;
    CHECK(!sparkResources(unparsable, &parse_err) && !parse_err.empty());
    CHECK(sparkResources(unrepresentable, nullptr).has_value());
    // ---- scanForUnschedulablePods
    bool served = false;
    err.clear();
    ScanResult r = ext.scanForUnschedulablePods({unparsable, behind}, 0, ext.nodes, {}, &served, &err);
    CHECK(r.empty() && served && err == parse_err);
    served = true;
    err.clear();
    r = ext.scanForUnschedulablePods({unrepresentable, behind}, 0, ext.nodes, {}, &served, &err);
    CHECK(r.empty() && !served && err == "pod unrepresentable-spark-driver is not exactly representable");
    // ---- scanForUnschedulablePodsResident: what scanForUnschedulablePods says, by the installing route
    bool resident = true;
    served = false;
    err.clear();
    r = ext.scanForUnschedulablePodsResident({unparsable, behind}, 0, cluster, ext.nodes, {}, &served, &err, &resident);
    CHECK(r.empty() && served && err == parse_err && !resident);
    resident = true;
    served = true;
    err.clear();
    r = ext.scanForUnschedulablePodsResident({unrepresentable, behind}, 0, cluster, ext.nodes, {}, &served, &err, &resident);
    CHECK(r.empty() && !served && err == "pod unrepresentable-spark-driver is not exactly representable" && !resident);
}

// The listing of all three scans: a young driver, a bound one, a deleting one, an executor and a pod of another scheduler are
// skipped, so nothing is asked and no device is needed.
static void TestTheListingFilterOfTheScans() {
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", nullptr), NodeSorter(), true, FifoConfig{});
    ext.nodes = {NewNode("node1", "zone1")};
    ext.nowNanos = 10000ll * 1000000000;
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    const Pod young = Driver("young", StaticAnnotations(2), 9999);
    Pod bound = Driver("bound", StaticAnnotations(2), 1);
    bound.NodeName = "node1";
    Pod deleting = Driver("deleting", StaticAnnotations(2), 1);
    deleting.Deleting = true;
    Pod executor = Driver("executor", StaticAnnotations(2), 1);
    executor.labels[common::SparkRoleLabel] = common::Executor;
    Pod foreign = Driver("foreign", StaticAnnotations(2), 1);
    foreign.SchedulerName = "default-scheduler";
    // (each of them unparsable: a pod the filter let through would end the listing with an error)
    std::vector<Pod> skipped = {young, bound, deleting, executor, foreign};
    for (Pod& p : skipped) p.Annotations["spark-executor-count"] = "many";
    const std::map<std::string, std::vector<Node>> groups = {{"batch-medium-priority", ext.nodes}};
    bool served = false, resident = true;
    err.clear();
    ScanResult r = ext.scanForUnschedulablePods(skipped, 600ll * 1000000000, ext.nodes, {}, &served, &err);
    CHECK(r.empty() && served && err.empty());
    served = false;
    r = ext.scanForUnschedulablePodsResident(skipped, 600ll * 1000000000, cluster, ext.nodes, {}, &served, &err, &resident);
    CHECK(r.empty() && served && err.empty() && !resident);
    served = false;
    resident = true;
    r = ext.scanForUnschedulablePodsAllGroups(skipped, 600ll * 1000000000, cluster, groups, {}, &served, &err, &resident);
    CHECK(r.empty() && served && err.empty() && !resident);
}

// ------------------------------------------------------------------------------------------------ through the device
static void TestReferenceScenarios() {  // unschedulablepods_test.go:24-80 as one scan, then pod by pod
    for (const char* packer : {"single-az-tightly-pack", "tightly-pack", "single-az-minimal-fragmentation", "az-aware-tightly-pack"}) {
        SparkSchedulerExtender ext(SelectBinpacker(packer, g_ctx), NodeSorter(), true, FifoConfig{});
        ext.nodes = {NewNode("node1", "zone1"), NewNode("node2", "zone1")};
        ext.nowNanos = 10000ll * 1000000000;
        const Pod fits = Driver("2-executor-app", StaticAnnotations(2), 1), too_big = Driver("100-executor-app", StaticAnnotations(100), 2),
                  young = Driver("young-app", StaticAnnotations(100), 9999),
                  gpus = Driver("gpu-app", StaticAnnotations(2, "1", "1", "1", "1", true), 3);  // three gpus asked, two in the cluster
        Pod bound = Driver("bound-app", StaticAnnotations(100), 4);
        bound.NodeName = "node1";
        const std::vector<Pod> all = {fits, too_big, young, gpus, bound};
        FlatCluster cluster;
        std::string err;
        CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
        // the Filter that leaves the cluster on the device
        ext.pods = {Driver("filtered-app", StaticAnnotations(1), 1)};
        const SelectNodeResult f = ext.selectDriverNodeFlat("batch-medium-priority", ext.pods[0], {"node1", "node2"}, cluster);
        CHECK(f.served && f.outcome == std::string(outcome::success));
        uint64_t gen0[3], gen1[3];
        CHECK(gf_generation(g_ctx, gen0) == GF_OK);
        bool served = false, resident = false;
        const ScanResult got = ext.scanForUnschedulablePodsResident(all, 600ll * 1000000000, cluster, ext.nodes, {}, &served, &err, &resident);
        CHECK(served && resident);
        CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0] && gen1[1] == gen0[1] && gen1[2] == gen0[2]);
        CHECK(got.size() == 3);
        if (got.size() == 3) {
            CHECK(got[0].first == "2-executor-app-spark-driver" && !got[0].second);    // "should fit to the cluster"
            CHECK(got[1].first == "100-executor-app-spark-driver" && got[1].second);   // "should not fit to the cluster"
            CHECK(got[2].first == "gpu-app-spark-driver" && got[2].second);            // not enough nvidia gpus
        }
        const ScanResult want = ext.scanForUnschedulablePods(all, 600ll * 1000000000, ext.nodes, {}, &served, &err);
        CHECK(served && got == want);
    }
}

static void TestZonesOverheadSelectionAndTheNextFilter() {
    const int n = 300, n_pending = 40;
    for (const char* packer : {"tightly-pack", "single-az-tightly-pack"}) {
        SparkSchedulerExtender ext(SelectBinpacker(packer, g_ctx), NodeSorter(), true, FifoConfig{});
        const char* zones[] = {"az-a", "az-b", "az-c"};
        std::vector<std::string> names;
        NodeGroupResources nonSchedulable;
        for (int i = 0; i < n; ++i) {
            Node nd;
            nd.Name = "n" + std::to_string(next() % 100000) + "-" + std::to_string(i);
            nd.labels[kLabelZoneFailureDomain] = zones[next() % 3];
            nd.Allocatable = {{kResourceCPU, Quantity::FromInt(16 + 16 * (int64_t)(next() % 3))},
                              {kResourceMemory, Quantity::FromInt((int64_t)(64 + 64 * (next() % 3)) * Gi)},
                              {kResourceNvidiaGPU, Quantity::FromInt(next() % 10 == 0 ? 4 : 0)}};
            nd.Ready = true;
            names.push_back(nd.Name);
            ext.nodes.push_back(nd);
            ext.overhead[nd.Name] = Resources{Quantity::FromMilli(100 + 50 * (int64_t)(next() % 20)),
                                              Quantity::FromInt((int64_t)(256 + 128 * (next() % 16)) * Mi), Quantity()};
            if (next() % 3 == 0)  // the non-schedulable part: what the marker subtracts
                nonSchedulable[nd.Name] = Resources{Quantity::FromMilli(250 * (int64_t)(1 + next() % 8)), Quantity::FromInt((int64_t)(1 + next() % 8) * Gi), Quantity()};
        }
        for (int r = 0; r < 30; ++r) {
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
        std::vector<Pod> scanned;  // what the marker lists: the Filter's queue, then drivers from a handful of executors to far
                                   // above what 300 nodes hold, a few of them with gpu executors
        for (int p = 0; p < n_pending; ++p) {
            Pod pod = Driver("pending-" + std::to_string(p), StaticAnnotations(1 + (int)(next() % 30), "2Gi", "1", emem[next() % 3], ecpu[next() % 3]), p + 1);
            pod.Annotations.erase("spark-driver-nvidia.com/gpu");
            pod.UID = "uid-" + std::to_string(p);
            pod.ResourceVersion = 100 + (uint64_t)p;
            ext.pods.push_back(pod);
            scanned.push_back(pod);
        }
        for (int p = 0; p < n_pending; ++p) {
            const int k = p % 2 == 1 ? 3000 + (int)(next() % 4000) : 1 + (int)(next() % 2500);
            Pod pod = Driver("unschedulable-" + std::to_string(p), StaticAnnotations(k, "2Gi", "1", emem[next() % 3], ecpu[next() % 3], p % 7 == 5), p + 1);
            pod.Annotations.erase("spark-driver-nvidia.com/gpu");
            scanned.push_back(pod);
        }
        ext.nowNanos = (int64_t)(n_pending + 700) * 1000000000;  // every pending driver is stale
        FlatCluster cluster;
        FlatReservations flat;
        std::string err;
        CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
        CHECK(FlatReservations::Build(ext.reservations, ext.softReservationUsage, cluster, &flat, &err));
        std::vector<Node> matching;  // the drivers' affinity leaves out zone az-c and a few more nodes
        for (const Node& nd : ext.nodes)
            if (nd.labels.at(kLabelZoneFailureDomain) != "az-c" && next() % 16 != 0) matching.push_back(nd);
        const Pod& last = ext.pods.back();
        // ---- warm Filter: twice, the second resumes
        const SelectNodeResult first = ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat);
        CHECK(first.served);
        const SelectNodeResult second = ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat);
        CHECK(second.served && second.outcome == first.outcome && second.node == first.node);
        uint64_t gen0[3], gen1[3], st[4];
        CHECK(gf_chain_cache_stats(g_ctx, 1, st) == GF_OK);
        CHECK(gf_generation(g_ctx, gen0) == GF_OK);
        // ---- the marker's minute, next to it
        bool served = false, resident = false;
        const ScanResult got = ext.scanForUnschedulablePodsResident(scanned, 600ll * 1000000000, cluster, matching, nonSchedulable, &served, &err, &resident);
        CHECK(served && resident && got.size() == scanned.size());
        CHECK(gf_chain_cache_stats(g_ctx, 0, st) == GF_OK && st[0] == 0);  // the scan is no chain
        CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0] && gen1[1] == gen0[1] && gen1[2] == gen0[2]);
        // ---- the Filter after the scan: no build, no upload, a resumed chain of at most two applications
        CHECK(gf_chain_cache_stats(g_ctx, 1, st) == GF_OK);
        const SelectNodeResult third = ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat);
        CHECK(third.served && third.outcome == first.outcome && third.node == first.node);
        CHECK(gf_chain_cache_stats(g_ctx, 0, st) == GF_OK);
        CHECK(st[0] == 1 && st[1] == 1 && st[2] <= 2);
        if (!(st[0] == 1 && st[1] == 1 && st[2] <= 2))
            std::printf("   %s: chains %llu resumed %llu evaluated %llu skipped %llu\n", packer, (unsigned long long)st[0],
                        (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3]);
        CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0] && gen1[1] == gen0[1] && gen1[2] == gen0[2]);
        // ---- the same list as the installing route (which ends the warm state: it runs last)
        const ScanResult want = ext.scanForUnschedulablePods(scanned, 600ll * 1000000000, matching, nonSchedulable, &served, &err);
        CHECK(served && got == want);
        size_t exceeds = 0;
        for (const auto& pr : want) exceeds += pr.second ? 1 : 0;
        CHECK(exceeds >= 5 && want.size() - exceeds >= 5);  // the comparison sees both answers
        if (got != want)
            for (size_t i = 0; i < got.size() && i < want.size(); ++i)
                if (got[i] != want[i]) std::printf("   %s: %s resident %d installed %d\n", packer, want[i].first.c_str(), (int)got[i].second, (int)want[i].second);
    }
}

static void TestARefusedQuestionFallsBack() {
    // single-AZ packer + a driver that asks for neither cpu nor memory: chooseBestResult's average could be 0, the entry point
    // refuses (GF_ERR_UNSUPPORTED) and the installing route answers — the reference's quirk included
    SparkSchedulerExtender ext(SelectBinpacker("single-az-tightly-pack", g_ctx), NodeSorter(), true, FifoConfig{});
    ext.nodes = {NewNode("node1", "zone1"), NewNode("node2", "zone1")};
    ext.nowNanos = 10000ll * 1000000000;
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    ext.pods = {Driver("filtered-app", StaticAnnotations(1), 1)};
    CHECK(ext.selectDriverNodeFlat("batch-medium-priority", ext.pods[0], {"node1", "node2"}, cluster).served);
    Pod nothing = Driver("asks-for-nothing", StaticAnnotations(2, "0", "0"), 1);
    nothing.Annotations.erase("spark-driver-nvidia.com/gpu");
    const std::vector<Pod> all = {Driver("2-executor-app", StaticAnnotations(2), 1), nothing, Driver("100-executor-app", StaticAnnotations(100), 2)};
    uint64_t gen0[3], gen1[3];
    CHECK(gf_generation(g_ctx, gen0) == GF_OK);
    bool served = false, resident = true;
    const ScanResult got = ext.scanForUnschedulablePodsResident(all, 600ll * 1000000000, cluster, ext.nodes, {}, &served, &err, &resident);
    CHECK(served && !resident && got.size() == 3);
    CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] > gen0[0]);  // the installing route answered
    const ScanResult want = ext.scanForUnschedulablePods(all, 600ll * 1000000000, ext.nodes, {}, &served, &err);
    CHECK(served && got == want);
    // a cluster that is not the one on the device (another Build of the same nodes): the other route as well
    FlatCluster other;
    CHECK(FlatCluster::Build(ext.nodes, &other, &err));
    resident = true;
    const ScanResult got2 = ext.scanForUnschedulablePodsResident({all[0], all[2]}, 600ll * 1000000000, other, ext.nodes, {}, &served, &err, &resident);
    CHECK(served && !resident && got2.size() == 2);
    if (got2.size() == 2) CHECK(!got2[0].second && got2[1].second);
}

static void CpuHalf() {
    TestNodesOutsideTheClusterTakeTheOtherRoute();
    TestRefusalsOfTheScans();
    TestTheListingFilterOfTheScans();
}

static void GpuHalf() {
    TestReferenceScenarios();
    TestZonesOverheadSelectionAndTheNextFilter();
    TestARefusedQuestionFallsBack();
}

int main(int argc, char** argv) { return RunHostTests(argc, argv, CpuHalf, GpuHalf); }
