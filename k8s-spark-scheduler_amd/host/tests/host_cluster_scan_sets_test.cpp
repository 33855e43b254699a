// host_cluster_scan_sets_test.cpp — the UnschedulablePodMarker's whole minute in one call
// (SparkSchedulerExtender::scanForUnschedulablePodsAllGroups -> gf_cluster_fit_feasible_sets): stale pending drivers of three
// instance groups plus one of a group nobody names, against one scanForUnschedulablePods per group (which installs the
// empty-cluster snapshot) merged back into listing order; the resident route answers after a flat Filter and not before one, and
// leaves gf_generation alone.
// `host_cluster_scan_sets_test cpu` needs no GPU (the listing: nothing stale, an unparsable pod, an unrepresentable one); `host_cluster_scan_sets_test gpu`
// drives the device through the C ABI.  Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#define HOST_TEST_SEED 0x5E75
#include "host_test_common.hpp"

static Pod Driver(const std::string& app, const std::string& group, int numExecutors, const char* executorMem, const char* executorCPU,
                  bool executorGpu, int64_t created_s) {
    Pod p;
    p.Name = app + "-spark-driver";
    p.Namespace = "namespace";
    p.labels = {{common::SparkRoleLabel, common::Driver}, {common::SparkAppIDLabel, app}};
    p.Annotations = {{"spark-driver-cpu", "1"},           {"spark-driver-mem", "2Gi"},
                     {"spark-executor-cpu", executorCPU}, {"spark-executor-mem", executorMem},
                     {"spark-executor-count", std::to_string(numExecutors)}};
    if (executorGpu) p.Annotations["spark-executor-nvidia.com/gpu"] = "1";
    p.SchedulerName = common::SparkSchedulerName;
    p.InstanceGroup = group;
    p.CreationTimestampNanos = created_s * 1000000000;
    return p;
}

typedef std::vector<std::pair<std::string, bool>> ScanResult;
static const int64_t kTimeout = 600ll * 1000000000;

// ------------------------------------------------------------------------------------------------ no device
static void TestTheListingNeedsNoDevice() {
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", nullptr), NodeSorter(), true, FifoConfig{});
    Node nd;
    nd.Name = "node1";
    nd.Allocatable = {{kResourceCPU, Quantity::FromInt(8)}, {kResourceMemory, Quantity::FromInt(8 * Gi)}, {kResourceNvidiaGPU, Quantity::FromInt(0)}};
    nd.Ready = true;
    ext.nodes = {nd};
    ext.nowNanos = 10000ll * 1000000000;
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    const std::map<std::string, std::vector<Node>> groups = {{"group-a", ext.nodes}};
    // nothing stale: a young driver, a bound one, an executor
    Pod young = Driver("young", "group-a", 2, "1Gi", "1", false, 9999);
    Pod bound = Driver("bound", "group-a", 2, "1Gi", "1", false, 1);
    bound.NodeName = "node1";
    Pod executor = Driver("executor", "group-a", 2, "1Gi", "1", false, 1);
    executor.labels[common::SparkRoleLabel] = common::Executor;
    bool served = false, resident = true;
    err.clear();
    ScanResult r = ext.scanForUnschedulablePodsAllGroups({young, bound, executor}, kTimeout, cluster, groups, {}, &served, &err, &resident);
    CHECK(r.empty() && served && !resident && err.empty());
    // an unparsable pod ends the scan there: with nothing before it, nothing is asked and *err says why
    Pod broken = Driver("broken", "group-a", 2, "1Gi", "1", false, 1);
    broken.Annotations["spark-executor-count"] = "many";
    Pod behind = Driver("behind", "group-a", 2, "1Gi", "1", false, 2);
    served = false;
    resident = true;
    r = ext.scanForUnschedulablePodsAllGroups({young, broken, behind}, kTimeout, cluster, groups, {}, &served, &err, &resident);
    CHECK(r.empty() && served && !resident && !err.empty());
    // an unrepresentable pod in a group that has nodes takes the per-group route, whose installing scan does not serve it
    Pod micro = Driver("micro", "group-a", 2, "1Gi", "1500u", false, 1);
    served = true;
    resident = true;
    err.clear();
    r = ext.scanForUnschedulablePodsAllGroups({young, micro, behind}, kTimeout, cluster, groups, {}, &served, &err, &resident);
    CHECK(r.empty() && !served && !resident);
    CHECK(err == "pod micro-spark-driver is not exactly representable");
}

// ------------------------------------------------------------------------------------------------ through the device
static void TestThreeGroupsAndAnUnknownOne() {
    const int n = 300, n_pending = 48;
    const char* group_names[] = {"group-a", "group-b", "group-c"};
    for (const char* packer : {"tightly-pack", "single-az-tightly-pack"}) {
        SparkSchedulerExtender ext(SelectBinpacker(packer, g_ctx), NodeSorter(), true, FifoConfig{});
        const char* zones[] = {"az-a", "az-b", "az-c"};
        std::vector<std::string> names;
        NodeGroupResources nonSchedulable;
        std::map<std::string, std::vector<Node>> groups;
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
            // the groups: a contiguous third, and two dealt node by node; group-c is the smallest
            const char* g = i < n / 3 ? group_names[0] : (i % 4 == 0 ? group_names[2] : group_names[1]);
            groups[g].push_back(nd);
            if (next() % 3 == 0)
                nonSchedulable[nd.Name] = Resources{Quantity::FromMilli(250 * (int64_t)(1 + next() % 8)), Quantity::FromInt((int64_t)(1 + next() % 8) * Gi), Quantity()};
        }
        const char* ecpu[] = {"1", "2", "4"};
        const char* emem[] = {"4Gi", "8Gi", "16Gi"};
        std::vector<Pod> scanned;  // the groups interleaved; every sixth pod asks a group the map does not name
        for (int p = 0; p < n_pending; ++p) {
            const std::string group = p % 6 == 5 ? "group-nobody-has" : group_names[p % 3];
            const int k = p % 2 == 1 ? 1500 + (int)(next() % 3000) : 1 + (int)(next() % 400);
            scanned.push_back(Driver("pending-" + std::to_string(p), group, k, emem[next() % 3], ecpu[next() % 3], p % 7 == 3, p + 1));
        }
        ext.pods = {scanned[0]};
        ext.nowNanos = (int64_t)(n_pending + 700) * 1000000000;  // every pending driver is stale
        FlatCluster cluster;
        std::string err;
        CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
        // ---- what the reference does: one scan per instance group, merged in listing order; nobody's group packs onto no node
        ScanResult want(scanned.size());
        for (const char* g : group_names) {
            std::vector<Pod> pods;
            std::vector<size_t> at;
            for (size_t i = 0; i < scanned.size(); ++i)
                if (scanned[i].InstanceGroup == g) {
                    pods.push_back(scanned[i]);
                    at.push_back(i);
                }
            bool ok = false;
            const ScanResult part = ext.scanForUnschedulablePods(pods, kTimeout, groups[g], nonSchedulable, &ok, &err);
            CHECK(ok && part.size() == at.size());
            for (size_t j = 0; j < at.size() && j < part.size(); ++j) want[at[j]] = part[j];
        }
        size_t exceeds = 0, unknown = 0;
        for (size_t i = 0; i < scanned.size(); ++i) {
            if (scanned[i].InstanceGroup == "group-nobody-has") {
                want[i] = {scanned[i].Name, true};
                ++unknown;
            } else {
                exceeds += want[i].second ? 1 : 0;
            }
        }
        CHECK(unknown == 8 && exceeds >= 5 && scanned.size() - unknown - exceeds >= 5);  // the comparison sees both answers
        // ---- before a flat Filter nothing of this cluster is resident: the per-group route answers
        bool served = false, resident = true;
        const ScanResult cold = ext.scanForUnschedulablePodsAllGroups(scanned, kTimeout, cluster, groups, nonSchedulable, &served, &err, &resident);
        CHECK(served && !resident && cold == want);
        // ---- the Filter that leaves the cluster on the device, then the scan next to it
        const SelectNodeResult f = ext.selectDriverNodeFlat(scanned[0].InstanceGroup, ext.pods[0], names, cluster);
        CHECK(f.served);
        uint64_t gen0[3], gen1[3];
        CHECK(gf_generation(g_ctx, gen0) == GF_OK);
        served = false;
        resident = false;
        const ScanResult got = ext.scanForUnschedulablePodsAllGroups(scanned, kTimeout, cluster, groups, nonSchedulable, &served, &err, &resident);
        CHECK(served && resident);
        CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0] && gen1[1] == gen0[1] && gen1[2] == gen0[2]);
        CHECK(got == want);
        if (got != want)
            for (size_t i = 0; i < got.size() && i < want.size(); ++i)
                if (got[i] != want[i])
                    std::printf("   %s: %s (%s) sets %d per group %d\n", packer, want[i].first.c_str(), scanned[i].InstanceGroup.c_str(),
                                (int)got[i].second, (int)want[i].second);
        // ---- a listed node outside the cluster: the per-group route, the same list
        std::map<std::string, std::vector<Node>> with_a_stranger = groups;
        Node stranger = ext.nodes[0];
        stranger.Name = "not-in-the-cluster";
        with_a_stranger["group-nobody-has"].push_back(stranger);
        std::vector<Pod> known;
        ScanResult want_known;
        for (size_t i = 0; i < scanned.size(); ++i)
            if (scanned[i].InstanceGroup != "group-nobody-has") {
                known.push_back(scanned[i]);
                want_known.push_back(want[i]);
            }
        known.push_back(scanned[5]);  // (one pod of the stranger's group: its one node holds a few executors)
        resident = true;
        const ScanResult got2 = ext.scanForUnschedulablePodsAllGroups(known, kTimeout, cluster, with_a_stranger, nonSchedulable, &served, &err, &resident);
        CHECK(served && !resident && got2.size() == known.size());
        if (got2.size() == known.size()) CHECK(ScanResult(got2.begin(), got2.end() - 1) == want_known);
    }
}

static void CpuHalf() {
    TestTheListingNeedsNoDevice();
}

static void GpuHalf() {
    TestThreeGroupsAndAnUnknownOne();
}

int main(int argc, char** argv) { return RunHostTests(argc, argv, CpuHalf, GpuHalf); }
