// host_executor_resident_test.cpp — the executor Filter answered from the resident cluster
// (SparkSchedulerExtender::rescheduleExecutorFlat -> gf_cluster_executor_fit): the same node, outcome and error as
// rescheduleExecutor, which installs a snapshot per call, on the scenarios of the reference's TestDynamicAllocationScheduling
// (resource_test.go:172-372, the same-AZ case included) and TestMinimalFragmentation*, on a cluster with zones, overhead and
// reservations, and for a call the entry point refuses (which must fall back); the driver Filter after a resident executor Filter
// resumes its chain.
// `host_executor_resident_test cpu` needs no GPU (what the flat route decides before it touches a context, the refusals of both routes);
// `host_executor_resident_test gpu` drives the device through the C ABI.  Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

#define HOST_TEST_SEED 0xE8EC
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

static Pod Driver(const std::string& app, std::map<std::string, std::string> annotations, int64_t created_s = 0) {
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

static Pod Executor(const std::string& app, int i) {
    Pod p;
    p.Name = app + "-spark-exec-" + std::to_string(i);
    p.Namespace = "namespace";
    p.labels = {{common::SparkRoleLabel, common::Executor}, {common::SparkAppIDLabel, app}};
    p.SchedulerName = common::SparkSchedulerName;
    p.Phase = "Pending";
    return p;
}

static std::map<std::string, std::string> StaticAnnotations(int numExecutors, const char* driverMem = "1", const char* driverCPU = "1",
                                                            const char* executorMem = "1", const char* executorCPU = "1") {
    return {{"spark-driver-cpu", driverCPU},      {"spark-driver-mem", driverMem},     {"spark-driver-nvidia.com/gpu", "1"},
            {"spark-executor-cpu", executorCPU}, {"spark-executor-mem", executorMem}, {"spark-executor-count", std::to_string(numExecutors)}};
}

static std::map<std::string, std::string> DynamicAnnotations(int minExecutors, int maxExecutors, const char* driverMem,
                                                             const char* driverCPU, const char* executorMem, const char* executorCPU) {
    return {{"spark-driver-cpu", driverCPU},
            {"spark-driver-mem", driverMem},
            {"spark-driver-nvidia.com/gpu", "1"},
            {"spark-executor-cpu", executorCPU},
            {"spark-executor-mem", executorMem},
            {"spark-dynamic-allocation-enabled", "true"},
            {"spark-dynamic-allocation-min-executor-count", std::to_string(minExecutors)},
            {"spark-dynamic-allocation-max-executor-count", std::to_string(maxExecutors)}};
}

static SparkSchedulerExtender NewTestExtender(const char* binpackAlgo, std::vector<Node> nodes) {
    SparkSchedulerExtender e(SelectBinpacker(binpackAlgo, g_ctx), NodeSorter(), true, FifoConfig{});
    e.nodes = std::move(nodes);
    e.nowNanos = 1000ll * 1000000000;
    return e;
}

static bool Same(const SelectNodeResult& a, const SelectNodeResult& b) {
    return a.node == b.node && a.outcome == b.outcome && a.error == b.error && a.served == b.served;
}

// Both routes on one request: the flat one first (the other installs); `resident` = must the resident entry point have answered.
static SelectNodeResult Both(SparkSchedulerExtender& ext, const FlatCluster& cluster, const Pod& executor, const Pod& driver,
                             const std::vector<Pod>& all, const std::vector<std::string>& names, const std::set<std::string>& hosting,
                             bool extra, int resident, int line) {
    bool took = false;
    const SelectNodeResult flat = ext.rescheduleExecutorFlat(executor, driver, all, names, hosting, extra, cluster, nullptr, nullptr, &took);
    const SelectNodeResult want = ext.rescheduleExecutor(executor, driver, all, names, hosting, extra);
    ++g_checked;
    if (!Same(flat, want) || (resident >= 0 && took != (resident != 0))) {
        ++g_failed;
        std::printf("FAIL line %d: flat (%s, %s, %s, resident %d) installed (%s, %s, %s)\n", line, flat.node.c_str(), flat.outcome.c_str(),
                    flat.error.c_str(), (int)took, want.node.c_str(), want.outcome.c_str(), want.error.c_str());
    }
    return flat;
}
#define BOTH(...) Both(__VA_ARGS__, __LINE__)  // (variadic: the name lists are braced and hold commas)

// ------------------------------------------------------------------------------------------------ no device
static void TestWhatIsDecidedBeforeTheDevice() {
    // the reference's errors come before any device call: a driver without resources, the zone step's own errors
    SparkSchedulerExtender ext(SelectBinpacker("single-az-tightly-pack", nullptr), NodeSorter(), true, FifoConfig{});
    ext.nodes = {NewNode("node1", "zone1"), NewNode("node2", "zone2")};
    ext.shouldScheduleDynamicallyAllocatedExecutorsInSameAZ = true;
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    Pod driver = Driver("app", DynamicAnnotations(0, 2, "1", "1", "1", "1"));
    Pod broken = driver;
    broken.Annotations.erase("spark-executor-cpu");
    bool resident = true;
    SelectNodeResult r = ext.rescheduleExecutorFlat(Executor("app", 0), broken, {}, {"node1", "node2"}, {}, true, cluster, nullptr, nullptr, &resident);
    CHECK(r.node.empty() && r.outcome == std::string(outcome::failureInternal) && !resident);
    r = ext.rescheduleExecutorFlat(Executor("app", 0), driver, {driver}, {"node1", "node2"}, {}, true, cluster, nullptr, nullptr, &resident);
    CHECK(r.node.empty() && r.outcome.empty() &&
          r.error == "Application has no scheduled pods, can't make scheduling decisions based on AZ" && !resident);
    Pod bare = Executor("app", 0);
    bare.labels.erase(common::SparkAppIDLabel);
    r = ext.rescheduleExecutorFlat(bare, driver, {driver}, {"node1", "node2"}, {}, true, cluster, nullptr, nullptr, &resident);
    CHECK(r.node.empty() && r.error == "Executor does not have a Spark app id label, could not create label selector");
    Pod running = driver;
    running.NodeName = "node2";
    running.Phase = "Running";
    ext.nodes[0].labels.erase(kLabelTopologyZone);
    r = ext.rescheduleExecutorFlat(Executor("app", 0), driver, {running}, {"node1", "node2"}, {}, true, cluster, nullptr, nullptr, &resident);
    CHECK(r.node.empty() && r.outcome == std::string(outcome::failureInternal) &&
          r.error == "Could not read zone label from node, unable to make scheduling decisions based on AZ");
}

// An unparsable driver is failure-internal with the bare parse error, an executor request that is not exactly representable is
// not served: by rescheduleExecutor and by rescheduleExecutorFlat (which hands the second to rescheduleExecutor) alike.
static void TestRefusalsOfTheExecutorFilters() {
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", nullptr), NodeSorter(), true, FifoConfig{});
    ext.nodes = {NewNode("node1", "zone1"), NewNode("node2", "zone2")};
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    const std::vector<std::string> names = {"node1", "node2"};
    Pod unparsable = Driver("app", StaticAnnotations(2));
    unparsable.Annotations["spark-executor-count"] = "many";
    std::string parse_err;
    CHECK(!sparkResources(unparsable, &parse_err) && !parse_err.empty());
    auto internal = [&](const SelectNodeResult& r) {
        return r.served && r.node.empty() && r.outcome == std::string(outcome::failureInternal) && r.error == parse_err;
    };
    CHECK(internal(ext.rescheduleExecutor(Executor("app", 0), unparsable, {unparsable}, names, {}, false)));
    CHECK(internal(ext.rescheduleExecutor(unparsable, names, ext.nodes, {}, false)));
    bool resident = true;
    CHECK(internal(ext.rescheduleExecutorFlat(Executor("app", 0), unparsable, {unparsable}, names, {}, false, cluster, nullptr, nullptr, &resident)));
    CHECK(!resident);
    const Pod micro = Driver("app", StaticAnnotations(2, "1", "1", "1", "1500u"));
    CHECK(sparkResources(micro, nullptr).has_value());
    auto not_served = [](const SelectNodeResult& r) {
        return !r.served && r.node.empty() && r.error == "executor resources are not exactly representable";
    };
    CHECK(not_served(ext.rescheduleExecutor(Executor("app", 0), micro, {micro}, names, {}, false)));
    CHECK(not_served(ext.rescheduleExecutor(micro, names, ext.nodes, {}, false)));
    resident = true;
    CHECK(not_served(ext.rescheduleExecutorFlat(Executor("app", 0), micro, {micro}, names, {}, false, cluster, nullptr, nullptr, &resident)));
    CHECK(!resident);
}

// ------------------------------------------------------------------------------------------------ through the device
// TestDynamicAllocationScheduling, "schedules an executor only in the same AZ as the original application" (resource_test.go:262-292)
static void TestDynamicAllocationSameAZ() {
    Node node1 = NewNode("node1", "zone1"), node2 = NewNode("node2", "zone2");
    auto ext = NewTestExtender("single-az-tightly-pack", {node1, node2});
    ext.shouldScheduleDynamicallyAllocatedExecutorsInSameAZ = true;
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    const std::vector<std::string> both = {"node1", "node2"};
    Pod staticDriver = Driver("static-allocation-app", StaticAnnotations(1));
    Pod dynDriver = Driver("dynamic-allocation-app", DynamicAnnotations(0, 2, "1", "1", "1", "1"), 1);
    std::vector<Pod> all = {staticDriver, Executor("static-allocation-app", 0), dynDriver, Executor("dynamic-allocation-app", 0),
                            Executor("dynamic-allocation-app", 1)};
    auto bind = [&](size_t i, const std::string& node) {
        all[i].NodeName = node;
        all[i].Phase = "Running";
    };
    SelectNodeResult r = ext.selectDriverNode("batch-medium-priority", all[0], {"node1"}, ext.nodes);
    CHECK(r.served && r.node == "node1" && r.created.has_value());
    if (r.created) ext.reservations.push_back(*r.created);
    bind(0, "node1");
    bind(1, "node1");
    r = ext.selectDriverNode("batch-medium-priority", all[2], {"node2"}, ext.nodes);
    CHECK(r.served && r.node == "node2" && r.created.has_value());
    if (r.created) ext.reservations.push_back(*r.created);
    bind(2, "node2");
    // the flag off: anywhere — node1 sorts first (less free memory)
    ext.shouldScheduleDynamicallyAllocatedExecutorsInSameAZ = false;
    r = BOTH(ext, cluster, all[3], all[2], all, both, {}, true, 1);
    CHECK(r.served && r.node == "node1");
    ext.shouldScheduleDynamicallyAllocatedExecutorsInSameAZ = true;
    // an application whose running pods span two zones (:628-630): anywhere
    std::vector<Pod> spread = all;
    spread[3].NodeName = "node1";
    spread[3].Phase = "Running";
    r = BOTH(ext, cluster, all[4], all[2], spread, both, {}, true, 1);
    CHECK(r.served && r.node == "node1");
    // executor-0 and executor-1: the application lives in zone2 — "node2" both times (:289-292)
    for (size_t i : {size_t(3), size_t(4)}) {
        r = BOTH(ext, cluster, all[i], all[2], all, both, {}, true, 1);
        CHECK(r.served && r.outcome == std::string(outcome::successScheduledExtraExecutor) && r.node == "node2");
        bind(i, r.node);
        ext.softReservationUsage["node2"].Add(Resources::Create(1, 1, 0));
    }
    // the reference's errors, by either route
    std::vector<Pod> none = all;
    for (Pod& p : none) p.Phase = "Pending";
    r = BOTH(ext, cluster, all[4], all[2], none, both, {}, true, 0);
    CHECK(r.node.empty() && r.outcome.empty());
    // the zone is full: failure-fit
    ext.softReservationUsage["node2"].Add(Resources::Create(8, 1, 0));
    r = BOTH(ext, cluster, all[4], all[2], all, both, {}, true, 1);
    CHECK(r.served && r.node.empty() && r.outcome == std::string(outcome::failureFit));
    // a rescheduled (not extra) executor of the static application, one node offered
    r = BOTH(ext, cluster, all[1], all[0], all, {"node1"}, {}, false, 1);
    CHECK(r.served && r.outcome == std::string(outcome::successRescheduled) && r.node == "node1");
}

// TestDynamicAllocationScheduling's soft-reservation cases (resource_test.go:197-243) and TestMinimalFragmentation*
// (resource_test.go:73-170) at the mirror's boundary
static void TestSoftReservationsAndMinimalFragmentation() {
    for (const char* packer : {"single-az-tightly-pack", "tightly-pack", "single-az-minimal-fragmentation"}) {
        Node node1 = NewNode("node1", "zone1"), node2 = NewNode("node2", "zone1");
        auto ext = NewTestExtender(packer, {node1, node2});
        FlatCluster cluster;
        std::string err;
        CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
        const std::vector<std::string> both = {"node1", "node2"};
        Pod dynDriver = Driver("dynamic-allocation-app", DynamicAnnotations(1, 3, "1", "1", "1", "1"), 1);
        std::vector<Pod> all = {dynDriver, Executor("dynamic-allocation-app", 0), Executor("dynamic-allocation-app", 1),
                                Executor("dynamic-allocation-app", 2)};
        SelectNodeResult r = ext.selectDriverNode("batch-medium-priority", all[0], {"node2"}, ext.nodes);
        CHECK(r.served && r.node == "node2" && r.created.has_value());
        if (r.created) ext.reservations.push_back(*r.created);
        // "soft reservations are created on full nodes first": the extra executors go where the application's reservations left
        // less free memory (the first-fit packers), or where its executors run (minimal fragmentation: the hosting hint)
        for (size_t i : {size_t(2), size_t(3)}) {
            r = BOTH(ext, cluster, all[i], all[0], all, both, {"node2"}, true, 1);
            CHECK(r.served && !r.node.empty());
            if (std::string(packer) == "single-az-minimal-fragmentation") CHECK(r.node == "node2");
            ext.softReservationUsage[r.node].Add(Resources::Create(1, 1, 0));
        }
        // quirk 5: node2 carries reservations, its overhead counts twice on the first-fit route; node1 carries none
        ext.overhead["node2"] = Resources{Quantity::FromMilli(2001), Quantity(), Quantity()};
        ext.overhead["node1"] = Resources{Quantity::FromInt(3), Quantity(), Quantity()};
        r = BOTH(ext, cluster, all[3], all[0], all, both, {}, false, 1);
        CHECK(r.served && !r.node.empty());
        r = BOTH(ext, cluster, all[3], all[0], all, both, {"node1"}, false, 1);
        CHECK(r.served && !r.node.empty());
        ext.overhead["node1"] = Resources{Quantity::FromInt(8), Quantity(), Quantity()};
        ext.overhead["node2"] = Resources{Quantity::FromInt(3), Quantity(), Quantity()};
        r = BOTH(ext, cluster, all[3], all[0], all, both, {}, true, 1);
        CHECK(r.served);
    }
    {  // resource_test.go:127-170: the smaller capacity wins, the first-fit packers take the first node of the order
        Node node1 = NewNode("node1", "zone1"), node2 = NewNode("node2", "zone1");
        auto ext = NewTestExtender("single-az-minimal-fragmentation", {node1, node2});
        FlatCluster cluster;
        std::string err;
        CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
        Pod staticDriver = Driver("static-app", StaticAnnotations(0, "4", "1", "1", "1"));
        Pod dynDriver = Driver("dyn-app", DynamicAnnotations(0, 1, "1", "4", "1", "3"), 1);
        SelectNodeResult r = ext.selectDriverNode("batch-medium-priority", staticDriver, {"node1"}, ext.nodes);
        if (r.created) ext.reservations.push_back(*r.created);
        r = ext.selectDriverNode("batch-medium-priority", dynDriver, {"node2"}, ext.nodes);
        if (r.created) ext.reservations.push_back(*r.created);
        const std::vector<Pod> all = {staticDriver, dynDriver};
        r = BOTH(ext, cluster, Executor("dyn-app", 0), dynDriver, all, {"node1", "node2"}, {}, true, 1);
        CHECK(r.served && r.outcome == std::string(outcome::successScheduledExtraExecutor) && r.node == "node2");
        r = BOTH(ext, cluster, Executor("dyn-app", 0), dynDriver, all, {"node1", "node2"}, {"node1"}, true, 1);
        CHECK(r.served && r.node == "node1");  // an executor already running on node1 attracts the next one (:73-125)
        auto tight = NewTestExtender("single-az-tightly-pack", {node1, node2});
        tight.reservations = ext.reservations;
        r = BOTH(tight, cluster, Executor("dyn-app", 0), dynDriver, all, {"node1", "node2"}, {}, false, 1);
        CHECK(r.served && r.outcome == std::string(outcome::successRescheduled) && r.node == "node1");
        tight.overhead["node1"] = Resources{Quantity::FromMilli(2001), Quantity(), Quantity()};
        r = BOTH(tight, cluster, Executor("dyn-app", 0), dynDriver, all, {"node1", "node2"}, {}, false, 1);
        CHECK(r.served && r.node == "node2");  // 8 - 1 - 2 * 2.001 < 3: the overhead counted twice
    }
}

static void TestOverheadReservationsAndTheNextFilter() {
    const int n = 300, n_pending = 24;
    for (const char* packer : {"single-az-tightly-pack", "single-az-minimal-fragmentation"}) {
        SparkSchedulerExtender ext(SelectBinpacker(packer, g_ctx), NodeSorter(), true, FifoConfig{});
        ext.shouldScheduleDynamicallyAllocatedExecutorsInSameAZ = true;
        const char* zones[] = {"az-a", "az-b", "az-c"};
        std::vector<std::string> names;
        for (int i = 0; i < n; ++i) {
            Node nd;
            nd.Name = "n" + std::to_string(next() % 100000) + "-" + std::to_string(i);
            const char* z = zones[next() % 3];
            nd.labels[kLabelZoneFailureDomain] = z;
            nd.labels[kLabelTopologyZone] = z;
            nd.Allocatable = {{kResourceCPU, Quantity::FromInt(8 + 8 * (int64_t)(next() % 3))},
                              {kResourceMemory, Quantity::FromInt((int64_t)(32 + 32 * (next() % 3)) * Gi)},
                              {kResourceNvidiaGPU, Quantity::FromInt(next() % 10 == 0 ? 4 : 0)}};
            nd.Ready = next() % 20 != 0;
            nd.Unschedulable = next() % 25 == 0;
            names.push_back(nd.Name);
            ext.nodes.push_back(nd);
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
        ext.softReservationUsage[ext.nodes[7].Name] = Resources::Create(0, 0, 0);  // an entry of all zeros: node 7 is a key all the same
        for (int p = 0; p < n_pending; ++p) {
            Pod pod = Driver("pending-" + std::to_string(p), StaticAnnotations(1 + (int)(next() % 30), "2Gi", "1", "8Gi", "2"), p + 1);
            pod.Annotations.erase("spark-driver-nvidia.com/gpu");
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
        // ---- executor Filters of applications from small to larger than any node, offered varying subsets of the nodes
        const char* ecpu[] = {"1", "3", "7", "15", "40"};
        const char* emem[] = {"1Gi", "8Gi", "30Gi", "70Gi"};
        int placed = 0, refused = 0;
        for (int q = 0; q < 40; ++q) {
            const std::string app = "dyn-" + std::to_string(q);
            Pod driver = Driver(app, DynamicAnnotations(0, 4, "1Gi", "1", emem[next() % 4], ecpu[next() % 5]), 1);
            driver.Annotations.erase("spark-driver-nvidia.com/gpu");
            driver.NodeName = ext.nodes[next() % n].Name;
            driver.Phase = q % 5 == 4 ? "Pending" : "Running";
            Pod other = Executor(app, 7);
            other.NodeName = ext.nodes[next() % n].Name;  // q % 3 == 0: a second running pod, mostly in another zone
            other.Phase = q % 3 == 0 ? "Running" : "Pending";
            const std::vector<Pod> all = {driver, other};
            std::vector<std::string> offered;
            for (const std::string& name : names)
                if (q % 4 == 0 || next() % 3 != 0) offered.push_back(name);
            std::set<std::string> hosting;
            for (int h = 0; h < 5; ++h) hosting.insert(names[next() % n]);
            bool took = false;
            const SelectNodeResult got = ext.rescheduleExecutorFlat(Executor(app, 0), driver, all, offered, hosting, q % 2 == 0, cluster, &flat, &over, &took);
            // the installing route on an extender of its own: this one's record of the device stays as the flat route left it
            SparkSchedulerExtender installs = ext;
            const SelectNodeResult want = installs.rescheduleExecutor(Executor(app, 0), driver, all, offered, hosting, q % 2 == 0);
            CHECK(Same(got, want));
            if (!Same(got, want))
                std::printf("   %s request %d: flat (%s, %s, %s) installed (%s, %s, %s)\n", packer, q, got.node.c_str(), got.outcome.c_str(),
                            got.error.c_str(), want.node.c_str(), want.outcome.c_str(), want.error.c_str());
            CHECK(took == want.error.empty() || want.outcome == std::string(outcome::failureFit));
            placed += want.node.empty() ? 0 : 1;
            refused += want.outcome == std::string(outcome::failureFit) ? 1 : 0;
        }
        CHECK(placed >= 5 && refused >= 3);  // the comparison sees both answers
        // ---- warm driver Filter: twice, the second resumes; an executor Filter in between changes nothing of that
        const Pod& last = ext.pods.back();
        const SelectNodeResult first = ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat, &over);
        CHECK(first.served);
        const SelectNodeResult second = ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat, &over);
        CHECK(second.served && second.outcome == first.outcome && second.node == first.node);
        uint64_t gen0[3], gen1[3], st[4];
        CHECK(gf_generation(g_ctx, gen0) == GF_OK);
        Pod driver = Driver("dyn-warm", DynamicAnnotations(0, 4, "1Gi", "1", "8Gi", "3"), 1);
        driver.Annotations.erase("spark-driver-nvidia.com/gpu");
        driver.NodeName = names[11];
        driver.Phase = "Running";
        bool took = false;
        const SelectNodeResult x = ext.rescheduleExecutorFlat(Executor("dyn-warm", 0), driver, {driver}, names, {}, true, cluster, &flat, &over, &took);
        CHECK(took && x.served && !x.node.empty());
        CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0] && gen1[1] == gen0[1] && gen1[2] == gen0[2]);
        CHECK(gf_chain_cache_stats(g_ctx, 1, st) == GF_OK);
        const SelectNodeResult third = ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat, &over);
        CHECK(third.served && third.outcome == first.outcome && third.node == first.node);
        CHECK(gf_chain_cache_stats(g_ctx, 0, st) == GF_OK);
        CHECK(st[0] == 1 && st[1] == 1 && st[2] <= 2);
        if (!(st[0] == 1 && st[1] == 1 && st[2] <= 2))
            std::printf("   %s: chains %llu resumed %llu evaluated %llu skipped %llu\n", packer, (unsigned long long)st[0],
                        (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3]);
        CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0]);
        // ... while the installing route in between makes the next driver Filter cold: it bumps the snapshot epoch
        const SelectNodeResult y = ext.rescheduleExecutor(Executor("dyn-warm", 0), driver, {driver}, names, {}, true);
        CHECK(Same(x, y));
        CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] > gen0[0]);
    }
}

static void TestARefusedCallFallsBack() {
    // 70 zones: the entry point refuses (GF_ERR_UNSUPPORTED) and the installing route answers
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", g_ctx), NodeSorter(), true, FifoConfig{});
    std::vector<std::string> names;
    for (int i = 0; i < 70; ++i) {
        Node nd = NewNode("node" + std::to_string(100 + i), "zone");
        nd.labels[kLabelZoneFailureDomain] = "fd-" + std::to_string(100 + i);
        nd.Allocatable[kResourceMemory] = Quantity::FromInt((int64_t)(8 + i) * Gi);
        ext.nodes.push_back(nd);
        names.push_back(nd.Name);
    }
    FlatCluster cluster;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    CHECK(cluster.zone_labels.size() == 70);
    Pod driver = Driver("dyn-app", DynamicAnnotations(0, 2, "1", "1", "1", "1"), 1);
    uint64_t gen0[3], gen1[3];
    CHECK(gf_generation(g_ctx, gen0) == GF_OK);
    const SelectNodeResult r = BOTH(ext, cluster, Executor("dyn-app", 0), driver, {driver}, names, {}, true, 0);
    CHECK(r.served && !r.node.empty());
    CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] > gen0[0]);  // the installing route answered
    // a node the lister knows and the flat cluster does not: the other route as well
    ext.nodes.push_back(NewNode("late-node", "zone"));
    names.push_back("late-node");
    const SelectNodeResult r2 = BOTH(ext, cluster, Executor("dyn-app", 0), driver, {driver}, names, {}, false, 0);
    CHECK(r2.served && !r2.node.empty());
}

static void CpuHalf() {
    TestWhatIsDecidedBeforeTheDevice();
    TestRefusalsOfTheExecutorFilters();
}

static void GpuHalf() {
    TestDynamicAllocationSameAZ();
    TestSoftReservationsAndMinimalFragmentation();
    TestOverheadReservationsAndTheNextFilter();
    TestARefusedCallFallsBack();
}

int main(int argc, char** argv) { return RunHostTests(argc, argv, CpuHalf, GpuHalf); }
