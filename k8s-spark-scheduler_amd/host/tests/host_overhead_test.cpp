// host_overhead_test.cpp — the flat Filter route on a cluster WITH overhead (internal/extender/overhead.go:91-153: every production
// node carries the requests of its daemonsets and non-Spark pods).  selectDriverNodeFlat keeps the overhead columns resident and
// sends the rows that changed (gf_overhead_update); every answer must be the one selectDriverNode gives through the string-keyed
// maps, which installs its own snapshot per call and replays the whole chain like the reference (resource.go:309-328).
// `host_overhead_test cpu` needs no GPU (the row diff against a brute-force compare, overhead columns of the wrong length); `host_overhead_test gpu` drives the device
// through the C ABI.  Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define HOST_TEST_SEED 0x0E4D
#include "host_test_common.hpp"

// ------------------------------------------------------------------------------------------------ the row diff (no device)
static void TestRowDiff() {
    for (int round = 0; round < 200; ++round) {
        const uint32_t n = 1 + (uint32_t)(next() % 300);
        std::vector<int64_t> want[3], have[3];
        const bool want_empty = round % 7 == 3, have_empty = round % 5 == 2;
        const uint64_t change_one_in = 1 + next() % 40;
        for (int j = 0; j < 3; ++j) {
            if (!have_empty) have[j].resize(n);
            if (!want_empty) want[j].resize(n);
        }
        for (uint32_t i = 0; i < n; ++i)
            for (int j = 0; j < 3; ++j) {
                const int64_t h = next() % 3 == 0 ? 0 : (int64_t)(next() % 5) * 250;
                if (!have_empty) have[j][i] = h;
                if (!want_empty) want[j][i] = next() % change_one_in == 0 ? (int64_t)(next() % 5) * 250 : (have_empty ? 0 : h);
            }
        std::vector<uint32_t> brute;  // the definition: a row differs when any of its three values does; missing columns read zero
        for (uint32_t i = 0; i < n; ++i) {
            bool d = false;
            for (int j = 0; j < 3; ++j) d = d || (want_empty ? 0 : want[j][i]) != (have_empty ? 0 : have[j][i]);
            if (d) brute.push_back(i);
        }
        std::vector<uint32_t> rows = {12345};  // (cleared by the call)
        overheadRowDiff(want, have, n, &rows);
        CHECK(rows == brute);
    }
    std::vector<int64_t> none[3];
    std::vector<uint32_t> rows = {1};
    overheadRowDiff(none, none, 10, &rows);
    CHECK(rows.empty());
    overheadRowDiff(none, nullptr, 10, &rows);
    CHECK(rows.empty());
    std::vector<int64_t> some[3] = {{0, 5, 0}, {0, 0, 0}, {0, 0, 7}};
    overheadRowDiff(some, nullptr, 3, &rows);
    CHECK((rows == std::vector<uint32_t>{1, 2}));
    overheadRowDiff(nullptr, some, 3, &rows);
    CHECK((rows == std::vector<uint32_t>{1, 2}));
}

static Pod Driver(const std::string& app, int k, const char* emem, const char* ecpu, int64_t created_s) {
    Pod p;
    p.Name = app + "-spark-driver";
    p.Namespace = "namespace";
    p.labels = {{common::SparkRoleLabel, common::Driver}, {common::SparkAppIDLabel, app}};
    p.Annotations = {{"spark-driver-cpu", "1"},      {"spark-driver-mem", "2Gi"},   {"spark-executor-cpu", ecpu},
                     {"spark-executor-mem", emem},   {"spark-executor-count", std::to_string(k)}};
    p.SchedulerName = common::SparkSchedulerName;
    p.InstanceGroup = "batch-medium-priority";
    p.CreationTimestampNanos = created_s * 1000000000;
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

static Resources RandomOverhead() {  // a daemonset's worth: some cpu, some memory
    return Resources{Quantity::FromMilli(100 + 50 * (int64_t)(next() % 20)), Quantity::FromInt((int64_t)(256 + 128 * (next() % 16)) * Mi), Quantity()};
}

// ------------------------------------------------------------------------------------------------ no device
// Flat overhead columns of another length than the cluster are not this cluster's: the flat Filter does not serve the request, and
// says so before it touches its caches or a device.
static void TestOverheadColumnsOfTheWrongLength() {
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", nullptr), NodeSorter(), true, FifoConfig{});
    for (const char* name : {"node1", "node2"}) {
        Node nd;
        nd.Name = name;
        nd.Allocatable = {{kResourceCPU, Quantity::FromInt(8)}, {kResourceMemory, Quantity::FromInt(8 * Gi)}, {kResourceNvidiaGPU, Quantity::FromInt(0)}};
        nd.Ready = true;
        ext.nodes.push_back(nd);
    }
    ext.overhead["node1"] = Resources{Quantity::FromMilli(500), Quantity::FromInt(256 * Mi), Quantity()};
    FlatCluster cluster;
    FlatOverhead fo;
    std::string err;
    CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
    CHECK(FlatOverhead::Build(ext.overhead, cluster, &fo, &err) && fo.over[0].size() == 2);
    const Pod d = Driver("app", 1, "1Gi", "1", 1);
    ext.pods = {d};
    for (int j = 0; j < 3; ++j) {  // any one column is enough
        FlatOverhead wrong = fo;
        wrong.over[j].pop_back();
        const SelectNodeResult r = ext.selectDriverNodeFlat("batch-medium-priority", d, {"node1", "node2"}, cluster, nullptr, &wrong);
        CHECK(!r.served && r.node.empty() && r.error == "the flat overhead columns do not belong to this cluster");
    }
    CHECK(ext.flatCalls() == 0 && ext.clusterSetCalls() == 0);
}

// ------------------------------------------------------------------------------------------------ through the device
static void TestFiltersWithOverhead() {
    const int n = 400, n_pending = 60;
    for (const char* packer : {"tightly-pack", "single-az-tightly-pack"}) {
        SparkSchedulerExtender ext(SelectBinpacker(packer, g_ctx), NodeSorter(), true, FifoConfig{});
        const char* zones[] = {"az-a", "az-b", "az-c"};
        std::vector<std::string> names;
        for (int i = 0; i < n; ++i) {
            Node nd;
            nd.Name = "n" + std::to_string(next() % 100000) + "-" + std::to_string(i);
            nd.labels[kLabelZoneFailureDomain] = zones[next() % 3];
            nd.Allocatable = {{kResourceCPU, Quantity::FromInt(16 + 16 * (int64_t)(next() % 3))},
                              {kResourceMemory, Quantity::FromInt((int64_t)(64 + 64 * (next() % 3)) * Gi)},
                              {kResourceNvidiaGPU, Quantity::FromInt(0)}};
            nd.Ready = true;
            names.push_back(nd.Name);
            ext.nodes.push_back(nd);
            ext.overhead[nd.Name] = RandomOverhead();  // overhead on EVERY node
        }
        for (int r = 0; r < 40; ++r) {
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
        for (int p = 0; p < n_pending; ++p) {
            Pod pod = Driver("pending-" + std::to_string(p), 1 + (int)(next() % 30), emem[next() % 3], ecpu[next() % 3], p + 1);
            pod.UID = "uid-" + std::to_string(p);
            pod.ResourceVersion = 100 + (uint64_t)p;
            ext.pods.push_back(pod);
        }
        ext.nowNanos = (int64_t)(n_pending + 10) * 1000000000;
        FlatCluster cluster;
        FlatReservations flat;
        std::string err;
        CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
        CHECK(FlatReservations::Build(ext.reservations, ext.softReservationUsage, cluster, &flat, &err));
        const Pod& last = ext.pods.back();
        const Pod& before_last = ext.pods[(size_t)n_pending - 2];
        auto both = [&](const Pod& d) {  // the map route's answer first (it installs its own snapshot), then the flat route's
            const SelectNodeResult w = ext.selectDriverNode("batch-medium-priority", d, names, ext.nodes);
            const SelectNodeResult g = ext.selectDriverNodeFlat("batch-medium-priority", d, names, cluster, &flat);
            if (!SameAnswer(g, w))
                std::printf("   %s: flat (%d %s %s %s) map (%d %s %s)\n", packer, (int)g.served, g.outcome.c_str(), g.node.c_str(), g.error.c_str(),
                            (int)w.served, w.outcome.c_str(), w.node.c_str());
            return SameAnswer(g, w);
        };
        uint64_t gen0[3], gen1[3], st[4];
        // ---- the first Filter puts the cluster with its overhead columns on the device
        CHECK(both(last));
        CHECK(ext.clusterSetCalls() == 1 && ext.overheadUpdateCalls() == 0);
        // ---- unchanged overhead: the same Filter through the flat route alone, twice.  The first call rebuilds (the map route
        //      installed a snapshot in between); the second neither builds nor replays: at most two applications are evaluated
        const SelectNodeResult want_prev = ext.selectDriverNode("batch-medium-priority", before_last, names, ext.nodes);
        SelectNodeResult want_last = ext.selectDriverNode("batch-medium-priority", last, names, ext.nodes);
        CHECK(SameAnswer(ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat), want_last));
        CHECK(gf_generation(g_ctx, gen0) == GF_OK);
        CHECK(gf_chain_cache_stats(g_ctx, 1, st) == GF_OK);
        CHECK(SameAnswer(ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat), want_last));
        CHECK(gf_generation(g_ctx, gen1) == GF_OK);
        CHECK(gf_chain_cache_stats(g_ctx, 0, st) == GF_OK);
        CHECK(gen1[0] == gen0[0] && gen1[1] == gen0[1] && gen1[2] == gen0[2]);  // no build, no upload
        CHECK(st[0] == 1 && st[1] == 1 && st[2] <= 2);                         // one chain, resumed, <= 2 applications evaluated
        CHECK(ext.clusterSetCalls() == 1 && ext.overheadUpdateCalls() == 0 && ext.overheadRowsSent() == 0);
        // ... and the driver before it in the queue: still nothing moves
        CHECK(SameAnswer(ext.selectDriverNodeFlat("batch-medium-priority", before_last, names, cluster, &flat), want_prev));
        CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0]);
        // ---- one node's overhead changes: one row travels, the snapshot is rebuilt from the resident columns and usage
        for (int step = 0; step < 4; ++step) {
            const std::string& victim = names[next() % n];
            Resources o = RandomOverhead();
            if (step == 1) o = Resources{Quantity::FromInt(12), Quantity::FromInt(48 * Gi), Quantity()};  // a big pod landed: answers move
            while (o.Eq(ext.overhead[victim])) o = RandomOverhead();
            ext.overhead[victim] = o;
            const uint64_t calls = ext.overheadUpdateCalls(), rows = ext.overheadRowsSent(), sets = ext.clusterSetCalls();
            CHECK(gf_generation(g_ctx, gen0) == GF_OK);
            want_last = ext.selectDriverNode("batch-medium-priority", last, names, ext.nodes);
            CHECK(SameAnswer(ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat), want_last));
            CHECK(ext.overheadUpdateCalls() == calls + 1 && ext.overheadRowsSent() == rows + 1 && ext.clusterSetCalls() == sets);
            CHECK(gf_generation(g_ctx, gen1) == GF_OK);
            CHECK(gen1[2] == gen0[2]);  // the resident usage was neither reset nor sent again
        }
        // ---- a handful of nodes at once, one of them back to no overhead at all (the entry leaves the map)
        {
            for (int i = 0; i < 17; ++i) ext.overhead[names[next() % n]] = RandomOverhead();
            ext.overhead.erase(names[5]);
            const uint64_t calls = ext.overheadUpdateCalls(), rows = ext.overheadRowsSent(), sets = ext.clusterSetCalls();
            CHECK(both(before_last));
            CHECK(ext.overheadUpdateCalls() == calls + 1 && ext.clusterSetCalls() == sets);
            CHECK(ext.overheadRowsSent() > rows && ext.overheadRowsSent() <= rows + 18);
        }
        // ---- most nodes change: the columns travel whole (gf_cluster_set), the usage sums are sent again
        {
            for (int i = 0; i < n; ++i)
                if (i % 4 != 0) {
                    Resources o = RandomOverhead();
                    while (ext.overhead.count(names[i]) && o.Eq(ext.overhead[names[i]])) o = RandomOverhead();
                    ext.overhead[names[i]] = o;
                }
            const uint64_t calls = ext.overheadUpdateCalls(), sets = ext.clusterSetCalls();
            CHECK(both(last));
            CHECK(ext.overheadUpdateCalls() == calls && ext.clusterSetCalls() == sets + 1);
            CHECK(both(before_last));  // and the next Filter is on the resident route again
            CHECK(ext.overheadUpdateCalls() == calls && ext.clusterSetCalls() == sets + 1);
        }
        // ---- another extender on the same context replaces the resident cluster between two Filters: noticed, answered correctly
        {
            SparkSchedulerExtender other(SelectBinpacker(packer, g_ctx), NodeSorter(), true, FifoConfig{});
            for (int i = 0; i < 3; ++i) {
                Node nd = ext.nodes[(size_t)i];
                nd.Name = "other-" + std::to_string(i);
                other.nodes.push_back(nd);
                other.overhead[nd.Name] = RandomOverhead();
            }
            other.nowNanos = ext.nowNanos;
            FlatCluster oc;
            CHECK(FlatCluster::Build(other.nodes, &oc, &err));
            Pod small = Driver("small", 1, "1Gi", "1", 5);
            other.pods = {small};
            const SelectNodeResult o = other.selectDriverNodeFlat("batch-medium-priority", small, {"other-0", "other-1", "other-2"}, oc);
            CHECK(o.served && o.outcome == std::string(outcome::success));
            const uint64_t sets = ext.clusterSetCalls();
            want_last = ext.selectDriverNode("batch-medium-priority", last, names, ext.nodes);
            CHECK(SameAnswer(ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat), want_last));
            CHECK(ext.clusterSetCalls() == sets + 1);  // its own columns went up again
            // a foreign gf_overhead_update (the cluster generation moves, the node set stays): also noticed
            const uint32_t row = 3;
            const int64_t big[3] = {15000, 60 * Gi, 0};
            CHECK(gf_overhead_update(g_ctx, 1, &row, &big[0], &big[1], &big[2]) == GF_OK);
            CHECK(SameAnswer(ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat), want_last));
            CHECK(ext.clusterSetCalls() == sets + 2);
        }
        // ---- the overhead goes away altogether, then comes back on a few nodes: still the map route's answers
        {
            NodeGroupResources saved = ext.overhead;
            ext.overhead.clear();
            CHECK(both(last));
            int k = 0;
            for (const auto& [name, r] : saved)
                if (k++ % 50 == 0) ext.overhead[name] = r;
            const uint64_t calls = ext.overheadUpdateCalls();
            CHECK(both(last));
            CHECK(ext.overheadUpdateCalls() == calls + 1);  // a cluster resident WITHOUT overhead columns takes rows too
        }
        // ---- the overhead handed over in flat form (FlatOverhead): the same answers; an unchanged version is not even compared,
        //      a patched row travels alone
        {
            FlatOverhead fo;
            CHECK(FlatOverhead::Build(ext.overhead, cluster, &fo, &err));
            CHECK(both(last));  // (the map canonicalised by the Filter: whatever differs from before goes up now)
            uint64_t calls = ext.overheadUpdateCalls(), sets = ext.clusterSetCalls();
            want_last = ext.selectDriverNode("batch-medium-priority", last, names, ext.nodes);
            CHECK(SameAnswer(ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat, &fo), want_last));
            CHECK(gf_generation(g_ctx, gen0) == GF_OK);
            CHECK(SameAnswer(ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat, &fo), want_last));
            CHECK(gf_generation(g_ctx, gen1) == GF_OK && gen1[0] == gen0[0] && gen1[1] == gen0[1]);
            CHECK(ext.overheadUpdateCalls() == calls && ext.clusterSetCalls() == sets);  // the same columns as the map's: nothing sent
            const uint32_t victim = (uint32_t)(next() % n);
            ext.overhead[cluster.names[victim]] = Resources{Quantity::FromInt(9), Quantity::FromInt(40 * Gi), Quantity()};
            int64_t v[3];
            CHECK(ext.overhead[cluster.names[victim]].canonical(v));
            for (int j = 0; j < 3; ++j) fo.over[j][victim] = v[j];
            const uint64_t rows = ext.overheadRowsSent();
            want_last = ext.selectDriverNode("batch-medium-priority", last, names, ext.nodes);
            // patched but NOT touched: the version says "unchanged", and the Filter believes it (the host's contract) ...
            const SelectNodeResult stale = ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat, &fo);
            CHECK(stale.served && ext.overheadRowsSent() == rows);
            fo.Touch();  // ... a new version is compared: one row travels
            CHECK(SameAnswer(ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat, &fo), want_last));
            CHECK(ext.overheadUpdateCalls() == calls + 1 && ext.overheadRowsSent() == rows + 1 && ext.clusterSetCalls() == sets);
            FlatOverhead wrong = fo;
            for (int j = 0; j < 3; ++j) wrong.over[j].pop_back();
            CHECK(!ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster, &flat, &wrong).served);
        }
        // ---- reservations flattened per call (no resident usage): the overhead rows are resident all the same
        {
            ext.overhead[names[7]] = Resources{Quantity::FromInt(3), Quantity::FromInt(5 * Gi), Quantity()};
            const uint64_t calls = ext.overheadUpdateCalls();
            const SelectNodeResult w = ext.selectDriverNode("batch-medium-priority", last, names, ext.nodes);
            CHECK(SameAnswer(ext.selectDriverNodeFlat("batch-medium-priority", last, names, cluster), w));
            CHECK(ext.overheadUpdateCalls() == calls + 1);
        }
    }
}

static void CpuHalf() {
    TestRowDiff();
    TestOverheadColumnsOfTheWrongLength();
}

static void GpuHalf() {
    TestFiltersWithOverhead();
}

int main(int argc, char** argv) { return RunHostTests(argc, argv, CpuHalf, GpuHalf); }
