// host_filter_efficiency_test.cpp — SelectNodeResult::efficiency of the driver Filters (gf_filter_efficiency): a Filter with two
// earlier drivers through the string route (selectDriverNode), the flat route (selectDriverNodeFlat) and the group route
// (selectDriverNodeFlatGroup).  `efficiency` equals, bit for bit, the average computed HERE from gf_packing_efficiencies' rows
// taken over the chain's residual (the residual installed as a snapshot on a second context), summed in the fixed tree of
// include/gangfit.h: chunk partials by a balanced binary tree over 64 positions, partials per position in ascending chunk order,
// the 64 sums by the same tree.
// `host_filter_efficiency_test cpu` needs no GPU; `host_filter_efficiency_test gpu` drives the device through the C ABI.
// Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#define HOST_TEST_SEED 0xEFF1
#include "host_test_common.hpp"

static gf_ctx* g_rows = nullptr;  // where the residual is installed for gf_packing_efficiencies

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

static Node NewNode(const std::string& name, const char* zone) {
    Node nd;
    nd.Name = name;
    nd.labels[kLabelZoneFailureDomain] = zone;
    nd.Allocatable = {{kResourceCPU, Quantity::FromInt(16 + 16 * (int64_t)(next() % 3))},
                      {kResourceMemory, Quantity::FromInt((int64_t)(64 + 64 * (next() % 3)) * Gi)},
                      {kResourceNvidiaGPU, Quantity::FromInt(next() % 3 == 0 ? 4 : 0)}};
    nd.Ready = true;
    return nd;
}

// ------------------------------------------------------------------------------------------------ the tree, on the host
static double Tree64(double* v) {
    for (int w = 64; w > 1; w /= 2)
        for (int i = 0; i < w / 2; ++i) v[i] = v[2 * i] + v[2 * i + 1];
    return v[0];
}

// rows: n x 3 {cpu, memory, gpu}; sched_gpu: n; members: nullable bit row.
static AvgPackingEfficiency TreeAverage(const std::vector<double>& rows, const std::vector<int64_t>& sched_gpu,
                                        const std::vector<uint64_t>* members, uint32_t n) {
    const uint32_t n_chunks = (n + 63) / 64, n_pad = (n_chunks + 63) / 64 * 64;
    std::vector<double> part[4];
    for (auto& p : part) p.assign(n_pad, 0.0);
    uint64_t len = 0, with_gpu = 0;
    for (uint32_t c = 0; c < n_chunks; ++c) {
        double v[4][64];
        for (int l = 0; l < 64; ++l) {
            const uint32_t node = c * 64 + (uint32_t)l;
            const bool key = node < n && (members == nullptr || (((*members)[node >> 6] >> (node & 63u)) & 1ull));
            const bool gpu = key && sched_gpu[node] != 0;
            const double e0 = key ? rows[3 * (size_t)node] : 0.0, e1 = key ? rows[3 * (size_t)node + 1] : 0.0;
            const double e2 = key ? rows[3 * (size_t)node + 2] : 0.0;
            const double m = e0 > e1 ? e0 : e1;
            v[0][l] = e0;
            v[1][l] = e1;
            v[2][l] = gpu ? e2 : 0.0;
            v[3][l] = key ? (e2 > m ? e2 : m) : 0.0;
            len += key ? 1 : 0;
            with_gpu += gpu ? 1 : 0;
        }
        for (int f = 0; f < 4; ++f) part[f][c] = Tree64(v[f]);
    }
    double sum[4];
    for (int f = 0; f < 4; ++f) {
        double acc[64];
        for (double& a : acc) a = 0.0;
        for (uint32_t c = 0; c < n_pad; ++c) acc[c & 63u] += part[f][c];
        sum[f] = Tree64(acc);
    }
    AvgPackingEfficiency out;
    if (len == 0) return out;
    out.CPU = sum[0] / (double)len;
    out.Memory = sum[1] / (double)len;
    out.GPU = with_gpu == 0 ? 1.0 : sum[2] / (double)with_gpu;
    out.Max = sum[3] / (double)len;
    return out;
}

static bool SameBits(const AvgPackingEfficiency& a, const AvgPackingEfficiency& b) {
    const double x[4] = {a.CPU, a.Memory, a.GPU, a.Max}, y[4] = {b.CPU, b.Memory, b.GPU, b.Max};
    return std::memcmp(x, y, sizeof x) == 0;
}

// What the Filter that just returned `r` on g_ctx must have reported: `names` = node index -> name of the snapshot it installed.
static bool Expected(gf_algo algo, const Pod& driver, const SelectNodeResult& r, const std::vector<std::string>& names,
                     const std::vector<uint64_t>* members, AvgPackingEfficiency* want, bool* chain_committed) {
    const uint32_t n = (uint32_t)names.size();
    std::map<std::string, uint32_t> index;
    for (uint32_t i = 0; i < n; ++i) index[names[i]] = i;
    std::vector<int64_t> snap(3 * (size_t)n), sched(3 * (size_t)n), resid(3 * (size_t)n);
    if (gf_snapshot_get(g_ctx, snap.data(), sched.data()) != GF_OK || gf_residual_get(g_ctx, resid.data()) != GF_OK) return false;
    *chain_committed = snap != resid;
    std::vector<int64_t> a[3], s[3];
    for (int j = 0; j < 3; ++j)
        for (uint32_t i = 0; i < n; ++i) {
            a[j].push_back(resid[3 * (size_t)i + j]);
            s[j].push_back(sched[3 * (size_t)i + j]);
        }
    if (gf_snapshot_set(g_rows, n, a[0].data(), a[1].data(), a[2].data(), s[0].data(), s[1].data(), s[2].data()) != GF_OK) return false;
    auto resources = sparkResources(driver, nullptr);
    if (!resources || !r.created) return false;
    gf_app app{};
    if (!resources->DriverResources.canonical(app.drv) || !resources->ExecutorResources.canonical(app.exe)) return false;
    app.k = resources->MinExecutorCount;
    gf_result res{};
    res.has_capacity = 1;
    res.driver_node = index.at(r.node);
    res.exec_len = (uint32_t)app.k;
    res.evaluated = 1;
    std::vector<uint32_t> exec;
    for (int i = 0; i < app.k; ++i) exec.push_back(index.at(r.created->Reservations.at(executorReservationName(i)).Node));
    exec.push_back(0);
    std::vector<double> rows(3 * (size_t)n);
    if (gf_packing_efficiencies(g_rows, algo, &app, &res, exec.data(), rows.data()) != GF_OK) return false;
    *want = TreeAverage(rows, s[2], members, n);
    return true;
}

// ------------------------------------------------------------------------------------------------ no device
static void TestWhatNeedsNoDevice() {
    SparkSchedulerExtender ext(SelectBinpacker("tightly-pack", nullptr), NodeSorter(), true, FifoConfig{});
    ext.nodes = {NewNode("node1", "az-a"), NewNode("node2", "az-b")};
    ext.nowNanos = 1000ll * 1000000000;
    // a driver whose reservation exists is answered from it: no pack, no efficiency
    Pod bound = Driver("bound", "group-a", 2, "1Gi", "1", 1);
    ResourceReservation rr;
    rr.Name = "bound";
    rr.Namespace = "namespace";
    Reservation res;
    res.Node = "node2";
    rr.Reservations["driver"] = res;
    ext.reservations.push_back(rr);
    const SelectNodeResult got = ext.selectDriverNode("group-a", bound, {"node1", "node2"}, ext.nodes);
    CHECK(got.served && got.node == "node2" && got.outcome == std::string(outcome::success) && !got.has_efficiency);
    // the tree: a pair inside one chunk survives where a serial sum loses it
    std::vector<double> rows(3 * 64, 0.0);
    rows[0] = 1.0;
    rows[3 * 2] = rows[3 * 3] = 0x1p-53;
    const AvgPackingEfficiency t = TreeAverage(rows, std::vector<int64_t>(64, 0), nullptr, 64);
    CHECK(t.CPU * 64.0 == 1.0 + 0x1p-52 && t.GPU == 1.0);
}

// ------------------------------------------------------------------------------------------------ through the device
static void TestFilterWithTwoEarlierDrivers() {
    const int n = 150;
    const char* zones[] = {"az-a", "az-b", "az-c"};
    for (const char* packer : {"tightly-pack", "distribute-evenly", "single-az-tightly-pack", "single-az-minimal-fragmentation"}) {
        const Binpacker bp = SelectBinpacker(packer, g_ctx);
        CHECK(bp.Name == packer);
        SparkSchedulerExtender ext(bp, NodeSorter(), true, FifoConfig{});
        std::vector<std::string> names;
        std::map<std::string, std::vector<Node>> groups;
        std::map<std::string, std::vector<std::string>> group_node_names;
        for (int i = 0; i < n; ++i) {
            Node nd = NewNode("n" + std::to_string(next() % 100000) + "-" + std::to_string(i), zones[next() % 3]);
            names.push_back(nd.Name);
            ext.nodes.push_back(nd);
            const char* g = i % 3 == 0 ? "group-b" : "group-a";
            groups[g].push_back(nd);
            group_node_names[g].push_back(nd.Name);
        }
        for (int r = 0; r < 25; ++r) {  // running applications
            ResourceReservation rr;
            rr.Name = "running-" + std::to_string(r);
            rr.Namespace = "namespace";
            const int k = 1 + (int)(next() % 8);
            for (int e = 0; e <= k; ++e) {
                Reservation res;
                res.Node = ext.nodes[next() % n].Name;
                res.Resources = {{kResourceCPU, Quantity::FromMilli(500 + 250 * (int64_t)(next() % 6))},
                                 {kResourceMemory, Quantity::FromInt((int64_t)(2 + next() % 6) * Gi + (int64_t)(next() % 1000))},
                                 {kResourceNvidiaGPU, Quantity::FromInt(0)}};
                rr.Reservations[e == 0 ? "driver" : executorReservationName(e - 1)] = res;
            }
            ext.reservations.push_back(rr);
        }
        for (int p = 0; p < 3; ++p) {  // two earlier drivers and the one being filtered, per group
            for (const char* g : {"group-a", "group-b"}) {
                Pod pod = Driver(std::string("pending-") + g + "-" + std::to_string(p), g, 3 + p, "4Gi", "1500m", 10 * p + (g[6] == 'a' ? 1 : 2));
                pod.UID = "uid-" + pod.Name;
                pod.ResourceVersion = 100 + (uint64_t)p;
                ext.pods.push_back(pod);
            }
        }
        ext.nowNanos = 1000ll * 1000000000;
        const Pod& a_driver = ext.pods[4];  // group-a's third
        const Pod& b_driver = ext.pods[5];
        CHECK(a_driver.InstanceGroup == "group-a" && b_driver.InstanceGroup == "group-b");
        AvgPackingEfficiency want;
        bool committed = false;

        // ---- the string route on the whole cluster: node index = rank of the name (metadata keys, sorted)
        {
            SparkSchedulerExtender maps = ext;
            const SelectNodeResult r = maps.selectDriverNode("group-a", a_driver, names, ext.nodes);
            CHECK(r.served && r.outcome == std::string(outcome::success) && r.has_efficiency);
            std::map<std::string, int> sorted;
            for (const std::string& nm : names) sorted[nm] = 0;
            std::vector<std::string> by_index;
            for (const auto& kv : sorted) by_index.push_back(kv.first);
            CHECK(Expected(bp.Algo, a_driver, r, by_index, nullptr, &want, &committed));
            CHECK(committed);  // against the residual, not the snapshot
            CHECK(SameBits(r.efficiency, want));
            CHECK(r.efficiency.Max > 0.0 && r.efficiency.GPU != 1.0);
            // FIFO off: one application, against the snapshot
            SparkSchedulerExtender plain(bp, NodeSorter(), false, FifoConfig{});
            plain.nodes = ext.nodes;
            plain.reservations = ext.reservations;
            plain.pods = ext.pods;
            plain.nowNanos = ext.nowNanos;
            const SelectNodeResult q = plain.selectDriverNode("group-a", a_driver, names, ext.nodes);
            CHECK(q.served && q.has_efficiency);
            CHECK(Expected(bp.Algo, a_driver, q, by_index, nullptr, &want, &committed));
            CHECK(!committed && SameBits(q.efficiency, want) && !SameBits(q.efficiency, r.efficiency));
        }
        // ---- the flat route on the whole cluster: node index = the cluster's
        FlatCluster cluster;
        FlatReservations flat;
        FlatOverhead over;
        std::string err;
        CHECK(FlatCluster::Build(ext.nodes, &cluster, &err));
        CHECK(FlatReservations::Build(ext.reservations, ext.softReservationUsage, cluster, &flat, &err));
        CHECK(FlatOverhead::Build(ext.overhead, cluster, &over, &err));
        {
            const SelectNodeResult r = ext.selectDriverNodeFlat("group-a", a_driver, names, cluster, &flat, &over);
            CHECK(r.served && r.outcome == std::string(outcome::success) && r.has_efficiency);
            CHECK(Expected(bp.Algo, a_driver, r, cluster.names, nullptr, &want, &committed));
            CHECK(committed);
            CHECK(SameBits(r.efficiency, want));
            SparkSchedulerExtender maps = ext;
            const SelectNodeResult s = maps.selectDriverNode("group-a", a_driver, names, ext.nodes);
            CHECK(s.node == r.node && s.outcome == r.outcome);  // (the two routes index the nodes differently: another tree, not another Filter)
        }
        // ---- the group route: the keys are group-b's members inside the resident cluster
        {
            std::vector<uint64_t> members((cluster.names.size() + 63) / 64, 0);
            for (const Node& node : groups["group-b"]) members[cluster.index.at(node.Name) >> 6] |= 1ull << (cluster.index.at(node.Name) & 63u);
            const SelectNodeResult r = ext.selectDriverNodeFlatGroup("group-b", b_driver, group_node_names["group-b"], cluster, groups["group-b"], &flat, &over);
            CHECK(r.served && r.outcome == std::string(outcome::success) && r.has_efficiency);
            uint32_t info[4];
            CHECK(gf_snapshot_set_info(g_ctx, info) == GF_OK && info[0] == 1 && info[1] == groups["group-b"].size());
            CHECK(Expected(bp.Algo, b_driver, r, cluster.names, &members, &want, &committed));
            CHECK(committed);
            CHECK(SameBits(r.efficiency, want));
        }
    }
}

static void CpuHalf() {
    TestWhatNeedsNoDevice();
}

static void GpuHalf() {
    if (gf_init(nullptr, 0, &g_rows) != GF_OK) {
        std::printf("FAIL gf_init: no gfx950 device (there is no CPU fallback)\n");
        std::exit(2);
    }
    TestFilterWithTwoEarlierDrivers();
    gf_destroy(g_rows);
}

int main(int argc, char** argv) { return RunHostTests(argc, argv, CpuHalf, GpuHalf); }
