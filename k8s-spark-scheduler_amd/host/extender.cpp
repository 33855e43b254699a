#include "extender.hpp"

#include <cstring>
#include <algorithm>
#include <atomic>

namespace gangfit::host {

// ---------------------------------------------------------------------------------------------------------------------------------
// The steps the routes below share, each written once.
namespace {

SelectNodeResult notServed(std::string why) {  // the accelerator cannot take the request: the Go host runs its own path
    SelectNodeResult r;
    r.served = false;
    r.error = std::move(why);
    return r;
}

SelectNodeResult failure(const char* outcome, std::string error) {  // the reference's own failure
    SelectNodeResult r;
    r.outcome = outcome;
    r.error = std::move(error);
    return r;
}

// A quantity triple the device columns can hold: exactly representable and not negative.
bool canonicalNonNegative(const Resources& r, int64_t v[3]) { return r.canonical(v) && v[0] >= 0 && v[1] >= 0 && v[2] >= 0; }

// an application that already holds a reservation keeps its driver node (resource.go:278-291); nullopt: it holds none
std::optional<SelectNodeResult> answerFromReservation(const std::vector<ResourceReservation>& reservations, const Pod& driver) {
    auto app_label = driver.labels.find(common::SparkAppIDLabel);
    const std::string app_id = app_label == driver.labels.end() ? "" : app_label->second;
    for (const ResourceReservation& rr : reservations)
        if (rr.Name == app_id && rr.Namespace == driver.Namespace) {
            SelectNodeResult out;
            auto d = rr.Reservations.find("driver");
            out.node = d == rr.Reservations.end() ? "" : d->second.Node;
            out.outcome = outcome::success;
            return out;
        }
    return std::nullopt;
}

// SparkResources as a chain application; false: not exactly representable (*app is then unspecified).
bool toApp(const SparkApplicationResources& r, gf_app* app) {
    *app = gf_app{};
    if (!r.DriverResources.canonical(app->drv) || !r.ExecutorResources.canonical(app->exe) || r.MinExecutorCount < 0 ||
        r.MinExecutorCount > GF_MAX_K)
        return false;
    app->k = r.MinExecutorCount;
    return true;
}

// {pod name, exceedsCapacity} of a feasibility batch, in listing order
std::vector<std::pair<std::string, bool>> scanResult(const std::vector<const Pod*>& pods, const std::vector<uint8_t>& fits) {
    std::vector<std::pair<std::string, bool>> out;
    for (size_t i = 0; i < pods.size(); ++i) out.emplace_back(pods[i]->Name, fits[i] == 0);
    return out;
}

// Dense overhead columns as the C ABI takes them: three NULLs stand for "no overhead anywhere" (empty columns).
struct OverheadColumns {
    const int64_t* col[3];
};
OverheadColumns nullableColumns(const std::vector<int64_t> over[3]) {
    const bool with_over = !over[0].empty();
    return {{with_over ? over[0].data() : nullptr, with_over ? over[1].data() : nullptr, with_over ? over[2].data() : nullptr}};
}

// `list` (Nodes, or pointers to them) as a bit row over `cluster`'s node index, ORed into row[ceil(n / 64)]; `keep` may narrow
// the list.  false: the list names a node outside the cluster, and the walk ended there.
const Node& nodeOf(const Node& n) { return n; }
const Node& nodeOf(const Node* n) { return *n; }
bool everyNode(const Node&) { return true; }
template <class List, class Keep = bool (*)(const Node&)>
bool nodeBitRow(const FlatCluster& cluster, const List& list, uint64_t* row, Keep keep = everyNode) {
    for (const auto& item : list) {
        const Node& node = nodeOf(item);
        const auto at = cluster.index.find(node.Name);
        if (at == cluster.index.end()) return false;
        if (keep(node)) row[at->second >> 6] |= UINT64_C(1) << (at->second & 63u);
    }
    return true;
}

// A request's NodeNames as one number, order-sensitive across names.
// (eight bytes per multiply: a byte-at-a-time hash of 100 000 names is a 1.5 ms dependent chain)
uint64_t hashNodeNames(const std::vector<std::string>& nodeNames) {
    uint64_t names_hash = 1469598103934665603ull;
    for (const std::string& name : nodeNames) {
        const char* p = name.data();
        size_t left = name.size();
        uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)left;
        for (; left >= 8; left -= 8, p += 8) {
            uint64_t w;
            std::memcpy(&w, p, 8);
            h = (h ^ w) * 0xFF51AFD7ED558CCDull;
            h ^= h >> 29;
        }
        if (left) {
            uint64_t w = 0;
            std::memcpy(&w, p, left);
            h = (h ^ w) * 0xC4CEB9FE1A85EC53ull;
            h ^= h >> 31;
        }
        names_hash = (names_hash ^ h) * 1099511628211ull;  // order-sensitive across names; h of each name is independent work
    }
    return names_hash;
}

// The executor Filter's answer (resource.go:657-673): names = node index -> name of what the device was asked about.
SelectNodeResult executorAnswer(uint32_t node, const std::vector<std::string>& names, bool isExtraExecutor) {
    if (node == GF_NO_NODE) return failure(outcome::failureFit, "not enough capacity to reschedule the executor");
    SelectNodeResult out;
    out.node = names[node];
    out.outcome = isExtraExecutor ? outcome::successScheduledExtraExecutor : outcome::successRescheduled;
    return out;
}

}  // namespace

std::string executorReservationName(int i) { return "executor-" + std::to_string(i + 1); }

ResourceReservation newResourceReservation(const std::string& driverNode, const std::vector<std::string>& executorNodes,
                                           const Pod& driver, const Resources& d, const Resources& e) {
    ResourceReservation rr;
    auto list = [](const Resources& r) {
        return ResourceList{{kResourceCPU, r.CPU}, {kResourceMemory, r.Memory}, {kResourceNvidiaGPU, r.NvidiaGPU}};
    };
    rr.Reservations["driver"] = {driverNode, list(d)};
    for (size_t i = 0; i < executorNodes.size(); ++i)
        rr.Reservations[executorReservationName((int)i)] = {executorNodes[i], list(e)};
    auto app = driver.labels.find(common::SparkAppIDLabel);
    rr.Name = app == driver.labels.end() ? "" : app->second;
    rr.AppIDLabel = rr.Name;
    rr.Namespace = driver.Namespace;
    rr.OwnerPodName = driver.Name;
    rr.Pods["driver"] = driver.Name;
    return rr;
}

bool SparkSchedulerExtender::shouldSkipDriverFifo(const Pod& pod, const std::string& instanceGroup) const {
    int64_t age = fifo_.DefaultEnforceAfterPodAgeNanos;
    if (auto it = fifo_.EnforceAfterPodAgeByInstanceGroup.find(instanceGroup); it != fifo_.EnforceAfterPodAgeByInstanceGroup.end())
        age = it->second;
    return pod.CreationTimestampNanos + age > nowNanos;
}

// computeAvgPackingEfficiencyForResult (resource.go:329, 372-381) of the pack a chain just made: over every key of the installed
// snapshot (row: the keys inside a resident cluster, nullptr = all), against what fitEarlierDrivers left when FIFO is on.
static void fillEfficiency(gf_ctx* ctx, gf_algo algo, bool fifo, const gf_app& app, const gf_result& result, const uint32_t* exec_nodes,
                           const uint64_t* row, SelectNodeResult* out) {
    gf_avg_efficiency avg{};
    if (gf_filter_efficiency(ctx, algo, fifo ? GF_EFF_AGAINST_RESIDUAL : GF_EFF_AGAINST_SNAPSHOT, &app, &result, exec_nodes, row, &avg,
                             nullptr) != GF_OK)
        return;
    out->efficiency = AvgPackingEfficiency{avg.cpu, avg.memory, avg.gpu, avg.max};
    out->has_efficiency = true;
}

// A pod's annotations as a chain application (sparkResources, then toApp).  The flat route's cache holds what this returns per
// (pod, resourceVersion); the string route calls it afresh.
SparkSchedulerExtender::PodApp SparkSchedulerExtender::podApp(const Pod& pod, std::string* err) {
    PodApp pa;
    auto r = sparkResources(pod, err);
    pa.parsed = r.has_value();
    pa.representable = pa.parsed && toApp(*r, &pa.app);
    return pa;
}

// The stale pending drivers of this scheduler in listing order (unschedulablepods.go:93-129).  An unparsable pod ends the listing
// there, as the reference returns from the scan ("failed to check if pod was unschedulable", unschedulablepods.go:112-116); a pod
// that is not exactly representable is listed like any other (its app is unspecified) and the first such pod is reported.  What to
// do about either is each scan's own decision.
SparkSchedulerExtender::StaleDrivers SparkSchedulerExtender::listStaleDrivers(const std::vector<Pod>& allPods, int64_t timeoutNanos) const {
    if (timeoutNanos <= 0) timeoutNanos = 600ll * 1000000000;  // 10 minutes (unschedulablepods.go:62-64)
    StaleDrivers stale;
    for (const Pod& pod : allPods) {
        auto role = pod.labels.find(common::SparkRoleLabel);
        if (pod.SchedulerName != common::SparkSchedulerName || !pod.NodeName.empty() || pod.Deleting ||
            role == pod.labels.end() || role->second != common::Driver || pod.CreationTimestampNanos + timeoutNanos >= nowNanos)
            continue;
        const PodApp pa = podApp(pod, &stale.parse_error);
        if (!pa.parsed) {
            stale.stopped = true;
            break;
        }
        if (!pa.representable && stale.unrepresentable == nullptr) stale.unrepresentable = &pod;
        stale.pods.push_back(&pod);
        stale.apps.push_back(pa.app);
    }
    return stale;
}

// fitEarlierDrivers' applications in creation order (resource.go:224-270), appended to *apps; app_of(pod) gives a pod's PodApp.
// false: an earlier driver is not exactly representable (*why names it).
template <class AppOf>
bool SparkSchedulerExtender::earlierDriverApps(const std::string& instanceGroup, const Pod& driver, AppOf app_of, std::vector<gf_app>* apps,
                                               std::string* why) const {
    if (!isFIFO_) return true;
    for (const Pod* p : filterToEarliestAndSort(driver, pods)) {
        const PodApp& pa = app_of(*p);
        if (!pa.parsed) continue;  // "failed to get driver resources, skipping driver" (resource.go:231-237)
        if (!pa.representable) {
            *why = "earlier driver " + p->Name + " is not exactly representable";
            return false;
        }
        gf_app a = pa.app;
        a.flags = shouldSkipDriverFifo(*p, instanceGroup) ? GF_APP_SKIPPABLE : 0u;  // (the skip flag depends on the clock)
        apps->push_back(a);
    }
    return true;
}

// FIFO replay + final pack as one chain on the installed snapshot (resource.go:309-328), as the Filter's answer.  apps: the earlier
// drivers, then the one being filtered; names: node index -> name of the snapshot; row: the keys of the efficiency (fillEfficiency).
SelectNodeResult SparkSchedulerExtender::fitChain(gf_ctx* ctx, const std::vector<gf_app>& apps, const std::vector<std::string>& names,
                                                  const uint64_t* row, const Pod& driver, const SparkApplicationResources& resources) const {
    uint64_t total_k = 0;
    for (const gf_app& a : apps) total_k += (uint64_t)a.k;
    std::vector<gf_result> results(apps.size());
    std::vector<uint32_t> exec(total_k + 1);
    int32_t failed_at = -1;
    if (gf_fit_batch(ctx, GF_MODE_FIFO_CHAIN, binpacker_.Algo, (uint32_t)apps.size(), apps.data(), results.data(), exec.data(), total_k,
                     &failed_at) != GF_OK)
        return notServed(std::string("gf_fit_batch: ") + gf_last_error(ctx));
    if (failed_at >= 0)  // resource.go:315-318
        return failure(outcome::failureEarlierDriver, "earlier drivers do not fit to the cluster");
    const gf_app& cur = apps.back();
    const gf_result& last = results.back();
    if (!last.has_capacity)  // resource.go:346-349
        return failure(outcome::failureFit, "application does not fit to the cluster");
    SelectNodeResult out;
    std::vector<std::string> executorNodes;
    const uint64_t off = total_k - (uint64_t)cur.k;
    for (uint32_t i = 0; i < last.exec_len; ++i) executorNodes.push_back(names[exec[off + i]]);
    out.node = names[last.driver_node];
    out.outcome = outcome::success;
    fillEfficiency(ctx, binpacker_.Algo, isFIFO_, cur, last, exec.data() + off, row, &out);
    out.created = newResourceReservation(out.node, executorNodes, driver, resources.DriverResources, resources.ExecutorResources);
    return out;
}

SelectNodeResult SparkSchedulerExtender::selectDriverNode(const std::string& instanceGroup, const Pod& driver,
                                                          const std::vector<std::string>& nodeNames,
                                                          const std::vector<Node>& availableNodes) {
    if (auto held = answerFromReservation(reservations, driver)) return *held;
    // snapshot (resource.go:300-303)
    NodeGroupResources usage = UsageForNodes(reservations);
    for (const auto& [n, r] : softReservationUsage) usage[n].Add(r);
    NodeGroupSchedulingMetadata metadata = NodeSchedulingMetadataForNodes(availableNodes, usage, overhead);
    auto [driverNodeNames, executorNodeNames] = sorter_.PotentialNodes(metadata, nodeNames);
    std::string err;
    auto resources = sparkResources(driver, &err);
    if (!resources) return failure(outcome::failureInternal, "failed to get spark resources: " + err);
    // the applications: earlier drivers in creation order, then this one
    // (this route parses every pod afresh and never touches parsed_apps_: the cache and its prune belong to the flat route,
    //  under flat_mu_)
    std::vector<gf_app> apps;
    if (!earlierDriverApps(instanceGroup, driver, [](const Pod& p) { return podApp(p, nullptr); }, &apps, &err)) return notServed(err);
    gf_app cur;
    if (!toApp(*resources, &cur)) return notServed("application resources are not exactly representable");
    apps.push_back(cur);
    FlatSnapshot snap;
    CtxSequence seq(binpacker_.ctx);
    if (!flatten(metadata, driverNodeNames, executorNodeNames, &snap, &err) || !upload(binpacker_.ctx, snap, &err)) return notServed(err);
    return fitChain(binpacker_.ctx, apps, snap.names, nullptr, driver, *resources);
}

SelectNodeResult SparkSchedulerExtender::rescheduleExecutor(const Pod& driver, const std::vector<std::string>& nodeNames,
                                                            const std::vector<Node>& availableNodes,
                                                            const std::set<std::string>& nodesHostingApp,
                                                            bool isExtraExecutor) {
    std::string err;
    auto resources = sparkResources(driver, &err);
    if (!resources) return failure(outcome::failureInternal, err);
    int64_t exe[3];
    if (!canonicalNonNegative(resources->ExecutorResources, exe)) return notServed("executor resources are not exactly representable");
    NodeGroupResources usage = UsageForNodes(reservations);  // GetReservedResources
    for (const auto& [n, r] : softReservationUsage) usage[n].Add(r);
    std::set<std::string> had_usage;
    for (const auto& kv : usage) had_usage.insert(kv.first);
    NodeGroupSchedulingMetadata metadata = NodeSchedulingMetadataForNodes(availableNodes, usage, overhead);
    auto [driverOrder, executorNodeNames] = sorter_.PotentialNodes(metadata, nodeNames);
    (void)driverOrder;
    FlatSnapshot snap;
    CtxSequence seq(binpacker_.ctx);
    if (!flatten(metadata, {}, executorNodeNames, &snap, &err) || !upload(binpacker_.ctx, snap, &err)) return notServed(err);
    const bool minfrag = binpacker_.Name == "single-az-minimal-fragmentation";
    // what this path subtracts on top of the snapshot: `usage.Add(overhead)` (:642) counts the overhead a second time
    // for nodes NodeSchedulingMetadataForNodes already updated in place; GetNodeCapacities (:682) is handed the
    // overhead map as reservedResources
    std::vector<int64_t> reserved(3 * snap.names.size(), 0);
    bool any_reserved = false;
    for (size_t i = 0; i < snap.names.size(); ++i) {
        auto o = overhead.find(snap.names[i]);
        if (o == overhead.end()) continue;
        if (!minfrag && !had_usage.count(snap.names[i])) continue;
        int64_t v[3];
        if (!canonicalNonNegative(o->second, v)) return notServed("overhead of node " + snap.names[i] + " is not exactly representable");
        for (int j = 0; j < 3; ++j) reserved[3 * i + j] = v[j];
        any_reserved = true;
    }
    std::vector<uint32_t> hosts((snap.names.size() + 31) / 32, 0u);
    for (const std::string& n : nodesHostingApp)
        if (auto it = snap.index.find(n); it != snap.index.end()) hosts[it->second >> 5] |= 1u << (it->second & 31);
    uint32_t node = GF_NO_NODE;
    if (gf_executor_fit(binpacker_.ctx, minfrag ? 1 : 0, 1, exe, any_reserved ? reserved.data() : nullptr,
                        minfrag ? hosts.data() : nullptr, &node) != GF_OK)
        return notServed(std::string("gf_executor_fit: ") + gf_last_error(binpacker_.ctx));
    return executorAnswer(node, snap.names, isExtraExecutor);
}

bool filterNodesToZone(const std::vector<Node>& initialNodes, const std::string& zone, std::vector<Node>* out, std::string* err) {
    out->clear();
    for (const Node& node : initialNodes) {
        auto z = node.labels.find(kLabelTopologyZone);
        if (z == node.labels.end()) {  // resource.go:466-468
            if (err) *err = "Could not read zone label from node, unable to make scheduling decisions based on AZ";
            return false;
        }
        if (z->second == zone) out->push_back(node);
    }
    return true;
}

std::pair<std::string, bool> SparkSchedulerExtender::getCommonZoneForExecutorsApplication(const Pod& executor,
                                                                                         const std::vector<Pod>& allPods,
                                                                                         std::string* err) const {
    if (err) err->clear();
    auto label = executor.labels.find(common::SparkAppIDLabel);
    if (label == executor.labels.end()) {  // :494-497
        if (err) *err = "Executor does not have a Spark app id label, could not create label selector";
        return {"", false};
    }
    std::set<std::string> azs;
    for (const Pod& pod : allPods) {  // podLister.Pods(namespace).List(selector spark-app-id == label), :548-555
        if (pod.Namespace != executor.Namespace) continue;
        auto l = pod.labels.find(common::SparkAppIDLabel);
        if (l == pod.labels.end() || l->second != label->second) continue;
        if (pod.Phase != "Running") continue;  // filterToRunningPods, :535-545: other phases are not assigned to a node
        const Node* node = nullptr;            // getAzsOfPods, :521-533
        for (const Node& n : nodes)
            if (n.Name == pod.NodeName) {
                node = &n;
                break;
            }
        if (node == nullptr) {
            if (err) *err = "node \"" + pod.NodeName + "\" not found";  // the lister's NotFound error
            return {"", false};
        }
        auto z = node->labels.find(kLabelTopologyZone);
        if (z == node->labels.end()) {
            if (err) *err = "Could not read zone label from node, unable to make scheduling decisions based on AZ";
            return {"", false};
        }
        azs.insert(z->second);
    }
    if (azs.size() > 1) return {"", false};  // :511-513
    if (azs.empty()) {                        // :514-516
        if (err) *err = "Application has no scheduled pods, can't make scheduling decisions based on AZ";
        return {"", false};
    }
    return {*azs.begin(), true};
}

SelectNodeResult SparkSchedulerExtender::rescheduleExecutor(const Pod& executor, const Pod& driver, const std::vector<Pod>& allPods,
                                                            const std::vector<std::string>& nodeNames,
                                                            const std::set<std::string>& nodesHostingApp, bool isExtraExecutor) {
    std::string err;
    // sparkResources(driver) comes first in the reference (:599-602): its failure is failure-internal whatever the zones say
    if (!sparkResources(driver, &err)) return failure(outcome::failureInternal, err);
    std::vector<Node> availableNodes;  // getNodes (:448-460): lister order of nodeNames, unknown names skipped
    for (const std::string& name : nodeNames)
        for (const Node& n : nodes)
            if (n.Name == name) {
                availableNodes.push_back(n);
                break;
            }
    std::vector<std::string> names = nodeNames;
    if (binpacker_.IsSingleAz && shouldScheduleDynamicallyAllocatedExecutorsInSameAZ) {  // :608
        auto [zone, allPodsInSameAz] = getCommonZoneForExecutorsApplication(executor, allPods, &err);
        if (!err.empty()) return failure("", err);  // :611-613: ("", "", err)
        if (allPodsInSameAz) {                      // :614-627
            std::vector<Node> inZone;
            if (!filterNodesToZone(availableNodes, zone, &inZone, &err)) return failure(outcome::failureInternal, err);
            availableNodes = std::move(inZone);
            names.clear();
            for (const Node& n : availableNodes) names.push_back(n.Name);
        }
    }
    return rescheduleExecutor(driver, names, availableNodes, nodesHostingApp, isExtraExecutor);
}

bool SparkSchedulerExtender::DoesPodExceedClusterCapacity(const Pod& driver, const std::vector<Node>& availableNodes,
                                                          const NodeGroupResources& nonSchedulableOverhead, bool* served,
                                                          std::string* err) {
    if (served) *served = true;
    NodeGroupResources usage;  // empty cluster
    NodeGroupSchedulingMetadata metadata = NodeSchedulingMetadataForNodes(availableNodes, usage, nonSchedulableOverhead);
    std::vector<std::string> names;
    for (const Node& n : availableNodes) names.push_back(n.Name);
    std::string e;
    auto resources = sparkResources(driver, &e);
    if (!resources) {
        if (err) *err = e;
        return false;  // the reference returns (false, err)
    }
    Binpacker bp = binpacker_;
    bp.with_efficiencies = false;
    PackingResult r = bp.BinpackFunc(resources->DriverResources, resources->ExecutorResources, resources->MinExecutorCount,
                                     names, names, metadata);
    if (!r.served) {
        if (served) *served = false;
        if (err) *err = r.error;
        return false;
    }
    return !r.HasCapacity;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The UnschedulablePodMarker's scans.  All three list the stale drivers the same way (listStaleDrivers); what each does with a pod
// it cannot take is its own, stated where the listing returns:
//                            unparsable pod                          pod not exactly representable
//   scanForUnschedulablePods   *err, answers the pods before it        not served, *err names the pod
//   ...Resident                the installing scan decides             the installing scan decides
//   ...AllGroups               *err, answers the pods before it        the per-group route (installing scans) decides

std::vector<std::pair<std::string, bool>> SparkSchedulerExtender::scanForUnschedulablePods(
    const std::vector<Pod>& allPods, int64_t timeoutNanos, const std::vector<Node>& availableNodes,
    const NodeGroupResources& nonSchedulableOverhead, bool* served, std::string* err) {
    if (served) *served = true;
    const StaleDrivers stale = listStaleDrivers(allPods, timeoutNanos);
    if (stale.unrepresentable != nullptr) {
        if (served) *served = false;
        if (err) *err = "pod " + stale.unrepresentable->Name + " is not exactly representable";
        return {};
    }
    if (stale.stopped && err) *err = stale.parse_error;
    if (stale.apps.empty()) return {};
    NodeGroupResources usage;  // zeroUsage: the cluster as if nothing ran on it
    NodeGroupSchedulingMetadata metadata = NodeSchedulingMetadataForNodes(availableNodes, usage, nonSchedulableOverhead);
    std::vector<std::string> names;
    for (const Node& n : availableNodes) names.push_back(n.Name);
    FlatSnapshot snap;
    std::string e;
    CtxSequence seq(binpacker_.ctx);
    if (!flatten(metadata, names, names, &snap, &e) || !upload(binpacker_.ctx, snap, &e)) {
        if (served) *served = false;
        if (err) *err = e;
        return {};
    }
    // DoesPodExceedClusterCapacity reads HasCapacity and nothing else (unschedulablepods.go:165): the feasibility-only batch
    std::vector<uint8_t> fits(stale.apps.size());
    if (gf_fit_feasible(binpacker_.ctx, binpacker_.Algo, (uint32_t)stale.apps.size(), stale.apps.data(), fits.data()) != GF_OK) {
        if (served) *served = false;
        if (err) *err = std::string("gf_fit_feasible: ") + gf_last_error(binpacker_.ctx);
        return {};
    }
    return scanResult(stale.pods, fits);
}

// One question to the resident cluster next to the Filter's installed snapshot: under flat_mu_ (the record of what sits on the
// device) and then the context's sequence lock, `ask(ctx)` — the call of the entry point named `entry` — runs if the columns on the
// device are this cluster's.  fall_back: not resident, or the entry point refused (GF_ERR_UNSUPPORTED); the caller answers by an
// installing route once this has returned, outside both locks, since that route takes them itself.  failed: the device call went
// wrong, the scan is not served (*served) and *err says why.
template <class Ask>
SparkSchedulerExtender::Asked SparkSchedulerExtender::askResident(const FlatCluster& cluster, const char* entry, Ask ask, bool* served,
                                                                  std::string* err) {
    std::lock_guard<std::mutex> flat_lock(*flat_mu_);  // before the sequence lock
    gf_ctx* ctx = binpacker_.ctx;
    CtxSequence seq(ctx);
    uint64_t gen[3] = {0, 0, 0};
    (void)gf_generation(ctx, gen);
    // the columns on the device must be this cluster's: put there by this extender's Filter and not replaced since
    const bool resident = cluster.version != 0 && resident_cluster_ == cluster.version && gen[1] == seen_cluster_gen_;
    const int rc = resident ? ask(ctx) : GF_ERR_UNSUPPORTED;
    if (rc == GF_OK) return Asked::answered;
    if (rc == GF_ERR_UNSUPPORTED) return Asked::fall_back;
    if (served) *served = false;
    if (err) *err = std::string(entry) + ": " + gf_last_error(ctx);
    return Asked::failed;
}

std::vector<std::pair<std::string, bool>> SparkSchedulerExtender::scanForUnschedulablePodsResident(
    const std::vector<Pod>& allPods, int64_t timeoutNanos, const FlatCluster& cluster, const std::vector<Node>& availableNodes,
    const NodeGroupResources& nonSchedulableOverhead, bool* served, std::string* err, bool* residentRoute) {
    if (residentRoute) *residentRoute = false;
    auto installs = [&] { return scanForUnschedulablePods(allPods, timeoutNanos, availableNodes, nonSchedulableOverhead, served, err); };
    // the selection: the nodes the drivers' affinity matches, by the cluster's node index
    std::vector<uint8_t> select(cluster.names.size(), 0);
    for (const Node& nd : availableNodes) {
        auto it = cluster.index.find(nd.Name);
        if (it == cluster.index.end()) return installs();
        select[it->second] = 1;
    }
    FlatOverhead over;
    if (!FlatOverhead::Build(nonSchedulableOverhead, cluster, &over, nullptr)) return installs();
    const StaleDrivers stale = listStaleDrivers(allPods, timeoutNanos);
    if (stale.stopped || stale.unrepresentable != nullptr) return installs();  // (the other route says what the reference says)
    if (served) *served = true;
    if (stale.apps.empty()) return {};
    std::vector<uint8_t> fits(stale.apps.size());
    const OverheadColumns oc = nullableColumns(over.over);
    const Asked asked = askResident(
        cluster, "gf_cluster_fit_feasible",
        [&](gf_ctx* ctx) {
            return gf_cluster_fit_feasible(ctx, binpacker_.Algo, oc.col[0], oc.col[1], oc.col[2], select.data(), (uint32_t)stale.apps.size(),
                                           stale.apps.data(), fits.data());
        },
        served, err);
    if (asked == Asked::fall_back) return installs();
    if (asked == Asked::failed) return {};
    if (residentRoute) *residentRoute = true;
    return scanResult(stale.pods, fits);
}

std::vector<std::pair<std::string, bool>> SparkSchedulerExtender::scanForUnschedulablePodsAllGroups(
    const std::vector<Pod>& allPods, int64_t timeoutNanos, const FlatCluster& cluster,
    const std::map<std::string, std::vector<Node>>& nodesByInstanceGroup, const NodeGroupResources& nonSchedulableOverhead,
    bool* served, std::string* err, bool* residentRoute) {
    if (residentRoute) *residentRoute = false;
    if (served) *served = true;
    const StaleDrivers listing = listStaleDrivers(allPods, timeoutNanos);
    if (listing.stopped && err) *err = listing.parse_error;
    const std::vector<const Pod*>& stale = listing.pods;
    if (stale.empty()) return {};
    static const std::vector<Node> kNoNodes;
    auto nodes_of = [&](const std::string& group) -> const std::vector<Node>& {
        auto it = nodesByInstanceGroup.find(group);
        return it == nodesByInstanceGroup.end() ? kNoNodes : it->second;  // a group nobody names: an empty set
    };
    // one installing scan per instance group, merged back into listing order
    auto per_group = [&]() -> std::vector<std::pair<std::string, bool>> {
        std::vector<std::string> order;  // the groups by first appearance
        std::map<std::string, std::vector<size_t>> members;
        for (size_t i = 0; i < stale.size(); ++i) {
            auto [it, fresh] = members.try_emplace(stale[i]->InstanceGroup);
            if (fresh) order.push_back(stale[i]->InstanceGroup);
            it->second.push_back(i);
        }
        std::vector<std::pair<std::string, bool>> merged(stale.size());
        for (const std::string& group : order) {
            const std::vector<size_t>& idx = members[group];
            const std::vector<Node>& nodes = nodes_of(group);
            if (nodes.empty()) {  // the reference packs onto no node: no driver candidate, the pod exceeds the capacity
                for (size_t i : idx) merged[i] = {stale[i]->Name, true};
                continue;
            }
            std::vector<Pod> pods;
            for (size_t i : idx) pods.push_back(*stale[i]);
            bool ok = true;
            const auto part = scanForUnschedulablePods(pods, timeoutNanos, nodes, nonSchedulableOverhead, &ok, err);
            if (!ok || part.size() != idx.size()) {
                if (served) *served = false;
                return {};
            }
            for (size_t j = 0; j < idx.size(); ++j) merged[idx[j]] = part[j];
        }
        return merged;
    };
    if (listing.unrepresentable != nullptr) return per_group();  // (the other route says so)
    // the sets: one row of ceil(n / 64) words per instance group a stale driver asks, by the cluster's node index
    const size_t W = (cluster.names.size() + 63) / 64;
    std::map<std::string, uint32_t> row_of;
    std::vector<uint64_t> words;
    std::vector<uint32_t> app_set(stale.size());
    for (size_t i = 0; i < stale.size(); ++i) {
        auto [it, fresh] = row_of.try_emplace(stale[i]->InstanceGroup, (uint32_t)row_of.size());
        app_set[i] = it->second;
        if (!fresh) continue;
        words.resize(words.size() + W, 0);
        if (!nodeBitRow(cluster, nodes_of(stale[i]->InstanceGroup), words.data() + (size_t)it->second * W)) return per_group();
    }
    FlatOverhead over;
    if (!FlatOverhead::Build(nonSchedulableOverhead, cluster, &over, nullptr)) return per_group();
    std::vector<uint8_t> fits(listing.apps.size());
    const OverheadColumns oc = nullableColumns(over.over);
    const Asked asked = askResident(
        cluster, "gf_cluster_fit_feasible_sets",
        [&](gf_ctx* ctx) {
            return gf_cluster_fit_feasible_sets(ctx, binpacker_.Algo, oc.col[0], oc.col[1], oc.col[2], (uint32_t)row_of.size(), words.data(),
                                                app_set.data(), (uint32_t)listing.apps.size(), listing.apps.data(), fits.data());
        },
        served, err);
    if (asked == Asked::fall_back) return per_group();
    if (asked == Asked::failed) return {};
    if (residentRoute) *residentRoute = true;
    return scanResult(stale, fits);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The flat form of the cluster state, and the routes that keep it on the device.

static uint64_t nextClusterVersion() {  // unique per Build / Rebuild
    static std::atomic<uint64_t> next_version{1};
    return next_version.fetch_add(1);
}

bool FlatCluster::Build(const std::vector<Node>& nodes, FlatCluster* out, std::string* err) {
    FlatCluster c;
    c.version = nextClusterVersion();
    const size_t n = nodes.size();
    std::map<std::string, uint32_t> zone_ids;  // label order
    for (const Node& nd : nodes) {
        auto z = nd.labels.find(kLabelZoneFailureDomain);
        zone_ids.emplace(z == nd.labels.end() ? kZoneLabelPlaceholder : z->second, 0u);
    }
    uint32_t zi = 0;
    for (auto& kv : zone_ids) {
        kv.second = zi++;
        c.zone_labels.push_back(kv.first);
    }
    std::vector<std::pair<std::string, uint32_t>> by_name;
    by_name.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const Node& nd = nodes[i];
        Resources a = Resources::Zero();
        if (auto it = nd.Allocatable.find(kResourceCPU); it != nd.Allocatable.end()) a.CPU = it->second;
        if (auto it = nd.Allocatable.find(kResourceMemory); it != nd.Allocatable.end()) a.Memory = it->second;
        if (auto it = nd.Allocatable.find(kResourceNvidiaGPU); it != nd.Allocatable.end()) a.NvidiaGPU = it->second;
        int64_t v[3];
        if (!canonicalNonNegative(a, v)) {
            if (err) *err = "allocatable of node " + nd.Name + " is not exactly representable";
            return false;
        }
        for (int j = 0; j < 3; ++j) c.alloc[j].push_back(v[j]);
        c.names.push_back(nd.Name);
        if (!c.index.emplace(nd.Name, (uint32_t)i).second) {
            if (err) *err = "duplicate node name " + nd.Name;
            return false;
        }
        auto z = nd.labels.find(kLabelZoneFailureDomain);
        c.zone.push_back(zone_ids.at(z == nd.labels.end() ? kZoneLabelPlaceholder : z->second));
        c.base_flags.push_back((nd.Unschedulable ? GF_NODE_UNSCHEDULABLE : 0u) | (nd.Ready ? GF_NODE_READY : 0u));
        by_name.emplace_back(nd.Name, (uint32_t)i);
    }
    std::sort(by_name.begin(), by_name.end());
    c.name_rank.assign(n, 0);
    for (size_t r = 0; r < n; ++r) c.name_rank[by_name[r].second] = (uint32_t)r;
    *out = std::move(c);
    return true;
}

namespace {

// A node's allocatable, zone label and base flags as FlatCluster::Build reads them.
bool nodeAllocatable(const Node& nd, int64_t v[3]) {
    Resources a = Resources::Zero();
    if (auto it = nd.Allocatable.find(kResourceCPU); it != nd.Allocatable.end()) a.CPU = it->second;
    if (auto it = nd.Allocatable.find(kResourceMemory); it != nd.Allocatable.end()) a.Memory = it->second;
    if (auto it = nd.Allocatable.find(kResourceNvidiaGPU); it != nd.Allocatable.end()) a.NvidiaGPU = it->second;
    return canonicalNonNegative(a, v);
}
const std::string& nodeZoneLabel(const Node& nd) {
    static const std::string placeholder = kZoneLabelPlaceholder;
    auto z = nd.labels.find(kLabelZoneFailureDomain);
    return z == nd.labels.end() ? placeholder : z->second;
}

// present / name_rank of a cluster with absent rows (names[i] empty): the present names in lexicographic order, then the absent
// rows in index order; `present` stays empty when every row is present.
void rankRows(FlatCluster* c) {
    const size_t n = c->names.size();
    std::vector<std::pair<std::string, uint32_t>> by_name;
    std::vector<uint32_t> absent;
    for (size_t i = 0; i < n; ++i) {
        if (c->index.count(c->names[i]) != 0 && c->index.at(c->names[i]) == (uint32_t)i)
            by_name.emplace_back(c->names[i], (uint32_t)i);
        else
            absent.push_back((uint32_t)i);
    }
    std::sort(by_name.begin(), by_name.end());
    c->name_rank.assign(n, 0);
    for (size_t r = 0; r < by_name.size(); ++r) c->name_rank[by_name[r].second] = (uint32_t)r;
    for (size_t a = 0; a < absent.size(); ++a) c->name_rank[absent[a]] = (uint32_t)(by_name.size() + a);
    c->present.clear();
    if (absent.empty()) return;
    c->present.assign((n + 63) / 64, 0);
    for (const auto& [name, i] : by_name) c->present[i >> 6] |= UINT64_C(1) << (i & 63u);
}

}  // namespace

bool FlatCluster::BuildWithSpare(const std::vector<Node>& nodes, uint32_t spare, FlatCluster* out, std::string* err) {
    FlatCluster c;
    if (!Build(nodes, &c, err)) return false;
    if (spare != 0 && c.zone_labels.empty()) c.zone_labels.push_back(kZoneLabelPlaceholder);  // (no node yet: zone 0 must exist)
    const uint32_t zone0 = c.zone.empty() ? 0u : c.zone[0];
    for (uint32_t s = 0; s < spare; ++s) {
        c.names.emplace_back();
        for (int j = 0; j < 3; ++j) c.alloc[j].push_back(0);
        c.zone.push_back(zone0);
        c.base_flags.push_back(0u);
    }
    if (spare != 0) rankRows(&c);
    *out = std::move(c);
    return true;
}

bool FlatCluster::Rebuild(const FlatCluster& prev, const std::vector<Node>& nodes, const FlatReservations* carried, FlatCluster* out,
                          std::vector<uint32_t>* rows_out, std::string* err) {
    auto refuse = [&](std::string why) {
        if (err) *err = std::move(why);
        return false;
    };
    const size_t n = prev.names.size();
    // zone ids follow the label order: they are prev's exactly when the set of labels is
    std::map<std::string, uint32_t> zone_ids;
    for (const Node& nd : nodes) zone_ids.emplace(nodeZoneLabel(nd), 0u);
    if (zone_ids.size() != prev.zone_labels.size()) return refuse("the set of zone labels changed");
    uint32_t zi = 0;
    for (auto& kv : zone_ids) {
        if (kv.first != prev.zone_labels[zi]) return refuse("the set of zone labels changed");
        kv.second = zi++;
    }
    std::unordered_map<std::string, const Node*> listed;
    listed.reserve(nodes.size());
    for (const Node& nd : nodes)
        if (nd.Name.empty() || !listed.emplace(nd.Name, &nd).second) return refuse("duplicate node name " + nd.Name);
    FlatCluster c = prev;
    c.version = nextClusterVersion();
    c.derived_from = prev.version;
    // ---- the departed: the row becomes absent, the name leaves the index
    for (size_t i = 0; i < n; ++i) {
        if (prev.isAbsent((uint32_t)i) || listed.count(prev.names[i]) != 0) continue;
        c.index.erase(prev.names[i]);
        c.names[i].clear();
        for (int j = 0; j < 3; ++j) c.alloc[j][i] = 0;
        c.base_flags[i] = 0u;
    }
    // ---- the present and the joining, in the order of `nodes`
    std::vector<uint8_t> carries(n, 0);  // rows an entry of the carried list names: not for a newcomer
    if (carried != nullptr)
        for (const uint32_t at : carried->node)
            if (at < n) carries[at] = 1;
    size_t free_row = 0;
    for (const Node& nd : nodes) {
        int64_t v[3];
        if (!nodeAllocatable(nd, v)) return refuse("allocatable of node " + nd.Name + " is not exactly representable");
        uint32_t row;
        if (auto at = c.index.find(nd.Name); at != c.index.end()) {
            row = at->second;
        } else {
            while (free_row < n && (!c.names[free_row].empty() || carries[free_row])) ++free_row;
            if (free_row == n) return refuse("no absent row is free for node " + nd.Name);
            row = (uint32_t)free_row;
            c.names[row] = nd.Name;
            c.index.emplace(nd.Name, row);
        }
        for (int j = 0; j < 3; ++j) c.alloc[j][row] = v[j];
        c.zone[row] = zone_ids.at(nodeZoneLabel(nd));
        c.base_flags[row] = (nd.Unschedulable ? GF_NODE_UNSCHEDULABLE : 0u) | (nd.Ready ? GF_NODE_READY : 0u);
    }
    rankRows(&c);
    c.ranks_changed = c.name_rank != prev.name_rank;
    c.changed_rows.clear();
    for (size_t i = 0; i < n; ++i)
        if (c.alloc[0][i] != prev.alloc[0][i] || c.alloc[1][i] != prev.alloc[1][i] || c.alloc[2][i] != prev.alloc[2][i] ||
            c.base_flags[i] != prev.base_flags[i] || c.zone[i] != prev.zone[i])
            c.changed_rows.push_back((uint32_t)i);
    if (rows_out) *rows_out = c.changed_rows;
    *out = std::move(c);
    return true;
}

bool FlatReservations::Build(const std::vector<ResourceReservation>& reservations,
                             const NodeGroupResources& softReservationUsage, const FlatCluster& cluster,
                             FlatReservations* out, std::string* err) {
    static std::atomic<uint64_t> next_version{1};
    FlatReservations f;
    f.version = next_version.fetch_add(1);
    auto push = [&](const std::string& node, const Resources& r) {
        auto it = cluster.index.find(node);
        if (it == cluster.index.end()) return true;  // usage of a node outside this instance group is never read
        int64_t v[3];
        if (!canonicalNonNegative(r, v)) return false;
        f.node.push_back(it->second);
        for (int j = 0; j < 3; ++j) f.req[j].push_back(v[j]);
        return true;
    };
    for (const ResourceReservation& rr : reservations)
        for (const auto& [name, res] : rr.Reservations) {
            Resources r = Resources::Zero();
            if (auto it = res.Resources.find(kResourceCPU); it != res.Resources.end()) r.CPU = it->second;
            if (auto it = res.Resources.find(kResourceMemory); it != res.Resources.end()) r.Memory = it->second;
            if (auto it = res.Resources.find(kResourceNvidiaGPU); it != res.Resources.end()) r.NvidiaGPU = it->second;
            if (!push(res.Node, r)) {
                if (err) *err = "a reservation of " + rr.Name + " is not exactly representable";
                return false;
            }
        }
    for (const auto& [node, r] : softReservationUsage)
        if (!push(node, r)) {
            if (err) *err = "soft reservations on " + node + " are not exactly representable";
            return false;
        }
    *out = std::move(f);
    return true;
}

bool FlatOverhead::Build(const NodeGroupResources& overhead, const FlatCluster& cluster, FlatOverhead* out, std::string* err) {
    FlatOverhead f;
    const size_t n = cluster.names.size();
    if (!overhead.empty())
        for (int j = 0; j < 3; ++j) f.over[j].assign(n, 0);
    for (const auto& [node, r] : overhead) {
        auto it = cluster.index.find(node);
        if (it == cluster.index.end()) continue;
        int64_t v[3];
        if (!canonicalNonNegative(r, v)) {
            if (err) *err = "overhead of " + node + " is not exactly representable";
            return false;
        }
        for (int j = 0; j < 3; ++j) f.over[j][it->second] = v[j];
    }
    f.Touch();
    *out = std::move(f);
    return true;
}

void FlatOverhead::Touch() {
    static std::atomic<uint64_t> next_version{1};
    version = next_version.fetch_add(1);
}

void overheadRowDiff(const std::vector<int64_t> want[3], const std::vector<int64_t> have[3], uint32_t n, std::vector<uint32_t>* rows) {
    rows->clear();
    const bool w = want != nullptr && !want[0].empty(), h = have != nullptr && !have[0].empty();
    if (!w && !h) return;
    for (uint32_t i = 0; i < n; ++i) {
        bool differs = false;
        for (int j = 0; j < 3; ++j) differs = differs || (w ? want[j][i] : 0) != (h ? have[j][i] : 0);
        if (differs) rows->push_back(i);
    }
}

// What selectDriverNodeFlat and rescheduleExecutorFlat keep on the device, brought up to this request: the node-side columns
// (gf_cluster_set — or, for a cluster that FlatCluster::Rebuild derived from the resident one, the node rows that changed:
// gf_cluster_update), the overhead rows that differ from what is resident (gf_overhead_update) and, with `usage`, the usage sums of
// that entry list (gf_usage_reset + gf_usage_apply when the list's version changed).  Called under flat_mu_ and the context's
// sequence lock.  gen: the context's generations afterwards.
SparkSchedulerExtender::ResidentSync SparkSchedulerExtender::syncResident(gf_ctx* ctx, const FlatCluster& cluster, const FlatOverhead& fo,
                                                                          const FlatReservations* usage, uint64_t gen[3], std::string* err) {
    const uint32_t n = (uint32_t)cluster.names.size();
    const std::vector<int64_t>* const over = fo.over;
    bool resident_route = true;
    const bool with_over = !over[0].empty();
    const OverheadColumns oc = nullableColumns(over);
    const bool known_over = fo.version != 0 && fo.version == resident_over_version_;  // compared before
    (void)gf_generation(ctx, gen);
    bool own_cluster = resident_cluster_ == cluster.version && cluster.version != 0;
    // the node rows changed in place (FlatCluster::Rebuild): what is resident is the cluster this one was derived from, and nobody
    // else replaced it — the rows that differ travel (gf_cluster_update), with the name ranks when they moved; the overhead columns
    // and the usage sums on the device stay what they are.  Most of the cluster: the full set below is cheaper.
    if (!own_cluster && cluster.version != 0 && cluster.derived_from != 0 && resident_cluster_ == cluster.derived_from &&
        gen[1] == seen_cluster_gen_ && cluster.changed_rows.size() <= (size_t)n / 2) {
        const std::vector<uint32_t>& moved = cluster.changed_rows;
        std::vector<int64_t> acol[3];
        std::vector<uint32_t> fl, zn;
        for (const uint32_t r : moved) {
            for (int j = 0; j < 3; ++j) acol[j].push_back(cluster.alloc[j][r]);
            fl.push_back(cluster.base_flags[r]);
            zn.push_back(cluster.zone[r]);
        }
        ++cluster_update_calls_;
        cluster_rows_sent_ += moved.size();
        built_epoch_ = 0;  // the installed snapshot was built from other rows
        if (gf_cluster_update(ctx, (uint32_t)moved.size(), moved.data(), acol[0].data(), acol[1].data(), acol[2].data(), fl.data(), zn.data(),
                              cluster.ranks_changed ? cluster.name_rank.data() : nullptr) == GF_OK) {
            resident_cluster_ = cluster.version;
            own_cluster = true;
            (void)gf_generation(ctx, gen);
            seen_cluster_gen_ = gen[1];
        }  // (refused: the full set below decides)
    }
    bool set_cluster = !own_cluster || gen[1] != seen_cluster_gen_;
    std::vector<uint32_t> rows;  // the rows in which this request's overhead differs from what this extender last sent
    if (own_cluster && !known_over && (with_over || !resident_over_[0].empty())) {
        overheadRowDiff(over, resident_over_, n, &rows);
        if (rows.size() > (size_t)n / 2) set_cluster = true;  // most of the cluster: one upload of the columns is cheaper
    }
    if (set_cluster) {
        ++cluster_set_calls_;
        if (gf_cluster_set(ctx, n, cluster.alloc[0].data(), cluster.alloc[1].data(), cluster.alloc[2].data(), oc.col[0], oc.col[1], oc.col[2],
                           cluster.base_flags.data(), cluster.zone.data(), (uint32_t)cluster.zone_labels.size(),
                           cluster.name_rank.data()) != GF_OK) {
            resident_cluster_ = 0;
            *err = std::string("gf_cluster_set: ") + gf_last_error(ctx);
            return ResidentSync::failed;
        }
        if (!own_cluster || !rows.empty()) built_epoch_ = 0;  // the installed snapshot was built from other columns
        resident_cluster_ = cluster.version;
        resident_usage_ = 0;  // gf_cluster_set zeroed the resident usage
        for (int j = 0; j < 3; ++j) resident_over_[j] = over[j];  // (empty without overhead)
        resident_over_version_ = fo.version;
        (void)gf_generation(ctx, gen);
        seen_cluster_gen_ = gen[1];
        seen_usage_gen_ = gen[2];
    } else if (!rows.empty()) {
        std::vector<int64_t> rcol[3];
        for (int j = 0; j < 3; ++j) {
            rcol[j].reserve(rows.size());
            for (uint32_t r : rows) rcol[j].push_back(with_over ? over[j][r] : 0);
        }
        ++overhead_update_calls_;
        overhead_rows_sent_ += rows.size();
        built_epoch_ = 0;  // the installed snapshot was built from other rows
        resident_over_version_ = 0;
        if (gf_overhead_update(ctx, (uint32_t)rows.size(), rows.data(), rcol[0].data(), rcol[1].data(), rcol[2].data()) != GF_OK) {
            resident_route = false;  // (a value out of range, a failed device call): the full build below decides
        } else {
            if (resident_over_[0].empty())
                for (int j = 0; j < 3; ++j) resident_over_[j].assign(n, 0);
            for (size_t i = 0; i < rows.size(); ++i)
                for (int j = 0; j < 3; ++j) resident_over_[j][rows[i]] = rcol[j][i];
            resident_over_version_ = fo.version;
            (void)gf_generation(ctx, gen);
            seen_cluster_gen_ = gen[1];
        }
    } else if (own_cluster) {
        resident_over_version_ = fo.version;  // compared equal: the next Filter with this version need not look
    }
    // a caller that keeps its flattened reservations (version != 0) gets the usage sums kept on the device too: they
    // are sent when the list changes, and a Filter between two changes moves no reservation at all.  (A host that tracks
    // its ResourceReservation events would send only the K + 1 entries of the object that changed: gf_usage_apply.)
    if (resident_route && usage != nullptr && (resident_usage_ != usage->version || gen[2] != seen_usage_gen_)) {
        resident_usage_ = 0;
        ++usage_replay_calls_;
        if (gf_usage_reset(ctx) != GF_OK || gf_usage_apply(ctx, (uint32_t)usage->node.size(), usage->node.data(), usage->req[0].data(),
                                                           usage->req[1].data(), usage->req[2].data(), +1) != GF_OK) {
            *err = std::string("gf_usage_apply: ") + gf_last_error(ctx);
            return ResidentSync::failed;
        }
        resident_usage_ = usage->version;
        (void)gf_generation(ctx, gen);
        seen_usage_gen_ = gen[2];
    }
    return resident_route ? ResidentSync::ok : ResidentSync::no_resident_route;
}

SelectNodeResult SparkSchedulerExtender::selectDriverNodeFlat(const std::string& instanceGroup, const Pod& driver,
                                                              const std::vector<std::string>& nodeNames,
                                                              const FlatCluster& cluster, const FlatReservations* flat,
                                                              const FlatOverhead* flatOverhead) {
    return selectDriverNodeFlatOver(instanceGroup, driver, nodeNames, cluster, nullptr, flat, flatOverhead);
}

// The usage entries and overhead columns a flat request reads: the caller's (kept_usage / kept_over, versions and all) or, for a
// NULL one, this request's own, flattened here from `reservations` + `softReservationUsage` / `overhead`.  false: *why — a quantity
// is not exactly representable, or the kept overhead columns are not of this cluster's length.
bool SparkSchedulerExtender::requestColumns(const FlatCluster& cluster, const FlatReservations* kept_usage, const FlatOverhead* kept_over,
                                            RequestColumns* cols, std::string* why) const {
    const size_t n = cluster.names.size();
    cols->usage = kept_usage;
    if (kept_usage == nullptr) {
        if (!FlatReservations::Build(reservations, softReservationUsage, cluster, &cols->own_usage, why)) return false;
        cols->usage = &cols->own_usage;
    }
    cols->over = kept_over;
    if (kept_over == nullptr) {
        if (!FlatOverhead::Build(overhead, cluster, &cols->own_over, why)) return false;
        cols->own_over.version = 0;  // this request's own: compared with the resident columns on every Filter
        cols->over = &cols->own_over;
    } else if (!kept_over->over[0].empty() && (kept_over->over[0].size() != n || kept_over->over[1].size() != n || kept_over->over[2].size() != n)) {
        *why = "the flat overhead columns do not belong to this cluster";
        return false;
    }
    return true;
}

SelectNodeResult SparkSchedulerExtender::selectDriverNodeFlatGroup(const std::string& instanceGroup, const Pod& driver,
                                                                   const std::vector<std::string>& nodeNames,
                                                                   const FlatCluster& cluster, const std::vector<Node>& groupNodes,
                                                                   const FlatReservations* flat, const FlatOverhead* flatOverhead) {
    // availableNodes as one bit row of the resident cluster (include/gangfit.h, gf_snapshot_build_resident_set)
    std::vector<uint64_t> members((cluster.names.size() + 63) / 64, 0);
    if (nodeBitRow(cluster, groupNodes, members.data())) {  // (false: a node the lister knows and `cluster` does not)
        SelectNodeResult out = selectDriverNodeFlatOver(instanceGroup, driver, nodeNames, cluster, &members, flat, flatOverhead);
        if (out.served) return out;
    }
    return selectDriverNode(instanceGroup, driver, nodeNames, groupNodes);
}

// members: nullptr = `cluster` describes exactly the driver's nodes; else the row of the driver's nodes inside it.
SelectNodeResult SparkSchedulerExtender::selectDriverNodeFlatOver(const std::string& instanceGroup, const Pod& driver,
                                                                  const std::vector<std::string>& nodeNames,
                                                                  const FlatCluster& cluster, const std::vector<uint64_t>* members,
                                                                  const FlatReservations* flat, const FlatOverhead* flatOverhead) {
    if (auto held = answerFromReservation(reservations, driver)) return *held;
    const uint32_t n = (uint32_t)cluster.names.size();
    // "every node" of a cluster with absent rows is the row of its present nodes: an absent row must not become a metadata key
    if (members == nullptr && !cluster.present.empty()) members = &cluster.present;
    // ---- the per-request columns: one entry per reservation (UsageForNodes' input), overhead, request flags
    // (a caller that hands over no entry list gets this request's own, which travels whole with every Filter)
    std::string err;
    RequestColumns cols;
    if (!requestColumns(cluster, flat, flatOverhead, &cols, &err)) return notServed(err);
    const bool keep_usage = flat != nullptr && flat->version != 0;
    flat = cols.usage;
    flatOverhead = cols.over;
    const std::vector<uint32_t>& rnode = flat->node;
    const std::vector<int64_t>* rreq = flat->req;
    const std::vector<int64_t>* const over = flatOverhead->over;
    // ---- from here on this Filter reads and writes the extender's caches and its record of what sits on the device
    std::lock_guard<std::mutex> flat_lock(*flat_mu_);
    ++flat_calls_;
    // the request's NodeNames as candidate flags: the same list for every Filter of an instance group until the node set
    // changes, so the 10 000 map lookups are done once per (cluster version, list)
    // (a hash hit is confirmed on the list itself: comparing 10 000 short strings costs a fraction of the 10 000 map lookups
    //  it saves, and a collision would silently change the node the Filter returns)
    const uint64_t names_hash = hashNodeNames(nodeNames);
    if (cluster.version == 0 || flags_cluster_ != cluster.version || flags_hash_ != names_hash || flags_names_ != nodeNames) {
        flags_cache_ = cluster.base_flags;
        for (const std::string& name : nodeNames)
            if (auto it = cluster.index.find(name); it != cluster.index.end()) flags_cache_[it->second] |= GF_NODE_DRIVER_CANDIDATE;
        flags_cluster_ = cluster.version;
        flags_hash_ = names_hash;
        flags_names_ = nodeNames;
    }
    const std::vector<uint32_t>& flags = flags_cache_;
    // ---- the applications: earlier drivers in creation order, then this one
    auto resources = sparkResources(driver, &err);
    if (!resources) return failure(outcome::failureInternal, "failed to get spark resources: " + err);
    // annotations -> canonical requests, once per (pod, resourceVersion)
    PodApp uncached;
    auto cached_app = [&](const Pod& p) -> const PodApp& {
        if (p.ResourceVersion == 0) return uncached = podApp(p, nullptr);
        ParsedApp& pa = parsed_apps_[p.UID.empty() ? p.Namespace + "/" + p.Name : p.UID];
        pa.seen = flat_calls_;
        if (pa.version != p.ResourceVersion) {
            pa.version = p.ResourceVersion;
            pa.parsed = podApp(p, nullptr);
        }
        return pa.parsed;
    };
    std::vector<gf_app> apps;
    if (!earlierDriverApps(instanceGroup, driver, cached_app, &apps, &err)) return notServed(err);
    // pods come and go: entries no request has used lately are dropped once the map outgrows the pods it is asked about
    if (parsed_apps_.size() > 2 * pods.size() + 64)
        for (auto it = parsed_apps_.begin(); it != parsed_apps_.end();) it = it->second.seen == flat_calls_ ? std::next(it) : parsed_apps_.erase(it);
    gf_app cur;
    if (!toApp(*resources, &cur)) return notServed("application resources are not exactly representable");
    apps.push_back(cur);
    // ---- snapshot + orders on the device, then the chain
    gf_ctx* ctx = binpacker_.ctx;
    CtxSequence seq(ctx);
    // The node-side columns stay on the device (gf_cluster_set): all but the overhead change only when the node set does, and the
    // overhead changes by rows (gf_overhead_update).  A Filter moves the overhead rows that differ from what is resident, its
    // reservation entries and its own candidate flags only.  Another user of the context (the UnschedulablePodMarker shares it)
    // may have replaced the resident cluster or usage in between: the context's generations say so.
    // (syncResident, above: the cluster columns, the overhead rows that differ and — for a caller that keeps its flattened
    //  reservations — the usage sums, each sent only when it changed)
    uint64_t gen[3] = {0, 0, 0};
    const ResidentSync synced = syncResident(ctx, cluster, *flatOverhead, keep_usage ? flat : nullptr, gen, &err);
    if (synced == ResidentSync::failed) return notServed(err);
    const bool resident_route = synced == ResidentSync::ok;
    // (a NULL row is gf_snapshot_build_resident itself; another group's row rebuilds from the same resident columns and
    //  usage sums: no gf_cluster_set, no usage replay)
    const uint64_t* const row = members != nullptr ? members->data() : nullptr;
    // nothing changed since this extender's last Filter (no overhead row differed either: a change above cleared built_epoch_):
    // the installed snapshot IS this request's snapshot
    const bool same_snapshot = keep_usage && built_epoch_ != 0 && gen[0] == built_epoch_ && built_cluster_ == cluster.version &&
                               built_usage_ == flat->version && built_flags_ == flags &&
                               (members != nullptr ? built_set_ && built_members_ == *members : !built_set_);
    if (resident_route && !same_snapshot) {
        built_epoch_ = 0;
        const int brc = keep_usage
                            ? gf_snapshot_build_resident_set(ctx, row, GF_RESIDENT_USAGE, nullptr, nullptr, nullptr, nullptr,
                                                             flags.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)
                            : gf_snapshot_build_resident_set(ctx, row, (uint32_t)rnode.size(), rnode.data(), rreq[0].data(),
                                                             rreq[1].data(), rreq[2].data(), flags.data(), nullptr, nullptr,
                                                             nullptr, nullptr, nullptr, nullptr);
        if (brc != GF_OK) {
            resident_cluster_ = 0;
            resident_usage_ = 0;
            return notServed(std::string("gf_snapshot_build_resident_set: ") + gf_last_error(ctx));
        }
        if (keep_usage && gf_generation(ctx, gen) == GF_OK) {
            built_epoch_ = gen[0];
            built_cluster_ = cluster.version;
            built_usage_ = flat->version;
            built_flags_ = flags;
            built_set_ = members != nullptr;
            if (built_set_)
                built_members_ = *members;
            else
                built_members_.clear();
        }
    }
    if (!resident_route && members != nullptr)  // the full build below installs every node of `cluster`: not this group's snapshot
        return notServed("the resident route could not take this request");
    if (!resident_route) {  // what the resident route could not take: everything travels, nothing stays
        resident_cluster_ = 0;
        built_epoch_ = 0;
        if (gf_snapshot_build(ctx, n, cluster.alloc[0].data(), cluster.alloc[1].data(), cluster.alloc[2].data(), over[0].data(),
                              over[1].data(), over[2].data(), (uint32_t)rnode.size(), rnode.data(), rreq[0].data(), rreq[1].data(),
                              rreq[2].data(), flags.data(), cluster.zone.data(), (uint32_t)cluster.zone_labels.size(),
                              cluster.name_rank.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != GF_OK)
            return notServed(std::string("gf_snapshot_build: ") + gf_last_error(ctx));
    }
    // (the group route's keys are the row the snapshot was built from: built_members_ when recorded, this request's row always)
    return fitChain(ctx, apps, cluster.names, row, driver, *resources);
}

SelectNodeResult SparkSchedulerExtender::rescheduleExecutorFlat(const Pod& executor, const Pod& driver, const std::vector<Pod>& allPods,
                                                                const std::vector<std::string>& nodeNames,
                                                                const std::set<std::string>& nodesHostingApp, bool isExtraExecutor,
                                                                const FlatCluster& cluster, const FlatReservations* flat,
                                                                const FlatOverhead* flatOverhead, bool* residentRoute) {
    if (residentRoute) *residentRoute = false;
    auto installs = [&] { return rescheduleExecutor(executor, driver, allPods, nodeNames, nodesHostingApp, isExtraExecutor); };
    std::string err;
    auto resources = sparkResources(driver, &err);  // first in the reference (:599-602)
    if (!resources) return failure(outcome::failureInternal, err);
    int64_t exe[3];
    if (!canonicalNonNegative(resources->ExecutorResources, exe)) return installs();
    if (sorter_.hasExecutorLabelPriority() || cluster.version == 0) return installs();
    const uint32_t n = (uint32_t)cluster.names.size();
    // ---- the zone step on the host, as rescheduleExecutor does it (:606-632); its errors are the reference's
    bool narrow = false;
    std::string zone;
    if (binpacker_.IsSingleAz && shouldScheduleDynamicallyAllocatedExecutorsInSameAZ) {
        auto [z, allPodsInSameAz] = getCommonZoneForExecutorsApplication(executor, allPods, &err);
        if (!err.empty()) return failure("", err);  // :611-613: ("", "", err)
        narrow = allPodsInSameAz;
        zone = z;
    }
    // ---- nodeNames as a bit row over the cluster's node index: getNodes (:448-460) skips names the lister does not know
    std::unordered_map<std::string, const Node*> listed;
    listed.reserve(nodes.size());
    for (const Node& nd : nodes) listed.emplace(nd.Name, &nd);
    std::vector<const Node*> available;
    for (const std::string& name : nodeNames)
        if (auto nd = listed.find(name); nd != listed.end()) available.push_back(nd->second);
    bool unlabelled = false;
    auto in_zone = [&](const Node& node) {  // filterNodesToZone (:462-478)
        if (!narrow) return true;
        auto z = node.labels.find(kLabelTopologyZone);
        if (z == node.labels.end()) unlabelled = true;
        return z != node.labels.end() && z->second == zone;
    };
    std::vector<uint64_t> row(((size_t)n + 63) / 64, 0);
    const bool known = nodeBitRow(cluster, available, row.data(), in_zone);
    if (unlabelled)  // (met before any node outside the cluster: the walk ends at such a node)
        return failure(outcome::failureInternal, "Could not read zone label from node, unable to make scheduling decisions based on AZ");
    if (!known) return installs();  // `cluster` does not describe this request's nodes
    const bool minfrag = binpacker_.Name == "single-az-minimal-fragmentation";
    std::vector<uint32_t> hosts(((size_t)n + 31) / 32, 0u);
    for (const std::string& name : nodesHostingApp)
        if (auto it = cluster.index.find(name); it != cluster.index.end()) hosts[it->second >> 5] |= 1u << (it->second & 31);
    // ---- the per-request columns, as in selectDriverNodeFlat; the device reads the RESIDENT usage, so an entry list always travels
    // by version (a caller that keeps none, or one without a version, gets this request's own, with a version of its own)
    RequestColumns cols;
    if (!requestColumns(cluster, flat != nullptr && flat->version != 0 ? flat : nullptr, flatOverhead, &cols, &err)) return installs();
    uint32_t node = GF_NO_NODE;
    int rc = GF_ERR_UNSUPPORTED;
    {
        std::lock_guard<std::mutex> flat_lock(*flat_mu_);  // the record of what sits on the device; before the sequence lock
        gf_ctx* ctx = binpacker_.ctx;
        CtxSequence seq(ctx);
        uint64_t gen[3] = {0, 0, 0};
        if (syncResident(ctx, cluster, *cols.over, cols.usage, gen, &err) == ResidentSync::ok) {
            const uint32_t row0 = 0;
            rc = gf_cluster_executor_fit(ctx, minfrag ? 1 : 0, 1, row.data(), 1, exe, &row0, minfrag ? hosts.data() : nullptr, nullptr,
                                         nullptr, nullptr, &node);
        }
    }
    if (rc != GF_OK) return installs();  // refused, or not resident (outside the locks: that route takes them itself)
    if (residentRoute) *residentRoute = true;
    return executorAnswer(node, cluster.names, isExtraExecutor);
}

}  // namespace gangfit::host
