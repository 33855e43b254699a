// extender.hpp — the driver Filter decision around the gang-fit kernels (host side, C++ mirror of the Go code).
//
//   SparkSchedulerExtender.selectDriverNode          internal/extender/resource.go:272-370
//   fitEarlierDrivers / shouldSkipDriverFifo         internal/extender/resource.go:224-270
//   outcome strings                                  internal/extender/resource.go:46-55
//   newResourceReservation / executorReservationName internal/extender/resourcereservations.go:491-533
//   UnschedulablePodMarker.DoesPodExceedClusterCapacity  internal/extender/unschedulablepods.go:132-166
// The reference calls BinpackFunc once per earlier driver and once for the driver being filtered
// (resource.go:238, :321); here the whole FIFO replay + final pack is ONE GF_MODE_FIFO_CHAIN call (the "L-batch"
// insertion level of SURVEY.md section 8b).  Everything else — listers, caches, demands, metrics, the API write of the
// reservation — stays in the Go host and is represented by plain inputs / outputs.
#pragma once

#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "binpacker.hpp"
#include "nodesorting.hpp"
#include "sparkpods.hpp"

namespace gangfit::host {

namespace outcome {
constexpr const char* failureUnbound = "failure-unbound";
constexpr const char* failureInternal = "failure-internal";
constexpr const char* failureFit = "failure-fit";
constexpr const char* failureEarlierDriver = "failure-earlier-driver";
constexpr const char* failureNonSparkPod = "failure-non-spark-pod";
constexpr const char* success = "success";
constexpr const char* successRescheduled = "success-rescheduled";
constexpr const char* successScheduledExtraExecutor = "success-scheduled-extra-executor";
}  // namespace outcome

struct FifoConfig {  // config.FifoConfig
    int64_t DefaultEnforceAfterPodAgeNanos = 0;
    std::map<std::string, int64_t> EnforceAfterPodAgeByInstanceGroup;
};

// filterNodesToZone (resource.go:462-478): the nodes whose topology.kubernetes.io/zone label equals `zone`, in order; false
// (with the reference's message) when a node has no such label.
bool filterNodesToZone(const std::vector<Node>& initialNodes, const std::string& zone, std::vector<Node>* out, std::string* err);

ResourceReservation newResourceReservation(const std::string& driverNode, const std::vector<std::string>& executorNodes,
                                           const Pod& driver, const Resources& driverResources,
                                           const Resources& executorResources);
std::string executorReservationName(int i);  // "executor-<i+1>"

struct AvgPackingEfficiency {  // binpack.AvgPackingEfficiency (LIB/binpack/efficiency.go:25-31)
    double CPU = 0.0, Memory = 0.0, GPU = 0.0, Max = 0.0;
};

struct SelectNodeResult {
    std::string node;     // empty on failure
    std::string outcome;  // one of outcome::*
    std::string error;    // the reference's error text (or why the device could not serve the request)
    bool served = true;   // false: the accelerator could not serve the request -> the Go host must run its own path
    std::optional<ResourceReservation> created;  // what CreateReservations would persist
    // computeAvgPackingEfficiencyForResult (resource.go:329, 372-381): what metrics.ReportPackingEfficiency is given (:352), over
    // every metadata key, against the metadata after fitEarlierDrivers (gf_filter_efficiency).  Filled by the driver Filters on
    // `success` with a fresh pack; has_efficiency stays false when the call is refused — that does not fail the Filter.
    AvgPackingEfficiency efficiency;
    bool has_efficiency = false;
};

// The node side of the cluster in the flat form gf_snapshot_build consumes.  Built when the node set changes (an informer
// event in the Go host), reused by every Filter: names in lexicographic order give the name ranks, zone ids follow the
// label order (the tie-break documented at the C ABI).
struct FlatReservations;
struct FlatCluster {
    std::vector<std::string> names;                  // node index -> name (the order of `nodes` at Build time)
    std::unordered_map<std::string, uint32_t> index;
    std::vector<uint32_t> name_rank, zone, base_flags;  // base_flags: GF_NODE_UNSCHEDULABLE / GF_NODE_READY
    std::vector<std::string> zone_labels;            // zone id -> label
    std::vector<int64_t> alloc[3];
    uint64_t version = 0;  // unique per Build: lets a caller keep the columns resident on the device (gf_cluster_set)
    static bool Build(const std::vector<Node>& nodes, FlatCluster* out, std::string* err);
    // ---- node rows that change in place (include/gangfit.h, gf_cluster_update): a host whose cluster gains and loses nodes keeps
    // `spare` ABSENT rows behind the present ones, so that n_nodes stands while nodes come and go.  An absent row has no name (names[i]
    // is empty and `index` does not know it), allocatable 0, flags 0, a valid zone id (row 0's at BuildWithSpare) and a name rank
    // behind every present name, in index order.  It is never a candidate and never a member of a row built from node lists; calls
    // that mean "every node" pass `present` instead of NULL.
    std::vector<uint64_t> present;       // the row of present nodes, ceil(n / 64) words; EMPTY: every row is present
    uint64_t derived_from = 0;           // Rebuild: the version whose rows this cluster changed in place (0: Build / BuildWithSpare)
    std::vector<uint32_t> changed_rows;  // Rebuild: the indices whose allocatable, flags or zone differ from derived_from's, ascending
    bool ranks_changed = false;          // Rebuild: name_rank differs from derived_from's
    // Build, plus `spare` absent rows at the end.
    static bool BuildWithSpare(const std::vector<Node>& nodes, uint32_t spare, FlatCluster* out, std::string* err);
    // `prev` brought to `nodes` with every index kept: a name keeps its index, a departed node's row becomes absent and its name
    // leaves `index`, a joining node (in the order of `nodes`) takes the lowest absent index that no entry of `carried` names — a
    // stale reservation of a departed node must not land on the newcomer —, name ranks are recomputed over all rows.  rows_out
    // (nullable) receives changed_rows.  false (*err says why; the caller takes BuildWithSpare): no absent row is free, the set of
    // zone labels differs from prev's, a duplicate name, an allocatable that is not exactly representable.
    static bool Rebuild(const FlatCluster& prev, const std::vector<Node>& nodes, const FlatReservations* carried, FlatCluster* out,
                        std::vector<uint32_t>* rows_out, std::string* err);
    bool isAbsent(uint32_t i) const { return !present.empty() && ((present[i >> 6] >> (i & 63u)) & 1u) == 0u; }
};

// UsageForNodes' input in flat form: one (node index, cpu milli, memory bytes, gpus) entry per reservation of every
// ResourceReservation plus the soft reservations (GetReservedResources, resourcereservations.go:258-263).  A host keeps it
// next to its ResourceReservation cache and updates it on the same events; the replay itself (the sum per node) happens on
// the device at every Filter.
struct FlatReservations {
    std::vector<uint32_t> node;
    std::vector<int64_t> req[3];
    uint64_t version = 0;  // unique per Build: lets the extender keep the usage sums of this entry list resident on the device
                           // (gf_usage_apply) for as long as the list does not change
    static bool Build(const std::vector<ResourceReservation>& reservations, const NodeGroupResources& softReservationUsage,
                      const FlatCluster& cluster, FlatReservations* out, std::string* err);
};

// overheadComputer.GetOverhead in flat form: dense cpu | memory | gpu columns over the cluster's node order (nodes the map does
// not name read zero; names outside the cluster are skipped).  A host keeps it next to its overhead cache and rebuilds — or
// patches — it on the pod events that change a node's overhead; a Filter then neither walks the string-keyed map nor, while the
// version stands, compares a column.
#define GANGFIT_HOST_FLAT_OVERHEAD 1
struct FlatOverhead {
    std::vector<int64_t> over[3];  // empty: no overhead anywhere
    uint64_t version = 0;          // unique per Build; a caller that patches the columns in place takes a new one (Touch)
    static bool Build(const NodeGroupResources& overhead, const FlatCluster& cluster, FlatOverhead* out, std::string* err);
    void Touch();
};

// The rows in which two dense overhead column sets differ (selectDriverNodeFlat: what gf_overhead_update must send).  `want` /
// `have` are cpu | memory | gpu columns of n values each; an EMPTY column set stands for "no overhead anywhere" (all zero).
// rows: the node indices in ascending order.
void overheadRowDiff(const std::vector<int64_t> want[3], const std::vector<int64_t> have[3], uint32_t n, std::vector<uint32_t>* rows);

class SparkSchedulerExtender {
public:
    SparkSchedulerExtender(Binpacker binpacker, NodeSorter sorter, bool isFIFO, FifoConfig fifo)
        : binpacker_(std::move(binpacker)), sorter_(std::move(sorter)), isFIFO_(isFIFO), fifo_(std::move(fifo)) {}

    // Cluster state the listers / caches of the Go host would provide.
    std::vector<Node> nodes;                         // nodeLister
    std::vector<Pod> pods;                           // podLister (drivers)
    std::vector<ResourceReservation> reservations;   // resourceReservationManager
    NodeGroupResources softReservationUsage;         // added by GetReservedResources (resourcereservations.go:258-263)
    NodeGroupResources overhead;                     // overheadComputer.GetOverhead
    int64_t nowNanos = 0;                            // time.Now()
    // install.ShouldScheduleDynamicallyAllocatedExecutorsInSameAZ (config/config.go:33; the reference's test harness sets it,
    // extendertest/extender_test_utils.go:135): with a single-AZ packer an executor only goes to the zone its application's
    // running pods are in (resource.go:606-632)
    bool shouldScheduleDynamicallyAllocatedExecutorsInSameAZ = false;

    // availableNodes = nodes whose labels satisfy the driver's required node affinity; the caller passes the predicate's
    // result because affinity matching is k8s API bookkeeping (resource.go:292-298).
    SelectNodeResult selectDriverNode(const std::string& instanceGroup, const Pod& driver,
                                      const std::vector<std::string>& nodeNames, const std::vector<Node>& availableNodes);

    // The same decision with the snapshot built on the device (gf_snapshot_build): the reservation replay, the
    // available / schedulable columns and NodeSorter.PotentialNodes never touch a string-keyed map.  `cluster` must
    // describe exactly the nodes the driver's affinity matches.  Label-priority re-sorts are not configured on this path.
    // `flat` (nullable) = the reservations already in flat form; when null they are flattened from `reservations` here.
    // `flatOverhead` (nullable) = the overhead already in flat form, used INSTEAD of the `overhead` map; when null the map is
    // canonicalised here on every Filter.
    SelectNodeResult selectDriverNodeFlat(const std::string& instanceGroup, const Pod& driver,
                                          const std::vector<std::string>& nodeNames, const FlatCluster& cluster,
                                          const FlatReservations* flat = nullptr, const FlatOverhead* flatOverhead = nullptr);
    // The same Filter when `cluster` holds EVERY instance group (what scanForUnschedulablePodsAllGroups and rescheduleExecutorFlat
    // want resident) and groupNodes = availableNodes, the nodes the driver's required affinity matches (resource.go:292-304): the
    // snapshot is built over the members of that row only (include/gangfit.h, gf_snapshot_build_resident_set), so one resident
    // cluster, one usage stream and one overhead stream serve the Filters of every group.  The sync is selectDriverNodeFlat's;
    // "nothing changed => no rebuild" additionally compares the member row, so a Filter for another group rebuilds — without a
    // gf_cluster_set and without a usage replay.  Whatever this route cannot take (a group node outside `cluster`, a request that is
    // not exactly representable, a refusal of the device) is answered by selectDriverNode on groupNodes.
    SelectNodeResult selectDriverNodeFlatGroup(const std::string& instanceGroup, const Pod& driver,
                                               const std::vector<std::string>& nodeNames, const FlatCluster& cluster,
                                               const std::vector<Node>& groupNodes, const FlatReservations* flat = nullptr,
                                               const FlatOverhead* flatOverhead = nullptr);
    // The next selectDriverNodeFlat rebuilds the snapshot even if nothing changed (host_bench times both).
    void forgetInstalledSnapshot() { built_epoch_ = 0; }
    // What the flat route has sent so far (tests and host_bench read them): Filters served, gf_overhead_update calls and the rows
    // they carried, gf_cluster_set calls.
    uint64_t flatCalls() const { return flat_calls_; }
    uint64_t overheadUpdateCalls() const { return overhead_update_calls_; }
    uint64_t overheadRowsSent() const { return overhead_rows_sent_; }
    uint64_t clusterSetCalls() const { return cluster_set_calls_; }
    // ... gf_cluster_update calls and the rows they carried (node rows changed in place instead of a gf_cluster_set), and the
    // replays of the whole reservation list (gf_usage_reset + gf_usage_apply)
    uint64_t clusterUpdateCalls() const { return cluster_update_calls_; }
    uint64_t clusterRowsSent() const { return cluster_rows_sent_; }
    uint64_t usageReplayCalls() const { return usage_replay_calls_; }

    // unschedulablepods.go:132-166: does the application fit an EMPTY cluster (usage = 0, the given overhead)?
    // nodes are used in lister order for both candidate lists.
    bool DoesPodExceedClusterCapacity(const Pod& driver, const std::vector<Node>& availableNodes,
                                      const NodeGroupResources& nonSchedulableOverhead, bool* served, std::string* err);

    // rescheduleExecutor (resource.go:594-673) for an executor whose driver is `driver`: availableNodes = getNodes(nodeNames)
    // (already narrowed to one zone by the caller when single-AZ dynamic allocation applies, :606-633);
    // nodesHostingApp = getNodesWithExecutorsBelongingToSameApp (only read by single-az-minimal-fragmentation).
    SelectNodeResult rescheduleExecutor(const Pod& driver, const std::vector<std::string>& nodeNames,
                                        const std::vector<Node>& availableNodes,
                                        const std::set<std::string>& nodesHostingApp, bool isExtraExecutor);

    // The whole of rescheduleExecutor (resource.go:594-673) including its zone step: `executor` is the pod being filtered,
    // `allPods` what the pod lister holds (the application's pods are selected by namespace + spark-app-id label,
    // getSparkApplicationPodsForExecutor :548-555); availableNodes = getNodes(nodeNames) comes from `nodes` in nodeNames order
    // (:448-460, unknown names skipped).  With a single-AZ packer and shouldScheduleDynamicallyAllocatedExecutorsInSameAZ the
    // candidates are narrowed to the one zone (label topology.kubernetes.io/zone, quirk 7) the application's Running pods
    // are in — BEFORE the snapshot and the sort, like the reference — and an application spread over several zones is
    // scheduled anywhere (:628-630).  Errors are the reference's: (outcome "", error) from getCommonZone..., failure-internal
    // from filterNodesToZone.
    SelectNodeResult rescheduleExecutor(const Pod& executor, const Pod& driver, const std::vector<Pod>& allPods,
                                        const std::vector<std::string>& nodeNames, const std::set<std::string>& nodesHostingApp,
                                        bool isExtraExecutor);
    // The same Filter answered from the RESIDENT cluster (include/gangfit.h, gf_cluster_executor_fit): `cluster` is the flat cluster of
    // the driver Filter's flat route.  Overhead rows and usage entries are synced the way selectDriverNodeFlat syncs them (`flat` /
    // `flatOverhead` nullable: flattened here from `reservations` / `overhead`), nodeNames — narrowed to the common zone on the host,
    // as above — travels as one bit row, and the device answers from its columns: no string-keyed map, no sort, no install, so the
    // snapshot epoch and the driver Filter's chain cache stay.  Outcomes and error strings are rescheduleExecutor's.  Whatever the
    // resident route cannot take — a refusal of the entry point, a name the lister knows and `cluster` does not, an executor label
    // priority, quantities that are not exactly representable — is answered by rescheduleExecutor (which installs).
    // *residentRoute (nullable): true when the resident entry point answered.
    SelectNodeResult rescheduleExecutorFlat(const Pod& executor, const Pod& driver, const std::vector<Pod>& allPods,
                                            const std::vector<std::string>& nodeNames, const std::set<std::string>& nodesHostingApp,
                                            bool isExtraExecutor, const FlatCluster& cluster, const FlatReservations* flat = nullptr,
                                            const FlatOverhead* flatOverhead = nullptr, bool* residentRoute = nullptr);
    // getCommonZoneForExecutorsApplication (resource.go:493-519): {zone, all pods in one zone}; *err set = the reference's error
    std::pair<std::string, bool> getCommonZoneForExecutorsApplication(const Pod& executor, const std::vector<Pod>& allPods,
                                                                      std::string* err) const;

    // scanForUnschedulablePods (unschedulablepods.go:93-129) as ONE independent batch: every pending driver of this
    // scheduler that is older than timeoutNanos is checked against the EMPTY cluster (the per-pod BinpackFunc calls of the
    // reference batched into one launch).  Returns {pod name, exceedsCapacity} in listing order; like the reference the scan
    // stops at the first pod whose resources cannot be parsed (*err says why).  availableNodes = the nodes the drivers'
    // node affinity matches (drivers of several instance groups: scanForUnschedulablePodsAllGroups, below).
    std::vector<std::pair<std::string, bool>> scanForUnschedulablePods(const std::vector<Pod>& allPods, int64_t timeoutNanos,
                                                                       const std::vector<Node>& availableNodes,
                                                                       const NodeGroupResources& nonSchedulableOverhead,
                                                                       bool* served, std::string* err);

    // The same scan NEXT TO the Filter's installed snapshot instead of in its place (include/gangfit.h, gf_cluster_fit_feasible):
    // `cluster` is the flat cluster of the Filter's flat route, whose columns selectDriverNodeFlat keeps on the device.  The scan
    // sends the non-schedulable overhead as dense columns and availableNodes as a node selection, and asks the resident columns —
    // no flatten, no upload, no install: the snapshot epoch, the chain cache and the resident usage stay, and the next Filter
    // resumes.  Falls back to scanForUnschedulablePods (which installs) when the entry point refuses the question
    // (GF_ERR_UNSUPPORTED: a zone-aware packer with a driver that asks for neither cpu nor memory, an overhead above a node's
    // allocatable, more than 64 zones), when `cluster` is not what this extender's last Filter left on the device, or when
    // availableNodes names a node outside it.  *residentRoute (nullable): true when the resident entry point answered.
    std::vector<std::pair<std::string, bool>> scanForUnschedulablePodsResident(const std::vector<Pod>& allPods, int64_t timeoutNanos,
                                                                               const FlatCluster& cluster,
                                                                               const std::vector<Node>& availableNodes,
                                                                               const NodeGroupResources& nonSchedulableOverhead,
                                                                               bool* served, std::string* err,
                                                                               bool* residentRoute = nullptr);

    // The marker's whole minute in one call: scanForUnschedulablePods (unschedulablepods.go:93-129) walks EVERY stale pending
    // driver of the scheduler, and DoesPodExceedClusterCapacity (:132-166) builds the node list from that pod's own required
    // affinity.  Every stale driver asks the nodes nodesByInstanceGroup lists for its Pod::InstanceGroup (a group the map does not
    // name: no node — the reference packs onto nothing and the pod exceeds the capacity); the groups travel as node sets of one
    // gf_cluster_fit_feasible_sets call (include/gangfit.h), under the residency test of scanForUnschedulablePodsResident.  The
    // result is in listing order.  One scanForUnschedulablePods per instance group (which installs), merged back into listing
    // order, answers instead when the entry point refuses (GF_ERR_UNSUPPORTED), when `cluster` is not the resident one, or when a
    // listed node is outside it.  An unparsable pod ends the scan there, as the reference does, and *err says why.
    std::vector<std::pair<std::string, bool>> scanForUnschedulablePodsAllGroups(
        const std::vector<Pod>& allPods, int64_t timeoutNanos, const FlatCluster& cluster,
        const std::map<std::string, std::vector<Node>>& nodesByInstanceGroup, const NodeGroupResources& nonSchedulableOverhead,
        bool* served, std::string* err, bool* residentRoute = nullptr);

    bool shouldSkipDriverFifo(const Pod& pod, const std::string& instanceGroup) const;

private:
    SelectNodeResult selectDriverNodeFlatOver(const std::string& instanceGroup, const Pod& driver,
                                              const std::vector<std::string>& nodeNames, const FlatCluster& cluster,
                                              const std::vector<uint64_t>* members, const FlatReservations* flat,
                                              const FlatOverhead* flatOverhead);
    enum class ResidentSync { ok, no_resident_route, failed };
    ResidentSync syncResident(gf_ctx* ctx, const FlatCluster& cluster, const FlatOverhead& fo, const FlatReservations* usage,
                              uint64_t gen[3], std::string* err);
    // The steps the routes share (extender.cpp says what each does).
    struct PodApp {  // a pod's annotations as a chain application
        bool parsed = false, representable = false;
        gf_app app{};
    };
    static PodApp podApp(const Pod& pod, std::string* err);
    struct StaleDrivers {  // what a capacity scan lists: facts, no policy
        std::vector<const Pod*> pods;
        std::vector<gf_app> apps;
        bool stopped = false;  // at an unparsable pod:
        std::string parse_error;
        const Pod* unrepresentable = nullptr;  // the first listed pod that is not exactly representable
    };
    StaleDrivers listStaleDrivers(const std::vector<Pod>& allPods, int64_t timeoutNanos) const;
    template <class AppOf>
    bool earlierDriverApps(const std::string& instanceGroup, const Pod& driver, AppOf app_of, std::vector<gf_app>* apps, std::string* why) const;
    SelectNodeResult fitChain(gf_ctx* ctx, const std::vector<gf_app>& apps, const std::vector<std::string>& names, const uint64_t* row,
                              const Pod& driver, const SparkApplicationResources& resources) const;
    struct RequestColumns {  // the usage entries and overhead columns one flat request reads: the caller's, or its own
        FlatReservations own_usage;
        FlatOverhead own_over;
        const FlatReservations* usage = nullptr;
        const FlatOverhead* over = nullptr;
    };
    bool requestColumns(const FlatCluster& cluster, const FlatReservations* kept_usage, const FlatOverhead* kept_over, RequestColumns* cols,
                        std::string* why) const;
    enum class Asked { answered, fall_back, failed };
    template <class Ask>
    Asked askResident(const FlatCluster& cluster, const char* entry, Ask ask, bool* served, std::string* err);
    uint64_t resident_cluster_ = 0;  // FlatCluster::version whose static columns sit on the device (selectDriverNodeFlat)
    uint64_t resident_usage_ = 0;    // FlatReservations::version whose usage sums sit on the device (for resident_cluster_)
    // the dense overhead columns this extender last put on the device for resident_cluster_ (gf_cluster_set or
    // gf_overhead_update); empty = none (a cluster set with NULL columns).  A Filter sends the rows in which its request differs.
    std::vector<int64_t> resident_over_[3];
    uint64_t resident_over_version_ = 0;  // FlatOverhead::version those columns came from (0: from the map, always compared)
    uint64_t overhead_update_calls_ = 0, overhead_rows_sent_ = 0, cluster_set_calls_ = 0;
    uint64_t cluster_update_calls_ = 0, cluster_rows_sent_ = 0, usage_replay_calls_ = 0;
    // what the context held after this extender's last call (gf_generation): another user of the same gf_ctx that replaces the
    // cluster, its overhead rows, the usage or the snapshot moves these on, and the next Filter sends its own state again
    uint64_t seen_cluster_gen_ = 0, seen_usage_gen_ = 0;
    // the snapshot the last Filter installed: while cluster, overhead rows, usage and candidate flags are the same and nobody installed
    // another one (snapshot epoch), the next Filter neither rebuilds nor re-sorts — and its chain resumes from the previous
    // chain's checkpoints (include/gangfit.h, "Incremental FIFO chains")
    uint64_t built_epoch_ = 0, built_cluster_ = 0, built_usage_ = 0;
    std::vector<uint32_t> built_flags_;
    bool built_set_ = false;               // ... built over a node set (selectDriverNodeFlatGroup),
    std::vector<uint64_t> built_members_;  // this row of the resident cluster
    // The reference parses the nine annotations of every earlier driver on every Filter (sparkpods.go:73-137 from
    // resource.go:231) and matches the request's NodeNames against the node set again.  Both are pure functions of things
    // that carry a version: the flat route keeps the canonical requests per (pod UID, resourceVersion) and the candidate
    // flags per (cluster version, NodeNames).
    // Predicate requests run on per-request threads (cmd/endpoints.go:29-37): everything below is read and written under
    // flat_mu_, which a flat Filter takes before it touches the caches and holds until it returns (always before the
    // context's sequence lock, never the other way round).
    struct ParsedApp {
        uint64_t version = 0;
        uint64_t seen = 0;  // flat_calls_ of the last Filter that used the entry: what a prune keeps
        PodApp parsed;
    };
    std::shared_ptr<std::mutex> flat_mu_ = std::make_shared<std::mutex>();  // (the extender stays copyable: copies share it)
    uint64_t flat_calls_ = 0;
    std::unordered_map<std::string, ParsedApp> parsed_apps_;  // pruned to the pods of the current request when it outgrows them
    uint64_t flags_cluster_ = 0, flags_hash_ = 0;
    std::vector<std::string> flags_names_;  // the NodeNames the cached flags were computed from (a hash hit is confirmed on them)
    std::vector<uint32_t> flags_cache_;
    Binpacker binpacker_;
    NodeSorter sorter_;
    bool isFIFO_;
    FifoConfig fifo_;
};

}  // namespace gangfit::host
