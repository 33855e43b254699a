// failover.hpp — the one compute step of the failover reconciler, served by libgangfit (host side, C++ mirror).
//
//   findNodes                                    internal/extender/failover.go:412-436
//   constructResourceReservation (call site)     internal/extender/failover.go:350-390 (:368)
//   r.availableResources[ig].Sub(reserved)       internal/extender/failover.go:159
//   availableResourcesPerInstanceGroup           internal/extender/failover.go:286-322
// The reconciler itself (listing pods, patching / creating reservations, demands, soft reservations) is k8s API
// bookkeeping and stays in the Go host; what is mirrored here is where it asks "which nodes still hold k executors of this
// size, walking the nodes in order" — including the reference's over-add: the `reserved[n].Add(exe)` that fails the
// comparison is not taken back (:424-427), and the caller subtracts the whole map (:159).
#pragma once

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "gangfit.h"
#include "resources.hpp"

namespace gangfit::host {

struct FindNodesResult {
    std::vector<std::string> executorNodeNames;  // may hold fewer than executorCount names (:369-372 only logs)
    NodeGroupResources reserved;                 // what the reference returns as reservedResources
    bool served = true;                          // false: not evaluated on the device (see `error`)
    std::string error;
};

struct FindNodesRequest {
    int executorCount;            // MinExecutorCount - len(executors), > 0 (:366-367)
    Resources executorResources;
};

// findNodes(executorCount, executorResources, availableResources, orderedNodes): one request.
FindNodesResult findNodes(gf_ctx* ctx, int executorCount, const Resources& executorResources,
                          const NodeGroupResources& availableResources, const std::vector<Node>& orderedNodes);

// The reconciler's loop over the stale applications of ONE instance group as a single chained device call: request i sees
// availableResources after the `Sub` of requests 0..i-1.  *availableResources is updated like r.availableResources[ig].
std::vector<FindNodesResult> findNodesForStaleApplications(gf_ctx* ctx, const std::vector<FindNodesRequest>& requests,
                                                           NodeGroupResources* availableResources,
                                                           const std::vector<Node>& orderedNodes);

// What the resident reconcile sends beside the requests: one bit row per instance group over the flat cluster's node indices
// (schedulableNodes[instanceGroup], :296-314 — readiness is the device's to test, from the flags of gf_cluster_set) and the
// position at which the reconciler visits every node: newest creation timestamp first (:292-294; the reference's sort.Slice is
// unstable, ties here keep the input order).  A group only a request names gets an empty row.
struct ReconcileRows {
    std::vector<std::string> groups;    // row -> instance group: the nodes' groups by first appearance, then the requests' own
    size_t words_per_row = 0;           // ceil(nodes / 64)
    std::vector<uint64_t> words;        // groups.size() rows
    std::vector<uint32_t> create_rank;  // node -> position
    std::vector<uint32_t> visit;        // position -> node
    std::vector<uint32_t> req_set;      // request -> row
};
ReconcileRows buildReconcileRows(const std::vector<std::string>& nodeInstanceGroup, const std::vector<int64_t>& nodeCreationTimestamp,
                                 const std::vector<std::string>& requestInstanceGroup);

struct FlatCluster;  // extender.hpp

// The reconciler's findNodes for the stale applications of EVERY instance group as ONE gf_cluster_find_nodes call on the resident
// cluster (include/gangfit.h): nothing is installed, so the driver Filter this reconcile runs in front of keeps its snapshot, chain
// cache and resident worker.  `cluster` is the flat cluster whose columns, overhead rows and usage the extender's flat Filter keeps
// on ctx; nodeInstanceGroup / nodeCreationTimestamp hold one entry per node of it, requestInstanceGroup one per request.  Request i
// sees its group's table after the `Sub` of the earlier requests of that group; every request's `reserved` map is rebuilt from the
// results as the header describes and subtracted from (*availableResources)[group] like r.availableResources[ig] (:159).
// On any refusal of the entry point — and for quantities that are not exactly representable — every group is answered by
// findNodesForStaleApplications on its own ordered nodes (which installs).  *residentRoute (nullable): true when the resident entry
// point answered.
std::vector<FindNodesResult> findNodesForStaleApplicationsResident(
    gf_ctx* ctx, const FlatCluster& cluster, const std::vector<std::string>& nodeInstanceGroup,
    const std::vector<int64_t>& nodeCreationTimestamp, const std::vector<std::string>& requestInstanceGroup,
    const std::vector<FindNodesRequest>& requests, std::map<std::string, NodeGroupResources>* availableResources,
    bool* residentRoute = nullptr);

}  // namespace gangfit::host
