#include "failover.hpp"

#include <algorithm>
#include <map>

#include "binpacker.hpp"
#include "extender.hpp"

namespace gangfit::host {

namespace {

// executorResources x count, exactly (the reference reaches it by repeated Add)
Resources times(const int64_t exe[3], uint32_t count) {
    Resources r;
    r.CPU = Quantity::FromNano((i128)exe[0] * 1000000 * count);
    r.Memory = Quantity::FromNano((i128)exe[1] * 1000000000 * count);
    r.NvidiaGPU = Quantity::FromNano((i128)exe[2] * 1000000000 * count);
    return r;
}

std::vector<FindNodesResult> run(gf_ctx* ctx, bool chained, const std::vector<FindNodesRequest>& requests,
                                 const NodeGroupResources& available, const std::vector<Node>& orderedNodes) {
    std::vector<FindNodesResult> out(requests.size());
    auto not_served = [&](const std::string& why) {
        for (FindNodesResult& r : out) {
            r.served = false;
            r.error = why;
        }
        return out;
    };
    if (requests.empty()) return out;
    // flatten: node index = position in orderedNodes (each node once, :297-314); availableResources[n.Name] exists for every
    // ordered node (both derive from schedulableNodes)
    const uint32_t n = (uint32_t)orderedNodes.size();
    std::vector<int64_t> cols[3];
    std::vector<uint32_t> order(n);
    for (int j = 0; j < 3; ++j) cols[j].resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        auto it = available.find(orderedNodes[i].Name);
        if (it == available.end()) return not_served("node " + orderedNodes[i].Name + " has no availableResources entry");
        int64_t v[3];
        if (!it->second.canonical(v)) return not_served("available resources of node " + orderedNodes[i].Name + " are not exactly representable");
        for (int j = 0; j < 3; ++j) cols[j][i] = v[j];
        order[i] = i;
    }
    std::vector<int64_t> exe(3 * requests.size());
    std::vector<int32_t> k(requests.size());
    uint64_t total = 0;
    for (size_t q = 0; q < requests.size(); ++q) {
        if (!requests[q].executorResources.canonical(&exe[3 * q]) || exe[3 * q] < 0 || exe[3 * q + 1] < 0 || exe[3 * q + 2] < 0)
            return not_served("executor resources are not exactly representable");
        if (requests[q].executorCount <= 0 || requests[q].executorCount > GF_MAX_K) return not_served("executor count out of range");
        k[q] = requests[q].executorCount;
        total += (uint64_t)k[q];
    }
    CtxSequence seq(ctx);
    if (gf_snapshot_set(ctx, n, cols[0].data(), cols[1].data(), cols[2].data(), nullptr, nullptr, nullptr) != GF_OK ||
        gf_orders_set(ctx, nullptr, 0, order.data(), n) != GF_OK)
        return not_served(std::string("snapshot upload: ") + gf_last_error(ctx));
    std::vector<gf_find_result> res(requests.size());
    std::vector<uint32_t> nodes(total + 1);
    if (gf_find_nodes(ctx, chained ? 1 : 0, (uint32_t)requests.size(), exe.data(), k.data(), res.data(), nodes.data(), total,
                      nullptr) != GF_OK)
        return not_served(std::string("gf_find_nodes: ") + gf_last_error(ctx));
    uint64_t off = 0;
    for (size_t q = 0; q < requests.size(); ++q) {
        FindNodesResult& r = out[q];
        std::map<uint32_t, uint32_t> mult;
        for (uint32_t i = 0; i < res[q].placed; ++i) {
            const uint32_t node = nodes[off + i];
            r.executorNodeNames.push_back(orderedNodes[node].Name);
            ++mult[node];
        }
        // the `reserved` map, rebuilt as include/gangfit.h documents: every node up to last_node was reached and carries
        // one failing add on top of its placements, except last_node itself when the count was reached there
        if (res[q].last_node != GF_NO_NODE)
            for (uint32_t node = 0; node <= res[q].last_node && node < n; ++node) {
                uint32_t adds = (mult.count(node) ? mult[node] : 0u) + 1u;
                if (node == res[q].last_node && res[q].placed == (uint32_t)k[q]) --adds;
                r.reserved[orderedNodes[node].Name] = times(&exe[3 * q], adds);
            }
        off += (uint64_t)k[q];
    }
    return out;
}

}  // namespace

FindNodesResult findNodes(gf_ctx* ctx, int executorCount, const Resources& executorResources,
                          const NodeGroupResources& availableResources, const std::vector<Node>& orderedNodes) {
    return run(ctx, false, {{executorCount, executorResources}}, availableResources, orderedNodes)[0];
}

std::vector<FindNodesResult> findNodesForStaleApplications(gf_ctx* ctx, const std::vector<FindNodesRequest>& requests,
                                                           NodeGroupResources* availableResources,
                                                           const std::vector<Node>& orderedNodes) {
    std::vector<FindNodesResult> out = run(ctx, true, requests, *availableResources, orderedNodes);
    for (const FindNodesResult& r : out) {
        if (!r.served) break;
        for (const auto& [node, res] : r.reserved) (*availableResources)[node].Sub(res);  // NodeGroupResources.Sub (:159)
    }
    return out;
}

ReconcileRows buildReconcileRows(const std::vector<std::string>& nodeInstanceGroup, const std::vector<int64_t>& nodeCreationTimestamp,
                                 const std::vector<std::string>& requestInstanceGroup) {
    ReconcileRows rows;
    const size_t n = nodeInstanceGroup.size();
    std::map<std::string, uint32_t> row_of;
    const auto row = [&](const std::string& group) {
        auto it = row_of.find(group);
        if (it == row_of.end()) {
            it = row_of.emplace(group, (uint32_t)rows.groups.size()).first;
            rows.groups.push_back(group);
        }
        return it->second;
    };
    std::vector<uint32_t> node_row(n);
    for (size_t i = 0; i < n; ++i) node_row[i] = row(nodeInstanceGroup[i]);
    for (const std::string& group : requestInstanceGroup) rows.req_set.push_back(row(group));
    rows.words_per_row = (n + 63) / 64;
    rows.words.assign(rows.groups.size() * rows.words_per_row, 0);
    for (size_t i = 0; i < n; ++i) rows.words[node_row[i] * rows.words_per_row + i / 64] |= UINT64_C(1) << (i % 64);
    rows.visit.resize(n);
    for (size_t i = 0; i < n; ++i) rows.visit[i] = (uint32_t)i;
    std::stable_sort(rows.visit.begin(), rows.visit.end(), [&](uint32_t a, uint32_t b) {
        const int64_t ta = a < nodeCreationTimestamp.size() ? nodeCreationTimestamp[a] : 0;
        const int64_t tb = b < nodeCreationTimestamp.size() ? nodeCreationTimestamp[b] : 0;
        return ta > tb;  // newest first (failover.go:292-294)
    });
    rows.create_rank.resize(n);
    for (size_t p = 0; p < n; ++p) rows.create_rank[rows.visit[p]] = (uint32_t)p;
    return rows;
}

std::vector<FindNodesResult> findNodesForStaleApplicationsResident(
    gf_ctx* ctx, const FlatCluster& cluster, const std::vector<std::string>& nodeInstanceGroup,
    const std::vector<int64_t>& nodeCreationTimestamp, const std::vector<std::string>& requestInstanceGroup,
    const std::vector<FindNodesRequest>& requests, std::map<std::string, NodeGroupResources>* availableResources, bool* residentRoute) {
    if (residentRoute) *residentRoute = false;
    const size_t R = requests.size(), n = cluster.names.size();
    std::vector<FindNodesResult> out(R);
    if (R == 0) return out;
    if (nodeInstanceGroup.size() != n || nodeCreationTimestamp.size() != n || requestInstanceGroup.size() != R) {
        for (FindNodesResult& r : out) {
            r.served = false;
            r.error = "one instance group and one creation timestamp per node, one instance group per request";
        }
        return out;
    }
    const ReconcileRows rows = buildReconcileRows(nodeInstanceGroup, nodeCreationTimestamp, requestInstanceGroup);
    // every row's ordered nodes: its ready, schedulable members in visiting order — what the device walks, and what the route
    // that installs is given
    std::vector<std::vector<uint32_t>> ordered(rows.groups.size());
    for (const uint32_t node : rows.visit) {
        const uint32_t fl = cluster.base_flags[node];
        if ((fl & GF_NODE_READY) == 0u || (fl & GF_NODE_UNSCHEDULABLE) != 0u) continue;
        for (size_t s = 0; s < rows.groups.size(); ++s)
            if ((rows.words[s * rows.words_per_row + node / 64] >> (node % 64)) & 1u) ordered[s].push_back(node);
    }
    std::vector<int64_t> exe(3 * R);
    std::vector<int32_t> k(R);
    uint64_t total = 0;
    bool representable = true;
    for (size_t q = 0; q < R && representable; ++q) {
        representable = requests[q].executorResources.canonical(&exe[3 * q]) && exe[3 * q] >= 0 && exe[3 * q + 1] >= 0 &&
                        exe[3 * q + 2] >= 0 && requests[q].executorCount > 0 && requests[q].executorCount <= GF_MAX_K;
        k[q] = requests[q].executorCount;
        total += representable ? (uint64_t)k[q] : 0u;
    }
    std::vector<gf_find_result> res(R);
    std::vector<uint32_t> nodes(total + 1);
    bool answered = false;
    if (representable) {
        CtxSequence seq(ctx);
        answered = gf_cluster_find_nodes(ctx, 1, (uint32_t)rows.groups.size(), rows.words.data(), rows.create_rank.data(), (uint32_t)R,
                                         exe.data(), k.data(), rows.req_set.data(), res.data(), nodes.data(), total, nullptr,
                                         nullptr) == GF_OK;
    }
    if (!answered) {  // today's route, one instance group after the other
        for (size_t s = 0; s < rows.groups.size(); ++s) {
            std::vector<FindNodesRequest> mine;
            std::vector<size_t> at;
            for (size_t q = 0; q < R; ++q)
                if (rows.req_set[q] == s) {
                    mine.push_back(requests[q]);
                    at.push_back(q);
                }
            if (mine.empty() || ordered[s].empty()) continue;  // (no node to walk: findNodes returns nothing, served)
            std::vector<Node> orderedNodes(ordered[s].size());
            for (size_t i = 0; i < ordered[s].size(); ++i) orderedNodes[i].Name = cluster.names[ordered[s][i]];
            std::vector<FindNodesResult> got = findNodesForStaleApplications(ctx, mine, &(*availableResources)[rows.groups[s]], orderedNodes);
            for (size_t i = 0; i < at.size(); ++i) out[at[i]] = std::move(got[i]);
        }
        return out;
    }
    if (residentRoute) *residentRoute = true;
    uint64_t off = 0;
    for (size_t q = 0; q < R; ++q) {
        FindNodesResult& r = out[q];
        std::map<uint32_t, uint32_t> mult;
        for (uint32_t i = 0; i < res[q].placed; ++i) {
            const uint32_t node = nodes[off + i];
            r.executorNodeNames.push_back(cluster.names[node]);
            ++mult[node];
        }
        // the `reserved` map, rebuilt as include/gangfit.h documents, along the row's own order
        if (res[q].last_node != GF_NO_NODE)
            for (const uint32_t node : ordered[rows.req_set[q]]) {
                uint32_t adds = (mult.count(node) ? mult[node] : 0u) + 1u;
                const bool last = node == res[q].last_node;
                if (last && res[q].placed == (uint32_t)k[q]) --adds;
                r.reserved[cluster.names[node]] = times(&exe[3 * q], adds);
                if (last) break;
            }
        NodeGroupResources& available = (*availableResources)[rows.groups[rows.req_set[q]]];
        for (const auto& [node, reserved] : r.reserved) available[node].Sub(reserved);  // NodeGroupResources.Sub (:159)
        off += (uint64_t)k[q];
    }
    return out;
}

}  // namespace gangfit::host
