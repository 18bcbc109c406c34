// task_pipeline.h — which parts of a task graph can run as independent chunks.  Pure planning over the TaskGraph, plain C++17,
// no HIP: the runtime (task_runtime.hip) deals the chunks out to shards (shard_plan.h), tests/cpp/test_task_pipeline.cpp holds
// the plan's properties on committed graphs (CPU-only test).
#pragma once
#include <algorithm>
#include <functional>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "shard_plan.h"
#include "task_graph.h"

namespace lsa {

using Levels = std::vector<std::vector<ComputeNode*>>;   // [top_level] -> nodes

struct PipelinePlan {
    Levels shared_levels;                // key export / load: before every chunk
    std::vector<Levels> chunk_levels;    // [chunk][level] -> nodes; empty: not pipelined
};

inline bool is_key_datum(const DatumNode* d) {
    return d->datum_type == TYPE_RELIN_KEY || d->datum_type == TYPE_GALOIS_KEY || d->datum_type == TYPE_SWITCH_KEY;
}

// the graph's compute nodes by top_level, in node-index order within a level
inline Levels graph_levels(TaskGraph& g) {
    Levels levels(g.max_top_level + 1);
    for (auto& kv : g.computes) levels[kv.second.sched_meta.top_level].push_back(&kv.second);
    for (auto& lv : levels)
        std::sort(lv.begin(), lv.end(), [](const ComputeNode* a, const ComputeNode* b) { return a->index < b->index; });
    return levels;
}

// Independent subgraphs = connected components of the compute nodes over the non-key data (evaluation keys are shared
// read-only inputs).  Pipelining needs the simple shape every benchmark graph has: per chunk, CPU nodes only before
// the loads and after the stores, and all stores in one level.  `levels` are the graph's nodes by top_level; a graph whose
// non-key inputs hold fewer than `min_input_bytes` is not pipelined (the caller reads the switch).
inline PipelinePlan plan_pipeline(const TaskGraph& g, const Levels& levels, int n_shards, double min_input_bytes) {
    std::unordered_map<const ComputeNode*, const ComputeNode*> parent;
    std::function<const ComputeNode*(const ComputeNode*)> find = [&](const ComputeNode* x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    for (auto& kv : g.computes) parent[&kv.second] = &kv.second;
    std::unordered_set<const ComputeNode*> key_only;
    for (auto& kv : g.computes) {
        bool all_key = true;
        for (auto* d : kv.second.input_nodes) all_key = all_key && is_key_datum(d);
        for (auto* d : kv.second.output_nodes) all_key = all_key && is_key_datum(d);
        if (all_key) key_only.insert(&kv.second);
    }
    for (auto& kv : g.data) {
        const DatumNode& d = kv.second;
        if (is_key_datum(&d)) continue;
        const ComputeNode* first = nullptr;
        auto join = [&](const ComputeNode* c) {
            if (!first) first = c;
            else parent[find(c)] = find(first);
        };
        for (auto* c : d.predecessors) join(c);
        for (auto* c : d.successors) join(c);
    }
    std::map<NodeIndex, const ComputeNode*> comps;   // smallest node index -> representative
    std::unordered_map<const ComputeNode*, NodeIndex> lowest;
    for (auto& kv : g.computes) {
        if (key_only.count(&kv.second)) continue;
        const ComputeNode* r = find(&kv.second);
        auto it = lowest.find(r);
        if (it == lowest.end() || kv.first < it->second) lowest[r] = kv.first;
    }
    for (auto& kv : lowest) comps[kv.second] = kv.first;
    if (comps.size() < 4) return {};
    // worth it only when the copies dominate: small graphs keep the whole-level batches (fewer, larger launches)
    double in_bytes = 0;
    const double n_ring = (double)g.parameter["n"].as_int();
    for (NodeIndex idx : g.inputs) {
        const DatumNode& d = g.data.at(idx);
        if (is_key_datum(&d) || !d.fhe_prop) continue;
        const bool ringt = d.fhe_prop->p && d.fhe_prop->p->is_ringt;
        in_bytes += 8.0 * n_ring * (d.datum_type == TYPE_CIPHERTEXT ? d.fhe_prop->degree + 1 : 1) * (ringt ? 1 : d.fhe_prop->level + 1);
    }
    if (in_bytes < min_input_bytes) return {};   // (tests force the pipelined path on small graphs with 0)
    const int nchunks = plan_chunk_count(comps.size(), n_shards);
    std::unordered_map<const ComputeNode*, int> chunk_of;
    int ci = 0;
    for (auto& kv : comps) chunk_of[kv.second] = (int)((long long)ci++ * nchunks / (long long)comps.size());
    PipelinePlan plan{Levels(levels.size()), std::vector<Levels>(nchunks, Levels(levels.size()))};
    for (size_t l = 0; l < levels.size(); l++)
        for (ComputeNode* n : levels[l]) {
            if (key_only.count(n)) plan.shared_levels[l].push_back(n);
            else plan.chunk_levels[chunk_of.at(find(n))][l].push_back(n);
        }
    for (auto& chunk : plan.chunk_levels) {   // shape check
        int first_load = -1, store_level = -1;
        for (size_t l = 0; l < chunk.size(); l++)
            for (ComputeNode* n : chunk[l]) {
                if (n->op() == OperationType::LOAD_TO_BACKEND && first_load < 0) first_load = (int)l;
                if (n->op() == OperationType::STORE_FROM_BACKEND) {
                    if (store_level >= 0 && store_level != (int)l) return {};
                    store_level = (int)l;
                }
            }
        if (first_load < 0 || store_level < 0) return {};
        for (size_t l = 0; l < chunk.size(); l++)
            for (ComputeNode* n : chunk[l]) {
                if (n->on_cpu && (int)l >= first_load && (int)l <= store_level) return {};
                // from the store level on: nothing but the stores themselves and CPU-side nodes
                if ((int)l >= store_level && !n->on_cpu && n->op() != OperationType::STORE_FROM_BACKEND) return {};
            }
    }
    return plan;
}

}  // namespace lsa
