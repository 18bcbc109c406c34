// CPU-only test of the pipeline planner (lattisense_amd/csrc/task_pipeline.h), compiled by tests/test_task_pipeline.py with
// -fsanitize=address,undefined together with lattisense_amd/csrc/task_graph.cpp.  argv[1]: a graph of many independent
// subgraphs and a large input volume, argv[2]: a small graph of a few, argv[3]: a graph of one.  Properties of the plan are
// held, not recorded numbers: the components are counted here by a flood fill of its own, and so is the input volume the
// byte threshold is compared with.
#include <cstdio>
#include <map>
#include <set>
#include <string>

#include "../../lattisense_amd/csrc/task_pipeline.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

namespace {
using namespace lsa;

bool key(const DatumNode* d) { return d->datum_type == TYPE_RELIN_KEY || d->datum_type == TYPE_GALOIS_KEY || d->datum_type == TYPE_SWITCH_KEY; }

bool key_only(const ComputeNode& c) {
    for (auto* d : c.input_nodes)
        if (!key(d)) return false;
    for (auto* d : c.output_nodes)
        if (!key(d)) return false;
    return true;
}

// compute node -> component id, flooding over the data that are not keys; nodes that touch keys only get no component
std::map<const ComputeNode*, int> components(const TaskGraph& g, int* count) {
    std::map<const ComputeNode*, int> comp;
    *count = 0;
    for (auto& kv : g.computes) {
        if (key_only(kv.second) || comp.count(&kv.second)) continue;
        std::vector<const ComputeNode*> todo{&kv.second};
        comp[&kv.second] = *count;
        while (!todo.empty()) {
            const ComputeNode* c = todo.back();
            todo.pop_back();
            auto visit = [&](const DatumNode* d) {
                if (key(d)) return;
                for (auto* lists : {&d->predecessors, &d->successors})
                    for (const ComputeNode* o : *lists)
                        if (!comp.count(o)) {
                            comp[o] = *count;
                            todo.push_back(o);
                        }
            };
            for (auto* d : c->input_nodes) visit(d);
            for (auto* d : c->output_nodes) visit(d);
        }
        ++*count;
    }
    return comp;
}

double input_bytes(const TaskGraph& g) {
    double bytes = 0;
    const double n = (double)g.parameter["n"].as_int();
    for (NodeIndex idx : g.inputs) {
        const DatumNode& d = g.data.at(idx);
        if (key(&d) || !d.fhe_prop) continue;
        const bool ringt = d.fhe_prop->p && d.fhe_prop->p->is_ringt;
        bytes += 8.0 * n * (d.datum_type == TYPE_CIPHERTEXT ? d.fhe_prop->degree + 1 : 1) * (ringt ? 1 : d.fhe_prop->level + 1);
    }
    return bytes;
}

int check_plan(const TaskGraph& g, const Levels& levels, const PipelinePlan& plan, int n_components, const std::map<const ComputeNode*, int>& comp,
               int shards) {
    CHECK((int)plan.chunk_levels.size() == plan_chunk_count((size_t)n_components, shards));
    CHECK(plan.chunk_levels.size() >= 2);
    CHECK(plan.shared_levels.size() == levels.size());
    // every compute node exactly once, at its own top_level; the shared levels hold exactly the key-only nodes
    std::map<const ComputeNode*, int> seen;
    for (size_t l = 0; l < plan.shared_levels.size(); l++)
        for (ComputeNode* n : plan.shared_levels[l]) {
            CHECK(n->sched_meta.top_level == (int)l && key_only(*n));
            seen[n]++;
        }
    std::map<const DatumNode*, int> datum_chunk;
    std::map<int, int> comp_chunk;
    for (size_t ch = 0; ch < plan.chunk_levels.size(); ch++) {
        const Levels& cl = plan.chunk_levels[ch];
        CHECK(cl.size() == levels.size());
        int store_level = -1;
        size_t nodes = 0;
        for (size_t l = 0; l < cl.size(); l++)
            for (ComputeNode* n : cl[l]) {
                CHECK(n->sched_meta.top_level == (int)l && !key_only(*n));
                seen[n]++;
                nodes++;
                // a whole component lies in one chunk, so no datum other than a key is touched by two chunks
                auto cc = comp_chunk.emplace(comp.at(n), (int)ch);
                CHECK(cc.first->second == (int)ch);
                for (auto* lists : {&n->input_nodes, &n->output_nodes})
                    for (const DatumNode* d : *lists) {
                        if (key(d)) continue;
                        auto dc = datum_chunk.emplace(d, (int)ch);
                        CHECK(dc.first->second == (int)ch);
                    }
                // the stores sit in one level, with nothing but stores and CPU nodes from there on
                if (n->op() == OperationType::STORE_FROM_BACKEND) {
                    CHECK(store_level < 0 || store_level == (int)l);
                    store_level = (int)l;
                }
            }
        CHECK(nodes > 0 && store_level >= 0);
        for (size_t l = (size_t)store_level; l < cl.size(); l++)
            for (ComputeNode* n : cl[l]) CHECK(n->on_cpu || n->op() == OperationType::STORE_FROM_BACKEND);
    }
    CHECK(seen.size() == g.computes.size());
    for (auto& kv : g.computes) CHECK(seen.count(&kv.second) && seen.at(&kv.second) == 1);
    return 0;
}

bool same(const PipelinePlan& a, const PipelinePlan& b) { return a.shared_levels == b.shared_levels && a.chunk_levels == b.chunk_levels; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    TaskGraph g = TaskGraph::load_for_gpu(argv[1]);
    const Levels levels = graph_levels(g);
    int n_components = 0;
    const auto comp = components(g, &n_components);
    CHECK(n_components >= 16);   // the fixture is a batch of independent operations
    for (int shards : {1, 2, 5}) {
        const PipelinePlan plan = plan_pipeline(g, levels, shards, 0.0);
        if (check_plan(g, levels, plan, n_components, comp, shards)) return 1;
        std::printf("shards %d: %d components in %zu chunks\n", shards, n_components, plan.chunk_levels.size());
    }
    // the byte threshold: pipelined if and only if the non-key inputs hold at least that much (256 MiB is the switch's default)
    const double volume = input_bytes(g), dflt = 256.0 * 1048576.0;
    CHECK(volume > 0);
    const PipelinePlan at_default = plan_pipeline(g, levels, 1, dflt);
    CHECK(at_default.chunk_levels.empty() == (volume < dflt));
    if (volume >= dflt) CHECK(same(at_default, plan_pipeline(g, levels, 1, 0.0)));
    else CHECK(at_default.shared_levels.empty());
    CHECK(same(plan_pipeline(g, levels, 1, volume), plan_pipeline(g, levels, 1, 0.0)));   // the bound itself is inside
    const PipelinePlan above = plan_pipeline(g, levels, 1, volume * 1.000001);
    CHECK(above.chunk_levels.empty() && above.shared_levels.empty());
    std::printf("input volume %.1f MiB: %s at the default threshold\n", volume / 1048576.0, volume >= dflt ? "pipelined" : "not pipelined");

    // a small graph (four subgraphs of 128 KiB of input each): left alone at the default threshold; cut up like any other
    // when a test forces the pipelined path with a threshold of 0
    TaskGraph few = TaskGraph::load_for_gpu(argv[2]);
    const Levels few_levels = graph_levels(few);
    int few_components = 0;
    const auto few_comp = components(few, &few_components);
    CHECK(few_components >= 4 && input_bytes(few) < dflt);
    const PipelinePlan few_default = plan_pipeline(few, few_levels, 1, dflt);
    CHECK(few_default.chunk_levels.empty() && few_default.shared_levels.empty());
    for (int shards : {1, 2, 5})
        if (check_plan(few, few_levels, plan_pipeline(few, few_levels, shards, 0.0), few_components, few_comp, shards)) return 1;

    // one component: nothing to pipeline, whatever the threshold
    TaskGraph one = TaskGraph::load_for_gpu(argv[3]);
    const Levels one_levels = graph_levels(one);
    int one_components = 0;
    components(one, &one_components);
    CHECK(one_components == 1);
    for (int shards : {1, 2, 5}) {
        const PipelinePlan plan = plan_pipeline(one, one_levels, shards, 0.0);
        CHECK(plan.chunk_levels.empty() && plan.shared_levels.empty());
    }
    std::printf("OK task_pipeline\n");
    return 0;
}
