// task_runtime.hip — the GPU task runner: drop-in for mega_ag_runners/gpu/gpu_wrapper.cu (FheGpuTask, _run_mega_ag_impl,
// the extern "C" entry points :481-530), re-designed for MI355X.  This unit holds the task handle and run(); what a run is made
// of lives next to it (task_internal.h names the units):
//
//   * LEVEL-BATCHED scheduling instead of a 1 ms-polling dispatcher + 2 streams: the backend nodes of one topological level run
//     as a few batched launch sequences (task_dispatch.hip).
//   * H2D/D2H go through one pinned staging slab per level and ONE hipMemcpyAsync per group; evaluation keys stay on the device
//     across runs (task_transfer.hip).
//   * a graph of independent subgraphs is cut into chunks (task_pipeline.h), dealt out to shards = one device + two lanes each
//     (shard_plan.h), and pipelined over each shard's lanes.
//   * the device context (tables) is created once per (task, device, lane) and reused across run() calls.
//   * CPU-side nodes (caller's export/import executors, custom nodes) of a level run on a small thread pool.
//   * every failure is turned into a non-zero return code + lsa_last_error(); nothing throws across extern "C".
#include <chrono>
#include <future>

#include "shard_plan.h"
#include "task_internal.h"

using namespace lsa;
using namespace lsa::task;

struct fhe_task_handle_st {
    // Pools are keyed by (device, lane): one task handle may be run on any device, one run() at a time (the reference's
    // multi-GPU mode, README.md:195-202 / gpu_wrapper.cu:148-149); run() calls on one handle are serialised by run_mu.
    LanePools pools{BufAllocator{hip_buf_alloc, hip_buf_release}, (size_t)(sw::pool_max_dev_gib() * 1073741824.0),
                    (size_t)(sw::pool_max_pin_gib() * 1073741824.0)};   // declared first: destroyed last
    std::mutex run_mu;
    std::vector<int> devices_;   // lsa_task_set_devices: the shards of a run (a device may repeat); empty = the run's gpu_device alone
    KeyCache keys;
    TaskGraph g;
    Levels levels;
    PipelinePlan pipeline;       // planned for `planned_shards_` shards
    int planned_shards_ = 0;
    // key = LanePools::key(device, lane).  Entries are created by run() before any shard thread starts: concurrent callers
    // only look their own up.
    std::map<int, std::unique_ptr<Lane>> lanes;
    Dispatcher dispatch{g};      // (after `lanes`: its bootstrap plans go before the contexts they were built on)
    bool native_frontend = false;   // lsa_frontend_bind: output handles are lsa_host_ciphertext
    std::atomic<int> last_direct_loads{0}, last_direct_stores{0};
    int last_shards = 1, last_chunks = 0, last_key_peer_copies = 0;
    double last_ms = 0;

    explicit fhe_task_handle_st(const std::string& project_path) {
        g = TaskGraph::load_for_gpu(project_path + "/mega_ag.json");
        for (auto& kv : g.computes) {
            ComputeNode& c = kv.second;
            if (c.custom_prop || c.on_cpu) continue;
            const OperationType op = c.op();
            if (op == OperationType::LOAD_TO_BACKEND || op == OperationType::STORE_FROM_BACKEND) continue;
            bind_gpu_executor(c, g.algo);
        }
        levels = graph_levels(g);
        if (!sw::no_pipeline()) plan(1);
    }
    void plan(int n_shards) {
        planned_shards_ = n_shards;
        pipeline = plan_pipeline(g, levels, n_shards, sw::pipeline_min_mib() * 1048576.0);
    }

    // the lane's context and stream, created on first use
    Lane& lane(int device, int lane_no) {
        auto it = lanes.find(LanePools::key(device, lane_no));
        if (it != lanes.end()) {
            it->second->c.use_device();
            return *it->second;
        }
        const mjson::Value& P = g.parameter;
        const int n = (int)P["n"].as_int();
        const int max_level = (int)P["max_level"].as_int();
        std::vector<u64> q = P["q"].as_u64_vector(), p = P["p"].as_u64_vector();
        // frontend/parameter.json lists 30 primes for CKKS n=65536 but says max_level 33: use what exists
        if ((int)q.size() > max_level + 1) q.resize(max_level + 1);
        u64 t = 0;
        if (g.algo == ALGO_BFV) t = P["t"].as_u64();
        auto c = std::make_unique<Context>(g.algo == ALGO_BFV ? LSA_ALGO_BFV : LSA_ALGO_CKKS, n, q.data(), (int)q.size(),
                                           p.data(), (int)p.size(), t, device);
        auto ln = std::make_unique<Lane>(device, lane_no, std::move(c), pools);
        return *(lanes[LanePools::key(device, lane_no)] = std::move(ln));
    }

    // the devices a run is spread over: lsa_task_set_devices' list, else the caller's gpu_device (-1: every visible device)
    std::vector<int> run_devices(int device) {
        if (device >= 0 && devices_.empty()) return {device};
        if (!devices_.empty()) return devices_;
        int n = 0;
        LSA_HIP(hipGetDeviceCount(&n));
        LSA_REQUIRE(n >= 1, "no HIP device");
        std::vector<int> all(n);
        for (int i = 0; i < n; i++) all[i] = i;
        return all;
    }

    void run(CArgument* in_args, uint64_t n_in, CArgument* out_args, uint64_t n_out, progress_callback_t cb, void* user, int device);
};

namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// what the levels, shards and finishers of one run() share
struct RunState {
    Avail avail;                // the upload lane's view: handles, C structs, keys; every shard starts from a copy
    Refs refs;                  // remaining-consumer counts: device data is dropped as soon as its last consumer has been enqueued
    OutHandles out_handles;     // task output datum -> the caller's pre-allocated handle
    const OutHandles* native_out = nullptr;   // &out_handles where they are the native front-end's (stores_enqueue)
    const bool trace = sw::task_trace();
    const progress_callback_t cb;
    void* const user;
    const int total;
    RunState(progress_callback_t cb, void* user, int total) : cb(cb), user(user), total(total) {}
    void progress(size_t nodes_done) {   // the callback fires from whichever thread finished something (wrapper.h:39-40)
        std::lock_guard<std::mutex> lk(progress_mu);
        completed += (int)nodes_done;
        const auto now = Clock::now();
        if (cb && (completed == total || now - last_cb >= std::chrono::milliseconds(100))) {
            cb(completed, total, user);
            last_cb = now;
        }
    }

  private:
    std::mutex progress_mu;
    int completed = 0;
    Clock::time_point last_cb = Clock::now() - std::chrono::seconds(1);
};

// inputs: flatten every CArgument's handle array, consume in mega_ag.inputs order; all Galois-key data nodes share the first
// Galois handle (cpu_task_utils.h:235-319).  Outputs: one handle per task output, in order.
void bind_handles(const TaskGraph& g, CArgument* in_args, uint64_t n_in, CArgument* out_args, uint64_t n_out, RunState& rs) {
    std::vector<void*> handles;
    for (uint64_t i = 0; i < n_in; i++) {
        void** arr = (void**)in_args[i].data;
        for (int j = 0; j < in_args[i].size; j++) handles.push_back(arr[j]);
    }
    std::shared_ptr<void> glk_shared;
    size_t hi = 0;
    for (NodeIndex idx : g.inputs) {
        const DatumNode& d = g.data.at(idx);
        if (d.datum_type == TYPE_GALOIS_KEY) {
            if (!glk_shared) {
                LSA_REQUIRE(hi < handles.size(), "not enough input handles for the task's inputs");
                glk_shared = std::shared_ptr<void>(handles[hi++], [](void*) {});
            }
            rs.avail[idx] = glk_shared;
        } else {
            LSA_REQUIRE(hi < handles.size(), "not enough input handles for the task's inputs");
            rs.avail[idx] = std::shared_ptr<void>(handles[hi++], [](void*) {});
        }
    }
    size_t oi = 0;
    for (uint64_t i = 0; i < n_out; i++) {
        void** arr = (void**)out_args[i].data;
        for (int j = 0; j < out_args[i].size; j++) {
            LSA_REQUIRE(oi < g.outputs.size(), "more output handles than task outputs");
            rs.out_handles[g.outputs[oi++]] = arr[j];
        }
    }
    LSA_REQUIRE(oi == g.outputs.size(), "fewer output handles than task outputs");
    for (auto& kv : g.data) rs.refs[kv.first] = (int)kv.second.successors.size();
}

void release_inputs(const std::vector<ComputeNode*>& level, Avail& av, Refs& rf) {
    for (ComputeNode* n : level)
        for (auto* in : n->input_nodes)
            if (--rf[in->index] <= 0 && !in->is_input && !in->is_output) av.erase(in->index);
}

// ---------------------------------------------------------------- CPU-side nodes (export / import / custom)
void run_cpu_nodes(const std::vector<ComputeNode*>& nodes, Avail& avail, const OutHandles& out_handles) {
    if (nodes.empty()) return;
    std::vector<std::any> outputs(nodes.size());
    std::vector<std::string> errors(nodes.size());
    const int nthreads = std::min((int)nodes.size(), host_threads());
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= nodes.size()) return;
            const ComputeNode* node = nodes[i];
            try {
                if (!node->executor) throw std::runtime_error("no executor bound for CPU node '" + node->id + "'");
                std::unordered_map<NodeIndex, std::any> ins;
                for (auto* in : node->input_nodes) ins[in->index] = avail.at(in->index);
                ExecutionContext ec;
                if (node->op() == OperationType::IMPORT_FROM_ABI) {
                    auto it = out_handles.find(node->output_nodes[0]->index);
                    if (it != out_handles.end()) ec.other_args.push_back(it->second);
                }
                node->executor(ec, ins, outputs[i], *node);
            } catch (const std::exception& e) {
                errors[i] = e.what()[0] ? e.what() : "executor failed";
            } catch (...) {
                errors[i] = "executor failed with a non-standard exception";
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; t++) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
    for (size_t i = 0; i < nodes.size(); i++) {
        if (!errors[i].empty()) throw Error(LSA_ERR_INTERNAL, "node '" + nodes[i]->id + "': " + errors[i]);
        avail[nodes[i]->output_nodes[0]->index] = outputs[i];
    }
}

// one level, everything in order on one lane, host-synchronous at the copies (graphs that are not pipelined, shared levels)
void run_level_sync(fhe_task_handle_st& h, RunState& rs, Lane& ln, const std::vector<ComputeNode*>& level) {
    if (level.empty()) return;
    Split sp = h.dispatch.split(level);
    auto t0 = Clock::now();
    if (!sp.loads.empty()) {
        auto keep = run_loads(ln, sp.loads, rs.avail, h.keys, h.last_direct_loads);
        LSA_HIP(hipStreamSynchronize(ln.s));
    }
    const double t_load = ms_since(t0);
    t0 = Clock::now();
    h.dispatch.run_buckets(ln, sp, rs.avail);
    if (rs.trace && !sp.bucket_order.empty()) LSA_HIP(hipStreamSynchronize(ln.s));
    const double t_gpu = ms_since(t0);
    t0 = Clock::now();
    if (!sp.stores.empty()) {
        StoreJob j = stores_enqueue(ln, sp.stores, rs.avail, rs.native_out, h.last_direct_stores);
        LSA_HIP(hipStreamSynchronize(ln.s));
        stores_finish(ln, j, rs.avail);
    }
    const double t_store = ms_since(t0);
    t0 = Clock::now();
    run_cpu_nodes(sp.cpu, rs.avail, rs.out_handles);
    const double t_cpu = ms_since(t0);
    if (rs.trace)
        fprintf(stderr, "[lsa task] level: %zu nodes  load %.2f ms  gpu %.2f ms  store %.2f ms  cpu %.2f ms\n",
                level.size(), t_load, t_gpu, t_store, t_cpu);
    release_inputs(level, rs.avail, rs.refs);
    if (!ln.pending.empty()) {  // slabs whose last reference is dropped here are freed after their readers ran
        LSA_HIP(hipStreamSynchronize(ln.s));
        ln.pending.clear();
    }
    rs.progress(level.size());
}

// ---------------------------------------------------------------- key fan-out
// the device operations fan_out_keys (shard_plan.h) drives: a copy lands in the pool, and is enqueued on the stream, of the
// target device's first lane
struct PeerOps {
    fhe_task_handle_st& h;
    const ShardPlan& plan;
    std::map<void*, std::shared_ptr<Slab>> slabs;
    int copies = 0;
    Lane& target(int d) {
        for (auto& sh : plan.shards)
            if (sh.device == d) return *h.lanes.at(LanePools::key(d, sh.lane0));
        return *h.lanes.at(LanePools::key(d, 0));
    }
    void* alloc(int d, size_t nbytes) {
        auto sl = target(d).dslab(nbytes / sizeof(u64));
        slabs[sl->ptr] = sl;
        return sl->ptr;
    }
    void peer_copy(void* dst, int dd, const void* sp, int sd, size_t nbytes) {
        LSA_HIP(hipSetDevice(dd));
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, dd, sd) == hipSuccess && can) {
            const hipError_t e = hipDeviceEnablePeerAccess(sd, 0);   // direct xGMI copies; already enabled is fine
            if (e != hipSuccess) (void)hipGetLastError();
        }
        LSA_HIP(hipMemcpyPeerAsync(dst, dd, sp, sd, nbytes, target(dd).s));
        copies++;
    }
};

// The shared evaluation keys were exported, uploaded and converted ONCE, on the upload lane's device; here they are copied
// device-to-device to every other distinct device of the plan (shards of one device share its copy).  Returns every device's
// view of the run's data: the upload lane's, with the keys replaced by the device's own copies.
std::map<int, Avail> fan_out_keys_to_devices(fhe_task_handle_st& h, RunState& rs, const ShardPlan& plan, Lane& up) {
    std::map<int, Avail> dev_avail;
    dev_avail[up.device] = rs.avail;
    if (plan.key_devices.size() <= 1) return dev_avail;
    std::vector<NodeIndex> key_idx;
    std::vector<KeyP> key_src;
    for (auto& kv : rs.avail)
        if (auto* kp = std::any_cast<KeyP>(&kv.second)) {
            key_idx.push_back(kv.first);
            key_src.push_back(*kp);
        }
    PeerOps ops{h, plan, {}, 0};
    for (size_t i = 1; i < plan.key_devices.size(); i++) {
        const int d = plan.key_devices[i];
        Avail av = rs.avail;
        // keys whose peer copy an earlier run left valid are taken from the cache, the others are copied now
        std::vector<void*> src_d;
        std::vector<size_t> bytes_d;
        std::vector<size_t> which;
        for (size_t k = 0; k < key_idx.size(); k++) {
            if (KeyP cached = h.keys.peer(up.device, d, key_idx[k], key_src[k])) {
                av[key_idx[k]] = cached;
                continue;
            }
            src_d.push_back(key_src[k]->key.data);
            bytes_d.push_back(key_src[k]->slab->words * sizeof(u64));
            which.push_back(k);
        }
        ShardPlan one = plan;   // fan-out of the missing keys to this device only
        one.key_devices = {up.device, d};
        auto table = fan_out_keys(one, src_d, bytes_d, ops);
        LSA_HIP(hipSetDevice(d));
        LSA_HIP(hipStreamSynchronize(ops.target(d).s));
        for (size_t j = 0; j < which.size(); j++) {
            const size_t k = which[j];
            auto dk = std::make_shared<DevKey>();
            dk->slab = ops.slabs.at(table.at(d)[j]);
            dk->key = key_src[k]->key;
            dk->key.data = (u64*)table.at(d)[j];
            dk->key.owned = false;
            if (key_src[k]->key.fp)   // the double copy travelled in the same slab
                dk->key.fp = reinterpret_cast<const double*>(dk->key.data + key_layout(up.c, dk->key.level).words);
            av[key_idx[k]] = dk;
            h.keys.put_peer(up.device, d, key_idx[k], key_src[k], dk);
        }
        dev_avail[d] = std::move(av);
    }
    h.last_key_peer_copies = ops.copies;
    LSA_HIP(hipSetDevice(up.device));
    return dev_avail;
}

// ---------------------------------------------------------------- shards
struct InFlight {   // a chunk between the enqueue of its copy-out and the end of its import
    int chunk = -1;
    Lane* lane = nullptr;
    size_t resume_level = 0;
    StoreJob job;
    std::vector<std::shared_ptr<Slab>> keep;
};

// Wait for the chunk's stream, wrap the results into C structs, run the import executors.  It runs on its own thread while the
// shard's thread stages and enqueues the next chunk, and touches no shared container: the structs live in a local map (only
// the import nodes read them), the lane's temporaries are released by this thread while the shard's thread is, by
// construction, busy with the OTHER lane.
void finish_chunk(fhe_task_handle_st& h, RunState& rs, InFlight* f) {
    Lane& ln = *f->lane;
    ln.c.use_device();
    auto t0 = Clock::now();
    LSA_HIP(hipStreamSynchronize(ln.s));
    const double t_wait = ms_since(t0);
    ln.pending.clear();
    f->keep.clear();
    auto& cl = h.pipeline.chunk_levels[f->chunk];
    t0 = Clock::now();
    Avail local;
    stores_finish(ln, f->job, local);
    f->job = StoreJob{};
    rs.progress(cl[f->resume_level].size());
    for (size_t l = f->resume_level + 1; l < cl.size(); l++) {
        if (cl[l].empty()) continue;
        Split sp = h.dispatch.split(cl[l]);
        LSA_REQUIRE(sp.loads.empty() && sp.stores.empty() && sp.bucket_order.empty(), "pipeline plan violated");
        run_cpu_nodes(sp.cpu, local, rs.out_handles);
        rs.progress(cl[l].size());
    }
    if (rs.trace) fprintf(stderr, "[lsa task] chunk %d device %d lane %d: waited %.2f ms, import %.2f ms\n", f->chunk, ln.device, ln.lane, t_wait, ms_since(t0));
    f->chunk = -1;
}

// a chunk's levels up to its stores: export, stage and copy in, compute, enqueue the copy-out; the rest happens in finish_chunk
void enqueue_chunk(fhe_task_handle_st& h, RunState& rs, InFlight& f, Avail& avail, Refs& refs) {
    Lane& ln = *f.lane;
    auto& cl = h.pipeline.chunk_levels[f.chunk];
    const auto t0 = Clock::now();
    for (size_t l = 0; l < cl.size(); l++) {
        if (cl[l].empty()) continue;
        Split sp = h.dispatch.split(cl[l]);
        if (!sp.stores.empty()) {
            f.job = stores_enqueue(ln, sp.stores, avail, rs.native_out, h.last_direct_stores);   // holds the device data alive until the copy ran
            f.resume_level = l;
            for (size_t l2 = l; l2 < cl.size(); l2++) release_inputs(cl[l2], avail, refs);
            break;
        }
        if (!sp.cpu.empty()) run_cpu_nodes(sp.cpu, avail, rs.out_handles);   // export executors
        if (!sp.loads.empty()) f.keep.push_back(run_loads(ln, sp.loads, avail, h.keys, h.last_direct_loads));
        h.dispatch.run_buckets(ln, sp, avail);
        release_inputs(cl[l], avail, refs);
        rs.progress(cl[l].size());
    }
    if (rs.trace) fprintf(stderr, "[lsa task] chunk %d device %d lane %d: enqueued in %.2f ms\n", f.chunk, ln.device, ln.lane, ms_since(t0));
}

// One shard: its chunks in order, alternating its two lanes.  While one lane's chunk computes and copies its results out, the
// other lane's chunk is staged and copied in.
void run_shard(fhe_task_handle_st& h, RunState& rs, const ShardPlan& plan, const std::map<int, Avail>& dev_avail, int si) {
    const ShardPlan::Shard sh = plan.shards[(size_t)si];
    Lane* lane[2] = {h.lanes.at(LanePools::key(sh.device, sh.lane0)).get(), h.lanes.at(LanePools::key(sh.device, sh.lane0 + 1)).get()};
    Avail my_avail = dev_avail.at(sh.device);   // the shard's own view: its chunks' data + the device's keys
    Refs my_refs = rs.refs;
    InFlight fly[2];
    std::future<void> done[2];
    try {
        int mine = 0;
        for (size_t ch = 0; ch < h.pipeline.chunk_levels.size(); ch++) {
            if (plan.chunk_shard[ch] != si) continue;
            const int li = mine++ & 1;
            if (done[li].valid()) done[li].get();   // the lane's previous chunk (two chunks in flight at most per shard); rethrows what it threw
            lane[li]->c.use_device();
            fly[li].chunk = (int)ch;
            fly[li].lane = lane[li];
            enqueue_chunk(h, rs, fly[li], my_avail, my_refs);
            done[li] = std::async(std::launch::async, finish_chunk, std::ref(h), std::ref(rs), &fly[li]);
        }
        for (int li = 0; li < 2; li++)
            if (done[li].valid()) done[li].get();
    } catch (...) {
        for (int li = 0; li < 2; li++)     // never leave a finisher running on our stack frame
            if (done[li].valid()) {
                try {
                    done[li].get();
                } catch (...) {
                }
            }
        throw;
    }
}

std::exception_ptr run_shard_caught(fhe_task_handle_st& h, RunState& rs, const ShardPlan& plan, const std::map<int, Avail>& dev_avail, int si) {
    try {
        run_shard(h, rs, plan, dev_avail, si);
        return nullptr;
    } catch (...) {
        return std::current_exception();
    }
}

// one host thread per shard; the first failure is reported once every shard has stopped
void run_shards(fhe_task_handle_st& h, RunState& rs, const ShardPlan& plan, const std::map<int, Avail>& dev_avail) {
    if (plan.shards.size() == 1) return run_shard(h, rs, plan, dev_avail, 0);
    std::vector<std::exception_ptr> errs(plan.shards.size());
    std::vector<std::thread> workers;
    for (size_t si = 0; si < plan.shards.size(); si++)
        workers.emplace_back([&, si] { errs[si] = run_shard_caught(h, rs, plan, dev_avail, (int)si); });
    for (auto& w : workers) w.join();
    for (auto& e : errs)
        if (e) std::rethrow_exception(e);
}

}  // namespace

void fhe_task_handle_st::run(CArgument* in_args, uint64_t n_in, CArgument* out_args, uint64_t n_out, progress_callback_t cb, void* user,
                             int device) {
    std::lock_guard<std::mutex> run_lock(run_mu);   // one run at a time per handle (the graph state is shared)
    const auto t_start = Clock::now();
    const std::vector<int> devs = run_devices(device);
    if (!sw::no_pipeline() && planned_shards_ != (int)devs.size()) plan((int)devs.size());   // chunk count follows the shard count
    const bool pipelined = !pipeline.chunk_levels.empty();
    // shards: one device + two lanes each; chunks of independent subgraphs are dealt out to them (shard_plan.h)
    const ShardPlan shards = plan_shards(pipelined ? devs : std::vector<int>{devs[0]}, (int)pipeline.chunk_levels.size());
    for (const ShardPlan::Shard& sh : shards.shards)   // every lane exists before any worker thread looks it up
        for (int l = 0; l < (pipelined ? 2 : 1); l++) lane(sh.device, sh.lane0 + l);
    Lane& up = lane(shards.upload_device(), 0);
    RunState rs(cb, user, (int)g.computes.size());
    bind_handles(g, in_args, n_in, out_args, n_out, rs);
    rs.native_out = native_frontend ? &rs.out_handles : nullptr;
    last_direct_loads = 0;
    last_direct_stores = 0;
    dispatch.gpu_nodes = 0;
    dispatch.gpu_batches = 0;
    last_shards = 1;
    last_chunks = (int)pipeline.chunk_levels.size();
    last_key_peer_copies = 0;
    keys.uploads = keys.hits = 0;

    if (!pipelined) {
        for (auto& level : levels) run_level_sync(*this, rs, up, level);
    } else {
        // shared evaluation keys first: exported, uploaded and converted ONCE, on the first device of the list
        for (auto& level : pipeline.shared_levels) run_level_sync(*this, rs, up, level);
        LSA_HIP(hipStreamSynchronize(up.s));
        last_shards = (int)shards.shards.size();
        const std::map<int, Avail> dev_avail = fan_out_keys_to_devices(*this, rs, shards, up);
        run_shards(*this, rs, shards, dev_avail);
        up.c.use_device();
    }
    LSA_HIP(hipStreamSynchronize(up.s));
    last_ms = ms_since(t_start);
}

extern "C" {

fhe_task_handle create_fhe_gpu_task(const char* project_path) {
    fhe_task_handle h = nullptr;
    task_guard([&] {
        LSA_REQUIRE(project_path != nullptr, "null project path");
        h = new fhe_task_handle_st(project_path);
    });
    return h;
}

void release_fhe_gpu_task(fhe_task_handle handle) {
    task_guard([&] { delete handle; });
}

void bind_gpu_task_abi_bridge_executors(fhe_task_handle handle, void* abi_export_executor, void* abi_import_executor) {
    task_guard([&] {
        LSA_REQUIRE(handle && abi_export_executor && abi_import_executor, "null argument");
        // copied by value, the caller may free its std::function objects afterwards (gpu_wrapper.cu:492-497)
        handle->g.bind_bridge_executors(*reinterpret_cast<ExecutorFunc*>(abi_export_executor),
                                        *reinterpret_cast<ExecutorFunc*>(abi_import_executor));
        handle->native_frontend = false;   // output handles are the caller's own objects: never interpreted here
    });
}

void bind_gpu_task_custom_executors(fhe_task_handle handle, const char** custom_types, void** executors, uint64_t n_executors) {
    task_guard([&] {
        LSA_REQUIRE(handle != nullptr, "null task");
        std::unordered_map<std::string, ExecutorFunc> m;
        for (uint64_t i = 0; i < n_executors; i++) m[custom_types[i]] = *reinterpret_cast<ExecutorFunc*>(executors[i]);
        handle->g.bind_custom_executors(m);
    });
}

int run_fhe_gpu_task(fhe_task_handle handle, CArgument* input_args, uint64_t n_in_args, CArgument* output_args,
                     uint64_t n_out_args, progress_callback_t progress_cb, void* user_data, int gpu_device) {
    return task_guard([&] {
        LSA_REQUIRE(handle != nullptr, "null task");
        handle->run(input_args, n_in_args, output_args, n_out_args, progress_cb, user_data, gpu_device);
    });
}

int lsa_frontend_bind(fhe_task_handle handle) {
    return task_guard([&] {
        LSA_REQUIRE(handle != nullptr, "null task");
        handle->g.bind_bridge_executors(frontend_export(), frontend_import());
        handle->native_frontend = true;
    });
}

int lsa_task_set_devices(fhe_task_handle handle, const int* device_ids, int n_devices) {
    return task_guard([&] {
        LSA_REQUIRE(handle != nullptr && n_devices >= 0 && (n_devices == 0 || device_ids != nullptr), "bad device list");
        std::lock_guard<std::mutex> lk(handle->run_mu);
        std::vector<int> ids(device_ids, device_ids + n_devices);
        try {
            if (!ids.empty()) (void)plan_shards(ids, 0);   // validates the list
        } catch (const std::invalid_argument& e) {
            throw Error(LSA_ERR_ARG, e.what());
        }
        handle->devices_ = ids;
    });
}

int lsa_task_last_run_direct(fhe_task_handle handle, int* loads, int* stores) {
    return task_guard([&] {
        LSA_REQUIRE(handle != nullptr, "null task");
        if (loads) *loads = handle->last_direct_loads;
        if (stores) *stores = handle->last_direct_stores;
    });
}

int lsa_task_drop_keys(fhe_task_handle handle) {
    return task_guard([&] {
        LSA_REQUIRE(handle != nullptr, "null task");
        std::lock_guard<std::mutex> lk(handle->run_mu);
        handle->keys.drop();
    });
}

int lsa_task_last_run_keys(fhe_task_handle handle, int* uploaded, int* reused) {
    return task_guard([&] {
        LSA_REQUIRE(handle != nullptr, "null task");
        if (uploaded) *uploaded = handle->keys.uploads;
        if (reused) *reused = handle->keys.hits;
    });
}

int lsa_task_last_run_shards(fhe_task_handle handle, int* n_shards, int* n_chunks, int* key_peer_copies) {
    return task_guard([&] {
        LSA_REQUIRE(handle != nullptr, "null task");
        if (n_shards) *n_shards = handle->last_shards;
        if (n_chunks) *n_chunks = handle->last_chunks;
        if (key_peer_copies) *key_peer_copies = handle->last_key_peer_copies;
    });
}

int lsa_task_trim_pools(fhe_task_handle handle) {
    return task_guard([&] {
        LSA_REQUIRE(handle != nullptr, "null task");
        std::lock_guard<std::mutex> lk(handle->run_mu);
        for (auto& kv : handle->lanes) kv.second->pending.clear();
        handle->pools.trim_all();
    });
}

int lsa_task_counts(fhe_task_handle handle, int* n_data, int* n_compute, int* n_inputs, int* n_outputs) {
    return task_guard([&] {
        LSA_REQUIRE(handle != nullptr, "null task");
        if (n_data) *n_data = (int)handle->g.data.size();
        if (n_compute) *n_compute = (int)handle->g.computes.size();
        if (n_inputs) *n_inputs = (int)handle->g.inputs.size();
        if (n_outputs) *n_outputs = (int)handle->g.outputs.size();
    });
}

int lsa_task_last_run_stats(fhe_task_handle handle, int* gpu_nodes, int* gpu_batches, double* run_ms) {
    return task_guard([&] {
        LSA_REQUIRE(handle != nullptr, "null task");
        if (gpu_nodes) *gpu_nodes = handle->dispatch.gpu_nodes;
        if (gpu_batches) *gpu_batches = handle->dispatch.gpu_batches;
        if (run_ms) *run_ms = handle->last_ms;
    });
}

}  // extern "C"
