// task_internal.h — what the units of the task layer share: device data, the execution lane, the key cache and the entry points
// of each unit.
//   task_runtime.hip    the task handle, run(): plan, bind handles, shared levels, key fan-out, shards
//   task_transfer.hip   LOAD_TO_BACKEND / STORE_FROM_BACKEND (batched H2D / D2H), the evaluation-key cache
//   task_dispatch.hip   bind_gpu_executor, buckets of a level -> batched launches of the operator layer, bootstrap plans
//   task_frontend.hip   C-struct helpers, the native front-end's export / import executors, caller-pinned host memory
//   task_pipeline.h     which subgraphs can run as independent chunks (plain C++, host test)
// Nothing here is part of the library's interface: the namespace is hidden from the dynamic symbol table.
#pragma once
#include <any>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "buf_pool.h"
#include "lsa_internal.h"
#include "task_pipeline.h"

// The operator surface of mega_ag_runners/mega_ag_executors.h:53-54 (task_dispatch.hip)
void bind_gpu_executor(ComputeNode& node, Algo algorithm);

namespace lsa {
namespace task __attribute__((visibility("hidden"))) {

// ------------------------------------------------------------------------------------------------ caller-pinned host memory
// Zero-copy ingestion: a caller that keeps its limb buffers in memory it has registered with lsa_host_register
// (pinned in place, hipHostRegister) gets its ciphertexts DMA'd straight from / into those buffers -- no gather into a staging
// slab on the way in, no copy out of one on the way back.  The caller owns the lifetime: the range must stay allocated until
// lsa_host_unregister.  Unregistered buffers take the pinned-staging path as before.
struct HostRegistry {
    std::mutex mu;
    std::map<uintptr_t, size_t> ranges;   // base -> bytes
    bool covers(const void* p, size_t bytes) {
        std::lock_guard<std::mutex> lk(mu);
        if (ranges.empty()) return false;
        const uintptr_t a = (uintptr_t)p;
        auto it = ranges.upper_bound(a);
        if (it == ranges.begin()) return false;
        --it;
        return a >= it->first && a + bytes <= it->first + it->second;
    }
};
HostRegistry& host_registry();   // task_frontend.hip

// ------------------------------------------------------------------------------------------------ device data
// Buffers (device or pinned host) recycled across levels and run() calls: hipMalloc/hipFree and pinned allocation cost
// milliseconds and synchronise the device, so a task keeps what it allocated (buf_pool.h: best fit, a cap on what stays
// pooled).  Every device pool belongs to ONE (device, lane) = one in-order stream, so handing a released device buffer to a
// later kernel is ordered after its earlier readers, and a run on another device never sees this device's allocations.
void* hip_buf_alloc(size_t bytes, int device, bool pinned);   // task_transfer.hip
void hip_buf_release(void* p, int device, bool pinned);

struct Slab {
    u64* ptr = nullptr;
    size_t words = 0;       // requested
    size_t cap_words = 0;   // what the pool handed out (>= words)
    BufPool* pool;
    Slab(BufPool& p, size_t w) : words(w), pool(&p) { ptr = p.take(w, &cap_words); }
    ~Slab() { pool->give(cap_words, ptr); }
    Slab(const Slab&) = delete;
    Slab& operator=(const Slab&) = delete;
};

struct DevDatum {  // a ciphertext or plaintext living in (a slice of) a slab: [polys][level+1][N]
    std::shared_ptr<Slab> slab;
    u64* ptr = nullptr;
    int polys = 0, level = 0;
    bool is_plain = false;
    size_t words(long long N) const { return (size_t)polys * (level + 1) * N; }
};
struct DevKey {
    std::shared_ptr<Slab> slab;
    Key key;
};
using DatumP = std::shared_ptr<DevDatum>;
using KeyP = std::shared_ptr<DevKey>;
using Avail = std::unordered_map<NodeIndex, std::any>;   // datum -> handle, C struct, DatumP or KeyP, as the run proceeds
using Refs = std::unordered_map<NodeIndex, int>;         // datum -> consumers not yet enqueued
using OutHandles = std::unordered_map<NodeIndex, void*>;

inline bool is_plain_node(const DatumNode* d) { return d->datum_type == TYPE_PLAINTEXT; }
inline bool is_ringt_node(const DatumNode* d) { return d->fhe_prop && d->fhe_prop->p && d->fhe_prop->p->is_ringt; }
// pt_mul: the message lifted to Q, NTT domain, Montgomery form (frontend BfvPlaintextMulNode / CkksPlaintextMulNode)
inline bool is_ptmul_node(const DatumNode* d) {
    return is_plain_node(d) && d->fhe_prop && d->fhe_prop->is_ntt && d->fhe_prop->is_mform && !is_ringt_node(d);
}

// every failure becomes a non-zero return code + lsa_last_error(); nothing throws across extern "C"
template <typename F> int task_guard(F&& f) {
    try {
        f();
        return 0;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code ? e.code : LSA_ERR_INTERNAL;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return LSA_ERR_INTERNAL;
    } catch (...) {
        set_last_error("unknown error");
        return LSA_ERR_INTERNAL;
    }
}

// `m` items of one shape, back to back in `slab`, become the outputs of node_at(0) .. node_at(m-1)
template <class NodeAt>
void publish(Avail& avail, const std::shared_ptr<Slab>& slab, size_t m, const DevDatum& shape, long long N, NodeAt node_at) {
    for (size_t i = 0; i < m; i++) {
        auto d = std::make_shared<DevDatum>(shape);
        d->slab = slab;
        d->ptr = slab->ptr + shape.words(N) * i;
        avail[node_at(i)->output_nodes[0]->index] = d;
    }
}

// One execution lane: an in-order stream, the context whose workspace its kernels use, the device pool only this stream's
// work draws from, the device's pinned pool, and the temporaries that enqueued work still reads.  A run whose graph splits
// into independent subgraphs is pipelined over a shard's two lanes: while lane A's chunk computes and copies its results
// back, lane B's chunk is staged and copied in (PCIe is full duplex; the reference's runner overlaps nothing across its 2
// streams' copies).  A released device buffer only returns to ITS lane's pool, so reuse stays ordered by the lane's stream.
// One host thread enqueues on a lane at a time; the thread that waited for the stream is the one that clears `pending`.
struct Lane {
    const int device, lane;
    const std::unique_ptr<Context> ctx;
    Context& c;
    hipStream_t s = nullptr;
    BufPool &dev, &pin;
    std::vector<std::shared_ptr<Slab>> pending;   // freed after their readers ran: cleared once the stream has been waited for
    Lane(int device, int lane, std::unique_ptr<Context> context, LanePools& pools)
        : device(device), lane(lane), ctx(std::move(context)), c(*ctx), dev(pools.device_pool(device, lane)), pin(pools.pinned_pool(device)) {
        LSA_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
    ~Lane() {
        (void)hipSetDevice(device);
        (void)hipStreamDestroy(s);
    }
    std::shared_ptr<Slab> dslab(size_t words) { return std::make_shared<Slab>(dev, words); }
    std::shared_ptr<Slab> pslab(size_t words) { return std::make_shared<Slab>(pin, words); }
    void defer(std::shared_ptr<Slab> slab) { pending.push_back(std::move(slab)); }
    u64* temp(size_t words) {   // a device temporary that lives until `pending` is cleared
        defer(dslab(words));
        return pending.back()->ptr;
    }
};

// host threads for memcpy-bound or executor-bound work next to the thread that enqueues: the machine's share is 16 CPUs
inline int host_threads() {
    const int hw = (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(16, hw > 0 ? hw : 1) - 2);
}

// ------------------------------------------------------------------------------------------------ task_transfer.hip
// Evaluation keys stay on the device across run() calls (SURVEY f3 "persistent state"; the reference re-exports and
// re-uploads them every run, cxx_sdk_v2/cxx_argument.h:178-260): per (device, key datum) the converted key is kept together
// with the caller's handle and a fingerprint of the exported C struct (shape + three words of every limb).  A run whose
// export yields the same handle and fingerprint skips staging, upload and conversion; anything else (another key object, a
// regenerated key) replaces the entry.  CONTRACT: a caller that rewrites a key IN PLACE so that the sampled words stay the
// same must call lsa_task_drop_keys.  drop() / the task's release free the device copies.
// Touched by the thread that runs the shared levels / the fan-out only.
class KeyCache {
  public:
    int uploads = 0, hits = 0;   // of the last run
    static uint64_t fingerprint(const CKeySwitchKey* k, int n);
    // the resident key of (device, datum), if it was converted from this handle and fingerprint at this level
    KeyP find(int device, NodeIndex datum, const void* handle, uint64_t fingerprint, int level);
    void put(int device, NodeIndex datum, const void* handle, uint64_t fingerprint, const KeyP& key);   // a key uploaded by this run
    // A peer copy made by an earlier run is still valid while the upload device's entry it was made from is (same handle and
    // fingerprint).  peer(): device `dev`'s copy of `src`, if `src` is `up_dev`'s resident key of the datum and the copy was made
    // from it; put_peer(): records a fresh copy under the same condition.
    KeyP peer(int up_dev, int dev, NodeIndex datum, const KeyP& src) const;
    void put_peer(int up_dev, int dev, NodeIndex datum, const KeyP& src, const KeyP& copy);
    void drop() { map_.clear(); }   // the device copies return to their pools

  private:
    struct CachedKey {
        const void* handle = nullptr;
        uint64_t fingerprint = 0;
        KeyP key;
    };
    const bool keep_ = !sw::no_key_cache();
    std::map<std::pair<int, NodeIndex>, CachedKey> map_;
};

struct StoreJob {
    std::vector<ComputeNode*> nodes;
    std::vector<std::pair<DatumP, size_t>> items;   // offset into the pinned slab (staged results)
    std::vector<u64*> direct;                       // non-null: the result was copied straight into the caller's buffer
    std::shared_ptr<Slab> hslab;
};

// LOAD_TO_BACKEND nodes of one level; returns the pinned staging slab, which must outlive the enqueued copies (the caller
// synchronises or keeps it)
std::shared_ptr<Slab> run_loads(Lane& ln, const std::vector<ComputeNode*>& nodes, Avail& avail, KeyCache& keys, std::atomic<int>& direct_loads);
// STORE_FROM_BACKEND nodes of one level: enqueue the copies; once the stream has been synchronised, wrap the results into C
// structs for the import executor.  `native_out`: the run's output handles where they are the native front-end's
// (lsa_host_ciphertext: a result may then go straight into a registered buffer), else null.
StoreJob stores_enqueue(Lane& ln, const std::vector<ComputeNode*>& nodes, Avail& avail, const OutHandles* native_out, std::atomic<int>& direct_stores);
void stores_finish(Lane& ln, StoreJob& job, Avail& avail);

// ------------------------------------------------------------------------------------------------ task_dispatch.hip
struct Split {   // the nodes of one level by what runs them
    std::vector<ComputeNode*> cpu, loads, stores;
    std::map<std::string, std::vector<ComputeNode*>> buckets;   // signature -> backend nodes launched as one batch
    std::vector<std::string> bucket_order;
};

struct BootstrapDeleter {
    void operator()(Bootstrap* b) const { bootstrap_destroy(b); }
};

// Batched operator dispatch of one task: backend nodes of a level that perform the same operator on the same shapes run as
// one launch sequence of the operator layer.
class Dispatcher {
  public:
    explicit Dispatcher(const TaskGraph& g) : g(g) {}
    std::atomic<int> gpu_nodes{0}, gpu_batches{0};   // of the last run
    Split split(const std::vector<ComputeNode*>& level) const;
    void run_buckets(Lane& ln, Split& sp, Avail& avail);

  private:
    struct Operand {
        const u64* ptr;
        long long stride;
        std::shared_ptr<Slab> keep;
    };
    std::string signature(const ComputeNode* n) const;
    Operand gather(Lane& ln, const std::vector<ComputeNode*>& nodes, int pos, Avail& avail, size_t words);
    void run_gpu_bucket(Lane& ln, const std::vector<ComputeNode*>& nodes, Avail& avail);
    Bootstrap& bootstrap_plan(Lane& ln);
    const TaskGraph& g;
    std::mutex bootstrap_mu;
    std::map<Context*, std::unique_ptr<Bootstrap, BootstrapDeleter>> bootstrap_plans;   // built on first use, per lane context
};

// ------------------------------------------------------------------------------------------------ task_frontend.hip
ExecutorFunc frontend_export();
ExecutorFunc frontend_import();

}  // namespace task
}  // namespace lsa
