// task_transfer.hip — LOAD_TO_BACKEND / STORE_FROM_BACKEND of the task runner (the reference's gpu_abi_bridge_executors.h) and the
// evaluation-key cache.  H2D / D2H go through one pinned staging slab per level and ONE hipMemcpyAsync per group (the reference
// issues one pageable copy per limb, gpu_abi_bridge_executors.h:60-191); buffers the caller registered are copied in place.
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <tuple>

#include "task_internal.h"

using namespace lsa;
using namespace lsa::task;

namespace {

// Limb copy into the pinned staging slab with non-temporal stores: the destination is written once and read by the DMA
// engine, so the read-for-ownership traffic of an ordinary memcpy (a third of the gather's memory traffic) is wasted.
#if !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2"))) static void stream_copy_avx2(u64* dst, const u64* src, size_t words) {
    typedef long long v4 __attribute__((vector_size(32)));
    size_t i = 0;
    for (; i + 4 <= words; i += 4) {
        v4 v;
        __builtin_memcpy(&v, src + i, 32);
        __builtin_nontemporal_store(v, reinterpret_cast<v4*>(dst + i));
    }
    for (; i < words; i++) dst[i] = src[i];
}
static void stream_copy(u64* dst, const u64* src, size_t words) {
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2 && (reinterpret_cast<uintptr_t>(dst) & 31) == 0) stream_copy_avx2(dst, src, words);
    else memcpy(dst, src, words * sizeof(u64));
}
#else
static void stream_copy(u64* dst, const u64* src, size_t words) { memcpy(dst, src, words * sizeof(u64)); }
#endif

// Parallel loop on a few PERSISTENT host threads (memcpy-bound staging work; the staging loop calls this once per 32 MiB of
// input).  One loop at a time (callers on different shard threads queue on `run_mu_`).  LSA_STAGE_THREADS overrides the count.
// Measured (profiles/r03/t2_staging_and_lane_handback.log): the copies themselves bound the CKKS x64 graph -- 208 MiB per chunk
// staged at ~55 GB/s read + 55 GB/s written on the box's 16-core share while the DMA engine reads the previous 32 MiB --, not the
// thread start-up (this pool against a spawn per call: no change) and not the lane turnaround (handing a lane back before its
// chunk's import: no change either).
class StagePool {
  public:
    static StagePool& get() {
        static StagePool p;
        return p;
    }
    template <typename F> void run(size_t n, F&& fn) {
        if (n == 0) return;
        if (workers_.empty() || n == 1) {
            for (size_t i = 0; i < n; i++) fn(i);
            return;
        }
        std::lock_guard<std::mutex> one(run_mu_);
        std::function<void(size_t)> f = std::ref(fn);
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &f;
            n_ = n;
            next_.store(0);
            active_ = (int)workers_.size();
            gen_++;
        }
        cv_.notify_all();
        work(f, n);
        std::unique_lock<std::mutex> lk(mu_);
        cv_done_.wait(lk, [&] { return active_ == 0; });   // every worker has seen this generation and left work()
        fn_ = nullptr;
    }
    ~StagePool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }

  private:
    StagePool() {
        const int nthreads = std::min(sw::stage_threads(host_threads()), 32);
        for (int t = 1; t < nthreads; t++) workers_.emplace_back([this] { loop(); });
    }
    void work(const std::function<void(size_t)>& f, size_t n) {
        for (;;) {
            const size_t i = next_.fetch_add(1);
            if (i >= n) return;
            f(i);
        }
    }
    void loop() {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void(size_t)>* f;
            size_t n;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                f = fn_;
                n = n_;
            }
            work(*f, n);
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (--active_ == 0) cv_done_.notify_all();
            }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex mu_, run_mu_;
    std::condition_variable cv_, cv_done_;
    const std::function<void(size_t)>* fn_ = nullptr;
    size_t n_ = 0;
    std::atomic<size_t> next_{0};
    int active_ = 0;
    unsigned long long gen_ = 0;
    bool stop_ = false;
};
template <typename F> void parallel_for(size_t n, F&& fn) { StagePool::get().run(n, fn); }

// a load or store node's C struct disagrees with the task: name the caller's datum, i.e. what the export node in front of
// the load was given
const DatumNode* callers_datum(const DatumNode* in) {
    if (!in->predecessors.empty() && in->predecessors[0]->op() == OperationType::EXPORT_TO_ABI && !in->predecessors[0]->input_nodes.empty())
        return in->predecessors[0]->input_nodes[0];
    return in;
}

struct Item {   // a ciphertext or plaintext to load
    ComputeNode* node;
    std::shared_ptr<CCiphertext> ct;
    std::shared_ptr<CPlaintext> pt;
    int polys, level;
    size_t off;
    size_t words(long long N) const { return (size_t)polys * (level + 1) * N; }
};
struct KeyItem {   // a key to load, compact order [beta][2][comp][N]
    ComputeNode* node;
    const CKeySwitchKey* ksk;
    std::any keep;
    int level, beta, comp;
    size_t off;
    const void* handle;
    uint64_t fingerprint;
};
using GroupKey = std::tuple<int, int, int>;   // (plain, polys, level)
using Groups = std::map<GroupKey, std::vector<Item>>;

// the C struct of every ciphertext / plaintext load checked against the task's declaration and grouped by shape, in node
// order; loads of keys are returned in `key_nodes`.  Every operand is sized from the graph's fhe_prop downstream (gather /
// run_gpu_bucket): a C struct that disagrees with the declaration would make those kernels read past the loaded slab.
Groups group_loads(const Context& c, const std::vector<ComputeNode*>& nodes, const Avail& avail, std::vector<ComputeNode*>& key_nodes) {
    Groups groups;
    for (ComputeNode* node : nodes) {
        const DatumNode* in = node->input_nodes[0];
        const std::any& cs = avail.at(in->index);
        auto bad = [&](const std::string& what) {
            const DatumNode* orig = callers_datum(in);
            throw Error(LSA_ERR_ARG, "input '" + orig->id + "' (datum " + std::to_string(orig->index) + "): " + what);
        };
        if (in->datum_type == TYPE_CIPHERTEXT) {
            auto ct = std::any_cast<std::shared_ptr<CCiphertext>>(cs);
            if (!ct || !ct->polys) bad("null ciphertext C struct");
            if (in->fhe_prop && (ct->level != in->fhe_prop->level || ct->degree != in->fhe_prop->degree))
                bad("ciphertext C struct has level/degree " + std::to_string(ct->level) + "/" + std::to_string(ct->degree) +
                    ", the task declares " + std::to_string(in->fhe_prop->level) + "/" + std::to_string(in->fhe_prop->degree));
            if (ct->level < 0 || ct->level >= c.nq || ct->degree < 0) bad("ciphertext level/degree out of range");
            for (int p = 0; p <= ct->degree; p++) {
                if (!ct->polys[p].components || ct->polys[p].n_component != ct->level + 1) bad("ciphertext C struct: limb count != level+1");
                for (int j = 0; j <= ct->level; j++)
                    if (ct->polys[p].components[j].n != c.n || !ct->polys[p].components[j].data) bad("ciphertext C struct has a wrong ring degree");
            }
            groups[{0, ct->degree + 1, ct->level}].push_back({node, ct, nullptr, ct->degree + 1, ct->level, 0});
        } else if (in->datum_type == TYPE_PLAINTEXT) {
            auto pt = std::any_cast<std::shared_ptr<CPlaintext>>(cs);
            if (!pt || !pt->poly.components) bad("null plaintext C struct");
            const bool ringt = is_ringt_node(in);
            const int want = ringt ? 1 : (in->fhe_prop ? in->fhe_prop->level + 1 : pt->poly.n_component);
            if (pt->poly.n_component != want)
                bad("plaintext C struct has " + std::to_string(pt->poly.n_component) + " limbs, the task declares " + std::to_string(want));
            if (want < 1 || want > c.nq) bad("plaintext level out of range");
            for (int j = 0; j < want; j++)
                if (pt->poly.components[j].n != c.n || !pt->poly.components[j].data) bad("plaintext C struct has a wrong ring degree");
            groups[{1, 1, pt->poly.n_component - 1}].push_back({node, nullptr, pt, 1, pt->poly.n_component - 1, 0});
        } else {
            key_nodes.push_back(node);
        }
    }
    return groups;
}

// the key-switch key behind a key load, checked against the context's shape, with the caller's handle and the fingerprint
// the key cache goes by
KeyItem describe_key(const Context& c, ComputeNode* node, const Avail& avail) {
    const DatumNode* in = node->input_nodes[0];
    const std::any& cs = avail.at(in->index);
    KeyItem k{};
    k.node = node;
    k.keep = cs;
    if (in->datum_type == TYPE_RELIN_KEY) {
        k.ksk = std::any_cast<std::shared_ptr<CRelinKey>>(cs).get();
    } else if (in->datum_type == TYPE_SWITCH_KEY) {
        k.ksk = std::any_cast<std::shared_ptr<CKeySwitchKey>>(cs).get();
    } else {
        auto glk = std::any_cast<std::shared_ptr<CGaloisKey>>(cs);
        const uint32_t want = in->fhe_prop->p ? in->fhe_prop->p->galois_element : 0;
        k.ksk = nullptr;
        for (int i = 0; i < glk->n_key_switch_key; i++)
            if (glk->galois_elements[i] == want) k.ksk = &glk->key_switch_keys[i];
        LSA_REQUIRE(k.ksk != nullptr, "Galois key for element " + std::to_string(want) + " not found in the C struct");
    }
    LSA_REQUIRE(k.ksk && k.ksk->n_public_key >= 1, "empty key-switch key");
    k.level = k.ksk->public_keys[0].level;
    k.beta = k.ksk->n_public_key;
    k.comp = k.ksk->public_keys[0].polys[0].n_component;
    LSA_REQUIRE(k.comp == k.level + 1 + c.np, "key-switch key: limbs per polynomial != level+1+#special primes");
    LSA_REQUIRE(k.beta == (k.level + 1 + c.np - 1) / c.np, "key-switch key: digit count != ceil((level+1)/k)");
    LSA_REQUIRE(k.level >= 0 && k.level < c.nq, "key-switch key: level out of range");
    for (int d = 0; d < k.beta; d++) {
        const CPublicKey& pk = k.ksk->public_keys[d];
        LSA_REQUIRE(pk.polys && pk.degree == 1 && pk.level == k.level, "key-switch key: digits differ in level or degree");
        for (int h = 0; h < 2; h++) {
            LSA_REQUIRE(pk.polys[h].components && pk.polys[h].n_component == k.comp, "key-switch key: limb count differs between digits");
            for (int j = 0; j < k.comp; j++)
                LSA_REQUIRE(pk.polys[h].components[j].n == c.n && pk.polys[h].components[j].data, "key-switch key has a wrong ring degree");
        }
    }
    // the caller's handle behind the export node
    const DatumNode* orig = (!in->predecessors.empty() && !in->predecessors[0]->input_nodes.empty()) ? in->predecessors[0]->input_nodes[0] : in;
    const std::any* hv = avail.count(orig->index) ? &avail.at(orig->index) : nullptr;
    const std::shared_ptr<void>* hp = hv ? std::any_cast<std::shared_ptr<void>>(hv) : nullptr;
    k.handle = hp ? hp->get() : nullptr;
    k.fingerprint = KeyCache::fingerprint(k.ksk, c.n);
    return k;
}

// the item's host address if it is one contiguous block of caller-registered (pinned) memory, else null
const u64* registered_base(const Item& it, long long N) {
    const u64* base = (it.ct ? it.ct->polys[0] : it.pt->poly).components[0].data;
    const u64* want = base;
    for (int p = 0; p < it.polys; p++) {
        const CPolynomial& poly = it.ct ? it.ct->polys[p] : it.pt->poly;
        for (int j = 0; j <= it.level; j++, want += N)
            if (poly.components[j].data != want) return nullptr;
    }
    return host_registry().covers(base, it.words(N) * sizeof(u64)) ? base : nullptr;
}

// where a store node's result can be written directly: the native front-end's pre-allocated output ciphertext behind the
// import node that follows, if the caller registered (pinned) its buffer and it has the result's shape
u64* direct_store_target(const OutHandles* native_out, const ComputeNode* store, const DevDatum& d, int n) {
    if (!native_out) return nullptr;
    const DatumNode* cs = store->output_nodes[0];
    if (cs->successors.size() != 1 || cs->successors[0]->op() != OperationType::IMPORT_FROM_ABI) return nullptr;
    auto it = native_out->find(cs->successors[0]->output_nodes[0]->index);
    if (it == native_out->end() || !it->second) return nullptr;
    const auto* h = (const lsa_host_ciphertext*)it->second;
    if (!h->data || h->n != n || h->level != d.level || h->degree != d.polys - 1) return nullptr;
    return host_registry().covers(h->data, d.words(n) * sizeof(u64)) ? h->data : nullptr;
}

}  // namespace

namespace lsa {
namespace task {

void* hip_buf_alloc(size_t bytes, int device, bool pinned) {
    LSA_HIP(hipSetDevice(device));
    void* p = nullptr;
    if (pinned) LSA_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    else LSA_HIP(hipMalloc(&p, bytes));
    return p;
}
void hip_buf_release(void* p, int device, bool pinned) {
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (cur != device) (void)hipSetDevice(device);
    if (pinned) (void)hipHostFree(p);
    else (void)hipFree(p);
    if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
}

// ------------------------------------------------------------------------------------------------ evaluation-key cache
uint64_t KeyCache::fingerprint(const CKeySwitchKey* k, int n) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)k->n_public_key;
    auto mix = [&](uint64_t v) { h = (h ^ v) * 0x100000001B3ull + (h >> 29); };
    for (int d = 0; d < k->n_public_key; d++) {
        const CPublicKey& pk = k->public_keys[d];
        mix((uint64_t)pk.level * 131 + (uint64_t)pk.degree);
        for (int p = 0; p <= pk.degree; p++)
            for (int j = 0; j < pk.polys[p].n_component; j++) {
                const uint64_t* w = pk.polys[p].components[j].data;
                mix(w[0]);
                mix(w[n / 2]);
                mix(w[n - 1]);
            }
    }
    return h;
}
KeyP KeyCache::find(int device, NodeIndex datum, const void* handle, uint64_t fingerprint, int level) {
    auto hit = keep_ ? map_.find({device, datum}) : map_.end();
    if (hit == map_.end() || hit->second.handle != handle || hit->second.fingerprint != fingerprint || hit->second.key->key.level != level)
        return nullptr;
    hits++;
    return hit->second.key;
}
void KeyCache::put(int device, NodeIndex datum, const void* handle, uint64_t fingerprint, const KeyP& key) {
    uploads++;
    if (keep_) map_[{device, datum}] = CachedKey{handle, fingerprint, key};
}
KeyP KeyCache::peer(int up_dev, int dev, NodeIndex datum, const KeyP& src) const {
    auto up = map_.find({up_dev, datum}), pe = map_.find({dev, datum});
    const bool valid = keep_ && up != map_.end() && pe != map_.end() && up->second.key == src && pe->second.handle == up->second.handle &&
                       pe->second.fingerprint == up->second.fingerprint;
    return valid ? pe->second.key : nullptr;
}
void KeyCache::put_peer(int up_dev, int dev, NodeIndex datum, const KeyP& src, const KeyP& copy) {
    auto up = map_.find({up_dev, datum});
    if (keep_ && up != map_.end() && up->second.key == src) map_[{dev, datum}] = CachedKey{up->second.handle, up->second.fingerprint, copy};
}

// ------------------------------------------------------------------------------------------------ LOAD_TO_BACKEND (batched H2D)
std::shared_ptr<Slab> run_loads(Lane& ln, const std::vector<ComputeNode*>& nodes, Avail& avail, KeyCache& cache, std::atomic<int>& direct_loads) {
    Context& c = ln.c;
    const long long N = c.n;
    // 1. ciphertexts / plaintexts grouped into one slab per (kind, polys, level) in node order
    std::vector<ComputeNode*> key_nodes;
    Groups groups = group_loads(c, nodes, avail, key_nodes);
    // a group whose every item is one contiguous block of caller-registered (pinned) memory is copied from where it lies
    std::map<GroupKey, std::vector<const u64*>> direct;   // group -> per-item host base (all or nothing)
    for (auto& kv : groups) {
        std::vector<const u64*> bases;
        for (auto& it : kv.second) {
            const u64* b = registered_base(it, N);
            if (!b) break;
            bases.push_back(b);
        }
        if (bases.size() == kv.second.size()) direct[kv.first] = std::move(bases);
    }
    size_t total = 0;
    for (auto& kv : groups) {
        if (direct.count(kv.first)) continue;
        for (auto& it : kv.second) {
            it.off = total;
            total += it.words(N);
        }
    }
    std::vector<KeyItem> keys;
    for (ComputeNode* node : key_nodes) {
        KeyItem k = describe_key(c, node, avail);
        // resident already?  (same caller handle behind the export node, same fingerprint of what it exported)
        if (KeyP hit = cache.find(c.device, node->output_nodes[0]->index, k.handle, k.fingerprint, k.level)) {
            avail[node->output_nodes[0]->index] = hit;
            continue;
        }
        k.off = total;
        total += key_layout(c, k.level).words;
        keys.push_back(std::move(k));
    }
    // a group's device slab; its items become the outputs of their load nodes
    auto group_slab = [&](const GroupKey& gk, const std::vector<Item>& items) {
        auto slab = ln.dslab(items[0].words(N) * items.size());
        const DevDatum shape{nullptr, nullptr, items[0].polys, items[0].level, std::get<0>(gk) == 1};
        publish(avail, slab, items.size(), shape, N, [&](size_t i) { return items[i].node; });
        return slab;
    };
    // 1b. direct groups: device slab + one copy per item straight from the caller's pinned buffer
    for (auto& kv : direct) {
        auto& items = groups.at(kv.first);
        const size_t per = items[0].words(N);
        auto slab = group_slab(kv.first, items);
        for (size_t i = 0; i < items.size(); i++)
            LSA_HIP(hipMemcpyAsync(slab->ptr + per * i, kv.second[i], per * sizeof(u64), hipMemcpyHostToDevice, ln.s));
        direct_loads += (int)items.size();
    }
    if (total == 0) return nullptr;
    // 2. gather limbs into a pinned staging slab, one H2D copy per group
    auto hstage = ln.pslab(total);
    u64* host = hstage->ptr;
    struct Job {
        u64* dst;
        const u64* src;
    };
    std::vector<Job> jobs;   // one limb each, gathered by a few threads (single-threaded this was ~55 % of LOAD)
    for (auto& kv : groups) {
        if (direct.count(kv.first)) continue;
        for (auto& it : kv.second) {
            u64* dst = host + it.off;
            for (int p = 0; p < it.polys; p++) {
                const CPolynomial& poly = it.ct ? it.ct->polys[p] : it.pt->poly;
                for (int j = 0; j <= it.level; j++) {
                    jobs.push_back({dst, poly.components[j].data});
                    dst += N;
                }
            }
        }
    }
    for (auto& k : keys) {
        u64* dst = host + k.off;
        for (int d = 0; d < k.beta; d++)
            for (int h = 0; h < 2; h++)
                for (int j = 0; j < k.comp; j++) {
                    jobs.push_back({dst, k.ksk->public_keys[d].polys[h].components[j].data});
                    dst += N;
                }
    }
    // device destinations first (one slab per group / key), as segments of the staging order
    struct Seg {
        size_t off, words;
        u64* dev;
    };
    std::vector<Seg> segs;
    for (auto& kv : groups) {
        if (direct.count(kv.first)) continue;
        auto slab = group_slab(kv.first, kv.second);
        segs.push_back({kv.second[0].off, slab->words, slab->ptr});
    }
    std::vector<KeyP> dkeys;
    for (auto& k : keys) {
        const KeyLayout kl = key_layout(c, k.level);
        auto dk = std::make_shared<DevKey>();
        dk->slab = ln.dslab(kl.alloc_words());
        segs.push_back({k.off, kl.words, dk->slab->ptr});
        dkeys.push_back(dk);
    }
    // gather and copy in chunks: while the DMA engine moves chunk k, the host threads gather chunk k+1 (the staging
    // slab holds the whole level, so no chunk waits for a buffer)
    const size_t chunk_jobs = std::max<size_t>(1, (32u << 20) / (sizeof(u64) * (size_t)N));
    for (size_t j0 = 0; j0 < jobs.size(); j0 += chunk_jobs) {
        const size_t j1 = std::min(jobs.size(), j0 + chunk_jobs);
        parallel_for(j1 - j0, [&](size_t i) { stream_copy(jobs[j0 + i].dst, jobs[j0 + i].src, (size_t)N); });
        const size_t h0 = j0 * (size_t)N, h1 = j1 * (size_t)N;   // jobs are in staging order, one limb each
        for (const Seg& sg : segs) {
            const size_t a = std::max(h0, sg.off), b = std::min(h1, sg.off + sg.words);
            if (a < b)
                LSA_HIP(hipMemcpyAsync(sg.dev + (a - sg.off), host + a, (b - a) * sizeof(u64), hipMemcpyHostToDevice, ln.s));
        }
    }
    for (size_t i = 0; i < keys.size(); i++) {
        auto& k = keys[i];
        auto& dk = dkeys[i];
        dk->key.owned = false;
        key_prepare(c, dk->key, dk->slab->ptr, k.level, key_layout(c, k.level).fp_of(dk->slab->ptr), ln.s);
        avail[k.node->output_nodes[0]->index] = dk;
        cache.put(c.device, k.node->output_nodes[0]->index, k.handle, k.fingerprint, dk);
    }
    return hstage;
}

// ------------------------------------------------------------------------------------------------ STORE_FROM_BACKEND (batched D2H)
StoreJob stores_enqueue(Lane& ln, const std::vector<ComputeNode*>& nodes, Avail& avail, const OutHandles* native_out, std::atomic<int>& direct_stores) {
    const long long N = ln.c.n;
    size_t total = 0;
    std::vector<std::pair<DatumP, size_t>> items;
    std::vector<u64*> direct;
    for (ComputeNode* node : nodes) {
        const DatumNode* in = node->input_nodes[0];
        LSA_REQUIRE(in->datum_type == TYPE_CIPHERTEXT, "Unsupported data type for D2H transfer");
        auto d = std::any_cast<DatumP>(avail.at(in->index));
        u64* tgt = direct_store_target(native_out, node, *d, ln.c.n);
        direct.push_back(tgt);
        items.push_back({d, total});
        if (!tgt) total += d->words(N);
    }
    // staged results land in ONE pooled pinned slab; the C structs handed to the caller's import executor only index it
    // (no malloc per limb, no second host copy).  The slab returns to the pool when the last struct is released.
    std::shared_ptr<Slab> hslab = total ? ln.pslab(total) : nullptr;
    u64* host = hslab ? hslab->ptr : nullptr;
    // merge runs that are contiguous on the device into single copies.  Only within one slab: two slabs are two allocations
    // even where their addresses happen to follow each other (results of two buckets stored in one level), and one copy must
    // not span them
    for (size_t i = 0; i < items.size();) {
        if (direct[i]) {
            LSA_HIP(hipMemcpyAsync(direct[i], items[i].first->ptr, items[i].first->words(N) * sizeof(u64), hipMemcpyDeviceToHost, ln.s));
            direct_stores++;
            i++;
            continue;
        }
        size_t j = i, words = 0;
        while (j < items.size() && !direct[j] && items[j].first->slab == items[i].first->slab &&
               items[j].first->ptr == items[i].first->ptr + words) {
            words += items[j].first->words(N);
            j++;
        }
        LSA_HIP(hipMemcpyAsync(host + items[i].second, items[i].first->ptr, words * sizeof(u64), hipMemcpyDeviceToHost, ln.s));
        i = j;
    }
    return StoreJob{nodes, std::move(items), std::move(direct), hslab};
}

// after the stream has been synchronised: wrap the pinned result slab into C structs for the import executor
void stores_finish(Lane& ln, StoreJob& job, Avail& avail) {
    const int n = ln.c.n;
    auto hslab = job.hslab;
    u64* host = hslab ? hslab->ptr : nullptr;
    for (size_t i = 0; i < job.nodes.size(); i++) {
        const DatumP& d = job.items[i].first;
        auto* ct = (CCiphertext*)malloc(sizeof(CCiphertext));
        ct->level = d->level;
        ct->degree = d->polys - 1;
        ct->polys = (CPolynomial*)malloc(sizeof(CPolynomial) * (size_t)d->polys);
        u64* src = job.direct[i] ? job.direct[i] : host + job.items[i].second;   // (direct: the struct indexes the caller's own buffer)
        for (int p = 0; p < d->polys; p++) {
            ct->polys[p].n_component = d->level + 1;
            ct->polys[p].components = (CComponent*)malloc(sizeof(CComponent) * (size_t)(d->level + 1));
            for (int j = 0; j <= d->level; j++) {
                ct->polys[p].components[j].n = n;
                ct->polys[p].components[j].data = src;
                src += n;
            }
        }
        std::shared_ptr<CCiphertext> sp(ct, [hslab](CCiphertext* q) {
            for (int p = 0; p <= q->degree; p++) free(q->polys[p].components);
            free(q->polys);
            free(q);
        });
        avail[job.nodes[i]->output_nodes[0]->index] = sp;
    }
}

}  // namespace task
}  // namespace lsa
