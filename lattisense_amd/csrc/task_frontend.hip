// task_frontend.hip — the caller's side of a task run that this library provides itself: the C-struct helpers of
// include/lattisense_task.h, the native front-end's export / import executors (lsa_frontend_bind: handles are lsa_host_*
// structs over the caller's limb buffers) and caller-pinned host memory (lsa_host_register / lsa_host_alloc).
#include <cstdlib>
#include <cstring>

#include "task_internal.h"

using namespace lsa;
using namespace lsa::task;

// ------------------------------------------------------------------------------------------------ C-struct helpers
extern "C" {
void lsa_alloc_component(CComponent* c, int n) {
    c->n = n;
    c->data = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)n);
}
void lsa_alloc_polynomial(CPolynomial* p, int n_component, int n) {
    p->n_component = n_component;
    p->components = (CComponent*)malloc(sizeof(CComponent) * (size_t)n_component);
    for (int i = 0; i < n_component; i++) lsa_alloc_component(&p->components[i], n);
}
void lsa_alloc_ciphertext(CCiphertext* ct, int degree, int level, int n) {
    ct->level = level;
    ct->degree = degree;
    ct->polys = (CPolynomial*)malloc(sizeof(CPolynomial) * (size_t)(degree + 1));
    for (int i = 0; i <= degree; i++) lsa_alloc_polynomial(&ct->polys[i], level + 1, n);
}
void lsa_free_polynomial(CPolynomial* p) {
    if (!p || !p->components) return;
    for (int i = 0; i < p->n_component; i++) free(p->components[i].data);
    free(p->components);
    p->components = nullptr;
}
void lsa_free_ciphertext(CCiphertext* ct) {
    if (!ct || !ct->polys) return;
    for (int i = 0; i <= ct->degree; i++) lsa_free_polynomial(&ct->polys[i]);
    free(ct->polys);
    ct->polys = nullptr;
}
}

namespace lsa {
namespace task {

HostRegistry& host_registry() {
    static HostRegistry r;
    return r;
}

// ------------------------------------------------------------------------------------------------ native front-end
namespace {

template <typename T> std::shared_ptr<T> owned_struct(T* p, void (*fin)(T*)) {
    return std::shared_ptr<T>(p, [fin](T* q) {
        fin(q);
        free(q);
    });
}

void view_polynomial(CPolynomial* poly, uint64_t* base, int limbs, int n) {  // components point INTO the caller's buffer
    poly->n_component = limbs;
    poly->components = (CComponent*)malloc(sizeof(CComponent) * (size_t)limbs);
    for (int j = 0; j < limbs; j++) {
        poly->components[j].n = n;
        poly->components[j].data = base + (size_t)j * n;
    }
}

void fill_ksk_view(CKeySwitchKey* dst, const lsa_host_kskey* k) {
    const int comp = k->level + 1 + k->n_special;
    const int beta = (k->level + 1 + k->n_special - 1) / k->n_special;
    dst->n_public_key = beta;
    dst->public_keys = (CPublicKey*)malloc(sizeof(CPublicKey) * (size_t)beta);
    for (int d = 0; d < beta; d++) {
        CPublicKey& pk = dst->public_keys[d];
        pk.level = k->level;
        pk.degree = 1;
        pk.polys = (CPolynomial*)malloc(sizeof(CPolynomial) * 2);
        for (int h = 0; h < 2; h++) view_polynomial(&pk.polys[h], k->data + ((size_t)(d * 2 + h) * comp) * k->n, comp, k->n);
    }
}
void free_ksk_view(CKeySwitchKey* k) {
    for (int d = 0; d < k->n_public_key; d++) {
        for (int h = 0; h < 2; h++) free(k->public_keys[d].polys[h].components);
        free(k->public_keys[d].polys);
    }
    free(k->public_keys);
}

}  // namespace

// handle -> C struct, zero-copy: the structs only index the caller's limb buffers (no per-limb malloc+copy)
ExecutorFunc frontend_export() {
    return [](ExecutionContext&, const std::unordered_map<NodeIndex, std::any>& inputs, std::any& output, const ComputeNode& self) {
        const DatumNode* in = self.input_nodes[0];
        void* h = std::any_cast<std::shared_ptr<void>>(inputs.at(in->index)).get();
        if (!h) throw std::runtime_error("null input handle for '" + in->id + "'");
        switch (in->datum_type) {
            case TYPE_CIPHERTEXT: {
                auto* src = (lsa_host_ciphertext*)h;
                if (src->level != in->fhe_prop->level || src->degree != in->fhe_prop->degree)
                    throw std::runtime_error("ciphertext '" + in->id + "' has level/degree " + std::to_string(src->level) + "/" +
                                             std::to_string(src->degree) + ", task expects " + std::to_string(in->fhe_prop->level) +
                                             "/" + std::to_string(in->fhe_prop->degree));
                auto* ct = (CCiphertext*)malloc(sizeof(CCiphertext));
                ct->level = src->level;
                ct->degree = src->degree;
                ct->polys = (CPolynomial*)malloc(sizeof(CPolynomial) * (size_t)(src->degree + 1));
                for (int p = 0; p <= src->degree; p++)
                    view_polynomial(&ct->polys[p], src->data + (size_t)p * (src->level + 1) * src->n, src->level + 1, src->n);
                output = owned_struct<CCiphertext>(ct, [](CCiphertext* c) {
                    for (int p = 0; p <= c->degree; p++) free(c->polys[p].components);
                    free(c->polys);
                });
                break;
            }
            case TYPE_PLAINTEXT: {
                auto* src = (lsa_host_plaintext*)h;
                auto* pt = (CPlaintext*)malloc(sizeof(CPlaintext));
                pt->level = src->level;
                view_polynomial(&pt->poly, src->data, src->level + 1, src->n);
                output = owned_struct<CPlaintext>(pt, [](CPlaintext* p) { free(p->poly.components); });
                break;
            }
            case TYPE_RELIN_KEY:
            case TYPE_SWITCH_KEY: {
                auto* src = (lsa_host_kskey*)h;
                auto* k = (CKeySwitchKey*)malloc(sizeof(CKeySwitchKey));
                fill_ksk_view(k, src);
                if (in->datum_type == TYPE_RELIN_KEY) output = std::shared_ptr<CRelinKey>(k, [](CRelinKey* q) { free_ksk_view(q); free(q); });
                else output = std::shared_ptr<CKeySwitchKey>(k, [](CKeySwitchKey* q) { free_ksk_view(q); free(q); });
                break;
            }
            case TYPE_GALOIS_KEY: {
                auto* src = (lsa_host_galois_key*)h;
                const uint64_t want = in->fhe_prop->p ? in->fhe_prop->p->galois_element : 0;
                const lsa_host_kskey* found = nullptr;
                for (int i = 0; i < src->n_keys; i++)
                    if (src->galois_elements[i] == want) found = &src->keys[i];
                if (!found) throw std::runtime_error("The rotation key glk_" + std::to_string(want) + " is not prepared");
                auto* gk = (CGaloisKey*)malloc(sizeof(CGaloisKey));
                gk->n_key_switch_key = 1;
                gk->galois_elements = (uint64_t*)malloc(sizeof(uint64_t));
                gk->galois_elements[0] = want;
                gk->key_switch_keys = (CKeySwitchKey*)malloc(sizeof(CKeySwitchKey));
                fill_ksk_view(&gk->key_switch_keys[0], found);
                output = std::shared_ptr<CGaloisKey>(gk, [](CGaloisKey* q) {
                    free_ksk_view(&q->key_switch_keys[0]);
                    free(q->key_switch_keys);
                    free(q->galois_elements);
                    free(q);
                });
                break;
            }
            case TYPE_CUSTOM:
                // custom input data (e.g. a message a custom "encode" node turns into a plaintext) never reaches the device: the
                // opaque caller handle is handed through to the custom executors that consume it
                // (cxx_abi_bridge_executors.h:212-220 does the same with CustomData)
                output = inputs.at(in->index);
                break;
            default:   // an unknown or garbled type must not reach downstream any_casts (the reference throws here too, ibid.)
                throw std::runtime_error("Unsupported data type " + std::to_string((int)in->datum_type) + " for input '" + in->id + "' (datum " +
                                         std::to_string(in->index) + ")");
        }
    };
}

namespace {

// an intermediate ciphertext handle owned by the run (a device result that a custom CPU node consumes, or a custom node's
// input for the next device stage): header + limbs in one allocation, released with the last reference
struct OwnedHostCiphertext {
    lsa_host_ciphertext h;
    std::vector<uint64_t> limbs;
};
std::shared_ptr<void> new_intermediate_ciphertext(int degree, int level, int n) {
    auto o = std::make_shared<OwnedHostCiphertext>();
    o->limbs.resize((size_t)(degree + 1) * (level + 1) * n);
    o->h.level = level;
    o->h.degree = degree;
    o->h.n = n;
    o->h.data = o->limbs.data();
    return std::shared_ptr<void>(o, &o->h);   // aliasing: callers see the lsa_host_ciphertext, the block stays alive
}

}  // namespace

// C struct -> pre-allocated output handle (other_args[0], as in gpu_wrapper.cu:354-365); without one (a device result that
// feeds a custom CPU node) -> a fresh intermediate handle (cxx_abi_bridge_executors.h:428-431).  A custom node's own
// output that is a task output arrives as a handle already and is copied into the caller's.
ExecutorFunc frontend_import() {
    return [](ExecutionContext& ctx, const std::unordered_map<NodeIndex, std::any>& inputs, std::any& output, const ComputeNode& self) {
        const DatumNode* in = self.input_nodes[0];
        const std::any& src_any = inputs.at(in->index);
        lsa_host_ciphertext* dst = nullptr;
        std::shared_ptr<void> owned;
        if (!ctx.other_args.empty()) {
            dst = (lsa_host_ciphertext*)std::any_cast<void*>(ctx.other_args[0]);
            if (!dst || !dst->data) throw std::runtime_error("import: null output handle");
        }
        if (auto* hp = std::any_cast<std::shared_ptr<void>>(&src_any)) {   // produced by a custom node: already a handle
            auto* src = (lsa_host_ciphertext*)hp->get();
            if (!src || !src->data) throw std::runtime_error("import: custom node '" + in->id + "' produced no ciphertext handle");
            if (!dst) {
                output = *hp;
                return;
            }
            if (dst->level != src->level || dst->degree != src->degree || dst->n != src->n)
                throw std::runtime_error("output ciphertext '" + self.output_nodes[0]->id + "' was allocated at level/degree " +
                                         std::to_string(dst->level) + "/" + std::to_string(dst->degree) + ", result has " +
                                         std::to_string(src->level) + "/" + std::to_string(src->degree));
            memcpy(dst->data, src->data, sizeof(uint64_t) * (size_t)(src->degree + 1) * (src->level + 1) * src->n);
            output = std::shared_ptr<void>(dst, [](void*) {});
            return;
        }
        auto ct = std::any_cast<std::shared_ptr<CCiphertext>>(src_any);
        const int n = ct->polys[0].components[0].n;
        if (!dst) {
            owned = new_intermediate_ciphertext(ct->degree, ct->level, n);
            dst = (lsa_host_ciphertext*)owned.get();
        }
        if (dst->level != ct->level || dst->degree != ct->degree)
            throw std::runtime_error("output ciphertext '" + self.output_nodes[0]->id + "' was allocated at level/degree " +
                                     std::to_string(dst->level) + "/" + std::to_string(dst->degree) + ", result has " +
                                     std::to_string(ct->level) + "/" + std::to_string(ct->degree));
        for (int p = 0; p <= ct->degree; p++)
            for (int j = 0; j <= ct->level; j++) {
                uint64_t* to = dst->data + ((size_t)p * (ct->level + 1) + j) * n;
                if (to != ct->polys[p].components[j].data)   // (equal: the backend wrote the result straight into this handle's pinned buffer)
                    memcpy(to, ct->polys[p].components[j].data, sizeof(uint64_t) * (size_t)n);
            }
        output = owned ? owned : std::shared_ptr<void>(dst, [](void*) {});
    };
}

}  // namespace task
}  // namespace lsa

// ------------------------------------------------------------------------------------------------ caller-pinned host memory
extern "C" {

int lsa_host_register(void* ptr, size_t bytes) {
    return task_guard([&] {
        LSA_REQUIRE(ptr != nullptr && bytes > 0, "null range");
        LSA_HIP(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
        std::lock_guard<std::mutex> lk(host_registry().mu);
        host_registry().ranges[(uintptr_t)ptr] = bytes;
    });
}

int lsa_host_unregister(void* ptr) {
    return task_guard([&] {
        {
            std::lock_guard<std::mutex> lk(host_registry().mu);
            LSA_REQUIRE(host_registry().ranges.erase((uintptr_t)ptr) == 1, "range was not registered");
        }
        LSA_HIP(hipHostUnregister(ptr));
    });
}

// pinned memory allocated FOR the caller (hipHostMalloc: the DMA engines reach it at full PCIe rate; memory pinned in place
// with lsa_host_register measured slower than the staged path on MI355X hosts, profiles/r03/t2_zero_copy_ab.log)
int lsa_host_alloc(size_t bytes, void** out) {
    return task_guard([&] {
        LSA_REQUIRE(out != nullptr && bytes > 0, "null argument");
        void* p = nullptr;
        LSA_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        std::lock_guard<std::mutex> lk(host_registry().mu);
        host_registry().ranges[(uintptr_t)p] = bytes;
        *out = p;
    });
}

int lsa_host_free(void* ptr) {
    return task_guard([&] {
        {
            std::lock_guard<std::mutex> lk(host_registry().mu);
            LSA_REQUIRE(host_registry().ranges.erase((uintptr_t)ptr) == 1, "not an lsa_host_alloc block");
        }
        LSA_HIP(hipHostFree(ptr));
    });
}

}  // extern "C"
