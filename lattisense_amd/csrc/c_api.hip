// c_api.hip — extern "C" operator layer (include/lattisense_amd.h).  Every entry point converts C++ exceptions into
// error codes: nothing throws across the C boundary (the reference does, SURVEY §8b "Errors").
#include "bfv_encode.h"
#include "bfv_poly.h"
#include "build_flags.h"
#include "linear_transform.h"
#include "poly_eval.h"
#include "lsa_internal.h"

namespace lsa {
const char* kernels_build_flags();   // kernels.hip / context.hip: what THOSE translation units were compiled with
const char* context_build_flags();
}  // namespace lsa

using namespace lsa;

struct lsa_context_st {
    Context ctx;
    lsa_context_st(int algo, int n, const u64* q, int nq, const u64* p, int np, u64 t, int dev)
        : ctx(algo, n, q, nq, p, np, t, dev) {}
};
struct lsa_key_st {
    Key key;
    double* fp_owned = nullptr;   // the double copy of an adopted key (the caller's buffer has no room for it)
};

template <typename F>
static int guard(F&& f) {
    try {
        f();
        return LSA_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return LSA_ERR_INTERNAL;
    } catch (...) {
        set_last_error("unknown error");
        return LSA_ERR_INTERNAL;
    }
}

static Context& C(lsa_context h) {
    LSA_REQUIRE(h != nullptr, "null context");
    h->ctx.use_device();
    return h->ctx;
}
static const Key& K(lsa_key k, const char* who = nullptr) {
    LSA_REQUIRE(k != nullptr && k->key.data != nullptr, who ? std::string(who) + ": null key" : std::string("null key"));
    return k->key;
}
static hipStream_t S(void* s) { return (hipStream_t)s; }

// ---- plan handles.  The operators that work through a plan (bootstrap, the two linear transforms, the two slot sums, the BFV expansion and packing, the two
// polynomial evaluators) hand out one kind of handle: the plan with its deleter and the context it was made on.  The public header keeps a
// distinct opaque type per operator; each derives from PlanHandle.  Every entry point keeps its own message texts.
template <typename T>
struct PlanHandle {
    std::unique_ptr<T, void (*)(T*)> plan;
    Context* c;
};
template <typename T>
static void plan_delete(T* p) {
    delete p;
}
template <typename H, typename T>
static void make_plan(H** out, Context& c, T* plan, void (*destroy)(T*) = plan_delete<T>) {
    std::unique_ptr<T, void (*)(T*)> owned(plan, destroy);
    *out = new H{{std::move(owned), &c}};
}
template <typename H>
static auto& P(H* h, const char* null_msg) {   // the plan of a handle
    LSA_REQUIRE(h != nullptr, null_msg);
    return *h->plan;
}
template <typename H>
static auto& P(H* h, lsa_context ctx, const char* null_msg, const char* other_ctx_msg) {   // ... that an operator runs on ctx
    LSA_REQUIRE(h != nullptr, null_msg);
    LSA_REQUIRE(h->c == &C(ctx), other_ctx_msg);
    return *h->plan;
}
template <typename V, typename O>
static void copy_out(const V& v, O* out, int capacity, const char* too_small) {
    LSA_REQUIRE((int)v.size() <= capacity, too_small);
    std::copy(v.begin(), v.end(), out);
}
static GaloisKeys G(int n, const uint64_t* elements, const lsa_key* keys, const char* who = nullptr) {
    return GaloisKeys(n, elements, keys, [&](lsa_key k) { return &K(k, who); });
}

extern "C" {

const char* lsa_last_error(void) { return last_error().c_str(); }
const char* lsa_version(void) { return "lattisense_amd 0.1 (gfx950)"; }
// every LSA_* switch the library was compiled with (build_flags.h); "" for the product build.  The three translation units
// that carry switches must agree; if they do not, each view is reported.
const char* lsa_build_flags(void) {
    static const std::string text = [] {
        auto strip = [](const char* t) { return std::string(t[0] == ' ' ? t + 1 : t); };
        const std::string a = strip(LSA_BUILD_FLAGS_TEXT), k = strip(kernels_build_flags()), c = strip(context_build_flags());
        if (a == k && a == c) return a;
        return "MIXED c_api=[" + a + "] kernels=[" + k + "] context=[" + c + "]";
    }();
    return text.c_str();
}

int lsa_context_create(int algo, int n, const uint64_t* q, int nq, const uint64_t* p, int np, uint64_t t, int device,
                       lsa_context* out) {
    return guard([&] {
        LSA_REQUIRE(out != nullptr && q != nullptr && (np == 0 || p != nullptr), "null argument");
        *out = new lsa_context_st(algo, n, q, nq, p, np, t, device);
    });
}
int lsa_context_destroy(lsa_context ctx) {
    return guard([&] { delete ctx; });
}
int lsa_context_moduli(lsa_context ctx, uint64_t* out, int capacity, int* count) {
    return guard([&] {
        Context& c = C(ctx);
        if (count) *count = c.nmod;
        for (int i = 0; i < c.nmod && i < capacity; i++) out[i] = c.T.mod[i];
    });
}

int lsa_malloc(lsa_context ctx, void** dptr, size_t bytes) {
    return guard([&] {
        C(ctx);
        LSA_HIP(hipMalloc(dptr, bytes));
    });
}
int lsa_free(lsa_context ctx, void* dptr) {
    return guard([&] {
        C(ctx);
        LSA_HIP(hipFree(dptr));
    });
}
int lsa_memcpy_h2d(lsa_context ctx, void* dst, const void* src, size_t bytes, void* stream) {
    return guard([&] {
        C(ctx);
        LSA_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S(stream)));
    });
}
int lsa_memcpy_d2h(lsa_context ctx, void* dst, const void* src, size_t bytes, void* stream) {
    return guard([&] {
        C(ctx);
        LSA_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(stream)));
        LSA_HIP(hipStreamSynchronize(S(stream)));
    });
}
int lsa_memcpy_d2d(lsa_context ctx, void* dst, const void* src, size_t bytes, void* stream) {
    return guard([&] {
        C(ctx);
        LSA_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, S(stream)));
    });
}
int lsa_stream_create(lsa_context ctx, void** stream) {
    return guard([&] {
        C(ctx);
        hipStream_t s;
        LSA_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        *stream = (void*)s;
    });
}
int lsa_stream_destroy(lsa_context ctx, void* stream) {
    return guard([&] {
        C(ctx);
        LSA_HIP(hipStreamDestroy(S(stream)));
    });
}
int lsa_stream_synchronize(lsa_context ctx, void* stream) {
    return guard([&] {
        C(ctx);
        LSA_HIP(hipStreamSynchronize(S(stream)));
    });
}
int lsa_event_create(lsa_context ctx, void** ev) {
    return guard([&] {
        C(ctx);
        hipEvent_t e;
        LSA_HIP(hipEventCreate(&e));
        *ev = (void*)e;
    });
}
int lsa_event_record(lsa_context ctx, void* ev, void* stream) {
    return guard([&] {
        C(ctx);
        LSA_HIP(hipEventRecord((hipEvent_t)ev, S(stream)));
    });
}
int lsa_event_elapsed_ms(lsa_context ctx, void* ev_start, void* ev_stop, float* ms) {
    return guard([&] {
        C(ctx);
        LSA_HIP(hipEventSynchronize((hipEvent_t)ev_stop));
        LSA_HIP(hipEventElapsedTime(ms, (hipEvent_t)ev_start, (hipEvent_t)ev_stop));
    });
}
int lsa_event_destroy(lsa_context ctx, void* ev) {
    return guard([&] {
        C(ctx);
        LSA_HIP(hipEventDestroy((hipEvent_t)ev));
    });
}

// ---- keys
size_t lsa_key_bytes(lsa_context ctx, int key_level) {
    return ctx ? key_layout(ctx->ctx, key_level).words * sizeof(u64) : 0;
}

int lsa_key_upload(lsa_context ctx, const uint64_t* compact_host, int key_level, void* stream, lsa_key* out) {
    return guard([&] {
        Context& c = C(ctx);
        LSA_REQUIRE(out != nullptr && compact_host != nullptr, "null argument");
        const KeyLayout kl = key_layout(c, key_level);
        LSA_REQUIRE(kl.words > 0, "bad key level (or context has no special primes)");
        auto k = std::make_unique<lsa_key_st>();
        k->key.owned = true;
        LSA_HIP(hipMalloc((void**)&k->key.data, kl.alloc_words() * sizeof(u64)));   // the double copy, if any, behind the key
        LSA_HIP(hipMemcpyAsync(k->key.data, compact_host, kl.words * sizeof(u64), hipMemcpyHostToDevice, S(stream)));
        key_prepare(c, k->key, k->key.data, key_level, kl.fp_of(k->key.data), S(stream));
        LSA_HIP(hipStreamSynchronize(S(stream)));  // host buffer may be released by the caller on return
        *out = k.release();
    });
}
int lsa_key_adopt_device(lsa_context ctx, uint64_t* compact_dev, int key_level, void* stream, lsa_key* out) {
    return guard([&] {
        Context& c = C(ctx);
        LSA_REQUIRE(out != nullptr && compact_dev != nullptr, "null argument");
        const KeyLayout kl = key_layout(c, key_level);
        LSA_REQUIRE(kl.words > 0, "bad key level (or context has no special primes)");
        auto k = std::make_unique<lsa_key_st>();
        k->key.owned = false;
        if (kl.fp)   // the caller's buffer has no room: the double copy is this handle's own allocation
            LSA_HIP(hipMalloc((void**)&k->fp_owned, kl.words * sizeof(double)));
        key_prepare(c, k->key, compact_dev, key_level, k->fp_owned, S(stream));
        *out = k.release();
    });
}
int lsa_key_destroy(lsa_context ctx, lsa_key key) {
    return guard([&] {
        C(ctx);
        if (key) {
            if (key->key.owned && key->key.data) LSA_HIP(hipFree(key->key.data));
            if (key->fp_owned) LSA_HIP(hipFree(key->fp_owned));
            delete key;
        }
    });
}

// ---- polynomial ops
int lsa_ntt(lsa_context ctx, uint64_t* data, int batch, long long batch_stride, int rows, const int* mod_of, int period,
            int inverse, void* stream) {
    return guard([&] {
        Context& c = C(ctx);
        LSA_REQUIRE(data && mod_of && period >= 1 && period <= LSA_MAX_PERIOD, "bad arguments");
        RowMap rm;
        rm.period = period;
        for (int i = 0; i < period; i++) {
            LSA_REQUIRE(mod_of[i] == LSA_ROW_SKIP || (mod_of[i] >= 0 && mod_of[i] < c.nmod), "modulus index out of range");
            rm.mod_of[i] = (unsigned char)mod_of[i];
        }
        launch_ntt(c, data, data, batch, batch_stride, rows, rm, inverse != 0, S(stream));
    });
}
int lsa_poly_addsub(lsa_context ctx, int op, int level, int polys, const uint64_t* a, const uint64_t* b, uint64_t* out,
                    int batch, long long sa, long long sb, long long so, void* stream) {
    return guard([&] { poly_addsub(C(ctx), op, level, polys, a, b, out, batch, sa, sb, so, S(stream)); });
}

// ---- CKKS
int lsa_ckks_mult(lsa_context ctx, int level, const uint64_t* a, const uint64_t* b, uint64_t* d3, int batch,
                  long long sa, long long sb, long long sd, void* stream) {
    return guard([&] { ckks_mult(C(ctx), level, a, b, d3, batch, sa, sb, sd, S(stream)); });
}
int lsa_ckks_relin(lsa_context ctx, int level, const uint64_t* d3, lsa_key rlk, uint64_t* out, int batch, long long sd,
                   long long so, void* stream) {
    return guard([&] { ckks_relin(C(ctx), level, d3, K(rlk, "lsa_ckks_relin"), out, batch, sd, so, S(stream)); });
}
int lsa_ckks_rescale(lsa_context ctx, int level, int polys, const uint64_t* in, uint64_t* out, int batch, long long si,
                     long long so, void* stream) {
    return guard([&] { ckks_rescale(C(ctx), level, polys, in, out, batch, si, so, S(stream)); });
}
int lsa_ckks_rotate(lsa_context ctx, int level, const uint64_t* in, uint64_t g, lsa_key glk, uint64_t* out, int batch,
                    long long si, long long so, void* stream) {
    return guard([&] { ckks_rotate(C(ctx), level, in, g, K(glk, "lsa_ckks_rotate"), out, batch, si, so, S(stream)); });
}
int lsa_drop_level(lsa_context ctx, int level, int polys, const uint64_t* in, uint64_t* out, int batch, long long si,
                   long long so, void* stream) {
    return guard([&] { drop_level(C(ctx), level, polys, in, out, batch, si, so, S(stream)); });
}
int lsa_ckks_mult_relin_rescale(lsa_context ctx, int level, const uint64_t* a, const uint64_t* b, lsa_key rlk,
                                uint64_t* out, int batch, long long sa, long long sb, long long so, void* stream) {
    return guard([&] { ckks_mult_relin_rescale(C(ctx), level, a, b, K(rlk, "lsa_ckks_mult_relin_rescale"), out, batch, sa, sb, so, S(stream)); });
}

// ---- CKKS encrypted inner product (ops.hip ckks_mult_sum / ckks_dot)
int lsa_ckks_mult_sum(lsa_context ctx, int level, int n, const uint64_t* const* as, const long long* sas, const int* a_rpp,
                      const uint64_t* const* bs, const long long* sbs, const int* b_rpp, const uint64_t* addend, long long s_addend,
                      uint64_t* d3, int batch, long long sd, void* stream) {
    return guard([&] {
        const DotTerms t{n, as, sas, a_rpp, bs, sbs, b_rpp, addend, s_addend};
        ckks_mult_sum(C(ctx), level, t, d3, batch, sd, S(stream));
    });
}
int lsa_ckks_dot(lsa_context ctx, int level, int n, const uint64_t* const* as, const long long* sas, const int* a_rpp,
                 const uint64_t* const* bs, const long long* sbs, const int* b_rpp, const uint64_t* addend, long long s_addend,
                 lsa_key rlk, uint64_t* out, int batch, long long sout, int rescale, void* stream) {
    return guard([&] {
        Context& c = C(ctx);
        LSA_REQUIRE(rlk != nullptr && rlk->key.data != nullptr, "dot: the relinearisation key is missing");
        const DotTerms t{n, as, sas, a_rpp, bs, sbs, b_rpp, addend, s_addend};
        ckks_dot(c, level, t, rlk->key, out, batch, sout, rescale != 0, S(stream));
    });
}

// ---- CKKS plaintext and constant operands (ops.hip; the encoder is linear_transform.hip's).  No context can exist without a
// HIP device, so a null one is reported as what it is there: LSA_ERR_NO_DEVICE.  This differs from C() on purpose, and only in
// that case: the older entry points keep the LSA_ERR_ARG their callers and tests know; with a device present both say "null
// context".  Folding the device probe into C() for every entry point is a follow-up of its own, since it changes their codes.
static Context& CP(lsa_context h, const char* who) {
    if (h == nullptr) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            throw Error(LSA_ERR_NO_DEVICE, std::string(who) + ": no HIP device available: this library has no CPU fallback");
        throw Error(LSA_ERR_ARG, std::string(who) + ": null context");
    }
    h->ctx.use_device();
    return h->ctx;
}
int lsa_ckks_encode(lsa_context ctx, int level, int log_slots, const double* values, double scale, uint64_t* out_dev, long long sout,
                    int batch, void* stream) {
    return guard([&] { ckks_encode(CP(ctx, "lsa_ckks_encode"), level, log_slots, values, scale, out_dev, sout, batch, S(stream)); });
}
int lsa_ckks_mult_plain(lsa_context ctx, int level, const uint64_t* ct, long long sct, const uint64_t* pt, long long spt, uint64_t* out,
                        long long sout, int batch, int rescale, void* stream) {
    return guard([&] { ckks_mult_plain(CP(ctx, "lsa_ckks_mult_plain"), level, ct, sct, pt, spt, out, sout, batch, rescale != 0, S(stream)); });
}
int lsa_ckks_addsub_plain(lsa_context ctx, int op, int level, const uint64_t* ct, long long sct, const uint64_t* pt, long long spt,
                          uint64_t* out, long long sout, int batch, void* stream) {
    return guard([&] { ckks_addsub_plain(CP(ctx, "lsa_ckks_addsub_plain"), op, level, ct, sct, pt, spt, out, sout, batch, S(stream)); });
}
int lsa_ckks_mac_plain(lsa_context ctx, int level, int n, const uint64_t* const* cts, const long long* scts, const uint64_t* const* pts,
                       const long long* spts, const uint64_t* addend, long long s_addend, uint64_t* out, long long sout, int batch,
                       int rescale, void* stream) {
    return guard([&] {
        ckks_mac_plain(CP(ctx, "lsa_ckks_mac_plain"), level, n, cts, scts, pts, spts, addend, s_addend, out, sout, batch, rescale != 0,
                       S(stream));
    });
}
int lsa_ckks_mult_const(lsa_context ctx, int level, const uint64_t* ct, long long sct, double re, double im, double const_scale,
                        uint64_t* out, long long sout, int batch, int rescale, void* stream) {
    return guard([&] {
        ckks_mult_const(CP(ctx, "lsa_ckks_mult_const"), level, ct, sct, re, im, const_scale, out, sout, batch, rescale != 0, S(stream));
    });
}
int lsa_ckks_add_const(lsa_context ctx, int level, const uint64_t* ct, long long sct, double re, double im, double ct_scale,
                       uint64_t* out, long long sout, int batch, void* stream) {
    return guard([&] { ckks_add_const(CP(ctx, "lsa_ckks_add_const"), level, ct, sct, re, im, ct_scale, out, sout, batch, S(stream)); });
}
int lsa_ckks_affine_const(lsa_context ctx, int level, const uint64_t* ct, long long sct, double re, double im, double const_scale,
                          double add_re, double add_im, double ct_scale, uint64_t* out, long long sout, int batch, int rescale,
                          void* stream) {
    return guard([&] {
        ckks_affine_const(CP(ctx, "lsa_ckks_affine_const"), level, ct, sct, re, im, const_scale, add_re, add_im, ct_scale, out, sout,
                          batch, rescale != 0, S(stream));
    });
}

// ---- BFV
int lsa_bfv_mult(lsa_context ctx, int level, const uint64_t* a, const uint64_t* b, uint64_t* d3, int batch, long long sa,
                 long long sb, long long sd, void* stream) {
    return guard([&] { bfv_mult(C(ctx), level, a, b, d3, batch, sa, sb, sd, S(stream)); });
}
int lsa_bfv_relin(lsa_context ctx, int level, const uint64_t* d3, lsa_key rlk, uint64_t* out, int batch, long long sd,
                  long long so, void* stream) {
    return guard([&] { bfv_relin(C(ctx), level, d3, K(rlk, "lsa_bfv_relin"), out, batch, sd, so, S(stream)); });
}
int lsa_bfv_rotate(lsa_context ctx, int level, const uint64_t* in, uint64_t g, lsa_key glk, uint64_t* out, int batch,
                   long long si, long long so, void* stream) {
    return guard([&] { bfv_rotate(C(ctx), level, in, g, K(glk, "lsa_bfv_rotate"), out, batch, si, so, S(stream)); });
}
int lsa_bfv_rescale(lsa_context ctx, int level, int polys, const uint64_t* in, uint64_t* out, int batch, long long si,
                    long long so, void* stream) {
    return guard([&] { bfv_rescale(C(ctx), level, polys, in, out, batch, si, so, S(stream)); });
}
int lsa_bfv_mult_relin(lsa_context ctx, int level, const uint64_t* a, const uint64_t* b, lsa_key rlk, uint64_t* out,
                       int batch, long long sa, long long sb, long long so, void* stream) {
    return guard([&] { bfv_mult_relin(C(ctx), level, a, b, K(rlk, "lsa_bfv_mult_relin"), out, batch, sa, sb, so, S(stream)); });
}

// ---- BFV encrypted inner product (ops.hip bfv_mult_sum / bfv_dot; the plan is tables.cpp's and needs no device)
int lsa_bfv_mult_sum(lsa_context ctx, int level, int n, const uint64_t* const* as, const long long* sas, const uint64_t* const* bs,
                     const long long* sbs, const uint64_t* addend, long long s_addend, uint64_t* d3, int batch, long long sd,
                     void* stream) {
    return guard([&] {
        const DotTerms t{n, as, sas, nullptr, bs, sbs, nullptr, addend, s_addend};
        bfv_mult_sum(C(ctx), level, t, d3, batch, sd, S(stream));
    });
}
int lsa_bfv_dot(lsa_context ctx, int level, int n, const uint64_t* const* as, const long long* sas, const uint64_t* const* bs,
                const long long* sbs, const uint64_t* addend, long long s_addend, lsa_key rlk, uint64_t* out, int batch, long long sout,
                void* stream) {
    return guard([&] {
        const DotTerms t{n, as, sas, nullptr, bs, sbs, nullptr, addend, s_addend};
        bfv_dot(C(ctx), level, t, rlk ? &rlk->key : nullptr, out, batch, sout, S(stream));
    });
}
int lsa_bfv_dot_plan(int n_ring, const uint64_t* q, int nq, int level, int terms, int* max_terms, int* n_groups, int* aux_limbs) {
    return guard([&] {
        LSA_REQUIRE(n_ring >= 2 && n_ring <= (1 << 20) && (n_ring & (n_ring - 1)) == 0, "bfv_dot: the ring degree must be a power of two");
        LSA_REQUIRE(q != nullptr && nq >= 1, "bfv_dot: null argument");
        LSA_REQUIRE(level >= 0 && level < nq, "bfv_dot: level out of range");
        LSA_REQUIRE(terms >= 1, "bfv_dot: needs at least one term");
        for (int i = 0; i < nq; i++) LSA_REQUIRE(q[i] >= 2 && (q[i] >> 61) == 0, "bfv_dot: a modulus is out of range");
        int logn = 0;
        while ((1 << logn) < n_ring) logn++;
        const BfvDotPlan p = bfv_dot_plan(q, nq, level, logn, terms);
        if (max_terms) *max_terms = p.max_terms;
        if (n_groups) *n_groups = p.n_groups;
        if (aux_limbs) *aux_limbs = p.aux_limbs;
    });
}

int lsa_profile_begin(lsa_context ctx, int stride) {
    return guard([&] {
        Context& c = C(ctx);
        LSA_REQUIRE(stride >= 1, "stride must be >= 1");
        for (auto& sm : c.prof_samples) {
            c.prof_pool.push_back(sm.e0);
            c.prof_pool.push_back(sm.e1);
        }
        c.prof_samples.clear();
        for (auto& n : c.prof_launched) n = 0;
        c.prof_stride = stride;
        c.prof_on = true;
    });
}
int lsa_profile_end(lsa_context ctx) {
    return guard([&] { C(ctx).prof_on = false; });
}
int lsa_profile_read(lsa_context ctx, int kind, double* total_ms, double* total_bytes, long long* sampled,
                     long long* launched) {
    return guard([&] {
        Context& c = C(ctx);
        LSA_REQUIRE(kind >= 0 && kind < LSA_PROF_KINDS, "unknown kernel kind");
        double ms = 0, by = 0;
        long long n = 0;
        for (auto& sm : c.prof_samples) {
            if (sm.kid != kind) continue;
            LSA_HIP(hipEventSynchronize(sm.e1));
            float t = 0;
            LSA_HIP(hipEventElapsedTime(&t, sm.e0, sm.e1));
            ms += t;
            by += sm.bytes;
            n++;
        }
        if (total_ms) *total_ms = ms;
        if (total_bytes) *total_bytes = by;
        if (sampled) *sampled = n;
        if (launched) *launched = c.prof_launched[kind];
    });
}

// the same samples with only the kind's OWN algorithmic bytes (a fused launch -- the transform pass that also performs the key
// MAC -- counts both functions' bytes in lsa_profile_read and the transform's alone here)
int lsa_profile_read_primary(lsa_context ctx, int kind, double* total_bytes_primary) {
    return guard([&] {
        Context& c = C(ctx);
        LSA_REQUIRE(kind >= 0 && kind < LSA_PROF_KINDS && total_bytes_primary, "bad argument");
        double by = 0;
        for (auto& sm : c.prof_samples)
            if (sm.kid == kind) by += sm.bytes_primary;
        *total_bytes_primary = by;
    });
}

int lsa_set_fuse_tails(lsa_context ctx, int enable) {
    return guard([&] { C(ctx).fuse_tails = enable ? 1 : 0; });
}
int lsa_set_modup_lift(lsa_context ctx, int enable) {
    return guard([&] { C(ctx).modup_lift = enable ? 1 : 0; });
}
int lsa_set_rgsw_pair_mac(lsa_context ctx, int enable) {
    return guard([&] { C(ctx).rgsw_pair_mac = enable ? 1 : 0; });
}
int lsa_set_ks_tail_in_mac(lsa_context ctx, int mode) {
    return guard([&] {
        LSA_REQUIRE(mode >= 0 && mode <= 2, "lsa_set_ks_tail_in_mac: mode is 0, 1 or 2");
        C(ctx).ks_tail_in_mac = mode;
    });
}
int lsa_set_rescale_head_in_conv(lsa_context ctx, int mode) {
    return guard([&] {
        LSA_REQUIRE(mode >= 0 && mode <= 2, "lsa_set_rescale_head_in_conv: mode is 0, 1 or 2");
        C(ctx).rescale_head_in_conv = mode;
    });
}
int lsa_set_dual_stream(lsa_context ctx, int enable) {
    return guard([&] { C(ctx).dual_stream = enable ? 1 : 0; });
}
int lsa_debug_set_ntt_stamps(lsa_context ctx, void* device_buffer) {
    return guard([&] { C(ctx).ntt_diag = static_cast<unsigned long long*>(device_buffer); });
}
int lsa_debug_baseconv_plans(lsa_context ctx, int capacity, int* count, int* ns, int* nd, int* split) {
    return guard([&] {
        Context& c = C(ctx);
        LSA_REQUIRE(count != nullptr && (capacity == 0 || (ns && nd && split)), "null argument");
        std::lock_guard<std::mutex> lk(c.mu);
        *count = (int)c.bconv.size();
        int i = 0;
        for (auto& kv : c.bconv) {
            if (i >= capacity) break;
            ns[i] = kv.second.ns;
            nd[i] = kv.second.nd;
            split[i] = kv.second.split29 ? 1 : 0;
            i++;
        }
    });
}
int lsa_debug_key_switch_fused(lsa_context ctx, int level, lsa_key key, int* fused) {
    return guard([&] {
        Context& c = C(ctx);
        LSA_REQUIRE(fused != nullptr && level >= 0 && level < c.nq, "bad argument");
        *fused = ks_fuse_mac(c, level, K(key)) ? 1 : 0;
    });
}

int lsa_ckks_rotate_many(lsa_context ctx, int level, const uint64_t* in, int n_rot, const uint64_t* galois_elements,
                         const lsa_key* glk, uint64_t* const* outs, int batch, long long sin, long long sout, void* stream) {
    return guard([&] {
        LSA_REQUIRE(in != nullptr && n_rot >= 0 && (n_rot == 0 || (galois_elements && glk && outs)), "lsa_ckks_rotate_many: null argument");
        std::vector<const Key*> keys(n_rot);
        for (int i = 0; i < n_rot; i++) {
            LSA_REQUIRE(glk[i] != nullptr && outs[i] != nullptr, "lsa_ckks_rotate_many: null key or output");
            keys[i] = &K(glk[i], "lsa_ckks_rotate_many");
        }
        ckks_rotate_many(C(ctx), level, in, n_rot, galois_elements, keys.data(), outs, batch, sin, sout, S(stream));
    });
}
int lsa_bfv_rotate_many(lsa_context ctx, int level, const uint64_t* in, int n_rot, const uint64_t* galois_elements,
                        const lsa_key* glk, uint64_t* const* outs, int batch, long long sin, long long sout, void* stream) {
    return guard([&] {
        LSA_REQUIRE(in != nullptr && n_rot >= 0 && (n_rot == 0 || (galois_elements && glk && outs)), "lsa_bfv_rotate_many: null argument");
        std::vector<const Key*> keys(n_rot);
        for (int i = 0; i < n_rot; i++) {
            LSA_REQUIRE(glk[i] != nullptr && outs[i] != nullptr, "lsa_bfv_rotate_many: null key or output");
            keys[i] = &K(glk[i], "lsa_bfv_rotate_many");
        }
        bfv_rotate_many(C(ctx), level, in, n_rot, galois_elements, keys.data(), outs, batch, sin, sout, S(stream));
    });
}

int lsa_bfv_mult_plain_mul(lsa_context ctx, int level, const uint64_t* ct, const uint64_t* pt, uint64_t* out, int batch,
                           long long sct, long long spt, long long sout, void* stream) {
    return guard([&] {
        LSA_REQUIRE(ct != nullptr && pt != nullptr && out != nullptr, "lsa_bfv_mult_plain_mul: null argument");
        bfv_mult_plain_mul(C(ctx), level, ct, pt, out, batch, sct, spt, sout, S(stream));
    });
}
int lsa_bfv_mac_plain_mul(lsa_context ctx, int level, int n, const uint64_t* const* cts, const long long* scts,
                          const uint64_t* const* pts, const long long* spts, const uint64_t* partial, long long spartial,
                          uint64_t* out, int batch, long long sout, void* stream) {
    return guard([&] {
        LSA_REQUIRE(n >= 1, "lsa_bfv_mac_plain_mul: needs at least one term");
        LSA_REQUIRE(cts && scts && pts && spts && out, "lsa_bfv_mac_plain_mul: null argument");
        for (int i = 0; i < n; i++) LSA_REQUIRE(cts[i] != nullptr && pts[i] != nullptr, "lsa_bfv_mac_plain_mul: null ciphertext or plaintext");
        bfv_mac_plain_mul(C(ctx), level, n, cts, scts, pts, spts, partial, spartial, out, batch, sout, S(stream));
    });
}
int lsa_bfv_rotate_mac_plain_mul(lsa_context ctx, int level, const uint64_t* in, int n, const uint64_t* galois_elements,
                                 const lsa_key* glk, const uint64_t* const* pts, const long long* spts, const uint64_t* partial,
                                 long long spartial, uint64_t* out, int batch, long long sin, long long sout, void* stream) {
    return guard([&] {
        LSA_REQUIRE(n >= 1, "lsa_bfv_rotate_mac_plain_mul: needs at least one term");
        LSA_REQUIRE(in && galois_elements && glk && pts && spts && out, "lsa_bfv_rotate_mac_plain_mul: null argument");
        std::vector<const Key*> keys(n, nullptr);
        for (int i = 0; i < n; i++) keys[i] = glk[i] ? &K(glk[i], "lsa_bfv_rotate_mac_plain_mul") : nullptr;
        bfv_rotate_mac_plain_mul(C(ctx), level, in, n, galois_elements, keys.data(), pts, spts, partial, spartial, out, batch, sin,
                                 sout, S(stream));
    });
}


// ---- CKKS bootstrapping
struct lsa_bootstrap_st : PlanHandle<Bootstrap> {};
int lsa_bootstrap_create_ex(lsa_context ctx, int cts_depth, int stc_depth, int k, int double_angle, double message_ratio,
                            double in_scale, double out_scale, int log_slots, int sine_deg, int arcsine_deg, void* stream,
                            lsa_bootstrap* out) {
    return guard([&] {
        LSA_REQUIRE(out != nullptr, "null argument");
        LSA_REQUIRE(k >= 1 && double_angle >= 0 && double_angle <= 8 && message_ratio > 0 && in_scale > 0, "bad bootstrap parameters");
        Context& c = C(ctx);
        LSA_REQUIRE(log_slots >= 0 && (log_slots == 0 || (2 << log_slots) <= c.n), "bad slot count");
        make_plan(out, c, bootstrap_create(c, cts_depth, stc_depth, k, double_angle, message_ratio, in_scale, out_scale, log_slots, S(stream),
                                           sine_deg, arcsine_deg), bootstrap_destroy);
    });
}
int lsa_bootstrap_create(lsa_context ctx, int cts_depth, int stc_depth, int k, int double_angle, double message_ratio,
                         double in_scale, double out_scale, int log_slots, void* stream, lsa_bootstrap* out) {
    // the reference's default EvalMod: sine degree 30 (32 Chebyshev coefficients), no arcsine (frontend/custom_task.py:443-453)
    return lsa_bootstrap_create_ex(ctx, cts_depth, stc_depth, k, double_angle, message_ratio, in_scale, out_scale, log_slots, 30, 0, stream, out);
}
// polynomial constants of the plan's EvalMod: n_cheb Chebyshev coefficients, n_asin monomial coefficients of the arcsine
// correction (0: none); either output pointer may be null to query the counts
int lsa_bootstrap_evalmod_constants(lsa_bootstrap b, int* n_cheb, double* cheb, int* n_asin, double* asin_coef) {
    return guard([&] {
        const Bootstrap& bt = P(b, "null bootstrap handle");
        const auto& c = bootstrap_chebyshev(bt);
        const auto& a = bootstrap_arcsine(bt);
        if (n_cheb) *n_cheb = (int)c.size();
        if (n_asin) *n_asin = (int)a.size();
        if (cheb) std::copy(c.begin(), c.end(), cheb);
        if (asin_coef) std::copy(a.begin(), a.end(), asin_coef);
    });
}
void lsa_bootstrap_destroy(lsa_bootstrap b) { delete b; }
int lsa_bootstrap_info(lsa_bootstrap b, int* out_level, double* out_scale, int* n_galois, int* n_matrices, int* n_cts,
                       int* sparse) {
    return guard([&] {
        const Bootstrap& bt = P(b, "null bootstrap handle");
        if (out_level) *out_level = bootstrap_out_level(bt);
        if (out_scale) *out_scale = bootstrap_out_scale(bt);
        if (n_galois) *n_galois = (int)bootstrap_galois(bt).size();
        if (n_matrices) *n_matrices = bootstrap_matrices(bt);
        if (n_cts) *n_cts = bootstrap_cts_matrices(bt);
        if (sparse) *sparse = bootstrap_is_sparse(bt) ? 1 : 0;
    });
}
int lsa_bootstrap_galois_elements(lsa_bootstrap b, uint64_t* out, int capacity) {
    return guard([&] {
        LSA_REQUIRE(b != nullptr && out != nullptr, "null argument");
        copy_out(bootstrap_galois(*b->plan), out, capacity, "buffer too small");
    });
}
int lsa_bootstrap_chebyshev(lsa_bootstrap b, double* out32) {
    return guard([&] {
        LSA_REQUIRE(b != nullptr && out32 != nullptr, "null argument");
        const auto& cf = bootstrap_chebyshev(*b->plan);
        LSA_REQUIRE(cf.size() <= 32, "more than 32 Chebyshev coefficients: use lsa_bootstrap_evalmod_constants");
        for (size_t i = 0; i < 32; i++) out32[i] = i < cf.size() ? cf[i] : 0.0;
    });
}
int lsa_bootstrap_matrix_info(lsa_bootstrap b, int index, int* level, int* n1, int* n_diagonals, int* diagonals, int capacity) {
    return guard([&] {
        int lv, n1v;
        const std::vector<int>* ks;
        const std::vector<u64*>* pl;
        bootstrap_matrix(P(b, "null bootstrap handle"), index, &lv, &n1v, &ks, &pl);
        if (level) *level = lv;
        if (n1) *n1 = n1v;
        if (n_diagonals) *n_diagonals = (int)ks->size();
        if (diagonals) copy_out(*ks, diagonals, capacity, "buffer too small");
    });
}
int lsa_bootstrap_plaintext(lsa_bootstrap b, int matrix, int diag_pos, uint64_t* host_out) {
    return guard([&] {
        LSA_REQUIRE(b != nullptr && host_out != nullptr, "null argument");
        int lv, n1v;
        const std::vector<int>* ks;
        const std::vector<u64*>* pl;
        bootstrap_matrix(*b->plan, matrix, &lv, &n1v, &ks, &pl);
        LSA_REQUIRE(diag_pos >= 0 && diag_pos < (int)pl->size(), "diagonal position out of range");
        b->c->use_device();
        // the rows at q_0..q_level only, whatever the plan keeps behind them: what this entry point has always written
        LSA_HIP(hipMemcpy(host_out, (*pl)[diag_pos], (size_t)(lv + 1) * b->c->n * sizeof(u64), hipMemcpyDeviceToHost));
    });
}
int lsa_bootstrap_plaintext_ext(lsa_bootstrap b, int matrix, int diag_pos, uint64_t* host_out, long long capacity_words) {
    return guard([&] {
        LSA_REQUIRE(b != nullptr && host_out != nullptr, "null argument");
        int lv, n1v, rows = 0;
        const std::vector<int>* ks;
        const std::vector<u64*>* pl;
        bootstrap_matrix(*b->plan, matrix, &lv, &n1v, &ks, &pl, &rows);
        LSA_REQUIRE(diag_pos >= 0 && diag_pos < (int)pl->size(), "diagonal position out of range");
        LSA_REQUIRE(capacity_words >= (long long)rows * b->c->n, "buffer too small for the plaintext's rows (lsa_bootstrap_plaintext_rows)");
        b->c->use_device();
        LSA_HIP(hipMemcpy(host_out, (*pl)[diag_pos], (size_t)rows * b->c->n * sizeof(u64), hipMemcpyDeviceToHost));
    });
}
int lsa_bootstrap_plaintext_rows(lsa_bootstrap b, int matrix, int* rows) {
    return guard([&] {
        LSA_REQUIRE(b != nullptr && rows != nullptr, "null argument");
        int lv, n1v;
        const std::vector<int>* ks;
        const std::vector<u64*>* pl;
        bootstrap_matrix(*b->plan, matrix, &lv, &n1v, &ks, &pl, rows);
    });
}
int lsa_ckks_bootstrap(lsa_context ctx, lsa_bootstrap b, const uint64_t* in, uint64_t* out, int batch, long long sin, long long sout,
                       lsa_key rlk, int n_glk, const uint64_t* glk_elements, const lsa_key* glk, lsa_key swk_dts, lsa_key swk_std,
                       void* stream) {
    return guard([&] {
        LSA_REQUIRE(b != nullptr && in != nullptr && out != nullptr && rlk != nullptr, "null argument");
        Bootstrap& bt = P(b, ctx, "null argument", "bootstrap plan belongs to another context");
        LSA_REQUIRE((swk_dts == nullptr) == (swk_std == nullptr), "swk_dts and swk_std come as a pair");
        const GaloisKeys g = G(n_glk, glk_elements, glk);
        bootstrap_run(bt, in, sin, out, sout, batch, K(rlk), g, swk_dts ? &K(swk_dts) : nullptr, swk_std ? &K(swk_std) : nullptr,
                      S(stream));
    });
}

// ---- CKKS linear transform (linear_transform.hip)
struct lsa_linear_transform_st : PlanHandle<LinearTransform> {};
int lsa_lt_create(lsa_context ctx, int level, int log_slots, int n_diag, const int* diag_index, const double* values,
                  double pt_scale, double bsgs_ratio, int double_hoist, void* stream, lsa_linear_transform* out) {
    return guard([&] {
        LSA_REQUIRE(out != nullptr, "null argument");
        Context& c = C(ctx);
        make_plan(out, c, lt_create(c, level, log_slots, n_diag, diag_index, values, pt_scale, bsgs_ratio, double_hoist != 0, S(stream)));
    });
}
void lsa_lt_destroy(lsa_linear_transform lt) { delete lt; }
int lsa_lt_info(lsa_linear_transform lt, int* level, int* period, int* n_diag, int* n1, int* rows, int* n_galois,
                int* double_hoist, double* pt_scale) {
    return guard([&] {
        const LinearTransform& p = P(lt, "null linear-transform handle");
        const BtMatrix& m = p.m;
        if (level) *level = m.level;
        if (period) *period = m.period;
        if (n_diag) *n_diag = (int)m.ks.size();
        if (n1) *n1 = m.naive ? 0 : m.n1;
        if (rows) *rows = m.rows;
        if (n_galois) *n_galois = (int)p.galois.size();
        if (double_hoist) *double_hoist = p.double_hoist ? 1 : 0;
        if (pt_scale) *pt_scale = m.pt_scale;
    });
}
int lsa_lt_diagonals(lsa_linear_transform lt, int* index_out, int capacity) {
    return guard([&] {
        LSA_REQUIRE(lt != nullptr && index_out != nullptr, "null argument");
        copy_out(lt->plan->m.ks, index_out, capacity, "buffer too small");
    });
}
int lsa_lt_galois_elements(lsa_linear_transform lt, uint64_t* out, int capacity) {
    return guard([&] {
        LSA_REQUIRE(lt != nullptr && out != nullptr, "null argument");
        copy_out(lt->plan->galois, out, capacity, "buffer too small");
    });
}
int lsa_lt_plaintext(lsa_linear_transform lt, int diag_pos, uint64_t* host_out, long long capacity_words) {
    return guard([&] {
        LSA_REQUIRE(lt != nullptr && host_out != nullptr, "null argument");
        const BtMatrix& m = lt->plan->m;
        LSA_REQUIRE(diag_pos >= 0 && diag_pos < (int)m.plains.size(), "diagonal position out of range");
        LSA_REQUIRE(capacity_words >= (long long)m.rows * lt->c->n, "buffer too small for the plaintext's rows (lsa_lt_info)");
        lt->c->use_device();
        LSA_HIP(hipMemcpy(host_out, m.plains[diag_pos], (size_t)m.rows * lt->c->n * sizeof(u64), hipMemcpyDeviceToHost));
    });
}
int lsa_ckks_linear_transform(lsa_context ctx, lsa_linear_transform lt, const uint64_t* in, uint64_t* out, int batch,
                              long long sin, long long sout, int rescale, int n_glk, const uint64_t* glk_elements,
                              const lsa_key* glk, void* stream) {
    return guard([&] {
        LinearTransform& p = P(lt, ctx, "null linear-transform handle", "linear-transform plan belongs to another context");
        if (batch <= 0) return;
        LSA_REQUIRE(in != nullptr && out != nullptr && n_glk >= 0 && (n_glk == 0 || (glk_elements && glk)), "linear transform: null argument");
        lt_run(p, in, sin, out, sout, batch, rescale != 0, G(n_glk, glk_elements, glk), S(stream));
    });
}
int lsa_lt_plan_rotations(int period, int n_diag, const int* diag_index, double bsgs_ratio, int* n1, int* rotations,
                          int capacity, int* count) {
    return guard([&] {
        LSA_REQUIRE(period >= 1 && (period & (period - 1)) == 0, "period must be a power of two");
        LSA_REQUIRE(n_diag >= 1 && diag_index != nullptr && bsgs_ratio >= 0, "bad argument");
        std::map<int, bool> seen;
        for (int i = 0; i < n_diag; i++) {
            const int k = ((diag_index[i] % period) + period) % period;
            LSA_REQUIRE(!seen.count(k), "diagonal index " + std::to_string(diag_index[i]) + " repeats another modulo the period");
            seen[k] = true;
        }
        std::vector<int> ks, rot;
        for (auto& kv : seen) ks.push_back(kv.first);
        const int split = lt_plan(ks, period, bsgs_ratio > 0 ? bsgs_ratio : 2.0, rot);
        if (n1) *n1 = split;
        if (count) *count = (int)rot.size();
        if (rotations) copy_out(rot, rotations, capacity, "buffer too small");
    });
}

// ---- BFV slot encoder and linear transform (bfv_encode.h, linear_transform.h)
int lsa_bfv_encode(lsa_context ctx, int level, int form, const uint64_t* values, uint64_t* out_dev, long long sout, int batch,
                   void* stream) {
    return guard([&] {
        LSA_REQUIRE(ctx != nullptr, "lsa_bfv_encode: null context");
        bfv_encode(C(ctx), level, form, values, out_dev, sout, batch, S(stream));
    });
}
// ---- BFV ring-t plaintext operands (bfv_plain.hip)
int lsa_bfv_addsub_plain(lsa_context ctx, int op, int level, const uint64_t* ct, long long sct, const uint64_t* pt, long long spt,
                         uint64_t* out, long long sout, int batch, void* stream) {
    return guard([&] {
        LSA_REQUIRE(ctx != nullptr, "lsa_bfv_addsub_plain: null context");
        bfv_addsub_plain(C(ctx), op, level, ct, sct, pt, spt, out, sout, batch, S(stream));
    });
}
int lsa_bfv_plain_lift(lsa_context ctx, int level, int form, const uint64_t* pt, long long spt, uint64_t* out, long long sout,
                       int batch, void* stream) {
    return guard([&] {
        LSA_REQUIRE(ctx != nullptr, "lsa_bfv_plain_lift: null context");
        bfv_plain_lift(C(ctx), level, form, pt, spt, out, sout, batch, S(stream));
    });
}
int lsa_bfv_mult_plain(lsa_context ctx, int level, const uint64_t* ct, long long sct, const uint64_t* pt, long long spt,
                       uint64_t* out, long long sout, int batch, void* stream) {
    return guard([&] {
        LSA_REQUIRE(ctx != nullptr, "lsa_bfv_mult_plain: null context");
        bfv_mult_plain(C(ctx), level, ct, sct, pt, spt, out, sout, batch, S(stream));
    });
}
struct lsa_bfv_lt_st : PlanHandle<BfvLinearTransform> {};
int lsa_bfv_lt_create(lsa_context ctx, int level, int period, int n_diag, const int* diag_index, const uint64_t* values,
                      double bsgs_ratio, void* stream, lsa_bfv_lt* out) {
    return guard([&] {
        LSA_REQUIRE(ctx != nullptr && out != nullptr, "lsa_bfv_lt_create: null argument");
        Context& c = C(ctx);
        make_plan(out, c, bfv_lt_create(c, level, period, n_diag, diag_index, values, bsgs_ratio, S(stream)));
    });
}
void lsa_bfv_lt_destroy(lsa_bfv_lt lt) { delete lt; }
int lsa_bfv_lt_info(lsa_bfv_lt lt, int* level, int* period, int* n_diag, int* n1, int* n_baby, int* n_giant, int* rows,
                    int* n_galois, int* n_moddown) {
    return guard([&] {
        const BfvLinearTransform& p = P(lt, "lsa_bfv_lt_info: null plan handle");
        const BtMatrix& m = p.m;
        if (level) *level = m.level;
        if (period) *period = m.period;
        if (n_diag) *n_diag = (int)m.ks.size();
        if (n1) *n1 = m.naive ? 0 : m.n1;
        if (n_baby) *n_baby = p.n_baby;
        if (n_giant) *n_giant = p.n_giant;
        if (rows) *rows = m.rows;
        if (n_galois) *n_galois = (int)p.galois.size();
        if (n_moddown) *n_moddown = p.n_moddown;
    });
}
int lsa_bfv_lt_diagonals(lsa_bfv_lt lt, int* index_out, int capacity) {
    return guard([&] {
        LSA_REQUIRE(lt != nullptr && index_out != nullptr, "lsa_bfv_lt_diagonals: null argument");
        copy_out(lt->plan->m.ks, index_out, capacity, "lsa_bfv_lt_diagonals: capacity: buffer too small");
    });
}
int lsa_bfv_lt_galois_elements(lsa_bfv_lt lt, uint64_t* out, int capacity) {
    return guard([&] {
        LSA_REQUIRE(lt != nullptr && out != nullptr, "lsa_bfv_lt_galois_elements: null argument");
        copy_out(lt->plan->galois, out, capacity, "lsa_bfv_lt_galois_elements: capacity: buffer too small");
    });
}
int lsa_bfv_lt_plaintext(lsa_bfv_lt lt, int diag_pos, uint64_t* host_out, long long capacity_words) {
    return guard([&] {
        LSA_REQUIRE(lt != nullptr && host_out != nullptr, "lsa_bfv_lt_plaintext: null argument");
        const BtMatrix& m = lt->plan->m;
        LSA_REQUIRE(diag_pos >= 0 && diag_pos < (int)m.plains.size(), "lsa_bfv_lt_plaintext: diagonal position out of range");
        LSA_REQUIRE(capacity_words >= (long long)m.rows * lt->c->n, "lsa_bfv_lt_plaintext: capacity: buffer too small for the plaintext's rows");
        lt->c->use_device();
        LSA_HIP(hipMemcpy(host_out, m.plains[diag_pos], (size_t)m.rows * lt->c->n * sizeof(u64), hipMemcpyDeviceToHost));
    });
}
int lsa_bfv_linear_transform(lsa_context ctx, lsa_bfv_lt lt, const uint64_t* in, uint64_t* out, int batch, long long sin,
                             long long sout, int n_keys, const uint64_t* galois_elements, const lsa_key* keys, void* stream) {
    return guard([&] {
        LSA_REQUIRE(ctx != nullptr, "lsa_bfv_linear_transform: null context");
        BfvLinearTransform& p = P(lt, ctx, "lsa_bfv_linear_transform: null plan handle", "lsa_bfv_linear_transform: the plan belongs to another context");
        LSA_REQUIRE(n_keys >= 0 && (n_keys == 0 || (galois_elements && keys)), "lsa_bfv_linear_transform: null key argument");
        bfv_lt_run(p, in, sin, out, sout, batch, G(n_keys, galois_elements, keys, "lsa_bfv_linear_transform"), S(stream));
    });
}

// ---- CKKS slot sum (slot_sum.h, slot_sum.hip slot_sum_run)
struct lsa_slot_sum_st : PlanHandle<SlotSum> {};
// the counts the plan and info entry points of both slot sums report (null: not asked for)
static void slot_sum_counts(const SlotSumPlanHost& p, int* count, int* radix, int* n_steps, int* n_keyswitch, int* n_moddown,
                            int* n_galois) {
    if (count) *count = p.count;
    if (radix) *radix = p.radix;
    if (n_steps) *n_steps = (int)p.steps.size();
    if (n_keyswitch) *n_keyswitch = p.n_keyswitch;
    if (n_moddown) *n_moddown = p.n_moddown;
    if (n_galois) *n_galois = (int)p.galois.size();
}
int lsa_slot_sum_plan(int n_ring, long long step, int count, int radix, int* n_steps, int* n_keyswitch, int* n_moddown,
                      int* rotations, int capacity, int* n_rot) {
    return guard([&] {
        const SlotSumPlanHost p = slot_sum_plan_checked(n_ring, step, count, radix);
        slot_sum_counts(p, nullptr, nullptr, n_steps, n_keyswitch, n_moddown, n_rot);   // (as many rotations as elements)
        if (rotations) copy_out(p.rotations, rotations, capacity, "slot sum: buffer too small for the rotations");
    });
}
int lsa_slot_sum_create(lsa_context ctx, int level, long long step, int count, int radix, lsa_slot_sum* out) {
    return guard([&] {
        LSA_REQUIRE(out != nullptr, "null argument");
        Context& c = C(ctx);
        make_plan(out, c, slot_sum_create(c, level, step, count, radix));
    });
}
void lsa_slot_sum_destroy(lsa_slot_sum plan) { delete plan; }
int lsa_slot_sum_info(lsa_slot_sum plan, int* level, int* count, int* radix, int* n_steps, int* n_keyswitch, int* n_moddown,
                      int* n_galois) {
    return guard([&] {
        const SlotSum& p = P(plan, "null slot-sum handle");
        if (level) *level = p.level;
        slot_sum_counts(p.plan, count, radix, n_steps, n_keyswitch, n_moddown, n_galois);
    });
}
int lsa_slot_sum_galois_elements(lsa_slot_sum plan, uint64_t* out, int capacity) {
    return guard([&] {
        LSA_REQUIRE(plan != nullptr && out != nullptr, "null argument");
        copy_out(plan->plan->plan.galois, out, capacity, "buffer too small");
    });
}
int lsa_slot_sum_set_multi_mac(lsa_slot_sum plan, int enable) {
    return guard([&] { P(plan, "null slot-sum handle").multi_mac = enable != 0; });
}
int lsa_ckks_slot_sum(lsa_context ctx, lsa_slot_sum plan, const uint64_t* in, uint64_t* out, int batch, long long sin,
                      long long sout, int n_keys, const uint64_t* galois_elements, const lsa_key* keys, void* stream) {
    return guard([&] {
        SlotSum& p = P(plan, ctx, "null slot-sum handle", "slot sum: the plan belongs to another context");
        LSA_REQUIRE(n_keys >= 0 && (n_keys == 0 || (galois_elements && keys)), "slot sum: null argument");
        slot_sum_run(p, in, sin, out, sout, batch, G(n_keys, galois_elements, keys, "lsa_ckks_slot_sum"), S(stream));
    });
}

// ---- BFV slot sum (slot_sum.h, slot_sum.hip bfv_slot_sum_run)
struct lsa_bfv_slot_sum_st : PlanHandle<BfvSlotSum> {};
int lsa_bfv_slot_sum_plan(int n_ring, long long step, int count, int radix, int rows, int* n_steps, int* n_keyswitch, int* n_moddown,
                          uint64_t* galois_elements, int capacity, int* n_galois) {
    return guard([&] {
        const SlotSumPlanHost p = bfv_slot_sum_plan_checked(n_ring, step, count, radix, rows);
        slot_sum_counts(p, nullptr, nullptr, n_steps, n_keyswitch, n_moddown, n_galois);
        if (galois_elements)
            copy_out(p.galois, galois_elements, capacity, "lsa_bfv_slot_sum_plan: capacity: buffer too small for the Galois elements");
    });
}
int lsa_bfv_slot_sum_create(lsa_context ctx, int level, long long step, int count, int radix, int rows, lsa_bfv_slot_sum_handle* out) {
    return guard([&] {
        LSA_REQUIRE(out != nullptr, "lsa_bfv_slot_sum_create: null argument");
        Context& c = C(ctx);
        make_plan(out, c, bfv_slot_sum_create(c, level, step, count, radix, rows));
    });
}
void lsa_bfv_slot_sum_destroy(lsa_bfv_slot_sum_handle plan) { delete plan; }
int lsa_bfv_slot_sum_info(lsa_bfv_slot_sum_handle plan, int* level, int* count, int* radix, int* rows, int* n_steps, int* n_keyswitch,
                          int* n_moddown, int* n_galois, int* gather) {
    return guard([&] {
        const BfvSlotSum& p = P(plan, "lsa_bfv_slot_sum_info: null plan handle");
        if (level) *level = p.level;
        if (rows) *rows = p.plan.rows;
        slot_sum_counts(p.plan, count, radix, n_steps, n_keyswitch, n_moddown, n_galois);
        if (gather) *gather = p.gather ? 1 : 0;
    });
}
int lsa_bfv_slot_sum_galois_elements(lsa_bfv_slot_sum_handle plan, uint64_t* out, int capacity) {
    return guard([&] {
        LSA_REQUIRE(plan != nullptr && out != nullptr, "lsa_bfv_slot_sum_galois_elements: null argument");
        copy_out(plan->plan->plan.galois, out, capacity, "lsa_bfv_slot_sum_galois_elements: capacity: buffer too small");
    });
}
int lsa_bfv_slot_sum_set_gather(lsa_bfv_slot_sum_handle plan, int enable) {
    return guard([&] {
        BfvSlotSum& p = P(plan, "lsa_bfv_slot_sum_set_gather: null plan handle");
        LSA_REQUIRE(!enable || p.c.logn <= LSA_PERM_LDS_MAX_LOGN,
                    "lsa_bfv_slot_sum_set_gather: enable: the gathering tail stages a limb in LDS and needs N <= 2^14");
        p.gather = enable != 0;
    });
}
int lsa_bfv_slot_sum(lsa_context ctx, lsa_bfv_slot_sum_handle plan, const uint64_t* in, uint64_t* out, int batch, long long sin,
                     long long sout, int n_keys, const uint64_t* galois_elements, const lsa_key* keys, void* stream) {
    return guard([&] {
        BfvSlotSum& p = P(plan, ctx, "lsa_bfv_slot_sum: null plan handle", "lsa_bfv_slot_sum: the plan belongs to another context");
        LSA_REQUIRE(n_keys >= 0 && (n_keys == 0 || (galois_elements && keys)), "lsa_bfv_slot_sum: null key argument");
        bfv_slot_sum_run(p, in, sin, out, sout, batch, G(n_keys, galois_elements, keys, "lsa_bfv_slot_sum"), S(stream));
    });
}

// ---- BFV oblivious expansion (bfv_expand.h, bfv_expand.hip bfv_expand_run)
struct lsa_bfv_expand_st : PlanHandle<BfvExpand> {};
static void expand_counts(const BfvExpandPlanHost& p, int* count, int* n_levels, int* n_keyswitch, int* n_galois) {
    if (count) *count = p.count;
    if (n_levels) *n_levels = (int)p.levels.size();
    if (n_keyswitch) *n_keyswitch = p.n_keyswitch;
    if (n_galois) *n_galois = (int)p.galois.size();
}
int lsa_bfv_expand_plan(int n_ring, int count, int* n_levels, int* n_keyswitch, uint64_t* galois_elements, int capacity, int* n_galois) {
    return guard([&] {
        const BfvExpandPlanHost p = bfv_expand_plan_checked(n_ring, count);
        expand_counts(p, nullptr, n_levels, n_keyswitch, n_galois);
        if (galois_elements)
            copy_out(p.galois, galois_elements, capacity, "lsa_bfv_expand_plan: capacity: buffer too small for the Galois elements");
    });
}
int lsa_bfv_expand_create(lsa_context ctx, int level, int count, lsa_bfv_expand_handle* out) {
    return guard([&] {
        LSA_REQUIRE(out != nullptr, "lsa_bfv_expand_create: null argument");
        Context& c = C(ctx);
        make_plan(out, c, bfv_expand_create(c, level, count));
    });
}
void lsa_bfv_expand_destroy(lsa_bfv_expand_handle plan) { delete plan; }
int lsa_bfv_expand_info(lsa_bfv_expand_handle plan, int* level, int* count, int* n_levels, int* n_keyswitch, int* n_galois, int* gather) {
    return guard([&] {
        const BfvExpand& p = P(plan, "lsa_bfv_expand_info: null plan handle");
        if (level) *level = p.level;
        expand_counts(p.plan, count, n_levels, n_keyswitch, n_galois);
        if (gather) *gather = p.gather ? 1 : 0;
    });
}
int lsa_bfv_expand_galois_elements(lsa_bfv_expand_handle plan, uint64_t* out, int capacity) {
    return guard([&] {
        LSA_REQUIRE(plan != nullptr && out != nullptr, "lsa_bfv_expand_galois_elements: null argument");
        copy_out(plan->plan->plan.galois, out, capacity, "lsa_bfv_expand_galois_elements: capacity: buffer too small");
    });
}
int lsa_bfv_expand_set_gather(lsa_bfv_expand_handle plan, int enable) {
    return guard([&] {
        BfvExpand& p = P(plan, "lsa_bfv_expand_set_gather: null plan handle");
        LSA_REQUIRE(!enable || p.c.logn <= LSA_PERM_LDS_MAX_LOGN,
                    "lsa_bfv_expand_set_gather: enable: the gathering tail stages a limb in LDS and needs N <= 2^14");
        p.gather = enable != 0;
    });
}
int lsa_bfv_expand(lsa_context ctx, lsa_bfv_expand_handle plan, const uint64_t* in, long long sin, uint64_t* out, long long sout,
                   long long s_index, int batch, int n_keys, const uint64_t* galois_elements, const lsa_key* keys, void* stream) {
    return guard([&] {
        BfvExpand& p = P(plan, ctx, "lsa_bfv_expand: null plan handle", "lsa_bfv_expand: the plan belongs to another context");
        LSA_REQUIRE(n_keys >= 0 && (n_keys == 0 || (galois_elements && keys)), "lsa_bfv_expand: null key argument");
        bfv_expand_run(p, in, sin, out, sout, s_index, batch, G(n_keys, galois_elements, keys, "lsa_bfv_expand"), S(stream));
    });
}
int lsa_bfv_mul_monomial(lsa_context ctx, int level, int polys, long long exponent, const uint64_t* in, uint64_t* out, int batch,
                         long long sin, long long sout, void* stream) {
    return guard([&] { bfv_mul_monomial(C(ctx), level, polys, exponent, in, out, batch, sin, sout, S(stream)); });
}

// ---- BFV coefficient packing (bfv_pack.h, bfv_pack.hip bfv_pack_run)
struct lsa_bfv_pack_st : PlanHandle<BfvPack> {};
static void pack_counts(const BfvPackPlanHost& p, int* count, int* trace, int* n_levels, int* n_trace_levels, int* n_keyswitch, int* n_galois) {
    if (count) *count = p.count;
    if (trace) *trace = p.trace;
    if (n_levels) *n_levels = (int)p.levels.size();
    if (n_trace_levels) *n_trace_levels = (int)p.trace_g.size();
    if (n_keyswitch) *n_keyswitch = p.n_keyswitch;
    if (n_galois) *n_galois = (int)p.galois.size();
}
int lsa_bfv_pack_plan(int n_ring, int count, int trace, int* n_levels, int* n_trace_levels, int* n_keyswitch, uint64_t* galois_elements,
                      int capacity, int* n_galois) {
    return guard([&] {
        const BfvPackPlanHost p = bfv_pack_plan_checked(n_ring, count, trace);
        pack_counts(p, nullptr, nullptr, n_levels, n_trace_levels, n_keyswitch, n_galois);
        if (galois_elements)
            copy_out(p.galois, galois_elements, capacity, "lsa_bfv_pack_plan: capacity: buffer too small for the Galois elements");
    });
}
int lsa_bfv_pack_create(lsa_context ctx, int level, int count, int trace, lsa_bfv_pack_handle* out) {
    return guard([&] {
        LSA_REQUIRE(out != nullptr, "lsa_bfv_pack_create: null argument");
        Context& c = C(ctx);
        make_plan(out, c, bfv_pack_create(c, level, count, trace));
    });
}
void lsa_bfv_pack_destroy(lsa_bfv_pack_handle plan) { delete plan; }
int lsa_bfv_pack_info(lsa_bfv_pack_handle plan, int* level, int* count, int* trace, int* n_levels, int* n_trace_levels, int* n_keyswitch,
                      int* n_galois, int* gather) {
    return guard([&] {
        const BfvPack& p = P(plan, "lsa_bfv_pack_info: null plan handle");
        if (level) *level = p.level;
        pack_counts(p.plan, count, trace, n_levels, n_trace_levels, n_keyswitch, n_galois);
        if (gather) *gather = p.gather ? 1 : 0;
    });
}
int lsa_bfv_pack_galois_elements(lsa_bfv_pack_handle plan, uint64_t* out, int capacity) {
    return guard([&] {
        LSA_REQUIRE(plan != nullptr && out != nullptr, "lsa_bfv_pack_galois_elements: null argument");
        copy_out(plan->plan->plan.galois, out, capacity, "lsa_bfv_pack_galois_elements: capacity: buffer too small");
    });
}
int lsa_bfv_pack_set_gather(lsa_bfv_pack_handle plan, int enable) {
    return guard([&] {
        BfvPack& p = P(plan, "lsa_bfv_pack_set_gather: null plan handle");
        LSA_REQUIRE(!enable || p.c.logn <= LSA_PERM_LDS_MAX_LOGN,
                    "lsa_bfv_pack_set_gather: enable: the gathering tail stages a limb in LDS and needs N <= 2^14");
        p.gather = enable != 0;
    });
}
int lsa_bfv_pack(lsa_context ctx, lsa_bfv_pack_handle plan, uint64_t* in, long long sin, long long s_index, uint64_t* out, long long sout,
                 int batch, int n_keys, const uint64_t* galois_elements, const lsa_key* keys, void* stream) {
    return guard([&] {
        BfvPack& p = P(plan, ctx, "lsa_bfv_pack: null plan handle", "lsa_bfv_pack: the plan belongs to another context");
        LSA_REQUIRE(n_keys >= 0 && (n_keys == 0 || (galois_elements && keys)), "lsa_bfv_pack: null key argument");
        bfv_pack_run(p, in, sin, s_index, out, sout, batch, G(n_keys, galois_elements, keys, "lsa_bfv_pack"), S(stream));
    });
}

// ---- BFV external product, CMux and select by an encrypted index (bfv_select.h, bfv_select.hip)
struct lsa_bfv_select_st : PlanHandle<BfvSelect> {};
static const Key* KP(lsa_key k) { return k != nullptr && k->key.data != nullptr ? &k->key : nullptr; }   // null: the runner names the argument
int lsa_bfv_external_product(lsa_context ctx, int level, const uint64_t* ct, long long sct, lsa_key r0, lsa_key r1, const uint64_t* base,
                             long long sbase, uint64_t* out, long long sout, int batch, void* stream) {
    return guard([&] { bfv_external_product(C(ctx), level, ct, sct, KP(r0), KP(r1), base, sbase, out, sout, batch, S(stream)); });
}
int lsa_bfv_cmux(lsa_context ctx, int level, const uint64_t* c0, long long s0, const uint64_t* c1, long long s1, lsa_key r0, lsa_key r1,
                 uint64_t* out, long long sout, int batch, void* stream) {
    return guard([&] { bfv_cmux(C(ctx), level, c0, s0, c1, s1, KP(r0), KP(r1), out, sout, batch, S(stream)); });
}
int lsa_bfv_select_plan(int count, int* n_levels, int* n_products) {
    return guard([&] {
        const BfvSelectPlanHost p = bfv_select_plan_checked(count);
        if (n_levels) *n_levels = (int)p.levels.size();
        if (n_products) *n_products = p.n_products;
    });
}
int lsa_bfv_select_create(lsa_context ctx, int level, int count, lsa_bfv_select_handle* out) {
    return guard([&] {
        LSA_REQUIRE(out != nullptr, "lsa_bfv_select_create: null argument");
        Context& c = C(ctx);
        make_plan(out, c, bfv_select_create(c, level, count));
    });
}
void lsa_bfv_select_destroy(lsa_bfv_select_handle plan) { delete plan; }
int lsa_bfv_select_info(lsa_bfv_select_handle plan, int* level, int* count, int* n_levels, int* n_products) {
    return guard([&] {
        const BfvSelect& p = P(plan, "lsa_bfv_select_info: null plan handle");
        if (level) *level = p.level;
        if (count) *count = p.plan.count;
        if (n_levels) *n_levels = (int)p.plan.levels.size();
        if (n_products) *n_products = p.plan.n_products;
    });
}
int lsa_bfv_select(lsa_context ctx, lsa_bfv_select_handle plan, uint64_t* in, long long sin, long long s_index, uint64_t* out, long long sout,
                   int batch, int n_sel, const lsa_key* r0s, const lsa_key* r1s, void* stream) {
    return guard([&] {
        BfvSelect& p = P(plan, ctx, "lsa_bfv_select: null plan handle", "lsa_bfv_select: the plan belongs to another context");
        LSA_REQUIRE(n_sel >= 0 && (n_sel == 0 || (r0s && r1s)), "lsa_bfv_select: r0s / r1s is null");
        std::vector<const Key*> k0(n_sel), k1(n_sel);
        for (int j = 0; j < n_sel; j++) k0[j] = KP(r0s[j]), k1[j] = KP(r1s[j]);
        bfv_select_run(p, in, sin, s_index, out, sout, batch, n_sel, k0.data(), k1.data(), S(stream));
    });
}

// ---- BFV plaintext matrix x ciphertext vector (bfv_matvec.h, bfv_matvec.hip)
int lsa_bfv_matvec_plain_mul(lsa_context ctx, int level, int rows, int cols, const uint64_t* cts, long long s_col, long long sct,
                             const uint64_t* pts, long long s_prow, long long s_pcol, long long spt, const uint64_t* partial,
                             long long s_partial_row, long long spartial, uint64_t* out, long long s_row, long long sout, int batch,
                             void* stream) {
    return guard([&] {
        const BfvMatvecLayout a{cts, s_col, sct, pts, s_prow, s_pcol, spt, partial, s_partial_row, spartial, out, s_row, sout};
        bfv_matvec_plain_mul(C(ctx), level, rows, cols, a, batch, S(stream));
    });
}
int lsa_bfv_matvec_plan(int n_ring, int level_limbs, int rows, int cols, int batch, size_t workspace_bytes, int* row_block, int* col_block,
                        int* n_launches, size_t* workspace_rows) {
    return guard([&] {
        const BfvMatvecPlanHost p = bfv_matvec_plan_checked(n_ring, level_limbs, rows, cols, batch, workspace_bytes, 0, 0);
        if (row_block) *row_block = p.row_block;
        if (col_block) *col_block = p.col_block;
        if (n_launches) *n_launches = p.n_launches;
        if (workspace_rows) *workspace_rows = p.workspace_rows;
    });
}
int lsa_set_bfv_matvec_block(lsa_context ctx, int row_block, int col_block) {
    return guard([&] {
        LSA_REQUIRE(bfv_matvec_row_block_legal(row_block), "lsa_set_bfv_matvec_block: row_block must be 0, 1, 2, 4 or 8");
        LSA_REQUIRE(col_block >= 0, "lsa_set_bfv_matvec_block: col_block must be >= 0");
        Context& c = C(ctx);
        c.matvec_row_block = row_block;
        c.matvec_col_block = col_block;
    });
}

// ---- CKKS polynomial evaluation (poly_eval.hip)
struct lsa_polynomial_st : PlanHandle<Polynomial> {};
int lsa_poly_plan(int basis, int n_coef, const double* coef, int log_baby, int level_in, int with_interval, int* depth,
                  int* log_baby_out, int* n_mult, int* n_leaves, int* n_leaf_launches) {
    return guard([&] { poly_plan(basis, n_coef, coef, log_baby, level_in, with_interval != 0, depth, log_baby_out, n_mult, n_leaves, n_leaf_launches); });
}
int lsa_poly_create(lsa_context ctx, int basis, int n_coef, const double* coef, double a, double b, int level_in, double scale_in,
                    double scale_out, int log_baby, lsa_polynomial* out) {
    return guard([&] {
        LSA_REQUIRE(out != nullptr, "null argument");
        Context& c = C(ctx);
        make_plan(out, c, poly_create(c, basis, n_coef, coef, a, b, level_in, scale_in, scale_out, log_baby, nullptr));
    });
}
void lsa_poly_destroy(lsa_polynomial p) { delete p; }
int lsa_poly_info(lsa_polynomial p, int* level_in, int* level_out, double* scale_out, int* depth, int* log_baby, int* n_mult,
                  int* n_leaves, int* n_leaf_launches, int* n_constants) {
    return guard([&] {
        const Polynomial& poly = P(p, "null polynomial handle");
        if (level_in) *level_in = poly.level_in;
        if (level_out) *level_out = poly.level_out;
        if (scale_out) *scale_out = poly.scale_out;
        if (depth) *depth = poly.depth;
        if (log_baby) *log_baby = poly.st.log_baby;
        if (n_mult) *n_mult = poly.st.mults;
        if (n_leaves) *n_leaves = (int)poly.st.jobs.size();
        if (n_leaf_launches) *n_leaf_launches = (int)poly.st.groups.size();
        if (n_constants) *n_constants = (int)poly.constants.size();
    });
}
int lsa_poly_constants(lsa_polynomial p, long long* out, int capacity) {
    return guard([&] {
        LSA_REQUIRE(p != nullptr && out != nullptr, "null argument");
        copy_out(p->plan->constants, out, capacity, "buffer too small");
    });
}
int lsa_ckks_poly_eval(lsa_context ctx, lsa_polynomial p, const uint64_t* in, uint64_t* out, int batch, long long sin,
                       long long sout, lsa_key rlk, void* stream) {
    return guard([&] {
        Polynomial& poly = P(p, ctx, "null polynomial handle", "poly: the plan belongs to another context");
        if (batch <= 0) return;
        LSA_REQUIRE(in != nullptr && out != nullptr, "poly: null argument");
        LSA_REQUIRE(rlk != nullptr && rlk->key.data != nullptr, "poly: the relinearisation key is missing");
        poly_run(poly, in, sin, out, sout, batch, K(rlk), S(stream));
    });
}

// ---- BFV polynomial evaluation and constant operands (bfv_poly.hip; the planner is bfv_poly.h's and needs no device)
struct lsa_bfv_polynomial_st : PlanHandle<BfvPolynomial> {};
static void bfv_poly_counts(const BfvPolyPlan& p, int* log_baby, int* depth, int* n_mult, int* n_leaves, int* n_leaf_launches,
                            int* n_pairs) {
    if (log_baby) *log_baby = p.log_baby;
    if (depth) *depth = p.depth;
    if (n_mult) *n_mult = p.n_mult;
    if (n_leaves) *n_leaves = p.n_leaves;
    if (n_leaf_launches) *n_leaf_launches = p.n_leaf_launches;
    if (n_pairs) *n_pairs = p.n_pairs;
}
int lsa_bfv_poly_plan(uint64_t t, int n_coef, const uint64_t* coef, int log_baby, int* log_baby_out, int* depth, int* n_mult,
                      int* n_leaves, int* n_leaf_launches, int* n_pairs) {
    return guard([&] {
        bfv_poly_counts(bfv_poly_plan_checked(t, n_coef, coef, log_baby), log_baby_out, depth, n_mult, n_leaves, n_leaf_launches, n_pairs);
    });
}
int lsa_bfv_poly_create(lsa_context ctx, int level, int n_coef, const uint64_t* coef, int log_baby, void* stream,
                        lsa_bfv_polynomial* out) {
    return guard([&] {
        LSA_REQUIRE(out != nullptr, "bfv_poly: null argument (out)");
        LSA_REQUIRE(ctx != nullptr, "bfv_poly: null context");
        Context& c = C(ctx);
        make_plan(out, c, bfv_poly_create(c, level, n_coef, coef, log_baby, S(stream)), bfv_poly_destroy);
    });
}
void lsa_bfv_poly_destroy(lsa_bfv_polynomial p) { delete p; }
int lsa_bfv_poly_info(lsa_bfv_polynomial p, int* level, int* n_coef, int* log_baby, int* depth, int* n_mult, int* n_leaves,
                      int* n_leaf_launches, int* n_pairs) {
    return guard([&] {
        const BfvPolynomial& poly = P(p, "bfv_poly: null plan handle");
        if (level) *level = bfv_poly_level(poly);
        if (n_coef) *n_coef = bfv_poly_plan_of(poly).n_coef;
        bfv_poly_counts(bfv_poly_plan_of(poly), log_baby, depth, n_mult, n_leaves, n_leaf_launches, n_pairs);
    });
}
int lsa_bfv_poly_eval(lsa_context ctx, lsa_bfv_polynomial p, const uint64_t* in, uint64_t* out, int batch, long long sin,
                      long long sout, lsa_key rlk, void* stream) {
    return guard([&] {
        LSA_REQUIRE(ctx != nullptr, "bfv_poly: null context");
        BfvPolynomial& poly = P(p, ctx, "bfv_poly: null plan handle", "bfv_poly: the plan belongs to another context");
        bfv_poly_run(poly, in, sin, out, sout, batch, rlk ? &rlk->key : nullptr, S(stream));
    });
}
int lsa_bfv_affine_const(lsa_context ctx, int level, const uint64_t* ct, long long sct, uint64_t k, uint64_t c, uint64_t* out,
                         long long sout, int batch, void* stream) {
    return guard([&] {
        LSA_REQUIRE(ctx != nullptr, "lsa_bfv_affine_const: null context");
        bfv_affine_const(C(ctx), level, ct, sct, k, c, out, sout, batch, S(stream));
    });
}

int lsa_set_ntt_chunk_mib(lsa_context ctx, int mib) {
    return guard([&] {
        LSA_REQUIRE(mib >= 0, "chunk size must be >= 0");
        C(ctx).ntt_chunk_mib = mib;
    });
}
int lsa_set_bfv_dot_chunk(lsa_context ctx, int pairs) {
    return guard([&] {
        LSA_REQUIRE(pairs >= 0, "chunk size must be >= 0");
        C(ctx).bfv_dot_chunk = pairs;
    });
}
int lsa_set_fp64_ntt(lsa_context ctx, int enable) {
    return guard([&] { C(ctx).fp64_ntt = enable ? 1 : 0; });
}
int lsa_set_tile_batch(lsa_context ctx, int tile_batch) {
    return guard([&] {
        LSA_REQUIRE(tile_batch >= 0, "tile_batch must be >= 0");
        C(ctx).tile_batch = tile_batch;
    });
}
int lsa_probe_copy(lsa_context ctx, uint64_t* dst, const uint64_t* src, size_t n_u64, void* stream) {
    return guard([&] {
        C(ctx);
        launch_probe_copy(dst, src, n_u64, S(stream));
    });
}
int lsa_probe_mulhi(lsa_context ctx, uint64_t* buf, size_t n_u64, int iters, void* stream) {
    return guard([&] {
        C(ctx);
        launch_probe_mulhi(buf, n_u64, iters, S(stream));
    });
}

}  // extern "C"
