// lsa_internal.h — context, device tables, workspace and launcher declarations (host side, C++).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/lattisense_amd.h"
#include "bfv_expand.h"
#include "bfv_pack.h"
#include "bfv_matvec.h"
#include "bfv_select.h"
#include "galois_keys.h"
#include "ntt_plan.h"
#include "ntt_chunk.h"
#include "plain_ops.h"
#include "slot_sum.h"
#include "switches.h"
#include "tables.h"

namespace lsa {

void set_last_error(const std::string& m);

#define LSA_HIP(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess)                                                                             \
            throw lsa::Error(_e == hipErrorNoDevice || _e == hipErrorInvalidDevice ? LSA_ERR_NO_DEVICE    \
                                                                                   : LSA_ERR_HIP,        \
                             std::string(#expr) + ": " + hipGetErrorString(_e));                          \
    } while (0)

#define LSA_REQUIRE(cond, msg)                                   \
    do {                                                         \
        if (!(cond)) throw lsa::Error(LSA_ERR_ARG, (msg));       \
    } while (0)

// A launch with more than 64 KiB of dynamic LDS: the kernel opts in, once per kernel instance (the template argument keeps the
// flags apart) AND device (the attribute is per device; bit d: done on device d).  limit_bytes: what the instance may ask for
template <auto Kernel>
void raise_dynamic_lds(size_t lds_bytes, int limit_bytes) {
    if (lds_bytes <= 65536) return;
    static std::atomic<unsigned long long> raised{0};
    int dev = 0;
    LSA_HIP(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (raised.load(std::memory_order_acquire) & bit) return;
    LSA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, limit_bytes));
    raised.fetch_or(bit, std::memory_order_release);
}

// ---------------------------------------------------------------- exact RNS base conversion plan (device constants)
// k_baseconv (two points per thread, optional 29-bit SPLIT accumulate) takes up to LSA_BC_NARROW_SRC sources; wider
// conversions (the BFV multiply at N = 2^16: 24 Q limbs to 24 auxiliary limbs and back) run k_baseconv_wide, up to
// LSA_BC_MAX_SRC sources
#define LSA_BC_NARROW_SRC 16
#define LSA_BC_MAX_SRC 32
#define LSA_BC_MAX_DST 64

struct BaseConvConsts {
    int ns, nd, centered;
    int src_mod[LSA_BC_MAX_SRC];
    int dst_mod[LSA_BC_MAX_DST];
    u64 shat_inv_m[LSA_BC_MAX_SRC];                 // (S/q_i)^-1 mod q_i, Montgomery form
    u64 half_src[LSA_BC_MAX_SRC];                   // floor(S/2) mod q_i
    double qf[LSA_BC_MAX_SRC];                      // (double) q_i
    double rf[LSA_BC_MAX_SRC];                      // RN(1 / qf): reciprocal for the 3-operation exact division
    u64 shat_m[LSA_BC_MAX_DST][LSA_BC_MAX_SRC];     // (S/q_i) mod p_j, Montgomery form
    u64 vs[LSA_BC_MAX_DST][LSA_BC_MAX_SRC + 1];     // v*S mod p_j, v = 0..ns (v <= ns: a sum of ns quotients each <= 1)
    u64 half_dst[LSA_BC_MAX_DST];                   // floor(S/2) mod p_j
    // every source and target modulus below 2^58: shat_m split into 29-bit halves for the carry-free accumulate of
    // k_baseconv<.., SPLIT> (shat_m[j][i] = hi * 2^29 + lo)
    int split29;
    u32 shat_lo[LSA_BC_MAX_DST][LSA_BC_MAX_SRC];
    u32 shat_hi[LSA_BC_MAX_DST][LSA_BC_MAX_SRC];
    u32 shat_sum[LSA_BC_MAX_DST][LSA_BC_MAX_SRC];      // lo + hi: the middle column as ONE product (y0 + y1)(w0 + w1) - y0 w0 - y1 w1
    // the output corrections -v*S - [centred] floor(S/2), Montgomery form, as ONE addend v * corr_a + corr_b (< 17 * 2^58: SPLIT
    // runs only in k_baseconv, ns <= 16, v <= ns) of the 128-bit sum ahead of its single REDC: corr_a = (-S) * 2^64 mod p_j, corr_b = (-floor(S/2)) * 2^64 mod p_j or 0
    u64 corr_a[LSA_BC_MAX_DST], corr_b[LSA_BC_MAX_DST];
};

struct BaseConvPlan {
    BaseConvConsts* dev = nullptr;
    int ns = 0, nd = 0;
    bool split29 = false;
};

enum ProfKind { PROF_NTT = 0, PROF_BASECONV = 1, PROF_KSMAC = 2, PROF_TENSOR = 3, PROF_ELEMWISE = 4, LSA_PROF_KINDS = 5 };

struct Key {
    u64* data = nullptr;   // device, compact order [beta][2][klvl+1+np][N], NTT domain, MONTGOMERY form
    int level = 0;
    bool owned = true;
    // the same key as plain integer-valued doubles, same layout, valid for the limbs of the FP64 engine (q < 2^47) only: the
    // operand of the key MAC that is fused into the extension transform's second pass (k_ntt_r16_ksmac); null = not built
    // (that path is then not taken).  Lives and dies with `data` (same allocation, or owned by the key's holder).
    const double* fp = nullptr;
};

using GaloisKeys = GaloisKeySet<Key>;   // the Galois keys of one call (galois_keys.h)

struct Context {
    int algo, n, logn, nq, np, nmul, nmod, device;
    u64 t;
    HostTables T;
    NttPlan plan;        // 4096-point tiles: one pass up to N = 2^12, two passes above
    NttPlan plan_wide;   // N = 2^13 / 2^14 only: the whole limb in one 512 / 1024-thread workgroup, one pass
    int wide_mode = 2;   // LSA_NTT_WIDE: 0 never, 1 always, unset = per launch (launch_ntt)
    ModDev* d_mods = nullptr;
    u64* d_psi = nullptr;
    u64* d_psiinv = nullptr;
    u64* d_scale = nullptr;
    double* d_psi_d = nullptr;      // FP64-engine copies of the twiddle tables
    double* d_psiinv_d = nullptr;
    u64* d_psi_w = nullptr;         // the same four tables in the order of plan_wide (N = 2^13 / 2^14 only)
    u64* d_psiinv_w = nullptr;
    double* d_psi_d_w = nullptr;
    double* d_psiinv_d_w = nullptr;
    double* d_scale_d = nullptr;
    int fp64_ntt = 1;               // use the FP64 butterfly engine for limbs with q < 2^47
    int tile_batch = 0;
    int fp_raw = 1;                 // FP64-engine limbs cross between the two NTT passes as doubles (LSA_NTT_FP_RAW=0: canonical u64)
    int rgsw_pair_mac = 1;          // external product: both gadget products in ONE k_ks_mac_pair launch (key_switch.hip external_product); 0: two launch_ks_mac
    int matvec_row_block = 0, matvec_col_block = 0;   // lsa_set_bfv_matvec_block: forced blocks of bfv_matvec_plain_mul, 0 = the plan's own (bfv_matvec.h)
    int modup_lift = 1;            // single-limb key-switch digits lifted by the extension transform's load (key_switch.hip KsTile::decompose)
    int fuse_tails = 1;             // ModDown / rescale element-wise tails fused into the NTT load/store phases
    int ks_tail_in_mac = 1;         // merged rescale tail finished inside the fused key MAC (key_switch.h KsTile::plan_tail): 0 never,
                                    // 1 where the second pass has eight stages (the measured shape), 2 wherever the shape allows
    int rescale_head_in_conv = 1;   // merged rescale head formed inside ModDown's base conversion (key_switch.hip ks_head_in_conv): 0 never,
                                    // 1 rings with N >= 2^16 (the measured shape), 2 every ring
    int dual_stream = 0;            // 1: overlap alternate tiles of an operator on an auxiliary stream (+5% throughput,
                                    // but per-kernel timings then include the co-running kernel; off for clean accounting)
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    void fork_aux(hipStream_t s);   // aux stream waits for everything enqueued on s so far
    void join_aux(hipStream_t s);   // s waits for everything enqueued on the aux stream
    unsigned long long* ntt_diag = nullptr;   // device buffer for LSA_NTT_DIAG_STAMPS builds (8 stamps per workgroup)
    int ntt_chunk_mib = 0;          // >0: two-pass NTTs run pass A+B per chunk of this many MiB (Infinity-Cache reuse)
    int bfv_dot_chunk = 0;          // >0: pairs extended per k_tensor_sum launch of bfv_mult_sum / bfv_dot (0: LSA_BFV_DOT_CHUNK)

    // sampled HIP-event timing of kernel launches (bench.py roofline leg); off unless lsa_profile_begin was called
    struct ProfSample {
        hipEvent_t e0, e1;
        int kid;
        double bytes;
        double bytes_primary;   // the kind's own function only (a fused launch also does another kernel's work: `bytes` counts both)
    };
    bool prof_on = false;
    int prof_stride = 1;
    long long prof_launched[LSA_PROF_KINDS] = {0};
    std::vector<ProfSample> prof_samples;
    std::vector<hipEvent_t> prof_pool;

    std::mutex mu;
    std::map<std::string, BaseConvPlan> bconv;       // device copies, keyed by "c|src..|dst.."
    std::map<u64, u32*> perm_ntt;                   // galois element -> device gather table (NTT domain)
    std::map<u64, u32*> perm_coeff;                 // galois element -> device scatter table with sign bit
    std::map<std::string, u64*> consts;             // misc per-level device constant vectors
    // where NTT(X^(N/2)) is +I_j and where -I_j (ops.hip cconst_selector: measured once per context with launch_ntt, checked
    // on the host): the word at point x of limb j is I[j] when bit `bit` of x equals `pol`, q_j - I[j] otherwise
    struct CconstSelector {
        int bit = -1, pol = 0;
        std::vector<u64> I;   // [nq] psi_j^(N/2)
    } cconst;

    std::shared_ptr<const BfvEncodeTables> bfv_enc;   // the slot encoder's host tables (bfv_encode.h), built on first use

    // workspace arena: grows on demand, reused across calls (single in-flight operator per context)
    u64* ws = nullptr;
    size_t ws_words = 0;

    Context(int algo_, int n_, const u64* q, int nq_, const u64* p, int np_, u64 t_, int device_);
    ~Context();
    void use_device() const { LSA_HIP(hipSetDevice(device)); }
    u64* workspace(size_t words, hipStream_t s);
    u64* ws2 = nullptr;   // second arena: operator-to-operator intermediates of composed entry points
    size_t ws2_words = 0;
    u64* workspace2(size_t words, hipStream_t s);
    int p_mod(int i) const { return nq + i; }
    int aux_mod(int i) const { return nq + np + i; }
    int qp_mod(int L, int tl) const { return tl < L ? tl : p_mod(tl - L); }   // row tl of Q_level u P (L = level + 1) -> modulus
    bool fp_engine(int mod) const { return fp64_ntt && (T.mod[mod] >> LSA_FP64_MAX_BITS) == 0; }   // FP64 butterflies serve it
    // pinv_scaled: the outputs of every target but the last are multiplied by P^-1 mod p_j (merged ModDown + rescale)
    // rescale_head (with pinv_scaled, centred): the plan of k_baseconv<.., HEAD> -- those outputs also lose h = (q_l - 1) / 2,
    // q_l the last target's modulus, which the kernel's extra term c = t + h brings in (launch_baseconv's `head`)
    // fold: element-wise steps on either side of a conversion folded into its constants (both linear, so the residues are the
    // ones the separate steps give): src_pre[i] multiplies source limb i BEFORE the conversion (the centring offset and
    // (S/q_i)^-1 absorb it), dst_scale[j] multiplies target j's output; `tag` names the variant in the plan cache
    struct BaseConvFold {
        std::string tag;
        std::vector<u64> src_pre, dst_scale;   // plain residues; empty = none
    };
    const BaseConvPlan* baseconv(const std::vector<int>& src, const std::vector<int>& dst, bool centered,
                                 bool pinv_scaled = false, const BaseConvFold* fold = nullptr, bool rescale_head = false);
    const u64* pinv_vec(int level);
    const u64* pmodq_vec(int level);   // [level+1] P mod q_j, Montgomery form (extended ciphertexts: c0 * P)
    // [2][level+1] the P factors of the tensor-fold key MAC (TensorFold): row 0 the Montgomery form of P * 2^64 mod q_j
    // (mont_mul(x, .) = x * P in Montgomery form), row 1 P mod q_j as a plain residue (the FP64 engine's double)
    const u64* pfold_vec(int level);
    const u64* qlinv_vec(int level);
    // [2][level] the merged tail's factors of limb j < level as plain doubles' bits: row 0 P^-1 mod q_j, row 1 q_level^-1 mod q_j (the
    // values of pinv_vec and qlinv_vec out of Montgomery form; the tail variant of the fused key MAC reads them)
    const u64* tail_fp_vec(int level);
    const u32* ntt_perm(u64 g);
    const u32* coeff_perm(u64 g);
    // per-modulus constant vector on device, Montgomery form, built by `gen(mod_index)`
    const u64* const_vec(const std::string& name, const std::vector<int>& mods, const std::vector<u64>& plain_vals);
    const u64* raw_vec(const std::string& name, const std::vector<u64>& vals);   // cached device copy, no conversion
};

// RAII sample of one kernel launch: records an event pair around every prof_stride-th launch of a kind
struct ProfScope {
    Context& c;
    hipStream_t s;
    bool active = false;
    Context::ProfSample smp{};
    ProfScope(Context& c_, int kid, double bytes, hipStream_t s_, double bytes_primary = -1.0) : c(c_), s(s_) {
        if (!c.prof_on) return;
        const long long idx = c.prof_launched[kid]++;
        // every stride-th launch on average, picked by a hash of the launch index: a fixed stride would lock onto the
        // period of the operator's launch sequence and always time the same launch types
        if (c.prof_stride > 1 && ((unsigned long long)(idx + 1) * 0x9E3779B97F4A7C15ull >> 33) % (unsigned)c.prof_stride != 0) return;
        auto take = [&]() {
            hipEvent_t e;
            if (!c.prof_pool.empty()) {
                e = c.prof_pool.back();
                c.prof_pool.pop_back();
            } else {
                LSA_HIP(hipEventCreate(&e));
            }
            return e;
        };
        smp.e0 = take();
        smp.e1 = take();
        smp.kid = kid;
        smp.bytes = bytes;
        smp.bytes_primary = bytes_primary < 0 ? bytes : bytes_primary;
        LSA_HIP(hipEventRecord(smp.e0, s));
        active = true;
    }
    ~ProfScope() {
        if (!active) return;
        (void)hipEventRecord(smp.e1, s);
        c.prof_samples.push_back(smp);
    }
};

// ---------------------------------------------------------------- launchers (kernels.hip)
struct RowMap {   // rows of a batch item -> modulus index (0xFF = skip)
    int period;
    unsigned char mod_of[LSA_MAX_PERIOD];
    int row0 = 0, row_step = 1;   // the launch's i-th row is row row0 + i*row_step of the batch item (mod_of[row % period])
};

void launch_ntt(Context& c, const u64* src, u64* dst, int batch, long long batch_stride, int rows, const RowMap& rm,
                bool inverse, hipStream_t s);
// element-wise work fused into a forward transform's first-pass load / last-pass store (see NttPassArgs::fz_*), or (pro == 3,
// the only fusion an inverse transform takes) into the load of its first executed pass: in = a * b, a and b canonical
// NTT-domain residues, row r of the transform = limb r % limbs of polynomial r / limbs of each operand
struct NttFusion {
    int epi = 0, pro = 0, limbs = 1, base_polys = 0, ql_mod = 0;
    const u64* a = nullptr;
    long long a_stride = 0;
    int a_rpp = 0;
    const u64* base = nullptr;
    long long base_stride = 0;
    int base_rpp = 0;
    const u64* k = nullptr;
    u64* out = nullptr;
    long long out_stride = 0;
    int out_rpp = 0;
    const u64* last = nullptr;
    long long last_stride = 0;
    int last_rpp = 1;            // rows between the polynomials' last limbs in `last`
    const u64* k2 = nullptr;     // epi == 2: out = (a*k - v + base) * k2
    const u32* scatter = nullptr;   // epilogue only: out[scatter[x]] = value(x) within each row (the automorphism of a rotation)
    // epi == 4 (BFV rotate-and-MAC): out[scatter[x]] (+)= ((a - v) * k + base)(x) * pt[scatter[x]] * 2^-64, base on poly 0
    const u64* pt = nullptr;        // pt_mul plaintexts [batch][limbs][N]
    long long pt_stride = 0;
    bool accumulate = false;        // add to out (later terms) instead of writing it (the first)
    // pro == 3: the second operand (the first is a / a_stride / a_rpp)
    const u64* b = nullptr;
    long long b_stride = 0;
    int b_rpp = 0;
};
// passes: bit 0 = the first executed pass, bit 1 = the second (two-pass plans; a caller that fuses the second pass into
// another kernel asks for 1 only)
void launch_ntt(Context& c, const u64* src, u64* dst, int batch, long long src_stride, long long dst_stride, int rows,
                const RowMap& rm, bool inverse, hipStream_t s, const NttFusion* fz = nullptr, int passes = 3);

// limb-wise binary/unary ops on [batch][rows][N]; row r uses modulus rm.mod_of[r % period]
enum EwOp { EW_ADD = 0, EW_SUB = 1, EW_NEG = 2, EW_MUL = 3 };
void launch_elementwise(Context& c, EwOp op, const u64* a, const u64* b, u64* out, int batch, long long sa,
                        long long sb, long long so, int rows, const RowMap& rm, hipStream_t s);
void launch_muladd(Context& c, EwOp op, const u64* a, const u64* b, const u64* acc, long long sacc, u64* out, int batch,
                   long long sa, long long sb, long long so, int rows, const RowMap& rm, hipStream_t s);
// out[p][j] = (partial[p][j]) + sum_{i<terms} ct_i[p][j] * pt_i[j], one launch; each operand is (base, batch stride)
#define LSA_MAC_MAX_TERMS 16
#define LSA_MACM_MAX 8   // baby and giant steps per k_mac_plain_multi launch
void launch_mac_plain(Context& c, int terms, const u64* const* ct, const long long* sct, const u64* const* pt,
                      const long long* spt, const u64* partial, long long spartial, u64* out, long long so, int batch,
                      int polys, int limbs, const RowMap& rm, hipStream_t s);
void launch_mac_plain_multi(Context& c, int nb, const u64* const* ct, const long long* sct, int ng, const u64* const* pt,
                            u64* const* out, long long so, int batch, int polys, int limbs, const RowMap& rm, hipStream_t s,
                            bool accumulate = false);   // out[g] += the sums (one block of a matrix wider than LSA_MACM_MAX)
// out[g][b][poly][row] = sum_i K[g][i][row] * src_i[b][poly][row] (+ A[g][row] on polynomial 0) mod q_row, rows 0..rows-1 of
// every polynomial; src_i has rpp[i] >= rows rows per polynomial and batch stride ss[i]; out is [G][batch][2][rows][N]
void launch_poly_lincomb(Context& c, int nsrc, const u64* const* src, const long long* ss, const int* rpp, int n_out,
                         const u64* d_k, const u64* d_a, u64* out, int rows, int batch, hipStream_t s);
// out[p][j] = a[p][j] * pt[j] * 2^-64 mod q (+ acc[p][j]) over [batch][polys][limbs][N]: BFV ct x pt_mul in the NTT domain,
// unfused form (k_mont_muladd); acc / a may be out
void launch_mont_muladd(Context& c, const u64* a, long long sa, const u64* pt, long long spt, const u64* acc, long long sacc,
                        u64* out, long long so, int batch, int polys, int limbs, const RowMap& rm, hipStream_t s);
// ring-t plaintext limb -> [level+1][N] residues: mode 0 centred lift from q_0 (CKKS), 1 direct (BFV multiply),
// 2 scale-up by Q/t (BFV add/sub)
void launch_lift_ringt(Context& c, int mode, int level, const u64* pt, long long spt, u64* out, long long sout, int batch,
                       hipStream_t s);
// CKKS/BFV tensor: a,b [2][T][N] -> d [3][T][N]; limb i uses modulus rm.mod_of[i]
// a_rpp / b_rpp: rows per polynomial of the operands (0 = limbs; more when an operand is kept at a higher level: its first
// `limbs` rows of each polynomial are the operand at this level -- no copy needed to "drop" it)
void launch_tensor(Context& c, const u64* a, const u64* b, u64* d, int batch, long long sa, long long sb, long long sd,
                   int limbs, const RowMap& rm, hipStream_t s, int a_rpp = 0, int b_rpp = 0);
// d = sum_{i<terms} a_i (x) b_i (+ (addend_0, addend_1, 0)) (+ d when accumulate), terms <= LSA_DOT_MAX_TERMS (tensor_sum.h), one
// launch of k_tensor_sum; sa[i] / sb[i] batch strides (0: one ciphertext for the whole batch), a_rpp / b_rpp rows per polynomial
// (null or 0: limbs)
void launch_tensor_sum(Context& c, int terms, const u64* const* a, const long long* sa, const int* a_rpp, const u64* const* b,
                       const long long* sb, const int* b_rpp, const u64* addend, long long s_addend, bool accumulate, u64* d,
                       long long sd, int batch, int limbs, const RowMap& rm, hipStream_t s);
// the tensor product folded into the relinearisation's key MAC (CKKS HMult+relin+rescale): for a Q target limb j the MAC
// takes its own digit as d2_j = a1_j * b1_j and adds P * d0_j to the first and P * d1_j to the second running sum
// (d0 = a0 b0, d1 = a0 b1 + a1 b0): acc'_j = acc_j + P * d_j.  a / b point at the tile's first item, [2][rpp][N] each.
struct TensorFold {
    const u64* a;
    const u64* b;
    long long sa, sb;   // batch strides
    long long pa, pb;   // elements between the two polynomials of a / b
};
// exact base conversion: src limbs at rows src_row[i] of the source item, dst limbs at rows dst_row[j] of the dest item
struct BaseConvRows {
    int src_row[LSA_BC_MAX_SRC];
    int dst_row[LSA_BC_MAX_DST];
};
// sub (optional): converted is src - sub, limb for limb (rows.src_row indexes both; its own batch stride and row offsets
// sub_row) -- the subtraction of a preceding element-wise step done on the conversion's source load
// head (optional, narrow conversions without sub): the rescale-head form of ModDown's conversion.  k is a pinv_scaled plan in its
// rescale_head flavour, whose last target l is unscaled; a = INTT(acc[h][l]) and b = INTT(base[h][l]) (or null) are single rows with their batch strides,
// pinv points at P^-1 mod q_l (Montgomery form, device).  Target l is converted but not stored; every other target j gets
// in_j = conv_j * P^-1 + lift_j(t), t = (a - conv_l) * P^-1 (+ b), canonical (ntt_core.h rescale_head_in).
struct BaseConvHead {
    const u64* a;
    long long sa;
    const u64* b;
    long long sb;
    const u64* pinv;
};
void launch_baseconv(Context& c, const BaseConvPlan* k, const BaseConvRows& rows, const u64* src, u64* dst, int batch,
                     long long ssrc, long long sdst, hipStream_t s, const u64* sub = nullptr, long long ssub = 0,
                     const int* sub_row = nullptr, const BaseConvHead* head = nullptr);
// key-switch inner product: out[h][tl] = sum_d ext(d,tl) * key[d][h][tl];  ext(d,tl) = cx[tl] when tl is in digit d
// scatter (every target limb only): the result leaves as the ROTATED EXTENDED ciphertext out[h][tl][scatter[x]] = sum(x) + (h == 0, tl < L:
// P * base[tl][x]) -- gadget product, c0 * P and the automorphism of a baby-step rotation in one pass (base == nullptr: no P * c0);
// accumulate: added to what out holds there (a giant-step rotation joining a running sum)
struct KsMacDst {
    u64* out;   // [2][L+k][N] per batch item
    long long sout;
    const u32* scatter = nullptr;
    const u64* base = nullptr;
    long long sbase = 0;
    bool accumulate = false;
};
// unfused_only: only the target limbs that do not take the fused kernel (ks_fused_limb; k_ntt_r16_ksmac did the others), and
// limb extra_tl with them whatever its engine (-1: none)
void launch_ks_mac(Context& c, int level, const u64* cx, long long scx, const u64* ext, long long sext, const Key& key,
                   const KsMacDst& dst, int batch, hipStream_t s, bool unfused_only = false, const TensorFold* fold = nullptr,
                   int extra_tl = -1);
// out[h][i] = base[h][i] + (acc[h][i] - conv[h][i]) * Pinv_i       (base may be null)
void launch_moddown_final(Context& c, int level, const u64* acc, long long sacc, int acc_rows_per_poly, const u64* conv,
                          long long sconv, const u64* base, long long sbase, int base_rows_per_poly, int base_polys,
                          u64* out, long long sout, int batch, hipStream_t s);
// the largest ring whose limb a gathering tail stages in LDS (moddown_gather.h: 8N bytes)
#define LSA_PERM_LDS_MAX_LOGN 14
// out[p][i] = base[p][i] + (a[p][i] - b[p][i]) * kvec[i]; row of operand X = p*X_rpp + i; b/base optional
void launch_sub_mul_general(Context& c, int polys, int limbs, const unsigned char* limb_mod, const u64* kvec,
                            const u64* a, long long sa, int a_rpp, const u64* b, long long sb, int b_rpp,
                            const u64* base, long long sbase, int base_rpp, int base_polys, u64* out, long long so,
                            int out_rpp, int batch, hipStream_t s);
// rescale helpers (divide-and-round by the last modulus of `level`)
void launch_rescale_prep(Context& c, int level, int polys, const u64* last, long long slast, u64* tmp, long long stmp,
                         int batch, hipStream_t s);
void launch_rescale_final(Context& c, int level, int polys, const u64* in, long long sin, const u64* tmp, long long stmp,
                          u64* out, long long sout, int batch, hipStream_t s);
// gather rows: out[r][i] = in[r][perm[i]] (NTT domain automorphism) ; scatter with sign for coefficient domain
void launch_permute_ntt(Context& c, const u32* perm, const u64* in, long long sin, u64* out, long long sout, int rows,
                        int batch, hipStream_t s);
void launch_permute_coeff(Context& c, const u32* perm, const u64* in, long long sin, u64* out, long long sout, int rows,
                          const RowMap& rm, int batch, hipStream_t s);
// one decomposition, n_keys = 2..4 keys in ONE launch (slot_sum.hip k_ks_mac_multi; arithmetic: ks_mac_multi.h): key k's product
// leaves as launch_ks_mac's scattered extended form, outs[k][h][tl][scatter_k[x]] = sum_k(x) + (h == 0, tl < L: P * base[tl][x]), in key
// k's own buffer [batch][2][L+k][N] (batch stride sout); every digit value is read once for all keys.  The same words as n_keys
// launch_ks_mac calls with `scatter` and `base`.
struct KsMacMultiKey {
    const Key* key;
    const u32* scatter;
    u64* out;
};
void launch_ks_mac_multi(Context& c, int level, const u64* cx, long long scx, const u64* ext, long long sext, int n_keys,
                         const KsMacMultiKey* keys, long long sout, const u64* base, long long sbase, int batch, hipStream_t s);
// out (+)= sum_{k<n_in} in[k] over the 2(L+k) rows of extended ciphertexts, n_in = 1..3 (k_ext_sum); no addend is `out`
void launch_ext_sum(Context& c, int level, int n_in, const u64* const* in, long long sin, u64* out, long long sout, bool accumulate,
                    int batch, hipStream_t s);
// extended (Q_level u P) ciphertext: out (+)= perm(acc + P * base) -- a rotation without its division by P (k_permute_ext)
void launch_permute_ext(Context& c, int level, const u32* perm, const u64* acc, long long sacc, const u64* base, long long sbase,
                        int base_polys, u64* out, long long sout, bool accumulate, int batch, hipStream_t s);
// strided row copy: out[b][r] = in[b][src_row[r]]
void launch_copy_rows(Context& c, const u64* in, long long sin, u64* out, long long sout, int rows, const int* src_row,
                      int batch, hipStream_t s);
void launch_to_mont(Context& c, u64* data, int rows, const RowMap& rm, hipStream_t s);
bool ks_fused_enabled(const Context& c);   // the fused second-pass + key-MAC kernel applies to this context (and is not switched off)
// a key-switch key on the device: `words` u64 in compact order [beta][2][key_level+1+np][N]; where the fused key MAC applies
// (ks_fused_enabled) the key's double copy follows in the same allocation, `words` doubles more (words = 0: no such key)
struct KeyLayout {
    size_t words = 0;
    bool fp = false;
    size_t alloc_words() const { return fp ? 2 * words : words; }
    double* fp_of(u64* data) const { return fp ? reinterpret_cast<double*>(data + words) : nullptr; }
};
KeyLayout key_layout(const Context& c, int key_level);
// a freshly loaded key at `data` (plain residues) -> key: Montgomery form in place, its double copy written to `fp` (null: none)
void key_prepare(Context& c, Key& key, u64* data, int key_level, double* fp, hipStream_t s);
// second pass of the extension transform + gadget inner product in one launch (see k_ntt_r16_ksmac) for the target limbs that
// take it (ks_fused_limb); false = shape not covered
// limbs: which of them one launch covers.  The tail sequence of a merged ModDown + rescale (key_switch.hip, KsTile::mac_rescale)
// splits the set: KS_FUSED_P, the P limbs, before ModDown's head (it reads the accumulator's P rows); KS_FUSED_Q_TAIL, the Q limbs
// other than `level`, after it, finishing the rescaled limbs from their running sums (`tail`; FP64-engine limbs, seven- and
// eight-stage second passes).  Limb `level` takes neither: the head needs its accumulator row whole (launch_ks_mac's extra_tl)
enum KsFusedLimbs { KS_FUSED_ALL = 0, KS_FUSED_P = 1, KS_FUSED_Q_TAIL = 2 };
struct KsTailOperands {
    const u64* conv;   // [2][L][N] per item: pass-one output of the transform of in_j = conv_j * P^-1 + lift_j(t)
    long long sconv;
    u64* out;          // [2][level][N] per item: the rescaled ciphertext
    long long sout;
};
bool launch_ntt_ksmac(Context& c, int level, const u64* cx, long long scx, u64* ext, long long sext, const Key& key, u64* acc,
                      long long sacc, int batch, hipStream_t s, const TensorFold* fold = nullptr, KsFusedLimbs limbs = KS_FUSED_ALL,
                      const KsTailOperands* tail = nullptr);
int ks_fused_engines(const Context& c);   // which engines' target limbs take the fused kernel (LSA_KS_FUSED_ENGINES, default FP64 only)
bool ks_fuse_mac(const Context& c, int level, const Key& key);   // a single-key switch at this level runs k_ntt_r16_ksmac (key_switch.hip)
bool ks_fused_limb(const Context& c, int L, int tl);   // target limb tl of Q_level u P takes it (by its engine)
// out = (a - b) * k_i  with per-row constant (Montgomery form) ; out = a * k_i
void launch_sub_mul_const(Context& c, const u64* a, long long sa, const u64* b, long long sb, const u64* kvec, u64* out,
                          long long so, int rows, const RowMap& rm, int batch, hipStream_t s);
void launch_mul_const(Context& c, const u64* a, long long sa, const u64* kvec, u64* out, long long so, int rows,
                      const RowMap& rm, int batch, hipStream_t s);
// out[row] = a[row] * mvec[row] + kvec[row] (kvec: plain residues, mvec: Montgomery-form factors or null)
void launch_add_const(Context& c, const u64* a, long long sa, const u64* kvec, u64* out, long long so, int rows,
                      const RowMap& rm, int batch, hipStream_t s, const u64* mvec = nullptr);
// CKKS plaintext / constant operands (plain_ops.h).  out[b][j] = v[b] mod q_j, j < limbs: the rounded coefficients of `batch`
// plaintexts [N] (signed, |v| < 2^63) -> canonical residue rows [limbs][N], coefficient domain
void launch_lift_i64(Context& c, const long long* v, long long sv, u64* out, long long so, int limbs, int batch, hipStream_t s);
// out = a * k (mul) + beta (add; polynomial 0 only) over [batch][2][limbs][N], k / beta the "plus" or "minus" constant of limb j
// at point x by bit sel_bit of x (minus when the bit differs from sel_pol); an addition alone copies polynomial 1 (out != a)
void launch_cconst(Context& c, bool mul, bool add, const u64* a, long long sa, const CconstLimb* k, int sel_bit, int sel_pol,
                   u64* out, long long so, int limbs, int batch, hipStream_t s);
void launch_probe_copy(u64* dst, const u64* src, size_t n, hipStream_t s);
void launch_probe_mulhi(u64* buf, size_t n, int iters, hipStream_t s);

// ---------------------------------------------------------------- CKKS bootstrapping (bootstrap.hip)
struct Bootstrap;
Bootstrap* bootstrap_create(Context& c, int cts_depth, int stc_depth, int K, int double_angle, double message_ratio,
                            double in_scale, double out_scale, int log_slots, hipStream_t s, int sine_deg = 30, int arcsine_deg = 0);
const std::vector<double>& bootstrap_arcsine(const Bootstrap& bt);
bool bootstrap_is_sparse(const Bootstrap& bt);
void bootstrap_destroy(Bootstrap* b);
int bootstrap_out_level(const Bootstrap& bt);
double bootstrap_out_scale(const Bootstrap& bt);
const std::vector<u64>& bootstrap_galois(const Bootstrap& bt);
const std::vector<double>& bootstrap_chebyshev(const Bootstrap& bt);
int bootstrap_matrices(const Bootstrap& bt);
int bootstrap_cts_matrices(const Bootstrap& bt);
void bootstrap_matrix(const Bootstrap& bt, int i, int* level, int* n1, const std::vector<int>** ks, const std::vector<u64*>** plains,
                      int* rows = nullptr);
void bootstrap_run(Bootstrap& bt, const u64* in, long long sin, u64* out, long long sout, int batch, const Key& rlk,
                   const GaloisKeys& glk, const Key* swk_dts, const Key* swk_std, hipStream_t s);

// ---------------------------------------------------------------- operator pipelines (ops.hip)
const std::string& last_error();
// The first-generation operators below (mult, relin, rescale, rotate(_many), drop_level, addsub, mult_relin(_rescale), both
// schemes) check their own arguments -- scheme, level, polys, null / short / odd / misaligned operands, overlap -- before anything
// is queued, and return at once for batch <= 0: the contract of include/lattisense_amd.h, "Layout and aliasing".  Internal
// callers of these functions get the same refusals as the C entry points.  (task_dispatch.hip launches k_elementwise, k_tensor and
// k_copy_rows itself for add / sub / negate, the CKKS tensor and a drop of several levels: those paths do not come through here.)
void ckks_mult(Context& c, int level, const u64* a, const u64* b, u64* d3, int batch, long long sa, long long sb, long long sd,
               hipStream_t s);
void ckks_relin(Context& c, int level, const u64* d3, const Key& rlk, u64* out, int batch, long long sd, long long so,
                hipStream_t s);
void ckks_rescale(Context& c, int level, int polys, const u64* in, u64* out, int batch, long long sin, long long sout,
                  hipStream_t s);
void ckks_rotate(Context& c, int level, const u64* in, u64 g, const Key& glk, u64* out, int batch, long long sin,
                 long long sout, hipStream_t s);
void ckks_rotate_many(Context& c, int level, const u64* in, int n_rot, const u64* g, const Key* const* glk, u64* const* outs,
                      int batch, long long sin, long long sout, hipStream_t s);
void ckks_switch_key(Context& c, int level, const u64* in, const Key& swk, u64* out, int batch, long long sin, long long sout,
                     hipStream_t s);
void ckks_mult_relin_rescale(Context& c, int level, const u64* a, const u64* b, const Key& rlk, u64* out, int batch,
                             long long sa, long long sb, long long so, hipStream_t s);
void ckks_mult_relin_rescale_rpp(Context& c, int level, const u64* a, const u64* b, const Key& rlk, u64* out, int batch,
                                 long long sa, long long sb, long long so, hipStream_t s, int a_rpp, int b_rpp);
// Encrypted inner product.  The operands of sum_{i<n} a_i (x) b_i: NTT-domain ciphertexts [2][rpp][N], a batch stride each
// (0: one ciphertext shared by the batch) and rows per polynomial each (null array or 0: level + 1); addend (nullable): a
// ciphertext [2][level+1][N] at the product's scale
struct DotTerms {
    int n;
    const u64* const* as;
    const long long* sas;
    const int* a_rpp;
    const u64* const* bs;
    const long long* sbs;
    const int* b_rpp;
    const u64* addend;
    long long s_addend;
};
// d3 = the summed degree-2 tensor (+ addend on polynomials 0 and 1), [3][level+1][N]: the words of ckks_mult per pair and
// poly_addsub; d3 overlaps no input
void ckks_mult_sum(Context& c, int level, const DotTerms& t, u64* d3, int batch, long long sd, hipStream_t s);
// out = relin(d3 above), rescaled when `rescale`: ONE key switch for the whole sum; the words of ckks_relin (and ckks_rescale) on
// ckks_mult_sum's d3; out overlaps no input
void ckks_dot(Context& c, int level, const DotTerms& t, const Key& rlk, u64* out, int batch, long long so, bool rescale,
              hipStream_t s);
// CKKS plaintext and constant operands (the lsa_ckks_*_plain / *_const entry points; semantics in include/lattisense_amd.h).
// ct / out [2][level+1][N], pt [level+1][N] (batch stride 0: one plaintext for the whole batch), NTT domain; `rescale` runs
// ckks_rescale on the result, out then [2][level][N] and apart from every input
void ckks_mult_plain(Context& c, int level, const u64* ct, long long sct, const u64* pt, long long spt, u64* out, long long so,
                     int batch, bool rescale, hipStream_t s);
void ckks_addsub_plain(Context& c, int op, int level, const u64* ct, long long sct, const u64* pt, long long spt, u64* out,
                       long long so, int batch, hipStream_t s);
void ckks_mac_plain(Context& c, int level, int n, const u64* const* cts, const long long* scts, const u64* const* pts,
                    const long long* spts, const u64* addend, long long s_addend, u64* out, long long so, int batch, bool rescale,
                    hipStream_t s);
void ckks_mult_const(Context& c, int level, const u64* ct, long long sct, double re, double im, double const_scale, u64* out,
                     long long so, int batch, bool rescale, hipStream_t s);
void ckks_add_const(Context& c, int level, const u64* ct, long long sct, double re, double im, double ct_scale, u64* out,
                    long long so, int batch, hipStream_t s);
void ckks_affine_const(Context& c, int level, const u64* ct, long long sct, double re, double im, double const_scale, double add_re,
                       double add_im, double ct_scale, u64* out, long long so, int batch, bool rescale, hipStream_t s);
void ckks_lift_ext(Context& c, int level, const u64* in, u64* out, int batch, long long sin, long long sout, hipStream_t s);
// c1_coef (BFV: the caller holds the ciphertext in the coefficient domain as well): c1's coefficients, read by the decomposition
// in place of an inverse transform of in's c1 (key_switch.h KsSource::BOTH); the same words
void ckks_rotate_many_ext(Context& c, int level, const u64* in, int n_rot, const u64* g, const Key* const* glk, u64* const* outs,
                          int batch, long long sin, long long sout, hipStream_t s, const u64* c1_coef = nullptr, long long s_coef = 0);
void ckks_rotate_ext(Context& c, int level, const u64* in, u64 g, const Key& glk, u64* out, bool accumulate, int batch,
                     long long sin, long long sout, hipStream_t s, bool scatter_mac = false);
// coeff_out: the result leaves in the coefficient domain (key_switch.h KsOut::COEFF: every row of `in` leaves the NTT domain once
// and the tail runs there) -- INTT of the NTT-domain result, residue for residue
void ckks_moddown_ext(Context& c, int level, u64* in, u64* out, int batch, long long sin, long long sout, hipStream_t s,
                      bool coeff_out = false);
// ---- the slot sums (slot_sum.hip: kernels and runners, on the key-switch tile of key_switch.h)
// CKKS slot sum  out = sum_{i<count} rot(in, i*step)  (lsa_slot_sum_* / lsa_ckks_slot_sum; plan rule: slot_sum.h).  Every step is one
// decomposition whose 1..4 rotations stay over Q_level u P (the words of ckks_rotate_ext); the NEXT group is divided by P once with
// x riding on the ModDown tail's base, the TAIL rotations gather in an extended accumulator divided once at the end.
struct SlotSum {
    Context& c;
    int level;
    SlotSumPlanHost plan;
    // steps with 2..4 keys: true = one k_ks_mac_multi launch + k_ext_sum; false = one launch_ks_mac per key, each adding to its
    // destination.  The same words; the default is the faster form on the MI355X (the multi-key launch lost 6-10 %)
    bool multi_mac = false;
    SlotSum(Context& ctx, int level_) : c(ctx), level(level_) {}
};
#define LSA_SLOTSUM_DEFAULT_RADIX 4   // what radix 0 stands for: measured, DESIGN 4.11
SlotSumPlanHost slot_sum_plan_checked(int n_ring, long long step, int count, int radix);   // slot_sum_plan, refusals as LSA_ERR_ARG
SlotSum* slot_sum_create(Context& c, int level, long long step, int count, int radix);
void slot_sum_run(SlotSum& p, const u64* in, long long sin, u64* out, long long sout, int batch,
                  const GaloisKeys& glk, hipStream_t s);
// BFV slot sum  out = sum_{i<count} rot_cols(y, i*step), y = in + rot_rows(in) if rows (lsa_bfv_slot_sum_*; plan: slot_sum.h).
// Ciphertexts are in the coefficient domain.  gather: the rotated c0 terms never enter the NTT domain -- the key MAC adds no
// P * c0 and the ModDown tail gathers them from the c0 row staged in LDS (slot_sum.hip k_bfv_slot_tail; N <= 2^14); plain: c0 is
// transformed too and rides through the division as P * c0 (the CKKS form).  The same words, since ModDown(P z + a) = z + ModDown(a).
struct BfvSlotSum {
    Context& c;
    int level;
    SlotSumPlanHost plan;
    bool gather;
    BfvSlotSum(Context& ctx, int level_) : c(ctx), level(level_), gather(ctx.logn <= LSA_PERM_LDS_MAX_LOGN) {}
};
#define LSA_BFV_SLOTSUM_DEFAULT_RADIX 4   // what radix 0 stands for
SlotSumPlanHost bfv_slot_sum_plan_checked(int n_ring, long long step, int count, int radix, int rows);
BfvSlotSum* bfv_slot_sum_create(Context& c, int level, long long step, int count, int radix, int rows);
void bfv_slot_sum_run(BfvSlotSum& p, const u64* in, long long sin, u64* out, long long sout, int batch,
                      const GaloisKeys& glk, hipStream_t s);
// ---- BFV oblivious expansion (bfv_expand.hip: kernels and runner, on key_switch(); plan and point arithmetic: bfv_expand.h;
// semantics: include/lattisense_amd.h).  gather: the tail of a level's key switch forms both children from the rotation staged in LDS
// (k_bfv_expand_tail, N <= 2^14, fused tails); else the key switch leaves (c0 + ks0, ks1) in the workspace and
// k_bfv_expand_combine gathers it from there.  The same words.
struct BfvExpand {
    Context& c;
    int level;
    BfvExpandPlanHost plan;
    bool gather;
    BfvExpand(Context& ctx, int level_) : c(ctx), level(level_), gather(ctx.logn <= LSA_PERM_LDS_MAX_LOGN) {}
};
BfvExpandPlanHost bfv_expand_plan_checked(int n_ring, int count);   // bfv_expand_plan, refusals as LSA_ERR_ARG
BfvExpand* bfv_expand_create(Context& c, int level, int count);
void bfv_expand_run(BfvExpand& p, const u64* in, long long sin, u64* out, long long sout, long long s_index, int batch,
                    const GaloisKeys& glk, hipStream_t s);
// out = X^exponent * in on `polys` coefficient-domain polynomials (k_mul_monomial); the output overlaps nothing
void bfv_mul_monomial(Context& c, int level, int polys, long long exponent, const u64* in, u64* out, int batch, long long sin,
                      long long sout, hipStream_t s);
// ---- BFV coefficient packing (bfv_pack.hip: kernels and runner, on key_switch(); plan and point arithmetic: bfv_pack.h; semantics:
// include/lattisense_amd.h).  gather: the tail of a level's key switch adds the rotation staged in LDS to u = a + X^s b
// (k_bfv_pack_tail, N <= 2^14, fused tails); else the key switch leaves (v0 + ks0, ks1) in the workspace and k_bfv_pack_combine
// gathers it from there.  The same words.
struct BfvPack {
    Context& c;
    int level;
    BfvPackPlanHost plan;
    bool gather;
    BfvPack(Context& ctx, int level_) : c(ctx), level(level_), gather(ctx.logn <= LSA_PERM_LDS_MAX_LOGN) {}
};
BfvPackPlanHost bfv_pack_plan_checked(int n_ring, int count, int trace);   // bfv_pack_plan, refusals as LSA_ERR_ARG
BfvPack* bfv_pack_create(Context& c, int level, int count, int trace);
void bfv_pack_run(BfvPack& p, u64* in, long long sin, long long s_index, u64* out, long long sout, int batch, const GaloisKeys& glk,
                  hipStream_t s);
// ---- BFV external product RLWE x RGSW, CMux and select by an encrypted index (bfv_select.hip: the pair MAC kernel and the runners, on
// external_product() of key_switch.h; plan: bfv_select.h; semantics: include/lattisense_amd.h).  An RGSW ciphertext is the key pair
// (r0, r1) in lsa_key_upload's layout.
// acc[h][tl] = sum_d e0(d,tl) * r0[d][h][tl] + sum_d e1(d,tl) * r1[d][h][tl], e_i(d,tl) = cx_i[tl] when tl is in digit d, else ext_i[d][tl]
// (k_ks_mac_pair; the fold rule: ks_mac_pair.h).  cx0 / cx1 and ext0 / ext1 share their batch strides.  Called by key_switch.hip alone.
void launch_ks_mac_pair(Context& c, int level, const u64* cx0, const u64* cx1, long long scx, const u64* ext0, const u64* ext1,
                        long long sext, const Key& r0, const Key& r1, u64* acc, long long sacc, int batch, hipStream_t s);
struct BfvSelect {
    Context& c;
    int level;
    BfvSelectPlanHost plan;
    BfvSelect(Context& ctx, int level_) : c(ctx), level(level_) {}
};
BfvSelectPlanHost bfv_select_plan_checked(int count);   // bfv_select_plan, refusals as LSA_ERR_ARG
BfvSelect* bfv_select_create(Context& c, int level, int count);
void bfv_select_run(BfvSelect& p, u64* in, long long sin, long long s_index, u64* out, long long sout, int batch, int n_sel,
                    const Key* const* r0s, const Key* const* r1s, hipStream_t s);
// out = ct [.] (r0, r1) (+ base); out may be ct or base themselves
void bfv_external_product(Context& c, int level, const u64* ct, long long sct, const Key* r0, const Key* r1, const u64* base,
                          long long sbase, u64* out, long long sout, int batch, hipStream_t s);
// out = c0 + (r0, r1) [.] (c1 - c0); out may be c0 or c1 themselves
void bfv_cmux(Context& c, int level, const u64* c0, long long s0, const u64* c1, long long s1, const Key* r0, const Key* r1, u64* out,
              long long sout, int batch, hipStream_t s);
// ---- (ops.hip again)
void drop_level(Context& c, int level, int polys, const u64* in, u64* out, int batch, long long sin, long long sout,
                hipStream_t s);
void poly_addsub(Context& c, int op, int level, int polys, const u64* a, const u64* b, u64* out, int batch, long long sa,
                 long long sb, long long so, hipStream_t s);
void bfv_mult(Context& c, int level, const u64* a, const u64* b, u64* d3, int batch, long long sa, long long sb, long long sd,
              hipStream_t s);
void bfv_relin(Context& c, int level, const u64* d3, const Key& rlk, u64* out, int batch, long long sd, long long so,
               hipStream_t s);
void bfv_mult_relin(Context& c, int level, const u64* a, const u64* b, const Key& rlk, u64* out, int batch, long long sa,
                    long long sb, long long so, hipStream_t s);
// BFV encrypted inner product (semantics and the headroom rule: include/lattisense_amd.h, tables.h bfv_dot_plan).  The operands of
// DotTerms are coefficient-domain ciphertexts [2][level+1][N]; a_rpp / b_rpp are not used.  d3 = t * round(sum_i a_i (x) b_i / Q)
// (+ addend on polynomials 0 and 1), [3][level+1][N]: with n == 1 and no addend the words of bfv_mult
void bfv_mult_sum(Context& c, int level, const DotTerms& t, u64* d3, int batch, long long sd, hipStream_t s);
// out = bfv_relin(d3 above): ONE scale-down per group of terms and ONE key switch for the whole sum
void bfv_dot(Context& c, int level, const DotTerms& t, const Key* rlk, u64* out, int batch, long long so, hipStream_t s);
// BFV polynomial evaluation and constant operands (bfv_poly.hip; planner and counts: bfv_poly.h; semantics:
// include/lattisense_amd.h).  The plan is opaque outside its unit; ciphertexts are coefficient-domain [2][level+1][N].
struct BfvPolyPlan;
struct BfvPolynomial;
BfvPolyPlan bfv_poly_plan_checked(u64 t, int n_coef, const u64* coef, int log_baby);   // the planner's refusals as LSA_ERR_ARG
BfvPolynomial* bfv_poly_create(Context& c, int level, int n_coef, const u64* coef, int log_baby, hipStream_t s);
void bfv_poly_destroy(BfvPolynomial* p);
const BfvPolyPlan& bfv_poly_plan_of(const BfvPolynomial& p);
int bfv_poly_level(const BfvPolynomial& p);
// out = p(in) slot-wise; out overlaps no word of in; rlk null: refused
void bfv_poly_run(BfvPolynomial& p, const u64* in, long long sin, u64* out, long long sout, int batch, const Key* rlk, hipStream_t s);
// out = k * ct + c in every slot (k, c < t); out may be ct itself (same pointer, same stride)
void bfv_affine_const(Context& c, int level, const u64* ct, long long sct, u64 k, u64 cst, u64* out, long long sout, int batch,
                      hipStream_t s);
void bfv_rotate(Context& c, int level, const u64* in, u64 g, const Key& glk, u64* out, int batch, long long sin,
                long long sout, hipStream_t s);
void bfv_rotate_many(Context& c, int level, const u64* in, int n_rot, const u64* g, const Key* const* glk, u64* const* outs,
                     int batch, long long sin, long long sout, hipStream_t s);
void bfv_rescale(Context& c, int level, int polys, const u64* in, u64* out, int batch, long long sin, long long sout,
                 hipStream_t s);
// BFV ct x pt_mul (NTT-domain, Montgomery-form plaintexts [L][N]): out = ct . pt per poly; out may be ct
void bfv_mult_plain_mul(Context& c, int level, const u64* ct, const u64* pt, u64* out, int batch, long long sct, long long spt,
                        long long sout, hipStream_t s);
// BFV ct and a ring-t plaintext pt [N] (bfv_plain.hip; semantics: include/lattisense_amd.h).  The launcher serves the task runtime
// too: polys 2 or 3, out may be ct itself (same pointer and stride), nothing else is checked.
void launch_bfv_addsub_plain(Context& c, int op, int level, int polys, const u64* ct, long long sct, const u64* pt, long long spt,
                             u64* out, long long sout, int batch, hipStream_t s);
void bfv_addsub_plain(Context& c, int op, int level, const u64* ct, long long sct, const u64* pt, long long spt, u64* out,
                      long long sout, int batch, hipStream_t s);
void bfv_plain_lift(Context& c, int level, int form, const u64* pt, long long spt, u64* out, long long sout, int batch,
                    hipStream_t s);
void bfv_mult_plain(Context& c, int level, const u64* ct, long long sct, const u64* pt, long long spt, u64* out, long long sout,
                    int batch, hipStream_t s);
// out = sum_i cts[i] . pts[i] (+ partial), n >= 1 terms, one inverse transform per output; out overlaps no input
void bfv_mac_plain_mul(Context& c, int level, int n, const u64* const* cts, const long long* scts, const u64* const* pts,
                       const long long* spts, const u64* partial, long long spartial, u64* out, int batch, long long sout,
                       hipStream_t s);
// out = sum_{i<n} rot_{g[i]}(in) . pts[i] (+ partial), g[i] == 1: the input itself (no key); every output bit-identical to
// bfv_rotate_many + bfv_mac_plain_mul on the same terms, rotations kept in the NTT domain (fz_epi = 4); out overlaps no input
void bfv_rotate_mac_plain_mul(Context& c, int level, const u64* in, int n, const u64* g, const Key* const* glk,
                              const u64* const* pts, const long long* spts, const u64* partial, long long spartial, u64* out,
                              int batch, long long sin, long long sout, hipStream_t s);
// ---- BFV plaintext matrix x ciphertext vector (bfv_matvec.hip: k_bfv_matvec and the runner; plan: bfv_matvec.h; semantics:
// include/lattisense_amd.h): out[r] = sum_c cts[c] . pts[r][c] (+ partial[r]), the words of bfv_mac_plain_mul on row r's terms, every
// ciphertext transformed once.  Index-major cts and out; out overlaps no input.
struct BfvMatvecLayout {
    const u64* cts;
    long long s_col, sct;
    const u64* pts;
    long long s_prow, s_pcol, spt;
    const u64* partial;   // nullable
    long long s_partial_row, spartial;
    u64* out;
    long long s_row, sout;
};
BfvMatvecPlanHost bfv_matvec_plan_checked(int n_ring, int level_limbs, int rows, int cols, int batch, size_t workspace_bytes,
                                          int row_block, int col_block);   // bfv_matvec_plan, refusals as LSA_ERR_ARG
void bfv_matvec_plain_mul(Context& c, int level, int rows, int cols, const BfvMatvecLayout& a, int batch, hipStream_t s);

}  // namespace lsa
