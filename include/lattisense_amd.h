/*
 * lattisense_amd.h — C-ABI of the MI355X executor for LattiSense's RNS polynomial-arithmetic hot path.
 *
 * Two layers, both plain C (pointers + sizes, no C++/torch types):
 *
 *  (1) OPERATOR LAYER (lsa_*): what the reference obtains from the absent HEonGPU library through
 *      heongpu::HEContext / HEArithmeticOperator (call sites mega_ag_runners/gpu/gpu_wrapper.cu:53-138 and
 *      mega_ag_runners/gpu/mega_ag_executors_gpu.cu:71-426).  Ciphertexts are device-resident u64 limbs laid out
 *      [poly][limb][N] exactly like the reference's device buffers (gpu_abi_bridge_executors.h:76-80, :185-189);
 *      every call takes a `batch` of independent ciphertexts (batch_stride u64 elements apart) and a HIP stream.
 *
 *  (2) TASK LAYER (create/bind/run/release_fhe_gpu_task): declared in lattisense_task.h, the drop-in for
 *      mega_ag_runners/wrapper.h:67-85.
 *
 * All functions return 0 on success and a non-zero code on failure; lsa_last_error() returns the message of the
 * last failure on the calling thread (the reference throws std::runtime_error through extern "C",
 * gpu_abi_bridge_executors.h:51-55 — unusable from cgo/ctypes callers, SURVEY §8b "Errors").
 * There is no CPU fallback: without a HIP device every compute entry point fails with LSA_ERR_NO_DEVICE.
 */
#ifndef LATTISENSE_AMD_H
#define LATTISENSE_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lsa_context_st* lsa_context;
typedef struct lsa_key_st* lsa_key; /* one key-switch key (relin key, or the key of one Galois element) */

enum { LSA_OK = 0, LSA_ERR_ARG = 1, LSA_ERR_NO_DEVICE = 2, LSA_ERR_HIP = 3, LSA_ERR_INTERNAL = 4 };
enum { LSA_ALGO_BFV = 0, LSA_ALGO_CKKS = 1 }; /* same values as Algo in mega_ag_runners/c_argument.h:35-38 */

const char* lsa_last_error(void);
const char* lsa_version(void);
/* every compile-time switch (LSA_* macro) the library was built with; "" for the product build (csrc/build_flags.h) */
const char* lsa_build_flags(void);

/* ---- context: replaces init_gpu_context (gpu_wrapper.cu:53-138).  q = Q chain (max_level+1 primes),
 * p = special primes, t = BFV plaintext modulus (0 for CKKS).  Tables are built once and cached. */
int lsa_context_create(int algo, int n, const uint64_t* q, int nq, const uint64_t* p, int np, uint64_t t,
                       int device, lsa_context* out);
int lsa_context_destroy(lsa_context ctx);
/* all moduli in context order: Q chain, P, then the BFV auxiliary basis the context generated */
int lsa_context_moduli(lsa_context ctx, uint64_t* out, int capacity, int* count);

/* ---- device memory / streams (thin wrappers so a caller needs no HIP bindings; torch pointers work too) */
int lsa_malloc(lsa_context ctx, void** dptr, size_t bytes);
int lsa_free(lsa_context ctx, void* dptr);
int lsa_memcpy_h2d(lsa_context ctx, void* dst, const void* src, size_t bytes, void* stream);
int lsa_memcpy_d2h(lsa_context ctx, void* dst, const void* src, size_t bytes, void* stream);
int lsa_memcpy_d2d(lsa_context ctx, void* dst, const void* src, size_t bytes, void* stream);
int lsa_stream_create(lsa_context ctx, void** stream);
int lsa_stream_destroy(lsa_context ctx, void* stream);
int lsa_stream_synchronize(lsa_context ctx, void* stream);
/* HIP-event timing on `stream` (bench.py roofline leg): returns elapsed ms between two recorded events */
int lsa_event_create(lsa_context ctx, void** ev);
int lsa_event_record(lsa_context ctx, void* ev, void* stream);
int lsa_event_elapsed_ms(lsa_context ctx, void* ev_start, void* ev_stop, float* ms);
int lsa_event_destroy(lsa_context ctx, void* ev);

/* ---- evaluation keys.  `compact` is the ABI order of plug-in/lattigo/acc/c_struct_import_export.go:41-135:
 * [beta][2][key_level+1+np][N], beta = ceil((key_level+1)/np), NTT domain, non-Montgomery (GPU_MFORM_BITS = 0,
 * cxx_sdk_v2/cxx_fhe_task_gpu.cpp:30).  Replaces export_relin_key / export_galois_key / export_switching_key
 * (gpu_abi_bridge_executors.h:86-176). */
int lsa_key_upload(lsa_context ctx, const uint64_t* compact_host, int key_level, void* stream, lsa_key* out);
/* adopt a device buffer already holding the compact key (e.g. after an RCCL broadcast); converted in place */
int lsa_key_adopt_device(lsa_context ctx, uint64_t* compact_dev, int key_level, void* stream, lsa_key* out);
int lsa_key_destroy(lsa_context ctx, lsa_key key);
size_t lsa_key_bytes(lsa_context ctx, int key_level);

/* ---- K1/K2: batched negacyclic NTT / INTT, in place.  data = [batch][rows][N]; row r uses modulus index
 * mod_of[r % period] in context order (0xFF = leave the row untouched). */
int lsa_ntt(lsa_context ctx, uint64_t* data, int batch, long long batch_stride, int rows, const int* mod_of,
            int period, int inverse, void* stream);

/* ---- Layout and aliasing: the contract of the first-generation operators -- lsa_poly_addsub, lsa_ckks_mult / _relin / _rescale /
 * _rotate / _rotate_many / _mult_relin_rescale, lsa_drop_level, lsa_bfv_mult / _relin / _rotate / _rescale / _mult_relin.  The library's
 * own callers of these operators (task runtime, bootstrapping, linear transform, polynomial evaluation) go through the same checks;
 * the task runtime's add / sub / negate, CKKS ct x ct tensor and multi-level drop launch their kernels directly, on slabs of its own.
 *   Operands.  Item b of an operand is the `words` words at base + b * stride (stride in words): any base inside an allocation, any
 *     stride >= one item, padding is never read or written.  The kernels move 16 bytes per lane, so every base is 16-byte aligned
 *     and every stride even.
 *   Shared operands.  A stride of 0 on an INPUT means one operand for the whole batch.  Accepted on a and b of lsa_poly_addsub,
 *     lsa_ckks_mult, lsa_ckks_mult_relin_rescale (folded and unfolded paths), lsa_bfv_mult and lsa_bfv_mult_relin, whose kernels index
 *     base + b * stride and nothing else; a == b (squaring, doubling) is allowed with any strides.  The one-input operators (relin,
 *     rescale, rotate, rotate_many, drop_level) refuse it: batch copies of one result are no use, and "the output is the input"
 *     would stop meaning one thing.  An output stride of 0 is always refused.
 *   Overlap is exact: two operands overlap when an item of one shares a word with an item of the other.  Padding belongs to
 *     nobody, so operands may interleave (an output slab between two far-apart inputs is fine).
 *       lsa_poly_addsub: out may BE a and / or b (same pointer, same stride; element-wise), otherwise it overlaps neither.
 *       lsa_ckks_rotate, lsa_bfv_rotate: out may BE in (same pointer, same stride; the rotation then runs in two steps through the
 *         workspace), otherwise no overlap.
 *       lsa_ckks_rotate_many, lsa_bfv_rotate_many: one rule, checked by one function.  The outputs overlap each other nowhere; each is
 *         apart from the input or IS the input (same pointer, sout == sin); at most one is, and that rotation is computed last, from the
 *         intact input, in two steps.  An output that only partly overlaps the input is refused: a tile's store could land on a later
 *         tile's input.
 *       every other one: the output overlaps no input.  In particular rescale and drop_level store rows at other offsets than they
 *         load them, so an in-place call would corrupt rows still to be read.
 *   Refused with LSA_ERR_ARG before any kernel or copy is queued, the message beginning with the entry point's name: a null pointer
 *     (except b with op neg) or key; a stride that is non-zero and below one item, negative, odd, or 0 where not accepted; a pointer
 *     off the 16-byte grid; a level out of range (0..max, from 1 for rescale, drop_level, mult_relin_rescale); a key exported below
 *     `level`; polys outside 1..3; a context of the other scheme (lsa_poly_addsub and lsa_drop_level serve both); a forbidden
 *     overlap.  A refused call leaves every buffer untouched and the context usable.
 *   batch <= 0 returns LSA_OK and touches nothing (scheme, level, polys and op are still checked).
 *   The operators built on these keep the same contract -- operands, exact overlap, 16-byte bases and even strides, LSA_ERR_ARG before
 *   anything is queued -- each with its own rule for stride 0 and for the output; tests/test_gpu_operator_layout.py holds them to it:
 *       lsa_bfv_mult_plain_mul: out may BE ct (same pointer, same stride), otherwise it is apart from ct; always apart from the
 *         plaintexts.  Stride 0 on pt only.
 *       lsa_bfv_mac_plain_mul, lsa_bfv_rotate_mac_plain_mul: out overlaps no ciphertext, plaintext or partial sum.  Stride 0 on the
 *         plaintexts only.  Messages begin with the entry point's name, as for lsa_bfv_rotate_many and lsa_bfv_mult_plain_mul.
 *       lsa_ckks_slot_sum, lsa_bfv_slot_sum: out may BE in (same pointer, same stride), otherwise no overlap; no stride 0.
 *       lsa_bfv_affine_const: out may BE ct, otherwise no overlap; no stride 0.
 *       lsa_ckks_linear_transform, lsa_bfv_linear_transform, lsa_ckks_poly_eval, lsa_bfv_poly_eval: out overlaps no word of in; no
 *         stride 0.  (Messages begin "linear transform", "lsa_bfv_linear_transform", "poly", "bfv_poly".)
 *       lsa_ckks_mult_sum / _dot, lsa_bfv_mult_sum / _dot: stride 0 on every as[i], bs[i] and on the addend; as[i] == bs[i] squares;
 *         the output overlaps no operand.  (Messages begin "dot" / "bfv_dot".) */
/* ---- K3: limb-wise add / sub / negate over `polys` (1..3) polynomials of level+1 limbs (ct+ct, ct-ct, -ct).
 * op: 0 add, 1 sub, 2 neg (b ignored, may be null).  out may be a and / or b.  Either scheme.
 * Replaces HEArithmeticOperator::add/sub/negate (executors_gpu.cu:79-173). */
int lsa_poly_addsub(lsa_context ctx, int op, int level, int polys, const uint64_t* a, const uint64_t* b,
                    uint64_t* out, int batch, long long stride_a, long long stride_b, long long stride_out,
                    void* stream);

/* ---- CKKS (NTT-domain ciphertexts) ---------------------------------------------------------------------- */
/* multiply (executors_gpu.cu:185,223): a,b = [2][L][N] -> d3 = [3][L][N]; stride_a / stride_b 0: shared; d3 overlaps no input */
int lsa_ckks_mult(lsa_context ctx, int level, const uint64_t* a, const uint64_t* b, uint64_t* d3, int batch,
                  long long stride_a, long long stride_b, long long stride_d, void* stream);
/* relinearize (executors_gpu.cu:236): d3 -> out [2][L][N]; out overlaps no input */
int lsa_ckks_relin(lsa_context ctx, int level, const uint64_t* d3, lsa_key rlk, uint64_t* out, int batch,
                   long long stride_d, long long stride_out, void* stream);
/* rescale (executors_gpu.cu:246): in [polys][L][N] -> out [polys][L-1][N], level >= 1, polys 1..3; never in place */
int lsa_ckks_rescale(lsa_context ctx, int level, int polys, const uint64_t* in, uint64_t* out, int batch,
                     long long stride_in, long long stride_out, void* stream);
/* rotate_rows / conjugate (executors_gpu.cu:275,289): Galois element g, key of that element; out may be in (same stride) */
int lsa_ckks_rotate(lsa_context ctx, int level, const uint64_t* in, uint64_t galois_element, lsa_key glk,
                    uint64_t* out, int batch, long long stride_in, long long stride_out, void* stream);
/* mod_drop (executors_gpu.cu:257): keep the first L-1 limbs of each polynomial, level >= 1, polys 1..3; either scheme; never in place */
int lsa_drop_level(lsa_context ctx, int level, int polys, const uint64_t* in, uint64_t* out, int batch,
                   long long stride_in, long long stride_out, void* stream);
/* fused HMult + relinearize + rescale: the BASELINE.json headline operator. out = [2][L-1][N], level >= 1; stride_a / stride_b 0:
 * shared; out overlaps no input */
int lsa_ckks_mult_relin_rescale(lsa_context ctx, int level, const uint64_t* a, const uint64_t* b, lsa_key rlk,
                                uint64_t* out, int batch, long long stride_a, long long stride_b,
                                long long stride_out, void* stream);
/* Encrypted inner product: sum_{i<n} a_i x b_i of n >= 1 pairs of ciphertexts with ONE relinearisation (the degree-2 tensors are
 * summed, which is exact; one key switch and one rescale follow).  as[i], bs[i]: [2][rpp][N] per batch item, NTT domain; a_rpp[i],
 * b_rpp[i] rows per polynomial (a null array or an entry of 0: level + 1; an operand kept at a higher level is read through its
 * leading rows); sas[i], sbs[i] batch strides in words, 0 = one ciphertext shared by the whole batch; as[i] == bs[i] squares.
 * addend (nullable): a ciphertext [2][level+1][N] at the product's scale added before the key switch.  The output overlaps no
 * input.  Word for word the composition lsa_ckks_mult per pair, lsa_poly_addsub, lsa_ckks_relin (, lsa_ckks_rescale); with
 * n == 1, no addend and rescale != 0 that is lsa_ckks_mult_relin_rescale.  batch <= 0 is a no-op. */
/* d3 = sum_{i<n} a_i (x) b_i (+ (addend_0, addend_1, 0)):  [3][level+1][N], NTT domain */
int lsa_ckks_mult_sum(lsa_context ctx, int level, int n, const uint64_t* const* as, const long long* sas, const int* a_rpp,
                      const uint64_t* const* bs, const long long* sbs, const int* b_rpp, const uint64_t* addend,
                      long long s_addend, uint64_t* d3, int batch, long long sd, void* stream);
/* out = relin(d3 above), then rescaled when rescale != 0:  [2][level (rescale) | level+1][N] */
int lsa_ckks_dot(lsa_context ctx, int level, int n, const uint64_t* const* as, const long long* sas, const int* a_rpp,
                 const uint64_t* const* bs, const long long* sbs, const int* b_rpp, const uint64_t* addend,
                 long long s_addend, lsa_key rlk, uint64_t* out, int batch, long long sout, int rescale, void* stream);

/* ---- CKKS plaintext and constant operands: a ciphertext combined with something that is not encrypted.  Ciphertexts ct / out are
 * [2][level+1][N] per batch item, plaintexts pt [level+1][N], all NTT domain; batch strides (s*) in words; batch <= 0 is a no-op; a
 * BFV context is LSA_ERR_ARG; error messages begin with the entry point's name.  The words are those of oracle/ckks_bootstrap.py
 * Evaluator.mul_plain / add / sub / mul_const / add_const / mul_by_i on the same operands.  rescale != 0 (level >= 1) runs
 * lsa_ckks_rescale on the result: out is then [2][level][N] and may overlap no input.  Without a rescale the element-wise forms
 * (mult_plain, addsub_plain, mult_const, add_const, affine_const) accept out == ct with sout == sct, and otherwise no overlap.
 * The kernels move 16 bytes per lane: every device pointer must be 16-byte aligned and every batch stride even (LSA_ERR_ARG).
 *
 * lsa_ckks_encode: host complex vectors -> device plaintexts at `scale`.  values: [batch][2^log_slots][2] doubles (re, im),
 * log_slots in 0..log2(N)-1, a shorter vector is tiled over the N/2 slots; out_dev: [batch][level+1][N].  Word for word
 * lsa_lt_plaintext of an lsa_lt_create plan with n_diag = 1, index 0, the same values, pt_scale = scale, double_hoist = 0.
 * LSA_ERR_ARG: scale <= 0, level or log_slots out of range, a value that is not finite or encodes beyond 2^62 (then nothing is
 * written).  Returns after the plaintexts are complete on `stream`. */
int lsa_ckks_encode(lsa_context ctx, int level, int log_slots, const double* values, double scale, uint64_t* out_dev, long long sout,
                    int batch, void* stream);
/* out = ct x pt on both polynomials; spt == 0: one plaintext shared by the whole batch */
int lsa_ckks_mult_plain(lsa_context ctx, int level, const uint64_t* ct, long long sct, const uint64_t* pt, long long spt, uint64_t* out,
                        long long sout, int batch, int rescale, void* stream);
/* op 0: c0 + pt, 1: c0 - pt; c1 is copied when out != ct */
int lsa_ckks_addsub_plain(lsa_context ctx, int op, int level, const uint64_t* ct, long long sct, const uint64_t* pt, long long spt,
                          uint64_t* out, long long sout, int batch, void* stream);
/* out = sum_{i<n} cts[i] x pts[i] (+ addend, a ciphertext at the products' scale; nullable), n >= 1; spts[i] == 0: shared plaintext.
 * 16 terms per launch, later launches add to out; out overlaps no input */
int lsa_ckks_mac_plain(lsa_context ctx, int level, int n, const uint64_t* const* cts, const long long* scts, const uint64_t* const* pts,
                       const long long* spts, const uint64_t* addend, long long s_addend, uint64_t* out, long long sout, int batch,
                       int rescale, void* stream);
/* out = ct x (kre + kim X^(N/2)), kre = round(re * const_scale), kim = round(im * const_scale) (ties to even; beyond 2^62:
 * LSA_ERR_ARG): the slot-wise product with the complex constant re + i im, at scale ct_scale * const_scale.  No plaintext is read
 * (k_cconst).  const_scale = 1, re = 0, im = +-1 is the exact multiplication by +-i. */
int lsa_ckks_mult_const(lsa_context ctx, int level, const uint64_t* ct, long long sct, double re, double im, double const_scale,
                        uint64_t* out, long long sout, int batch, int rescale, void* stream);
/* c0 += round(re * ct_scale) + round(im * ct_scale) X^(N/2): re + i im added to every slot of a ciphertext at scale ct_scale.
 * The rounded integers are 64-bit like every other encoded constant: |re|, |im| times ct_scale must stay below 4.6e18 (about
 * 2^62), else LSA_ERR_ARG -- at ct_scale = 2^60 a constant up to 4 in magnitude, at 2^80 none worth adding.  (The oracle's
 * add_const works on Python integers and has no such cap.) */
int lsa_ckks_add_const(lsa_context ctx, int level, const uint64_t* ct, long long sct, double re, double im, double ct_scale,
                       uint64_t* out, long long sout, int batch, void* stream);
/* out = ct x (re + i im) + (add_re + i add_im) in one pass: the words of lsa_ckks_mult_const(re, im, const_scale) followed by
 * lsa_ckks_add_const(add_re, add_im, ct_scale * const_scale), ct_scale the scale of ct (, then the rescale).  The addend is
 * encoded at the PRODUCT of the two scales, so add_const's cap reads |add_re|, |add_im| < 2^62 / (ct_scale * const_scale): with
 * both scales at 2^40 (2^80) the fused form refuses any addend that does not round to zero.  Keep the product below 2^62 / |beta|
 * (2^30 x 2^30, 2^40 x 2^20), or multiply, rescale and add the constant at the rescaled scale with lsa_ckks_add_const. */
int lsa_ckks_affine_const(lsa_context ctx, int level, const uint64_t* ct, long long sct, double re, double im, double const_scale,
                          double add_re, double add_im, double ct_scale, uint64_t* out, long long sout, int batch, int rescale,
                          void* stream);

/* ---- BFV (coefficient-domain ciphertexts) ---------------------------------------------------------------- */
/* Shapes as for their CKKS namesakes, layout and aliasing as stated above: mult and mult_relin take shared operands (stride 0) and
 * overlap no input, relin and rescale overlap no input, rotate's out may be in (same stride). */
int lsa_bfv_mult(lsa_context ctx, int level, const uint64_t* a, const uint64_t* b, uint64_t* d3, int batch,
                 long long stride_a, long long stride_b, long long stride_d, void* stream);
int lsa_bfv_relin(lsa_context ctx, int level, const uint64_t* d3, lsa_key rlk, uint64_t* out, int batch,
                  long long stride_d, long long stride_out, void* stream);
int lsa_bfv_rotate(lsa_context ctx, int level, const uint64_t* in, uint64_t galois_element, lsa_key glk,
                   uint64_t* out, int batch, long long stride_in, long long stride_out, void* stream);
/* BFV ciphertext x pt_mul plaintext.  A pt_mul plaintext ([level+1][N] words) is the message lifted to Q, in the NTT domain
 * and in Montgomery form (the frontend's BfvPlaintextMulNode).  Per poly and limb: out = INTT(NTT(ct) . pt . 2^-64 mod q),
 * Lattigo v4's mulPlaintextMul.  ct / out: [2][level+1][N] per batch item; out may BE ct (same pointer, same stride) and otherwise
 * overlaps neither ct nor pt; spt == 0: one plaintext for the batch ("Layout and aliasing" above).  LSA_PTMUL_FUSED=0 selects the
 * unfused form (when it is read: INTEGRATION.md section 6). */
int lsa_bfv_mult_plain_mul(lsa_context ctx, int level, const uint64_t* ct, const uint64_t* pt, uint64_t* out, int batch,
                           long long sct, long long spt, long long sout, void* stream);
/* out = sum_{i<n} cts[i] x pts[i] (+ partial when not null), n >= 1, the same products as lsa_bfv_mult_plain_mul, summed in
 * the NTT domain with one inverse transform per output.  out may overlap no input; spts[i] == 0: one plaintext for the batch; no
 * other stride may be 0. */
int lsa_bfv_mac_plain_mul(lsa_context ctx, int level, int n, const uint64_t* const* cts, const long long* scts,
                          const uint64_t* const* pts, const long long* spts, const uint64_t* partial, long long spartial,
                          uint64_t* out, int batch, long long sout, void* stream);
/* Hoisted rotate-and-MAC, the diagonal (Halevi-Shoup) matrix-vector product:
 *   out = sum_{i<n} rotate(in, galois_elements[i]) x pts[i] (+ partial when not null),  n >= 1.
 * galois_elements[i] == 1 is the input itself and takes no key (glk[i] may be null); 2N-1 is the row rotation; every other
 * element needs its Galois key; elements may repeat.  pts[i]: pt_mul plaintexts as for lsa_bfv_mult_plain_mul, batch stride
 * spts[i] (0: one plaintext for the whole batch).  Bit-identical to lsa_bfv_rotate_many followed by lsa_bfv_mac_plain_mul
 * on the same terms.  The input is transformed and decomposed once; the rotations stay in the NTT domain and the rotated
 * ciphertexts are never written.  out may overlap no input.  LSA_ROTMAC_FUSED=0 selects the two-step form (section 6). */
int lsa_bfv_rotate_mac_plain_mul(lsa_context ctx, int level, const uint64_t* in, int n, const uint64_t* galois_elements,
                                 const lsa_key* glk, const uint64_t* const* pts, const long long* spts, const uint64_t* partial,
                                 long long spartial, uint64_t* out, int batch, long long sin, long long sout, void* stream);
int lsa_bfv_rescale(lsa_context ctx, int level, int polys, const uint64_t* in, uint64_t* out, int batch,
                    long long stride_in, long long stride_out, void* stream);
int lsa_bfv_mult_relin(lsa_context ctx, int level, const uint64_t* a, const uint64_t* b, lsa_key rlk,
                       uint64_t* out, int batch, long long stride_a, long long stride_b, long long stride_out,
                       void* stream);
/* Encrypted inner product: sum_{i<n} a_i x b_i of n >= 1 pairs of BFV ciphertexts with ONE scale-down by Q and ONE relinearisation.
 * Only the extension of the operands to Q u QMul and the tensor depend on the pair; the tensors are summed over Q u QMul, where the
 * sum is exact while the auxiliary basis holds it, and the inverse transform, the six base conversions of the division by Q and the
 * key switch run once per output.  The result carries one rounding and one key-switch error instead of n of each, so its words
 * differ from the eager sum of lsa_bfv_mult_relin.
 *   Operands.  as[i], bs[i]: [2][level+1][N] per batch item, coefficient domain, all at `level` (a BFV level change is no row
 *     prefix); sas[i], sbs[i] batch strides in words, 0 = one ciphertext shared by the whole batch (extended once); as[i] == bs[i]
 *     with equal strides is a square and is extended once.  addend (nullable): a ciphertext [2][level+1][N] added to polynomials 0
 *     and 1 AFTER the division, with the words of lsa_poly_addsub.  The output overlaps no input.  Layout as for the first-generation
 *     operators: 16-byte aligned pointers, even strides.
 *   Headroom rule.  The auxiliary basis is sized for ONE product: nmul = ceil((bitlen(Q_full) + log N) / 61) primes of 61 bits
 *     (a coefficient of one tensor is below N (Q/2)^2 * 2, and Q * QMul / 2 has to exceed it).  A sum of m products is at most m
 *     times as large: ceil(log2 m) bits more.  At `level` the context's nmul primes leave
 *         G = min(30, 61 nmul - bitlen(Q_level) - log N) >= 0 bits,   max_terms = 2^G.
 *     The n terms are cut into consecutive groups of max_terms (the last may be shorter).  A group of m terms runs over Q_level and
 *     the FIRST M(m) = (bitlen(Q_level) + log N + ceil(log2 m) + 60) / 61 auxiliary primes -- M(1) is lsa_bfv_mult's count and
 *     M(max_terms) <= nmul -- and is divided by Q on its own; the group results are added in Q (the words of lsa_poly_addsub), and
 *     ONE relinearisation follows.  At the shipped sets the split is rare (G = 24 at N = 2^14 with 6 Q primes, 17 at N = 2^15,
 *     7 at N = 2^13, 30 at every lower level): it is the fallback that keeps every n legal.  lsa_bfv_dot_plan states what a call will do.
 *   With n == 1 and no addend the words are exactly lsa_bfv_mult / lsa_bfv_mult_relin; lsa_bfv_dot equals lsa_bfv_relin of
 *     lsa_bfv_mult_sum word for word.  LSA_BFV_FOLD=0 selects the unfolded extension and tail as it does for lsa_bfv_mult.
 *   LSA_ERR_ARG before anything is queued, the message beginning "bfv_dot": a CKKS context, n < 1, level out of range, a null
 *     pointer, a short, negative or odd stride, a pointer off the 16-byte grid, a missing key or one exported below `level`, an
 *     overlap of the output with an input.  batch <= 0 is a no-op. */
/* d3 = t * round( sum_i a_i (x) b_i / Q ) (+ (addend_0, addend_1, 0)):  [3][level+1][N], coefficient domain */
int lsa_bfv_mult_sum(lsa_context ctx, int level, int n, const uint64_t* const* as, const long long* sas, const uint64_t* const* bs,
                     const long long* sbs, const uint64_t* addend, long long s_addend, uint64_t* d3, int batch, long long sd,
                     void* stream);
/* out = relin(d3 above):  [2][level+1][N] */
int lsa_bfv_dot(lsa_context ctx, int level, int n, const uint64_t* const* as, const long long* sas, const uint64_t* const* bs,
                const long long* sbs, const uint64_t* addend, long long s_addend, lsa_key rlk, uint64_t* out, int batch,
                long long sout, void* stream);
/* host only, no context and no device: what the two entry points above will do with `terms` pairs at `level` of the chain q[nq] at
 * ring degree n_ring -- max_terms = 2^G, the number of groups, and the auxiliary limbs M(min(terms, max_terms)) of the first group
 * (a full one when there are several).  Every output pointer is nullable. */
int lsa_bfv_dot_plan(int n_ring, const uint64_t* q, int nq, int level, int terms, int* max_terms, int* n_groups, int* aux_limbs);

/* ---- tuning / introspection */
/* pairs that lsa_bfv_mult_sum / lsa_bfv_dot extend per tensor launch (0 = the measured default; at most 16, and never so many that
 * the batch tile falls below lsa_bfv_mult's).  The words are the same for every value; workspace grows by 4 (L + M) rows per pair. */
int lsa_set_bfv_dot_chunk(lsa_context ctx, int pairs);
/* ciphertexts processed per kernel wave inside the fused operators (0 = automatic) */
int lsa_set_tile_batch(lsa_context ctx, int tile_batch);
/* NTT butterfly engine for limbs with q < 2^47: 1 (default) = exact FP64-FMA butterflies, 0 = integer Montgomery for
 * every limb.  Both produce identical residues; the switch exists for A/B measurement and parity tests. */
int lsa_set_fp64_ntt(lsa_context ctx, int enable);
/* 1: alternate tiles of a batched operator run on the caller's stream and on an internal auxiliary stream (fork/join
 * with events inside the call), so two independent tiles overlap (+5 % measured); 0 (default): everything on the
 * caller's stream, which keeps per-kernel timings attributable. */
int lsa_set_dual_stream(lsa_context ctx, int enable);
/* 1 (default): the ModDown and rescale element-wise tails run inside the NTT kernel's load/store phases; 0: separate
 * kernels (A/B measurement; identical results). */
int lsa_set_fuse_tails(lsa_context ctx, int enable);
/* 1 (default): a key-switch digit with one source limb below 2^53 gets no base-conversion launch, the load of its extension
 * transform lifts it (x mod p_t); 0: the conversion kernel for those digits too (A/B measurement and parity; identical
 * results).  Read by every operator call. */
int lsa_set_modup_lift(lsa_context ctx, int enable);
/* CKKS HMult+relin+rescale with the tensor fold: the fused key MAC finishes the rescaled FP64-engine limbs from its running sums
 * instead of writing the accumulator's Q rows for the epilogue pass to read back.  0: never; 1 (default): on rings whose second
 * NTT pass has eight stages (N = 2^16, the measured shape); 2: wherever the shape allows (also seven-stage second passes,
 * N = 2^14).  Identical results for every value; another value is refused (LSA_ERR_ARG).  Read by every operator call. */
int lsa_set_ks_tail_in_mac(lsa_context ctx, int mode);
/* Merged ModDown + rescale: ModDown's base conversion P -> Q also reads INTT(acc_l) (and INTT(base_l) where the caller has a
 * base), forms t = (INTT(acc_l) - conv_l) * P^-1 (+ base_l) in registers and stores in_j = conv_j * P^-1 + lift_j(t) itself, so
 * that the element-wise kernel that wrote t goes away and the forward transform of in_j runs without a load-side prologue.
 * 0: never; 1 (default): rings with N >= 2^16; 2: every ring.  Needs lsa_set_fuse_tails(ctx, 1) and level >= 1, else the
 * earlier sequence runs.  Identical results for every value; another value is refused (LSA_ERR_ARG).  Read by every operator
 * call. */
int lsa_set_rescale_head_in_conv(lsa_context ctx, int mode);
/* Two-pass NTTs (N > 2^12) run both passes over a chunk of at most `mib` MiB of limbs before moving on, so that the
 * second pass is served by the 256 MiB Infinity Cache (0, the default = one launch per pass over the whole batch).  Results are
 * identical for every value: the setting only changes how many batch items one launch covers, and the operands of the fused
 * load / store steps follow their chunk.  Single-pass rings (N <= 2^12) ignore it; a negative value is refused (LSA_ERR_ARG)
 * and leaves the setting as it was. */
int lsa_set_ntt_chunk_mib(lsa_context ctx, int mib);
/* Rotations of the same ciphertexts by several Galois elements with ONE decomposition of the input ("hoisting"):
 * outs[i] = rotate(in, galois_elements[i]), each bit-identical to lsa_ckks_rotate's result.  The outputs (all with stride sout)
 * overlap each other nowhere; at most one may BE the input (same pointer, sout == sin), every other one is apart from it. */
int lsa_ckks_rotate_many(lsa_context ctx, int level, const uint64_t* in, int n_rot, const uint64_t* galois_elements,
                         const lsa_key* glk, uint64_t* const* outs, int batch, long long sin, long long sout, void* stream);
/* The same for BFV (coefficient-domain ciphertexts): outs[i] = rotate(in, galois_elements[i]), each bit-identical to
 * lsa_bfv_rotate's result.  The input's c1 is transformed and decomposed once; each key then costs its MAC and ModDown only,
 * the automorphism riding on the ModDown tail.  Layout as for lsa_ckks_rotate_many: the outputs overlap each other nowhere, at most
 * one may BE the input (same pointer, sout == sin), every other one is apart from it; no stride 0; a key exported below `level` is
 * refused. */
int lsa_bfv_rotate_many(lsa_context ctx, int level, const uint64_t* in, int n_rot, const uint64_t* galois_elements,
                        const lsa_key* glk, uint64_t* const* outs, int batch, long long sin, long long sout, void* stream);

/* ---- CKKS bootstrapping: the `bootstrap` node of a task graph (reference: mega_ag_executors_gpu.cu:410-426 calls HEonGPU's
 * regular_bootstrapping_v2; configuration gpu_wrapper.cu:86-117 / custom_task.py:383-468).  A plan holds the encoded
 * CoeffsToSlots / SlotsToCoeffs diagonals (depths cts_depth / stc_depth, full-slot encoding), the EvalMod constants
 * (cosine of range k with `double_angle` doublings, message ratio) and the list of Galois elements a run needs -- the
 * rotation set of the reference's planner (frontend/bootstrap_params.py:104-263) plus the conjugation.  in_scale: scale
 * of the level-0 input; out_scale: scale the refreshed ciphertext must have (0: whatever falls out).  The context's chain
 * must have cts_depth + 5 + double_angle + stc_depth levels above the output level.  log_slots: 0 or log2(N)-1 for dense
 * packing, smaller for sparsely packed ciphertexts (SubSum, one EvalMod on the packed real|imaginary halves, repacking
 * SlotsToCoeffs).  The matrices of a sparse plan (lsa_bootstrap_info: sparse = 1) are ordered
 * [n_cts leading CoeffsToSlots ..., P1, P2, SlotsToCoeffs ...], those of a dense plan [n_cts CoeffsToSlots, SlotsToCoeffs ...].
 * lsa_ckks_bootstrap: in [batch][2][1][N] -> out [batch][2][out_level+1][N]; swk_dts / swk_std (both or neither) are the
 * sparse-secret encapsulation keys at level 0 / top level (custom_task.py:1989-1996). */
typedef struct lsa_bootstrap_st* lsa_bootstrap;
int lsa_bootstrap_create(lsa_context ctx, int cts_depth, int stc_depth, int k, int double_angle, double message_ratio,
                         double in_scale, double out_scale, int log_slots, void* stream, lsa_bootstrap* out);
/* the same with the EvalMod polynomial degrees the reference forwards (gpu_wrapper.cu:100-103): sine_deg 1..63 (the cosine
 * interpolant takes ceil(log2(sine_deg+1)) levels), arcsine_deg 0 (none) or odd <= 15 (ceil(log2(arcsine_deg+1)) more levels) */
int lsa_bootstrap_create_ex(lsa_context ctx, int cts_depth, int stc_depth, int k, int double_angle, double message_ratio,
                            double in_scale, double out_scale, int log_slots, int sine_deg, int arcsine_deg, void* stream,
                            lsa_bootstrap* out);
int lsa_bootstrap_evalmod_constants(lsa_bootstrap b, int* n_cheb, double* cheb, int* n_asin, double* asin_coef);
void lsa_bootstrap_destroy(lsa_bootstrap b);
int lsa_bootstrap_info(lsa_bootstrap b, int* out_level, double* out_scale, int* n_galois, int* n_matrices, int* n_cts,
                       int* sparse);
int lsa_bootstrap_galois_elements(lsa_bootstrap b, uint64_t* out, int capacity);
/* the plan's floating-point constants, exported so that a checker can replay the program with the same integers */
int lsa_bootstrap_chebyshev(lsa_bootstrap b, double* out32);
int lsa_bootstrap_matrix_info(lsa_bootstrap b, int index, int* level, int* n1, int* n_diagonals, int* diagonals, int capacity);
/* lsa_bootstrap_plaintext writes the (level + 1) * N words at q_0..q_level.  A baby-step / giant-step matrix of a double-hoisting
 * plan (the default; LSA_BT_DOUBLE_HOIST=0 at plan creation turns it off) also carries the residues at the k special primes, because
 * its inner sums are formed over Q u P before ONE division by P per giant step (Lattigo v4 ckks/linear_transform.go,
 * MultiplyByDiagMatrixBSGS): lsa_bootstrap_plaintext_rows reports level + 1 or level + 1 + k, lsa_bootstrap_plaintext_ext writes
 * all rows * N words (capacity checked). */
int lsa_bootstrap_plaintext(lsa_bootstrap b, int matrix, int diag_pos, uint64_t* host_out);
int lsa_bootstrap_plaintext_rows(lsa_bootstrap b, int matrix, int* rows);
int lsa_bootstrap_plaintext_ext(lsa_bootstrap b, int matrix, int diag_pos, uint64_t* host_out, long long capacity_words);
int lsa_ckks_bootstrap(lsa_context ctx, lsa_bootstrap b, const uint64_t* in, uint64_t* out, int batch, long long sin, long long sout,
                       lsa_key rlk, int n_glk, const uint64_t* glk_elements, const lsa_key* glk, lsa_key swk_dts, lsa_key swk_std,
                       void* stream);

/* ---- CKKS linear transform: plaintext matrix x encrypted vector, the matrix in diagonal form (matrix-vector products,
 * convolutions, CoeffsToSlots / SlotsToCoeffs steps).  The evaluator is the one bootstrapping runs on its own matrices; the CPU
 * oracle of both is oracle/ckks_bootstrap.py linear_transform, whose semantics these are exactly:
 *   fewer than three diagonals: one rotation per diagonal, no baby-step / giant-step split;
 *   otherwise n1 = the reference planner's split at bsgs_ratio (frontend/bootstrap_params.py:193-207), diagonal k = giant + baby
 *   with giant = floor(k / n1) * n1, M x = sum_giant rot_giant( sum_baby rot_{-giant}(d_k) . rot_baby(x) ), giant step 0 first.
 * M in diagonal form: diagonal k (index taken mod period, period = 2^log_slots; negative indices allowed) holds `period`
 * complex values, d_k[t] multiplies x[(t + k) mod period].  values: [n_diag][period][2] doubles (re, im).  level: the level of
 * the ciphertexts the plan will be applied to.  pt_scale: encoding scale of the diagonals, 0 = q_level (then the rescale leaves
 * the ciphertext's scale unchanged); in general the result decrypts at in_scale * pt_scale (/ q_level after the rescale).
 * bsgs_ratio: 0 = 2.0, the reference planner's ratio.  double_hoist: 1 = the baby-step rotations and the inner sums stay over
 * Q_level u P and are divided by P once per giant step and once at the end (giant steps + 1 divisions: Lattigo v4
 * MultiplyByDiagMatrixBSGS); 0 = one division per rotation.  The plaintext of diagonal k is the encoding of rot_{-giant}(d_k)
 * tiled over the N/2 slots, over Q_level (no double hoisting, or fewer than three diagonals) or Q_level u P.
 * Errors (LSA_ERR_ARG): level out of range, a BFV context, log_slots > log2(N) - 1, two indices equal modulo the period, a value
 * that encodes beyond 2^62.  The plan keeps its plaintexts and the temporaries of its runs on the device until destroyed; it
 * belongs to its context and runs on one stream at a time. */
typedef struct lsa_linear_transform_st* lsa_linear_transform;
int lsa_lt_create(lsa_context ctx, int level, int log_slots, int n_diag, const int* diag_index, const double* values,
                  double pt_scale, double bsgs_ratio, int double_hoist, void* stream, lsa_linear_transform* out);
void lsa_lt_destroy(lsa_linear_transform lt);
/* n1: the baby-step count, 0 = no split (fewer than three diagonals); rows: rows of each plaintext, level + 1 or level + 1 + k;
 * any output pointer may be null */
int lsa_lt_info(lsa_linear_transform lt, int* level, int* period, int* n_diag, int* n1, int* rows, int* n_galois,
                int* double_hoist, double* pt_scale);
int lsa_lt_diagonals(lsa_linear_transform lt, int* index_out, int capacity); /* ascending, reduced mod period */
/* Galois elements of the rotations a run needs a key for (ascending) */
int lsa_lt_galois_elements(lsa_linear_transform lt, uint64_t* out, int capacity);
/* the encoded diagonal at position diag_pos of lsa_lt_diagonals' order: rows * N words, NTT domain */
int lsa_lt_plaintext(lsa_linear_transform lt, int diag_pos, uint64_t* host_out, long long capacity_words);
/* in [batch][2][level+1][N] (NTT domain) -> out [batch][2][level (rescale) | level+1 (no rescale)][N], batch strides sin / sout in
 * words; out may not overlap in (LSA_ERR_ARG); batch <= 0 is a no-op.  glk_elements / glk: n_glk Galois keys, in any order and
 * possibly more than needed; a missing one fails with LSA_ERR_ARG (the message names the element) before any work is queued.
 * Switches (when each is read: INTEGRATION.md section 6): LSA_LT_BLOCKED_MAC=0 (matrices beyond 8 x 8 baby / giant steps: one
 * multiply-accumulate launch per giant step instead of 8 x 8 blocks), LSA_ROT_SCATTER=0 (rotations as MAC + permutation kernel), LSA_LT_GIANT_SCATTER=0 / 1
 * (giant-step rotations alone).  Every combination produces the same words. */
int lsa_ckks_linear_transform(lsa_context ctx, lsa_linear_transform lt, const uint64_t* in, uint64_t* out, int batch,
                              long long sin, long long sout, int rescale, int n_glk, const uint64_t* glk_elements,
                              const lsa_key* glk, void* stream);
/* host only, needs no device: the split (n1, 0 = none) and the non-zero rotations (ascending, reduced mod period) that a
 * diagonal index set gets -- what lsa_lt_create will pick.  count receives their number; LSA_ERR_ARG if capacity is less. */
int lsa_lt_plan_rotations(int period, int n_diag, const int* diag_index, double bsgs_ratio, int* n1, int* rotations,
                          int capacity, int* count);

/* ---- CKKS slot sum: out = sum_{i<count} rot(ct, i*step), the sum over slots that follows a packed product (Lattigo InnerSum);
 * Replicate is the same operation with a negative step (step = -batch_size).  The plan is a state (x, s, n, tail) starting at
 * (ct, step, count, none) with the invariant  result = sum_{i<n} rot(x, i*s) + tail.  While n > 1 one STEP runs, one decomposition of
 * x's c1 with up to four Galois keys:
 *   1. n odd: the rotation (n-1)*s joins the step with destination TAIL, n -= 1;
 *   2. radix 4 and n % 4 == 0: the rotations s, 2s, 3s with destination NEXT, s *= 4, n /= 4;
 *      otherwise: the rotation s with destination NEXT, s *= 2, n /= 2;
 *   3. x <- x + ModDown(sum of the NEXT rotations), the sum formed over Q_level u P and divided by P once; the TAIL rotation is
 *      added to an extended accumulator that is not divided.
 * At n == 1: out = x + ModDown(tail) if a tail exists, else x.  Rotations are reduced mod N/2.  Every extended rotation is
 * automorphism_g(P c0 + ks0, ks1) with ks the gadget product of c1 with the key of g = 5^rotation mod 2N; the CPU restatement is
 * tests/slot_sum_model.py on oracle/ckks_bootstrap.py (rotate_ext, add_ext, moddown, add), whose words the device gives exactly.
 * radix: 2 (the key set of Lattigo's InnerSumLog: 2^i * step for i < floor(log2 count), plus one offset per set bit of count
 * below the highest), 4 (one decomposition and one division less per two bits of count, one more key MAC and Galois key), or
 * 0 = the default, 4: faster than 2 on the MI355X at every measured shape.  count == 1 is a copy and needs no key.
 * Errors (LSA_ERR_ARG, the message names the argument): count < 1, count > N/2, radix not 0 / 2 / 4, a step that makes a planned
 * rotation a multiple of N/2; for a plan also a BFV context and a level out of range. */
typedef struct lsa_slot_sum_st* lsa_slot_sum;
/* host only, needs no device and no context: the counts of the plan (steps = decompositions, key MACs, divisions by P) and its
 * rotations (ascending, distinct, reduced mod N/2).  Any output pointer may be null; n_rot receives the number of rotations;
 * LSA_ERR_ARG if `rotations` is given and capacity is less. */
int lsa_slot_sum_plan(int n_ring, long long step, int count, int radix, int* n_steps, int* n_keyswitch, int* n_moddown,
                      int* rotations, int capacity, int* n_rot);
int lsa_slot_sum_create(lsa_context ctx, int level, long long step, int count, int radix, lsa_slot_sum* out);
void lsa_slot_sum_destroy(lsa_slot_sum plan);
/* radix: the one in force (never 0); any output pointer may be null */
int lsa_slot_sum_info(lsa_slot_sum plan, int* level, int* count, int* radix, int* n_steps, int* n_keyswitch, int* n_moddown,
                      int* n_galois);
/* Galois elements of the rotations a run needs a key for (ascending) */
int lsa_slot_sum_galois_elements(lsa_slot_sum plan, uint64_t* out, int capacity);
/* A/B and parity: 1 makes the steps with several keys run ONE multi-key MAC launch (k_ks_mac_multi: every digit value read once
 * for all keys, each key's product in its own buffer, k_ext_sum joining them) instead of one single-key MAC launch per key, each
 * adding to its destination (default 0: the multi-key launch measured 6-10 % slower).  The same words either way. */
int lsa_slot_sum_set_multi_mac(lsa_slot_sum plan, int enable);
/* in [batch][2][level+1][N] (NTT domain) -> out, the same shape; batch strides sin / sout in words.  out may be in itself (same
 * pointer, same stride) and otherwise may not overlap it (LSA_ERR_ARG); batch <= 0 is a no-op.  galois_elements / keys: n_keys
 * Galois keys at the plan's level or above, in any order and possibly more than needed; a missing one fails with LSA_ERR_ARG (the
 * message names the element) before any work is queued.  The plan belongs to its context. */
int lsa_ckks_slot_sum(lsa_context ctx, lsa_slot_sum plan, const uint64_t* in, uint64_t* out, int batch, long long sin,
                      long long sout, int n_keys, const uint64_t* galois_elements, const lsa_key* keys, void* stream);

/* ---- BFV slot sum: out = sum_{i<count} rot_cols(y, i*step), y = ct + rot_rows(ct) if rows != 0, else ct -- the sum over slots
 * that finishes a packed BFV inner product (lsa_bfv_dot).  BFV slots form a 2 x N/2 matrix: the column rotation r is the Galois
 * element 5^(r mod N/2) mod 2N, the row swap is 2N-1; count = N/2 with rows = 1 leaves the total in every slot.  ct and out are
 * [2][level+1][N] in the coefficient domain.  The plan is the one of the CKKS slot sum above -- state (x, s, n, tail), radix 2 or
 * 4, TAIL and NEXT keys, at most four keys per step -- started at x = y; with rows != 0 one more step runs before the column
 * steps, one decomposition of ct's c1 with one NEXT key, the key of 2N-1.  count == 1, rows == 0 is a copy and needs no key;
 * count == 1, rows != 0 is the row step alone.
 * The words: every limb of ct transformed to the NTT domain, the steps run as tests/bfv_slot_sum_model.py states them on
 * oracle/ckks_bootstrap.py's rotate_ext, add_ext, moddown and add (the row step is rotate_ext with g = 2N-1), the result transformed
 * back.  One step is x <- x + ModDown(sum of the NEXT extended rotations of x): the sum is formed over Q_level u P and divided by P
 * ONCE; the TAIL rotations join an accumulator that is divided once, after the last step.  These words DIFFER from the chain of
 * lsa_bfv_rotate + lsa_poly_addsub, which divides (and rounds) once per rotation; both decrypt to the same slot sum mod t.
 * radix: 2, 4 or 0 = the default, 4.  Errors are LSA_ERR_ARG before anything is queued, with a message that begins
 * "lsa_bfv_slot_sum" and names the argument: a CKKS context, a level out of range, count < 1, count > N/2, radix not 0 / 2 / 4, a
 * planned rotation that is a multiple of N/2, a missing key (the message names the element), a key below the plan's level, a plan
 * of another context, lsa_bfv_slot_sum_set_gather(plan, 1) on a ring above 2^14. */
/* (the handle cannot be called lsa_bfv_slot_sum: C keeps typedef and function names in one name space) */
typedef struct lsa_bfv_slot_sum_st* lsa_bfv_slot_sum_handle;
/* host only, needs no device and no context: the counts of the plan (steps = decompositions, key MACs, divisions by P) and the
 * Galois elements a run needs a key for (ascending, distinct).  Any output pointer may be null; n_galois receives their number;
 * LSA_ERR_ARG if `galois_elements` is given and capacity is less. */
int lsa_bfv_slot_sum_plan(int n_ring, long long step, int count, int radix, int rows, int* n_steps, int* n_keyswitch, int* n_moddown,
                          uint64_t* galois_elements, int capacity, int* n_galois);
int lsa_bfv_slot_sum_create(lsa_context ctx, int level, long long step, int count, int radix, int rows, lsa_bfv_slot_sum_handle* out);
void lsa_bfv_slot_sum_destroy(lsa_bfv_slot_sum_handle plan);
/* radix: the one in force (never 0); rows: 0 or 1; gather: the tail in force (below); any output pointer may be null */
int lsa_bfv_slot_sum_info(lsa_bfv_slot_sum_handle plan, int* level, int* count, int* radix, int* rows, int* n_steps, int* n_keyswitch,
                          int* n_moddown, int* n_galois, int* gather);
int lsa_bfv_slot_sum_galois_elements(lsa_bfv_slot_sum_handle plan, uint64_t* out, int capacity);   /* ascending */
/* 1 (the default where N <= 2^14): the rotated c0 terms never enter the NTT domain -- the division by P is exact on a multiple
 * of P, ModDown(P z + a) = z + ModDown(a) residue for residue, so the ModDown tail gathers them in the coefficient domain from
 * the c0 row staged in LDS (k_bfv_slot_tail).  0 (the only form above 2^14, selectable everywhere for A/B): c0 is transformed as
 * well and rides through the key MAC and the division as P c0, the CKKS form.  The same words either way. */
int lsa_bfv_slot_sum_set_gather(lsa_bfv_slot_sum_handle plan, int enable);
/* in [batch][2][level+1][N] (coefficient domain) -> out, the same shape; batch strides sin / sout in words, even, pointers
 * 16-byte aligned.  out may be in itself (same pointer, same stride) and otherwise may not overlap it; batch <= 0 is a no-op.
 * galois_elements / keys: n_keys Galois keys at the plan's level or above, in any order and possibly more than needed. */
int lsa_bfv_slot_sum(lsa_context ctx, lsa_bfv_slot_sum_handle plan, const uint64_t* in, uint64_t* out, int batch, long long sin,
                     long long sout, int n_keys, const uint64_t* galois_elements, const lsa_key* keys, void* stream);

/* ---- BFV oblivious expansion (coefficient extraction; the Expand of SealPIR / OnionPIR / Spiral, Lattigo's rlwe.Expand): one
 * ciphertext of m(X) = sum_i m_i X^i becomes `count` ciphertexts, 1 <= count <= N, k = ceil(log2 count) levels.  State: a list
 * c[a] of coefficient-domain ciphertexts [2][level+1][N], c[0] = in.  Level j = 0 .. k-1 has the Galois element g_j = N / 2^j + 1
 * and the shift s = 2^j; for every node a < min(2^j, count):
 *   sigma   = rotate(c[a], g_j)              the words of lsa_bfv_rotate
 *   c'[a]   = c[a] + sigma                   the words of lsa_poly_addsub op 0 on both polynomials
 *   c'[a+s] = X^(-s) * (c[a] - sigma)        only if a + s < count: lsa_poly_addsub op 1, then lsa_bfv_mul_monomial by -s
 *                                            (coefficient y lands on (y - s) mod N, negated when y < s)
 * Output i decrypts to 2^k * sum_u m_(i + 2^k u) X^(2^k u); the full expansion count = N leaves 2^k m_i in the constant coefficient.
 * The plaintext modulus t is odd, so the caller removes the factor by encrypting m * 2^-k mod t.  The key switches number
 * sum_j min(2^j, count), the keys are the Galois elements N / 2^j + 1, j < k; count == 1 is a copy and needs no key.
 * The words are those of the composition above (tests/bfv_expand_model.py), whichever tail runs.
 * Layout: the output is index-major, output i of batch item b at out + i * s_index + b * sout, s_index >= batch * sout; all levels
 * work inside the output array, nothing is allocated beyond the context workspace.  `in` (batch stride sin) may be output 0 itself
 * (same pointer, sin == sout) and otherwise overlaps no output.  On the dense layout (s_index == batch * sout) a level runs as one
 * batched key switch over its nodes x batch items, otherwise one per node.  Keys must be at the plan's level or above, in any
 * order and possibly more than needed; batch <= 0 is a no-op.
 * Errors are LSA_ERR_ARG before anything is queued, with a message that begins with the entry point's name and names the
 * argument: a CKKS context, a level out of range, count < 1 or count > N, a chain without a special prime when count > 1, a null
 * pointer, a pointer off the 16-byte grid, an odd or short stride, s_index < batch * sout, a forbidden overlap, a missing key (the
 * element is named), a key below the plan's level, a plan of another context, lsa_bfv_expand_set_gather(plan, 1) on a ring above
 * 2^14.  A refused call leaves the buffers untouched and the context usable. */
typedef struct lsa_bfv_expand_st* lsa_bfv_expand_handle;
/* host only, needs no device and no context: the levels, the key switches and the Galois elements a run needs a key for (ascending,
 * distinct).  Any output pointer may be null; LSA_ERR_ARG if `galois_elements` is given and capacity is less. */
int lsa_bfv_expand_plan(int n_ring, int count, int* n_levels, int* n_keyswitch, uint64_t* galois_elements, int capacity, int* n_galois);
int lsa_bfv_expand_create(lsa_context ctx, int level, int count, lsa_bfv_expand_handle* out);
void lsa_bfv_expand_destroy(lsa_bfv_expand_handle plan);
/* gather: the plan's setting (below); any output pointer may be null */
int lsa_bfv_expand_info(lsa_bfv_expand_handle plan, int* level, int* count, int* n_levels, int* n_keyswitch, int* n_galois, int* gather);
int lsa_bfv_expand_galois_elements(lsa_bfv_expand_handle plan, uint64_t* out, int capacity);   /* ascending */
/* 1 (the default where N <= 2^14): the ModDown tail of a level's key switch stages (acc - conv) / P (+ c0) in LDS, gathers the
 * rotation from there and writes both children (k_bfv_expand_tail).  0 (the only form above 2^14, and what lsa_set_fuse_tails(0)
 * runs): the key switch leaves (c0 + ks0, ks1) in the workspace and k_bfv_expand_combine gathers the rotation from global memory.
 * The same words either way. */
int lsa_bfv_expand_set_gather(lsa_bfv_expand_handle plan, int enable);
int lsa_bfv_expand(lsa_context ctx, lsa_bfv_expand_handle plan, const uint64_t* in, long long sin, uint64_t* out, long long sout,
                   long long s_index, int batch, int n_keys, const uint64_t* galois_elements, const lsa_key* keys, void* stream);
/* out = X^exponent * in on `polys` (1..3) coefficient-domain polynomials [polys][level+1][N] of a BFV context: the negacyclic shift,
 * coefficient y lands on (y + e) mod N and is negated when (y + e) mod 2N >= N, e = exponent mod 2N (any exponent).  Batch strides in
 * words, even, pointers 16-byte aligned; the output overlaps nothing; batch <= 0 is a no-op. */
int lsa_bfv_mul_monomial(lsa_context ctx, int level, int polys, long long exponent, const uint64_t* in, uint64_t* out, int batch,
                         long long sin, long long sout, void* stream);

/* ---- BFV coefficient packing (PackLWEs of Chen, Dai, Kim, Song, "Efficient homomorphic conversion between (Ring) LWE
 * ciphertexts", Alg. 3 plus the field trace; Lattigo's rlwe.Pack), the expansion run backwards: `count` coefficient-domain
 * ciphertexts c[i], each [2][level+1][N], 1 <= count <= N, become one.  Let k = ceil(log2 count).  Levels run j = k-1 down to 0;
 * with l = k - j a level has the shift s = N / 2^l and the Galois element g = 2^l + 1; for every node a < 2^j:
 *   paired (a + 2^j < count):   xb = X^s * c[a + 2^j]           the words of lsa_bfv_mul_monomial by +s
 *                               u  = c[a] + xb,  v = c[a] - xb   lsa_poly_addsub op 0 / op 1 on both polynomials
 *   unpaired:                   u  = v = c[a]
 *   c'[a] = u + rotate(v, g)                                     lsa_bfv_rotate, then lsa_poly_addsub op 0
 * Only the first level (j = k-1) can have unpaired nodes; its paired nodes are a < count - 2^(k-1).  With trace != 0 the levels
 * l = k+1 .. log2 N follow on c[0] alone: c[0] <- c[0] + rotate(c[0], 2^l + 1).  The result is c[0].  It decrypts to a polynomial
 * whose coefficient i * N/2^k is F * (coefficient 0 of input i) for i < count, F = 2^k without the trace and F = N with it.  With
 * the trace every other coefficient is 0, the positions i * N/2^k with i >= count among them; without it the other coefficients
 * are unspecified mixtures (zero if the inputs were zero there).  t is odd, so the caller removes F by scaling by F^-1 mod t.  The
 * key switches number (2^k - 1) + (trace ? log2 N - k : 0), the keys are the Galois elements 2^l + 1 for l = 1 .. k, or
 * l = 1 .. log2 N with the trace; count == 1 without the trace is a copy and needs no key.
 * The words are those of the composition above (tests/bfv_pack_model.py), whichever tail runs.
 * Layout: the inputs are index-major, as the expansion's outputs are: input i of batch item b at in + i * s_index + b * sin,
 * s_index >= batch * sin.  All levels but the last work inside the input array, so `in` is not const and the inputs count as
 * consumed; unchanged are the inputs i >= max(1, 2^(k-1)), which are only ever read, and every word of the array that is not part
 * of an input.  The last level (j = 0, or the last trace level) writes `out` with batch stride sout; `out` may be input 0 itself
 * (same pointer, sout == sin) and otherwise overlaps no input.  On the dense layout (s_index == batch * sin) a level runs as one
 * batched key switch over its nodes x batch items, otherwise one per node; nothing is allocated beyond the context workspace.  Keys
 * must be at the plan's level or above, in any order and possibly more than needed; batch <= 0 is a no-op.
 * Errors are LSA_ERR_ARG before anything is queued, with a message that begins with the entry point's name and names the
 * argument: a CKKS context, a level out of range, count < 1 or count > N, a ring below N = 512 when count > 1, a chain without a
 * special prime when a key switch is needed, a null pointer, a pointer off the 16-byte grid, an odd or short stride,
 * s_index < batch * sin, a forbidden overlap, a missing key (the element is named), a key below the plan's level, a plan of another
 * context, lsa_bfv_pack_set_gather(plan, 1) on a ring above 2^14.  A refused call leaves the buffers untouched and the context
 * usable. */
typedef struct lsa_bfv_pack_st* lsa_bfv_pack_handle;
/* host only, needs no device and no context: the tree levels (k), the trace levels, the key switches and the Galois elements a run
 * needs a key for (ascending, distinct).  Any output pointer may be null; LSA_ERR_ARG if `galois_elements` is given and capacity
 * is less. */
int lsa_bfv_pack_plan(int n_ring, int count, int trace, int* n_levels, int* n_trace_levels, int* n_keyswitch, uint64_t* galois_elements,
                      int capacity, int* n_galois);
int lsa_bfv_pack_create(lsa_context ctx, int level, int count, int trace, lsa_bfv_pack_handle* out);
void lsa_bfv_pack_destroy(lsa_bfv_pack_handle plan);
/* gather: the plan's setting (below); any output pointer may be null */
int lsa_bfv_pack_info(lsa_bfv_pack_handle plan, int* level, int* count, int* trace, int* n_levels, int* n_trace_levels, int* n_keyswitch,
                      int* n_galois, int* gather);
int lsa_bfv_pack_galois_elements(lsa_bfv_pack_handle plan, uint64_t* out, int capacity);   /* ascending */
/* 1 (the default where N <= 2^14): a paired level's head k_bfv_pack_diff writes v1 = a1 - X^s b1 as the key switch's source, and
 * the ModDown tail stages (acc - conv) / P (+ a0 - X^s b0) in LDS, gathers the rotation from there and adds u = a + X^s b
 * (k_bfv_pack_tail).  0 (the only form above 2^14, and what lsa_set_fuse_tails(0) runs): the head writes the whole v, the key
 * switch leaves (v0 + ks0, ks1) in the workspace and k_bfv_pack_combine gathers the rotation from global memory.  The same words
 * either way. */
int lsa_bfv_pack_set_gather(lsa_bfv_pack_handle plan, int enable);
int lsa_bfv_pack(lsa_context ctx, lsa_bfv_pack_handle plan, uint64_t* in, long long sin, long long s_index, uint64_t* out, long long sout,
                 int batch, int n_keys, const uint64_t* galois_elements, const lsa_key* keys, void* stream);

/* ---- BFV external product RLWE x RGSW, CMux and select by an encrypted index: the "compute" between lsa_bfv_expand and lsa_bfv_pack
 * in the schemes they were taken from (OnionPIR, Spiral, RGSW selectors, blind rotation).  Noise growth is additive and there is no
 * scale-down.
 *   RGSW ciphertext.  An RGSW ciphertext of a small polynomial m under the secret s is a pair of switching keys (R0, R1) in the layout
 *     lsa_key_upload takes ([beta][2][klvl+1+np][N], NTT domain) and uploaded with it: R0 is what oracle/client.py
 *     Client.gen_switching_key(s_in = m, s_out = s, klvl) makes (its rows encrypt P * m on the limbs of digit d), R1 is
 *     gen_switching_key(s_in = m * s, s_out = s, klvl); m is given as its NTT per modulus of Q u P, as Client.s_ntt is.
 *   External product.  ct is a coefficient-domain ciphertext [2][level+1][N]:
 *       acc = gadget_product(NTT(ct[0]), R0) + gadget_product(NTT(ct[1]), R1)     over Q_level u P, limb by limb, canonical
 *       out = INTT(moddown(acc)) (+ base on both polynomials)
 *     In oracle/pyoracle.py: Oracle.gadget_product twice, Oracle.vec("add") on every one of the level+1+np rows of both polynomials,
 *     Oracle.moddown (tests/rgsw_model.py).  ONE ModDown: two key switches and an add would round differently.  out decrypts to
 *     m * plaintext(ct) (+ plaintext(base)).  The tail reads base only at the points it writes: out may be base, or ct, itself.
 *   CMux.  lsa_bfv_cmux(c0, c1, R) = c0 + R [.] (c1 - c0): the difference is the words of lsa_poly_addsub op 1 on both polynomials,
 *     the sum is the ModDown tail's base.  R encrypts 0: c0 (plus noise); 1: c1.  out may be c0 or c1 itself.
 *   Select.  count >= 1 index-major inputs laid out as for lsa_bfv_pack: input i of item b at in + i * s_index + b * sin.  Let
 *     k = ceil(log2 count); the selectors R_0 .. R_{k-1} are RGSW ciphertexts, R_j of bit j of the index.  Levels run j = k-1 down to
 *     0; at level j every node a < 2^j that has a partner (a + 2^j < count) becomes c'[a] = cmux(c[a], c[a + 2^j], R_j); unpaired
 *     nodes are left alone.  The result is c[0]: it decrypts to input idx for every idx < count.  count == 1 is a copy and takes no
 *     selector.  count - 1 external products.  All levels but the last work inside the input array (`in` is not const; the inputs
 *     i >= max(1, 2^(k-1)) are only read); the last level writes `out`, which may be input 0 (same pointer, sout == sin) and otherwise
 *     overlaps no input.
 * Errors are LSA_ERR_ARG before anything is queued, with a message that begins with the entry point's name and names the argument: a
 * CKKS context, a level out of range, a chain without a special prime, N < 512, a null pointer or key, a pointer off the 16-byte
 * grid, an odd or short stride, s_index < batch * sin, a forbidden overlap (out may equal ct, base, c0 or c1 exactly; partial overlap
 * is refused), a key below the level, n_sel < k, a plan of another context.  A refused call leaves the buffers untouched and the
 * context usable.  batch <= 0 is a no-op. */
/* 1 (default): both gadget products of an external product run as one launch into one accumulator (k_ks_mac_pair); 0: two key MAC
 * launches, the second adding to the first's output (A/B measurement and parity; identical results).  Read by every call. */
int lsa_set_rgsw_pair_mac(lsa_context ctx, int enable);
int lsa_bfv_external_product(lsa_context ctx, int level, const uint64_t* ct, long long sct, lsa_key r0, lsa_key r1,
                             const uint64_t* base /* may be null */, long long sbase, uint64_t* out, long long sout, int batch, void* stream);
int lsa_bfv_cmux(lsa_context ctx, int level, const uint64_t* c0, long long s0, const uint64_t* c1, long long s1, lsa_key r0, lsa_key r1,
                 uint64_t* out, long long sout, int batch, void* stream);
typedef struct lsa_bfv_select_st* lsa_bfv_select_handle;
/* host only, needs no device and no context: the levels (k) and the external products (count - 1); any output pointer may be null */
int lsa_bfv_select_plan(int count, int* n_levels, int* n_products);
int lsa_bfv_select_create(lsa_context ctx, int level, int count, lsa_bfv_select_handle* out);
void lsa_bfv_select_destroy(lsa_bfv_select_handle plan);
int lsa_bfv_select_info(lsa_bfv_select_handle plan, int* level, int* count, int* n_levels, int* n_products);
/* r0s[j], r1s[j], j < n_sel: the selector of index bit j; n_sel >= k, the entries from k on are not read */
int lsa_bfv_select(lsa_context ctx, lsa_bfv_select_handle plan, uint64_t* in, long long sin, long long s_index, uint64_t* out, long long sout,
                   int batch, int n_sel, const lsa_key* r0s, const lsa_key* r1s, void* stream);

/* ---- BFV plaintext matrix x ciphertext vector, entries whole ring elements: the database scan of a PIR answer, between lsa_bfv_expand
 * (which makes the `cols` query ciphertexts) and lsa_bfv_select (which folds the `rows` results), and the general product of a resident
 * table of plaintexts with an encrypted vector.
 *   out[r] = INTT( sum_{c < cols} NTT(ct[c]) . pt[r][c] . 2^-64 mod q )  (+ partial[r])          r < rows
 * per polynomial and per limb.  ct[c] and out[r] are coefficient-domain ciphertexts [2][level+1][N]; pt[r][c] is a pt_mul plaintext
 * [level+1][N], NTT domain, Montgomery form: form 1 of lsa_bfv_encode and lsa_bfv_plain_lift, the operand of lsa_bfv_mult_plain_mul, so
 * a database is built by those entry points with batch = rows * cols.  partial[r], if given, is added in the coefficient domain after
 * the inverse transform.  Every output word equals lsa_bfv_mac_plain_mul on row r's terms: both sum canonical residues mod q, so
 * neither the order of the terms nor where the 128-bit sums are folded matters.  Each ct[c] is transformed once (the composition
 * transforms it `rows` times) and the sums stay in registers across the columns.  Plaintext words at or above q give unspecified
 * output words and never an out-of-range access.
 * Layout, strides in words: input c of item b at cts + c * s_col + b * sct, the index-major layout lsa_bfv_expand writes; output r of
 * item b at out + r * s_row + b * sout, the one lsa_bfv_select and lsa_bfv_pack read; partial as out with its own strides;
 * pt[r][c] of item b at pts + r * s_prow + c * s_pcol + b * spt, spt == 0: one database for the whole batch.  s_col >= batch * sct,
 * s_row >= batch * sout, s_partial_row >= batch * spartial; the database is only read, so s_prow, s_pcol and spt may nest in any order,
 * each at least one plaintext.  out shares no word with cts or partial and its hull (first to last word) is apart from the
 * database's; there is no in-place form, every output depends on every input.  On the dense layouts (s_col == batch * sct, s_row ==
 * batch * sout) the forward and the inverse transforms are one launch each per tile, otherwise one per column / row.
 * Errors are LSA_ERR_ARG before anything is queued, with a message that begins "lsa_bfv_matvec_plain_mul" and names the argument: a
 * CKKS context, a level out of range, rows < 1 or cols < 1, N < 512, a null pointer (partial may be null), a pointer off the 16-byte
 * grid, an odd stride, a stride shorter than what it spans, a forbidden overlap.  A refused call leaves the buffers untouched and the
 * context usable.  batch <= 0 is a no-op after the checks. */
int lsa_bfv_matvec_plain_mul(lsa_context ctx, int level, int rows, int cols,
                             const uint64_t* cts, long long s_col, long long sct,
                             const uint64_t* pts, long long s_prow, long long s_pcol, long long spt,
                             const uint64_t* partial /* may be null */, long long s_partial_row, long long spartial,
                             uint64_t* out, long long s_row, long long sout, int batch, void* stream);
/* host only, needs no device and no context: the plan of a call on a ring of n_ring coefficients and level_limbs = level + 1 limbs with
 * `workspace_bytes` of workspace (the runner plans with 8 GiB).  row_block: the output rows one workgroup sums from one read of the
 * transformed ciphertexts (the last block of a `rows` that is no multiple masks its rows); col_block: the columns transformed and
 * multiplied per launch, min(cols, what the workspace holds of one item), the blocks after the first adding to the sums in out;
 * workspace_rows: col_block * 2 * level_limbs rows of N words per batch item; n_launches: the launches of k_bfv_matvec of the call,
 * ceil(cols / col_block) per batch tile of floor(workspace / item) items (the context's own tile cap and lsa_set_tile_batch can
 * only make more tiles).  Any output pointer may be null.  LSA_ERR_ARG: a ring that is no power of two in 512 .. 2^20, level_limbs,
 * rows, cols or batch < 1, a workspace that does not hold one transformed ciphertext. */
int lsa_bfv_matvec_plan(int n_ring, int level_limbs, int rows, int cols, int batch, size_t workspace_bytes,
                        int* row_block, int* col_block, int* n_launches, size_t* workspace_rows);
/* forces the blocks of lsa_bfv_matvec_plain_mul on this context: row_block in {0, 1, 2, 4, 8}, col_block >= 0 (cut to cols and to what
 * the workspace holds); 0 = the plan's own.  A/B measurement and parity; identical results.  Read by every call. */
int lsa_set_bfv_matvec_block(lsa_context ctx, int row_block, int col_block);

/* ---- BFV slot encoder: `batch` host vectors of N integers in [0, t) -- row 0 of the 2 x N/2 slot matrix, then row 1 -- to device
 * plaintexts, the BFV counterpart of lsa_ckks_encode.  The coefficients are oracle/client.py Client.bfv_encode(values): the values
 * placed through Lattigo's batching index matrix, then the inverse negacyclic transform mod t.  The lift to the chain is the
 * pt_mul convention: the coefficient in [0, t) is used as it is at every modulus (t is below every q_j and p_i).
 * form: 0 = ring-t coefficients [N], words in [0, t): the operand of lsa_bfv_addsub_plain, lsa_bfv_mult_plain and
 *           lsa_bfv_plain_lift below;
 *       1 = pt_mul [level+1][N]: NTT domain, Montgomery form, the operand of lsa_bfv_mult_plain_mul / _mac_plain_mul /
 *           _rotate_mac_plain_mul;
 *       2 = extended [level+1+k][N] over Q_level u P: NTT domain, plain residues, the operand of lsa_bfv_linear_transform.
 * The transform mod t runs on the device, one workgroup per plaintext with the whole plaintext in LDS (k_bfv_encode_t), up to
 * N = 2^15; above that the image does not fit, the transform runs on the host and the device takes over from the coefficient
 * row.  out_dev: [batch][rows][N], batch stride sout words (even, at least rows * N), 16-byte aligned.  batch <= 0 is a no-op;
 * the call returns when the plaintexts are complete on `stream` (the lsa_ckks_encode contract).  Errors are LSA_ERR_ARG before
 * anything is queued, with a message that begins "lsa_bfv_encode": a CKKS context, level or form out of range, a value >= t,
 * t >= 2^32 or t not a prime that is 1 mod 2N, a null pointer, out_dev off the 16-byte grid, a short or odd stride. */
int lsa_bfv_encode(lsa_context ctx, int level, int form, const uint64_t* values, uint64_t* out_dev, long long sout, int batch,
                   void* stream);

/* ---- BFV ring-t plaintext operands: a ciphertext combined with a plaintext of form 0, the BFV counterparts of
 * lsa_ckks_addsub_plain / _mult_plain.  ct / out: [2][level+1][N] per batch item, coefficient domain; pt: ring-t coefficients [N]
 * per item, all on the device; batch strides in words.  spt == 0: one plaintext for the whole batch.  Everything is queued on
 * `stream`; nothing is allocated per call and nothing waits.  batch <= 0 is a no-op (the other arguments are still checked).
 * Errors are LSA_ERR_ARG before anything is queued, the message beginning with the entry point's name: a CKKS context, a level out
 * of range, op outside 0..2 or form outside 1..2, a null pointer, a pointer off the 16-byte grid, an odd stride, a stride below
 * one item (spt == 0 excepted; never sout), an output that overlaps an input other than "out IS ct" (same pointer, same stride;
 * lift: no overlap at all), t >= 2^32 (addsub), t not below every modulus written (lift, mult).
 *
 * lsa_bfv_addsub_plain: op 0: ct + pt, 1: ct - pt, 2: pt - ct.  The plaintext enters through Lattigo's scaleUp: with
 * u = ((pt[x] mod t) (Q_level mod t) + floor(t/2)) mod t, limb j of c0 takes +- (u - floor(t/2)) (-t^-1) mod q_j; c1 is copied
 * (op 2: negated).  Ops 0 and 1 are the words of oracle/pyoracle.py Oracle.plain_ringt(op, level, ct, pt), op 2 the word-wise
 * negation of op 1 (lsa_poly_addsub op 2 of it).  One launch (k_bfv_addsub_plain); in place, ops 0 and 1 touch c0 only.  A
 * plaintext word may be any 64-bit value: it is reduced mod t first. */
int lsa_bfv_addsub_plain(lsa_context ctx, int op, int level, const uint64_t* ct, long long sct, const uint64_t* pt, long long spt,
                         uint64_t* out, long long sout, int batch, void* stream);
/* Device ring-t plaintexts -> form 1 (pt_mul, [level+1][N]) or form 2 (extended, [level+1+k][N]): the device half of lsa_bfv_encode
 * from the coefficient row on, with its words for the same plaintext; no host copy, no synchronise.  Words in [0, t): a word >= t
 * gives unspecified output words, never an out-of-range access. */
int lsa_bfv_plain_lift(lsa_context ctx, int level, int form, const uint64_t* pt, long long spt, uint64_t* out, long long sout,
                       int batch, void* stream);
/* out = ct x pt slot-wise: the plaintext goes to form 1 in the context workspace (a shared one once per call, per-item ones tile by
 * tile), then lsa_bfv_mult_plain_mul.  The words of Oracle.plain_ringt(2, level, ct, pt); out may BE ct.  Plaintext words in
 * [0, t) as for lsa_bfv_plain_lift. */
int lsa_bfv_mult_plain(lsa_context ctx, int level, const uint64_t* ct, long long sct, const uint64_t* pt, long long spt,
                       uint64_t* out, long long sout, int batch, void* stream);

/* ---- BFV linear transform: plaintext matrix x encrypted vector in diagonal form, baby-step / giant-step with double hoisting.
 * The matrix acts on both rows of the 2 x N/2 slot matrix at once.  period: a power of two that divides N/2; rotations are column
 * rotations (Galois element 5^r mod 2N).  Diagonal k (taken mod period; negative indices allowed; no two equal mod period) holds one
 * vector per slot row, values[i][row][period] < t, tiled over that row's N/2 columns:
 *     out_row[c] = sum_k d_k,row[c mod period] * x_row[(c + k) mod N/2]  mod t,     row = 0, 1
 * (Lattigo's BGV/BFV LinearTransform).  Terms that mix the two rows (the row swap, element 2N-1) are out of scope: run a second plan on
 * lsa_bfv_rotate(ct, 2N-1) and add.  The split n1 is lsa_lt_plan_rotations(period, ...)'s; n1 = 0 (fewer than three diagonals) means
 * every diagonal is a baby step of the single giant step 0.  The plaintext of diagonal k = giant + baby is lsa_bfv_encode form 2 of
 * rot_{-giant}(d_k) (lsa_bfv_lt_plaintext reads it back).
 * The words, as tests/bfv_lt_model.py states them on oracle/ckks_bootstrap.py's rotate_ext / lift_ext, mul_plain_ext, add_ext and
 * moddown: (1) every limb of ct into the NTT domain; (2) baby_b = rotate_ext(x, b) for every baby step, lift_ext for b = 0;
 * (3) inner_g = sum_b pt_{g+b} . baby_b over Q_level u P; (4) the accumulator starts as inner_0 and every other giant step adds
 * rotate_ext(moddown(inner_g), g); (5) out = moddown(accumulator), transformed back.  That is (giant steps other than 0) + 1
 * divisions by P; for three or more diagonals the words of oracle linear_transform(double_hoist=True, rescale=False, plains=...).
 * They DIFFER from lsa_bfv_rotate_mac_plain_mul on the same diagonals, which divides once per rotation; both decrypt to the same slots.
 * ct and out are [2][level+1][N] in the coefficient domain; out may not overlap in; batch <= 0 is a no-op.  Errors are LSA_ERR_ARG
 * before anything is queued, messages beginning "lsa_bfv_lt_create" / "lsa_bfv_linear_transform": a CKKS context, level out of
 * range, no special prime, a bad period, two indices equal mod period, a value >= t, a missing key (the message names the element),
 * a key below the plan's level, a plan of another context, out overlapping in, a bad alignment or stride. */
typedef struct lsa_bfv_lt_st* lsa_bfv_lt;
int lsa_bfv_lt_create(lsa_context ctx, int level, int period, int n_diag, const int* diag_index, const uint64_t* values,
                      double bsgs_ratio, void* stream, lsa_bfv_lt* out);
void lsa_bfv_lt_destroy(lsa_bfv_lt lt);
/* n1: 0 or the split; n_baby / n_giant: distinct baby and giant steps, step 0 included; rows = level + 1 + k; any pointer may be null */
int lsa_bfv_lt_info(lsa_bfv_lt lt, int* level, int* period, int* n_diag, int* n1, int* n_baby, int* n_giant, int* rows,
                    int* n_galois, int* n_moddown);
int lsa_bfv_lt_diagonals(lsa_bfv_lt lt, int* index_out, int capacity);           /* ascending, reduced mod period */
int lsa_bfv_lt_galois_elements(lsa_bfv_lt lt, uint64_t* out, int capacity);       /* ascending */
/* the encoded diagonal at position diag_pos of lsa_bfv_lt_diagonals' order: rows * N words */
int lsa_bfv_lt_plaintext(lsa_bfv_lt lt, int diag_pos, uint64_t* host_out, long long capacity_words);
/* galois_elements / keys: n_keys Galois keys at the plan's level or above, in any order and possibly more than needed */
int lsa_bfv_linear_transform(lsa_context ctx, lsa_bfv_lt lt, const uint64_t* in, uint64_t* out, int batch, long long sin,
                             long long sout, int n_keys, const uint64_t* galois_elements, const lsa_key* keys, void* stream);

/* ---- CKKS polynomial evaluation: p(x) = sum_k coef[k] B_k(x) on a ciphertext, B_k the Chebyshev polynomial T_k (basis 0) or
 * the monomial x^k (basis 1), by a baby-step / giant-step (Paterson-Stockmeyer) plan of depth k = ceil(log2(n_coef)), k >= 1:
 * the powers P_j for j < 2^log_baby and P_(2^j) above them (P_j from P_ceil(j/2) and P_floor(j/2); only those that are used),
 * binary splitting p = hi * P_half + lo with top-down target scales down to LEAVES of degree < 2^log_baby, each leaf one
 * rescaled linear combination of the baby powers by integer constants.  All-zero halves cost nothing, a constant upper half
 * costs no multiplication.  The recursion is written out in DESIGN.md 4.8 and restated in tests/poly_model.py; with
 * log_baby = 1 it is oracle/ckks_bootstrap.py eval_chebyshev / eval_monomial word for word.
 * n_coef: 1..256, any value (zero-padded to 2^k); a polynomial of degree 0 is refused.  log_baby: 0 = the value in 1..min(4, k)
 * with the fewest ciphertext multiplications (ties: the smaller), else 1..4.  [a, b]: the interval of x; (-1, 1) = none,
 * otherwise u = (2x - a - b) / (b - a) is formed first and costs one more level.  level_in - depth >= 0 is required.
 * scale_out: 0 = q[level_out + 1] (the oracle's default).  Errors are LSA_ERR_ARG with a message that begins "poly". */
typedef struct lsa_polynomial_st* lsa_polynomial;
/* host only, needs no device and no context: the counts lsa_poly_create will arrive at (any output pointer may be null) */
int lsa_poly_plan(int basis, int n_coef, const double* coef, int log_baby, int level_in, int with_interval, int* depth,
                  int* log_baby_out, int* n_mult, int* n_leaves, int* n_leaf_launches);
int lsa_poly_create(lsa_context ctx, int basis, int n_coef, const double* coef, double a, double b, int level_in, double scale_in,
                    double scale_out, int log_baby, lsa_polynomial* out);
void lsa_poly_destroy(lsa_polynomial p);
int lsa_poly_info(lsa_polynomial p, int* level_in, int* level_out, double* scale_out, int* depth, int* log_baby, int* n_mult,
                  int* n_leaves, int* n_leaf_launches, int* n_constants);
/* every integer constant of the plan: the interval's two, one per Chebyshev power (ascending), per leaf its K_j (ascending j) and
 * its constant term if non-zero (leaves in the recursion's order, upper half first), then the constant lower halves */
int lsa_poly_constants(lsa_polynomial p, long long* out, int capacity);
/* in [batch][2][level_in+1][N] (NTT domain, scale_in) -> out [batch][2][level_out+1][N] at scale_out; batch strides in words;
 * out may not overlap in, pointers are 16-byte aligned and strides even; batch <= 0 is a no-op.  The only key is the
 * relinearisation key (at level_in or above). */
int lsa_ckks_poly_eval(lsa_context ctx, lsa_polynomial p, const uint64_t* in, uint64_t* out, int batch, long long sin,
                       long long sout, lsa_key rlk, void* stream);

/* ---- BFV polynomial evaluation: p(x) = sum_{k < n_coef} coef[k] x^k mod t, slot-wise on a ciphertext, by a FLAT baby-step /
 * giant-step plan.  m = 2^log_baby, G = ceil(n_coef / m), the coefficients zero-padded to G * m:
 *   baby powers   x^j = x^ceil(j/2) * x^floor(j/2) for 2 <= j < m, by lsa_bfv_mult_relin: only those a non-zero coefficient
 *                 needs, or another needed power needs;
 *   giant powers  y = x^m = x^(m/2) * x^(m/2) and y^g = y^ceil(g/2) * y^floor(g/2) for 2 <= g < G: only those a non-zero leaf needs,
 *                 and their halves;
 *   leaves        leaf_g = coef[g m] + sum_{1 <= j < m} coef[g m + j] x^j, up to 8 per launch of one kernel that reads every baby
 *                 power once per launch; an all-zero leaf does not exist, a leaf that is only a constant is the trivial
 *                 ciphertext (c1 = 0) and goes through the sum like any other;
 *   sum           out = leaf_0 + sum_{g >= 1, leaf_g != 0} leaf_g * y^g by lsa_bfv_dot with leaf_0 as its addend: ONE scale-down
 *                 by Q and ONE relinearisation for the whole sum.  With no term g >= 1, out is leaf_0 itself.
 * Counts: n_mult = key switches = baby powers computed + giant powers computed (y included) + 1 if the sum has a term;
 * n_pairs = terms of the sum; n_leaf_launches = ceil(n_leaves / 8); depth from d(x^j) = ceil(log2 j), d(y^g) = log_baby +
 * ceil(log2 g), d(leaf) = the maximum over its used powers (0 for a constant): depth = max(d(leaf_0), max_g(max(d(leaf_g), d(y^g)) + 1)).
 * depth is the multiplicative depth of the circuit, which is what the noise budget of a BFV parameter set runs out of: every
 * level of it takes bits off the margin between the noise and Q/2t, and a plan one level deeper can fail to decrypt where the
 * shallower one succeeds (DESIGN.md 4.15 has figures measured on the CPU oracle).  log_baby = 0 therefore asks for the least
 * depth first, then the least n_mult, then the smaller value; 1..4 forces it.
 * n_coef: 1..256; every coef[k] < t; a polynomial whose highest non-zero coefficient is coef[0] is refused.
 * A coefficient enters a leaf centred into (-t/2, t/2]; the constant c of a leaf is Lattigo's scaleUp of the constant polynomial
 * (c in every slot, one coefficient of c0), the words of lsa_bfv_affine_const below.  The words of the whole operator are those of
 * the composition of lsa_bfv_mult_relin, lsa_bfv_affine_const, lsa_poly_addsub and lsa_bfv_dot (tests/bfv_poly_model.py).
 * All ciphertexts are [2][level+1][N], coefficient domain, at the plan's ONE level (a BFV level change is no row prefix); the
 * relinearisation key is the only key.  A run holds (m-1) + (G-1) + n_leaves ciphertexts per batch item at most, in ONE
 * workspace of the plan, kept across runs (a plan runs on one stream at a time); a run at another batch size waits for `stream`,
 * gives the workspace back and takes one of its own size.  out overlaps no input; pointers are 16-byte aligned and strides
 * even; batch <= 0 is a no-op; everything runs on `stream`.  Errors are LSA_ERR_ARG before anything is queued, messages beginning
 * "bfv_poly": a CKKS context, a level out of range, n_coef outside 1..256, a coefficient >= t, degree 0, log_baby outside 0..4, a
 * null pointer, a missing key or one exported below `level`, a plan of another context, out overlapping in, a bad alignment or
 * stride, and (at create) a level whose auxiliary basis the context cannot hold for one product or for the sum's largest group,
 * which is what lsa_bfv_mult and lsa_bfv_dot would refuse in the middle of a run. */
typedef struct lsa_bfv_polynomial_st* lsa_bfv_polynomial;
/* host only, no context, no device; every output pointer nullable */
int lsa_bfv_poly_plan(uint64_t t, int n_coef, const uint64_t* coef, int log_baby, int* log_baby_out, int* depth, int* n_mult,
                      int* n_leaves, int* n_leaf_launches, int* n_pairs);
int lsa_bfv_poly_create(lsa_context ctx, int level, int n_coef, const uint64_t* coef, int log_baby, void* stream,
                        lsa_bfv_polynomial* out);
void lsa_bfv_poly_destroy(lsa_bfv_polynomial p);
int lsa_bfv_poly_info(lsa_bfv_polynomial p, int* level, int* n_coef, int* log_baby, int* depth, int* n_mult, int* n_leaves,
                      int* n_leaf_launches, int* n_pairs);
int lsa_bfv_poly_eval(lsa_context ctx, lsa_bfv_polynomial p, const uint64_t* in, uint64_t* out, int batch, long long sin,
                      long long sout, lsa_key rlk, void* stream);
/* out = k * ct + c in every slot, k and c below t: the kernel with one source and one output; out may BE ct (same stride).
 * Limb j of out is (k centred into (-t/2, t/2], mod q_j) * ct, plus on coefficient 0 of c0 the word of Lattigo's scaleUp of the
 * constant polynomial c.  The 2 (level + 1) constant words travel in the launch's arguments: the call allocates nothing, copies
 * nothing to the device and keeps nothing per (k, c), so any number of distinct constants costs the same; level + 1 <= 64.
 * Errors are LSA_ERR_ARG, messages beginning "lsa_bfv_affine_const". */
int lsa_bfv_affine_const(lsa_context ctx, int level, const uint64_t* ct, long long sct, uint64_t k, uint64_t c, uint64_t* out,
                         long long sout, int batch, void* stream);

/* diagnostic builds only (-DLSA_NTT_DIAG_STAMPS): device buffer of 8192*8 u64 receiving per-workgroup phase time stamps
 * of every following NTT launch; NULL turns it off.  Ignored by the normal build. */
int lsa_debug_set_ntt_stamps(lsa_context ctx, void* device_buffer);
/* Read-only views of decisions the context has taken, for tests.  The base-conversion plans built so far (one per distinct
 * source / destination list and flavour, in a fixed order): source and destination limb counts and whether the plan runs
 * the narrow kernel's 29-bit split accumulate.  count receives the number of plans; at most `capacity` are written. */
int lsa_debug_baseconv_plans(lsa_context ctx, int capacity, int* count, int* ns, int* nd, int* split);
/* Whether a key switch with this one key at this level runs the extension transform's second pass fused with the key MAC
 * (under the settings and environment switches in force at the call). */
int lsa_debug_key_switch_fused(lsa_context ctx, int level, lsa_key key, int* fused);
/* Sampled HIP-event timing of the library's own kernel launches, recorded on the stream they are launched on (every
 * `stride`-th launch of each kind gets an event pair).  kind: 0 NTT pass, 1 base conversion, 2 key-switch MAC,
 * 3 tensor, 4 other element-wise.  total_bytes = ALGORITHMIC bytes of the sampled launches. */
int lsa_profile_begin(lsa_context ctx, int stride);
int lsa_profile_end(lsa_context ctx);
int lsa_profile_read(lsa_context ctx, int kind, double* total_ms, double* total_bytes, long long* sampled,
                     long long* launched);
int lsa_profile_read_primary(lsa_context ctx, int kind, double* total_bytes_primary);
/* micro-benchmark kernels used by bench.py / DESIGN.md to report the integer-multiply and copy ceilings */
int lsa_probe_copy(lsa_context ctx, uint64_t* dst, const uint64_t* src, size_t n_u64, void* stream);
int lsa_probe_mulhi(lsa_context ctx, uint64_t* buf, size_t n_u64, int iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif
