// linear_transform.h — CKKS plaintext-matrix x encrypted-vector products in diagonal form: the matrix type, the diagonal
// encoder, the baby-step / giant-step planner and the device evaluator.  Shared by bootstrapping (bootstrap.hip: the
// CoeffsToSlots / SlotsToCoeffs matrices) and by the public operator (lsa_lt_* / lsa_ckks_linear_transform); the code is in
// linear_transform.hip.  Oracle twin: oracle/ckks_bootstrap.py linear_transform.
#pragma once
#include <cmath>
#include <complex>
#include <map>
#include <memory>

#include "lsa_internal.h"

namespace lsa {

using cplx = std::complex<double>;
using Diags = std::map<int, std::vector<cplx>>;   // diagonal k: d[t] multiplies x[(t + k) mod n]

// ------------------------------------------------------------------------------------------------ planner (host only)
std::vector<int> rot_group(int n_slots);   // 5^i mod 4 n_slots
void bsgs_sets(const std::vector<int>& ks, int n, int n1, std::vector<int>& giants, std::vector<int>& babies);
// the planner's baby-step count (frontend/bootstrap_params.py:193-207): the caller's Galois keys exist for this choice
int bsgs_split(const std::vector<int>& ks, int n, double ratio);
// the split (0: fewer than three diagonals, one rotation each) and the non-zero rotations of a reduced, ascending index set
int lt_plan(const std::vector<int>& ks, int period, double ratio, std::vector<int>& rotations);
// Python's round(): ties to even; a constant beyond 2^62 is refused (`who` prefixes the message)
long long round_even(double v, const char* who);

// ------------------------------------------------------------------------------------------------ matrix
struct BtMatrix {
    int level = 0, n1 = 1;
    int period = 0;                      // period of the diagonals (index arithmetic mod period); N/2 for dense packing
    bool naive = false;
    std::vector<int> ks;                 // diagonal indices, ascending
    std::vector<u64*> plains;            // per diagonal: NTT-domain plaintext [rows][N] of rot_{-giant}(diag)
    int rows = 0;                        // level + 1, or level + 1 + k (the special primes too) for a double-hoisted matrix
    double pt_scale = 0;                 // encoding scale of the diagonals
};

// real polynomial coefficients * scale -> NTT-domain plaintext on the device (appended to `owned`)
// ext: the same integer polynomial at the special primes too, rows level+1 .. level+k (operand of extended ciphertexts)
u64* lt_upload_plain(Context& c, const std::vector<double>& coef, double scale, int level, hipStream_t s, bool ext,
                     std::vector<u64*>& owned, const char* who);
// The public encoder (lsa_ckks_encode): `batch` complex vectors of 2^log_slots values, tiled over the N/2 slots, -> NTT-domain
// plaintexts [level+1][N] at `scale`, the words lt_upload_plain gives for the same values.  The floating-point work (slots to
// coefficients, rounding, the 2^62 refusal) is the host's and finishes before anything is queued; the device gets the N rounded
// coefficients of each plaintext and forms the residue rows itself (k_lift_i64).
void ckks_encode(Context& c, int level, int log_slots, const double* values, double scale, u64* out, long long sout, int batch,
                 hipStream_t s);
// one matrix -> plaintexts (diagonals of period `period`, tiled over the N/2 slots) + the Galois elements of its rotations
// (added to `gal`).  Keys of `mat` are reduced mod period.
BtMatrix lt_make_matrix(Context& c, const Diags& mat, int level, int period, double pt_scale, double ratio, bool double_hoist,
                        hipStream_t s, std::vector<u64*>& owned, std::map<u64, bool>& gal, const char* who);

// ------------------------------------------------------------------------------------------------ device evaluator
// temporaries of a run, kept across runs (hipMalloc / hipFree of GiB-sized buffers cost more than the kernels); a pool
// belongs to one plan, which is run on one in-order stream at a time, so reuse is ordered
struct DevPool {
    std::multimap<size_t, u64*> free;
    std::vector<u64*> all;
    void release();   // hipFree of everything (the owner has synchronised)
};
struct DBuf {
    u64* p = nullptr;
    size_t words = 0;
    DevPool* pool = nullptr;   // null: the caller's memory, wrapped
    ~DBuf() {
        if (pool) pool->free.emplace(words, p);
    }
};
struct DCt {
    std::shared_ptr<DBuf> buf;
    int level = 0;
    double scale = 0;
    size_t off = 0;   // words into the buffer: one ciphertext batch of several that share an allocation
    u64* data() const { return buf->p + off; }
};

// `words` words from the pool (an exact-size free buffer, else a fresh allocation); they go back to it with the last copy
DCt pool_alloc_words(DevPool& pool, size_t words);

struct LtEval {
    Context& c;
    DevPool& pool;   // released device buffers (single in-order stream: reuse is ordered)
    hipStream_t s;
    int m;   // batch
    const GaloisKeys& glk;
    long long N;
    std::string who;              // prefix of error messages
    bool giant_scatter = false;   // giant-step rotations through the accumulating scatter of the key MAC (ckks_rotate_ext)
    // BFV (bfv_lt_run): the ciphertext a double-hoisted transform is applied to is held in the coefficient domain as well.
    // Entrance: its baby-step decomposition reads c1's coefficients (no inverse transform).  Exit: the final division by P
    // writes coefficients straight to coeff_out (no NTT-domain ModDown followed by inverse transforms).  Both null: CKKS.
    const u64* c1_coef = nullptr;
    long long s_coef = 0;
    u64* coeff_out = nullptr;
    long long s_coeff_out = 0;

    LtEval(Context& c_, DevPool& p, hipStream_t s_, int m_, const GaloisKeys& g, const char* who_)
        : c(c_), pool(p), s(s_), m(m_), glk(g), N(c_.n), who(who_) {}
    long long stride(int level) const { return 2LL * (level + 1) * N; }
    DCt alloc(int level, double scale) {
        DCt o = alloc_words((size_t)m * stride(level));
        o.level = level;
        o.scale = scale;
        return o;
    }
    DCt alloc_words(size_t words);
    DCt wrap(u64* p, int level, double scale) const {   // the caller's [m][2][level+1][N], not pooled
        auto b = std::make_shared<DBuf>();
        b->p = p;
        return DCt{b, level, scale};
    }
    // extended ciphertext [2][level+1+k][N] over Q_level u P (ops.hip ckks_rotate_many_ext, on key_switch.h KsTile::mac_ext); `level` and `scale` as for the
    // ciphertext it will be divided down to
    long long stride_ext(int level) const { return 2LL * (level + 1 + c.np) * N; }
    DCt alloc_ext(int level, double scale) {
        DCt o = alloc_words((size_t)m * stride_ext(level));
        o.level = level;
        o.scale = scale;
        return o;
    }
    RowMap rm_ext(int level) const {   // both polynomials' rows of an extended ciphertext
        RowMap rm;
        rm.period = level + 1 + c.np;
        for (int j = 0; j <= level; j++) rm.mod_of[j] = (unsigned char)j;
        for (int i = 0; i < c.np; i++) rm.mod_of[level + 1 + i] = (unsigned char)c.p_mod(i);
        return rm;
    }
    RowMap rm2(int level) const {   // both polynomials' limbs
        RowMap rm;
        rm.period = level + 1;
        for (int j = 0; j <= level; j++) rm.mod_of[j] = (unsigned char)j;
        return rm;
    }
    double q(int level) const { return (double)c.T.mod[level]; }

    DCt addsub(const DCt& a, const DCt& b, EwOp op) {
        LSA_REQUIRE(a.level == b.level && std::fabs(a.scale / b.scale - 1) < 1e-9, who + ": operands of add/sub differ in level or scale");
        DCt o = alloc(a.level, a.scale);
        launch_elementwise(c, op, a.data(), b.data(), o.data(), m, stride(a.level), stride(a.level), stride(a.level),
                           2 * (a.level + 1), rm2(a.level), s);
        return o;
    }
    DCt add(const DCt& a, const DCt& b) { return addsub(a, b, EW_ADD); }
    DCt sub(const DCt& a, const DCt& b) { return addsub(a, b, EW_SUB); }
    DCt rescale(const DCt& a) {
        DCt o = alloc(a.level - 1, a.scale / q(a.level));
        ckks_rescale(c, a.level, 2, a.data(), o.data(), m, stride(a.level), stride(a.level - 1), s);
        return o;
    }
    const Key& gkey(u64 e) const { return glk.require(e, who); }
    u64 galois_of(int r) const { return galois_of_rotation(r, c.n); }   // r in [0, N/2)
    DCt rotate(const DCt& a, int r);
    // rotations of one ciphertext by several steps with a single decomposition (hoisted); same residues as rotate()
    std::map<int, DCt> rotate_many(const DCt& a, const std::vector<int>& steps);
    // the same rotations WITHOUT their division by P: extended ciphertexts (step 0: the ciphertext times P)
    std::map<int, DCt> rotate_many_ext(const DCt& a, const std::vector<int>& steps);
    DCt moddown(const DCt& a);   // extended -> ciphertext; `a` is consumed
    // out[g] = sum_b ct[b] * pt[g][b] for every giant step g, pt [ng][nb] (null: no such diagonal), rows = limbs per polynomial
    void inner_sums(int nb, const u64* const* ct, long long sct, int ng, const u64* const* pt, u64* const* out, long long so,
                    int limbs, const RowMap& rm);
    DCt linear_transform_dh(const DCt& ct, const BtMatrix& mt, bool do_rescale);
    DCt linear_transform(const DCt& ct, const BtMatrix& mt, bool do_rescale = true);
};

// ------------------------------------------------------------------------------------------------ public operator plan
struct LinearTransform {
    Context& c;
    BtMatrix m;
    bool double_hoist = true;
    std::vector<u64> galois;   // elements of the non-zero rotations, ascending
    std::vector<u64*> owned;
    DevPool pool;
    explicit LinearTransform(Context& ctx) : c(ctx) {}
    ~LinearTransform();
};
LinearTransform* lt_create(Context& c, int level, int log_slots, int n_diag, const int* diag_index, const double* values,
                           double pt_scale, double bsgs_ratio, bool double_hoist, hipStream_t s);
void lt_run(LinearTransform& lt, const u64* in, long long sin, u64* out, long long sout, int batch, bool rescale,
            const GaloisKeys& glk, hipStream_t s);

// ------------------------------------------------------------------------------------------------ BFV operator plan
// lsa_bfv_lt_* / lsa_bfv_linear_transform (include/lattisense_amd.h).  The matrix acts on both rows of the 2 x N/2
// slot matrix at once: diagonal k holds one vector of `period` values per slot row.  Always double-hoisted: the plaintexts are the
// encoder's extended form (bfv_encode.h, BFV_PT_EXT) of rot_{-giant}(d_k), one allocation for all diagonals.  Fewer than three
// diagonals: m.naive, m.n1 = period -- every diagonal a baby step of the single giant step 0, the same loop.
struct BfvLinearTransform {
    Context& c;
    BtMatrix m;
    int n_baby = 0, n_giant = 0, n_moddown = 0;   // distinct baby steps (0 included), giant steps (0 included), divisions by P
    std::vector<u64> galois;                      // elements of the non-zero rotations, ascending
    u64* plains_dev = nullptr;                    // [n_diag][m.rows][N]
    DevPool pool;
    explicit BfvLinearTransform(Context& ctx) : c(ctx) {}
    ~BfvLinearTransform();
};
// values: host [n_diag][2][period], every word < t
BfvLinearTransform* bfv_lt_create(Context& c, int level, int period, int n_diag, const int* diag_index, const u64* values,
                                  double bsgs_ratio, hipStream_t s);
// in / out [batch][2][level+1][N], coefficient domain; out overlaps no word of in
void bfv_lt_run(BfvLinearTransform& lt, const u64* in, long long sin, u64* out, long long sout, int batch,
                const GaloisKeys& glk, hipStream_t s);

}  // namespace lsa
