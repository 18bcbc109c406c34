// poly_eval.h — CKKS polynomial evaluation: the ciphertext helpers that bootstrapping's EvalMod and the public operator share
// (CtEval), the Paterson-Stockmeyer planner (host only) and the operator's plan (lsa_poly_* / lsa_ckks_poly_eval); the code is
// in poly_eval.hip.  The recursion is restated in tests/poly_model.py over oracle/ckks_bootstrap.py's Evaluator.
#pragma once
#include <string>
#include <vector>

#include "linear_transform.h"
#include "poly_lincomb.h"

namespace lsa {

// ------------------------------------------------------------------------------------------------ shared ciphertext helpers
struct CtEval : LtEval {
    const Key& rlk;
    CtEval(Context& c_, DevPool& p, hipStream_t s_, int m_, const Key& rlk_, const GaloisKeys& g, const char* who_)
        : LtEval(c_, p, s_, m_, g, who_), rlk(rlk_) {}
    DCt mul(const DCt& a0, const DCt& b0) {
        // operands at different levels: the leading rows of each polynomial of the higher one ARE it at the lower level, the
        // tensor kernel takes the rows per polynomial -- no copy (k_copy_rows was 2 % of a bootstrap)
        const int lvl = std::min(a0.level, b0.level);
        DCt o = alloc(lvl - 1, a0.scale * b0.scale / q(lvl));
        ckks_mult_relin_rescale_rpp(c, lvl, a0.data(), b0.data(), rlk, o.data(), m, stride(a0.level), stride(b0.level), stride(lvl - 1), s,
                                    a0.level + 1, b0.level + 1);
        return o;
    }
    // per-limb constant vectors, cached on the context by value
    const u64* kvec(long long k, int level, bool montgomery) {
        std::vector<int> mods(level + 1);
        std::vector<u64> vals(level + 1);
        for (int j = 0; j <= level; j++) {
            mods[j] = j;
            const long long qq = (long long)c.T.mod[j];
            long long r = k % qq;
            if (r < 0) r += qq;
            vals[j] = (u64)r;
        }
        const std::string name = std::string(montgomery ? "btm" : "btr") + std::to_string(level) + "_" + std::to_string(k);
        return montgomery ? c.const_vec(name, mods, vals) : c.raw_vec(name, vals);
    }
    // level < a.level: the product at that lower level, read from a's leading rows (no copy to drop it first)
    DCt mul_int_raw(const DCt& a, long long k, double new_scale, int level = -1) {
        if (level < 0) level = a.level;
        DCt o = alloc(level, new_scale);
        unsigned char lm[LSA_MAX_PERIOD];
        for (int j = 0; j <= level; j++) lm[j] = (unsigned char)j;
        launch_sub_mul_general(c, 2, level + 1, lm, kvec(k, level, true), a.data(), stride(a.level), a.level + 1, nullptr, 0,
                               0, nullptr, 0, 0, 0, o.data(), stride(level), level + 1, m, s);
        return o;
    }
    DCt mul_int(const DCt& a, long long k) { return mul_int_raw(a, k, a.scale); }
    DCt mul_const(const DCt& a, double cst, double const_scale, int level = -1) {
        return mul_int_raw(a, round_even(cst * const_scale, who.c_str()), a.scale * const_scale, level);
    }
    // per-row vectors over BOTH polynomials: [value for the L limbs of c0 | `second` for the L limbs of c1]
    const u64* kvec2(long long k0, long long k1, int level, bool montgomery) {
        const int L = level + 1;
        std::vector<int> mods(2 * L);
        std::vector<u64> vals(2 * L);
        for (int p = 0; p < 2; p++)
            for (int j = 0; j < L; j++) {
                mods[p * L + j] = j;
                const long long qq = (long long)c.T.mod[j];
                long long r = (p == 0 ? k0 : k1) % qq;
                if (r < 0) r += qq;
                vals[p * L + j] = (u64)r;
            }
        const std::string name = std::string(montgomery ? "b2m" : "b2r") + std::to_string(level) + "_" + std::to_string(k0) + "_" + std::to_string(k1);
        return montgomery ? c.const_vec(name, mods, vals) : c.raw_vec(name, vals);
    }
    RowMap rm_both(int level) const {
        RowMap rm;
        rm.period = 2 * (level + 1);
        for (int p = 0; p < 2; p++)
            for (int j = 0; j <= level; j++) rm.mod_of[p * (level + 1) + j] = (unsigned char)j;
        return rm;
    }
    // a * factor + k (the integer k at a's scale, in every slot), one pass (factor 1: plain addition)
    DCt mul_int_add_int(const DCt& a, long long factor, long long k) {
        DCt o = alloc(a.level, a.scale);
        launch_add_const(c, a.data(), stride(a.level), kvec2(k, 0, a.level, false), o.data(), stride(a.level), 2 * (a.level + 1),
                         rm_both(a.level), m, s, factor == 1 ? nullptr : kvec2(factor, factor, a.level, true));
        return o;
    }
    // a * factor + cst in every slot
    DCt mul_int_add_const(const DCt& a, long long factor, double cst) {
        return mul_int_add_int(a, factor, round_even(cst * a.scale, who.c_str()));
    }
    DCt add_const(const DCt& a, double cst) { return mul_int_add_const(a, 1, cst); }
};

// ------------------------------------------------------------------------------------------------ planner (host only)
enum { POLY_CHEBYSHEV = 0, POLY_MONOMIAL = 1 };

struct PolyPower {   // P_j = P_a (x) P_c, a = ceil(j/2), c = floor(j/2)
    int j = 0, a = 0, c = 0, level = 0;
    double scale = 0;
    long long k = 0;   // Chebyshev: the integer -1 * scale (even j) or K of 2 prod - K u (odd j)
};
struct PolyTerm {
    int j;
    double coef;
    long long k;
};
struct PolyJob {   // one output of k_poly_lincomb: rescale(sum K_j P_j[rows <= level + 1]) + k0, at (level, scale)
    int level = 0;
    double scale = 0;
    std::vector<PolyTerm> terms;   // ascending j
    double c0 = 0;
    long long k0 = 0;
    int group = -1, slot = -1;
};
struct PolyVal {   // NONE | the output of a job | the value of a split node
    enum { NONE, JOB, NODE } kind = NONE;
    int idx = -1;
};
struct PolyNode {   // hi * P_half + lo at (level, scale)
    int half = 0, level = 0;
    double scale = 0;
    PolyVal hi, lo;
    bool hi_is_product = false;   // a constant hi: the job's output is hi_0 * P_half itself, no multiplication
    bool lo_const = false;        // lo is the constant c0, added to the product
    double c0 = 0;
    long long k0 = 0;
};
struct PolyGroup {   // one k_poly_lincomb launch: jobs at one level
    int level = 0;
    std::vector<int> jobs;
    std::vector<int> sources;   // powers read, ascending
    u64* d_k = nullptr;         // device tables [G][nsrc][level+2] (Montgomery form), [G][level+2] (plain, polynomial 0)
    u64* d_a = nullptr;
};

struct PolyStructure {
    int basis = 0, k = 0, log_baby = 0, top_level = 0 /* level of u */, mults = 0;
    std::vector<char> needed;   // [2^k] power j is computed
    std::vector<PolyJob> jobs;
    std::vector<PolyNode> nodes;
    std::vector<PolyGroup> groups;
    PolyVal root;
    int level_of(int j) const;   // top_level - ceil(log2 j)
};
// coef padded to 2^k; log_baby in 1..min(4, k); `who` prefixes error messages
PolyStructure poly_structure(int basis, const std::vector<double>& coef, int log_baby, int top_level, const char* who);
// counts only; log_baby 0 = the planner's choice
void poly_plan(int basis, int n_coef, const double* coef, int log_baby, int level_in, bool interval, int* depth, int* chosen,
               int* mults, int* leaves, int* launches);

// ------------------------------------------------------------------------------------------------ public operator plan
struct Polynomial {
    Context& c;
    PolyStructure st;
    int level_in = 0, level_out = 0, depth = 0;
    double scale_in = 0, scale_out = 0;
    bool interval = false;
    long long k_mul = 0, k_add = 0;   // u = rescale(x * k_mul) + k_add
    double u_scale = 0;
    std::vector<PolyPower> powers;    // the needed ones, ascending j >= 2
    std::vector<u64*> odd_tables;     // Chebyshev odd powers: device table [2][level+1] of {2, -K}
    std::vector<long long> constants;
    std::vector<u64*> owned;
    DevPool pool;
    explicit Polynomial(Context& ctx) : c(ctx) {}
    ~Polynomial();
};
Polynomial* poly_create(Context& c, int basis, int n_coef, const double* coef, double a, double b, int level_in, double scale_in,
                        double scale_out, int log_baby, hipStream_t s);
void poly_run(Polynomial& p, const u64* in, long long sin, u64* out, long long sout, int batch, const Key& rlk, hipStream_t s);

}  // namespace lsa
