// tables.h — host-side precomputation for a parameter set (the part of HEonGPU's HEContext::generate that
// mega_ag_runners/gpu/gpu_wrapper.cu:53-138 rebuilds on every run; here it is built once per context and cached).
#pragma once
#include <cstdint>
#include <vector>
#include "modarith.h"

namespace lsa {

bool is_prime64(u64 n);
u64 pow_mod(u64 a, u64 e, u64 q);
u64 mul_mod_host(u64 a, u64 b, u64 q);
u64 inv_mod(u64 a, u64 q);
u64 smallest_primitive_root(u64 q);
int product_bitlen(const u64* q, int k);
// BFV auxiliary basis: count = ceil((bitlen(prod q) + logn)/61); primes = 61-bit, == 1 mod 2n, descending from 2^61
int bfv_aux_count(const u64* q, int k, int logn);
// BFV encrypted inner product (ops.hip bfv_mult_sum / bfv_dot): how a sum of `terms` tensors is laid over the auxiliary basis.
// bfv_aux_count sizes QMul for ONE product, 61 M >= bitlen(Q_level) + logn; a sum of m products is at most m times as large,
// ceil(log2 m) bits more.  The context holds nmul = bfv_aux_count(full chain) auxiliary primes, so at `level`
//   G = min(30, 61 nmul - bitlen(Q_level) - logn) >= 0 spare bits,   max_terms = 2^G products per group,
// the terms are cut into consecutive groups of max_terms (the last may be shorter), and a group of m terms runs over Q_level and
// the FIRST M(m) = (bitlen(Q_level) + logn + ceil(log2 m) + 60) / 61 auxiliary primes: M(1) = bfv_aux_count, M(max_terms) <= nmul.
int bfv_ceil_log2(int m);                                          // m >= 1
int bfv_dot_aux_count(const u64* q, int k, int logn, int m);   // M(m) over the first k limbs of q
struct BfvDotPlan {
    int headroom_bits, max_terms, n_groups;
    int aux_limbs;   // M(min(terms, max_terms)): of the first group, a full one when there are several
};
BfvDotPlan bfv_dot_plan(const u64* q, int nq, int level, int logn, int terms);   // 0 <= level < nq, terms >= 1
std::vector<u64> gen_aux_primes(int n, int count, const std::vector<u64>& avoid);

struct HostTables {
    int n = 0, logn = 0;
    std::vector<u64> mod;       // all moduli: Q chain, then P, then BFV aux
    std::vector<ModDev> mods;   // Montgomery constants per modulus
    // integer engine: every twiddle w with its Shoup quotient floor(w * 2^64 / q), interleaved {w, ws}
    std::vector<u64> psi;       // [nmod][n][2]  w = psi^{brv(x)}
    std::vector<u64> psiinv;    // [nmod][n][2]  w = psi^{-brv(x)}
    std::vector<u64> scale;     // [nmod][2][2]  w = n^-1 and psiinv[1] * n^-1 (the inverse transform's last stage)
    // the same tables as plain integer-valued doubles for the FP64 butterfly engine (used for q < 2^47 only)
    std::vector<double> psi_d, psiinv_d, scale_d;
    void build(int n_, const std::vector<u64>& moduli);
};

// BFV slot encoder (bfv_encode.h): the tables of the inverse negacyclic transform mod the plaintext modulus t, 32-bit words.
// index: Lattigo's batching index matrix -- slot i of the 2 x N/2 slot matrix (row 0 first) is evaluation point index[i] of the
// transform.  psiinv: {w, floor(w 2^32 / t)} with w = psi^-brv(x), psi = g^((t-1)/2N) for the smallest generator g of Z_t^* (the
// choice HostTables::build makes for the chain primes); ninv = N^-1 mod t the same way.
struct BfvEncodeTables {
    int n = 0, logn = 0;
    u64 t = 0;
    std::vector<uint32_t> index;    // [n]
    std::vector<uint32_t> psiinv;   // [n][2]
    uint32_t ninv = 0, ninv_shoup = 0;
    // throws std::invalid_argument (the message names what is wrong with t): t >= 2^32, t not 1 mod 2N, t not prime
    void build(int n_, u64 t_);
    // coef[x] in [0, t): the inverse transform of the N slot values (each < t) placed through `index` -- the host twin of
    // k_bfv_encode_t, used above its LDS limit and by the tests of the tables
    void encode(const u64* values, u64* coef) const;
};

inline u64 to_mont_host(u64 a, u64 q) { return (u64)(((unsigned __int128)a << 64) % q); }
inline u64 shoup_quotient_host(u64 a, u64 q) { return (u64)(((unsigned __int128)a << 64) / q); }

}  // namespace lsa
