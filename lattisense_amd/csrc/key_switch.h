// key_switch.h — the key switch and what every operator that key-switches shares: the tile (KsTile), its sources and outputs, the
// rescale that follows a relinearisation, the rotations' index maps and the tiling of a batch (key_switch.hip).
//   key-switch = per-digit exact ModUp (DecomposeSingleNTT) + gadget MAC + centred ModDown (ModDownQPtoQNTT)
// Callers: ops.hip (relinearisation, rotations, extended rotations, the BFV forms), slot_sum.hip (both slot sums), bfv_expand.hip, bfv_pack.hip,
// bfv_select.hip (the external product).  Nothing outside
// key_switch.hip launches a key MAC or a ModDown itself; an operator whose coefficient-domain tail is its own kernel hands it in as
// the hook KsOut::tail (KsCoeffTail) and stays unknown here.
#pragma once
#include <algorithm>

#include "lsa_internal.h"

namespace lsa {

RowMap rm_seq(int count, int first = 0);
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Merged tail: the key-switch result is rescaled straight away (CKKS HMult+relin+rescale).  ModDown ends with
// c_j = (acc_j - NTT(conv_j)) * P^-1 + base_j and the rescale continues with (c_j - NTT(lift_j(t))) * q_l^-1, t = INTT(c_l).
// Modular arithmetic being exact and the transforms linear, residue for residue
//   t   = (INTT(acc_l) - conv_l) * P^-1 + INTT(base_l)                      (two extra rows in transforms that run anyway)
//   out = (acc_j * P^-1 - NTT(conv_j * P^-1 + lift_j(t)) + base_j) * q_l^-1  (ONE forward transform per remaining limb; the
//                                                                            base conversion emits conv_j * P^-1 directly)
// 104 limb transforms per operation instead of 128, and 4 fewer launches.
struct KsRescale {
    u64* out;          // [2][level][N], level - 1 result
    long long sout;
};

struct RotMacTerm {   // the pt_mul factor of one rotate-and-MAC term (fz_epi = 4): p[scatter[x]] (+)= value(x) * pt[scatter[x]]
    const u64* pt;
    long long spt;
    bool accumulate;
};

// What ModDown writes: p[h][i] = (h < base_polys ? base[h][i] : 0) + ModDown(acc)[h][i], base row h * base_rpp + i.
//   NTT      NTT domain.  scatter (fused tails only): every result row is written through the index map, p[row][scatter[x]] =
//            value(x) -- the NTT-domain automorphism of a rotation applied by the last pass's store instead of a permutation
//            kernel afterwards.  rmac (with scatter): the scattered result is multiplied by a pt_mul plaintext and written or
//            added to p instead (p[row][y] (+)= value * pt[limb][y] * 2^-64, y = scatter[x]): one term of a BFV rotate-and-MAC
//   RESCALE  NTT domain, fused tails: p is scratch of the same shape and rs.out receives rescale(p)
//   COEFF    coefficient domain, `base` given there (BFV).  tail: the caller's kernel stands in place of launch_moddown_final
//            (KsCoeffTail below)
struct KsOut;
// The hook of a COEFF output: launch() is given the accumulator out of the NTT domain ([2][acc_rpp][N] per item) and the
// conversion ([2][L][N]) and writes o.p from them -- (acc - conv) * P^-1 combined with o.base as the operator defines, typically
// through an automorphism gathered from the row staged in LDS (moddown_gather.h).  base_polys: the base the tail needs, o.base a
// [base_polys][L][N] part of a ciphertext (rows per polynomial L); -1: any base launch_moddown_final takes, none included.
struct KsCoeffTail {
    const int base_polys;
    explicit KsCoeffTail(int base_polys_) : base_polys(base_polys_) {}
    virtual void launch(Context& c, int level, const u64* acc, long long s_acc, int acc_rpp, const u64* conv, long long s_conv,
                        const KsOut& o, int nb, hipStream_t s) const = 0;

protected:
    ~KsCoeffTail() = default;
};
// the coefficient-domain automorphism of a BFV rotation, perm = Context::coeff_perm(g), applied by the tail's loads (kernels.hip
// k_sub_mul_perm): p[row][x] = sign_x * value(pi_x), value = (acc - conv) * P^-1 (+ base)
struct KsPermTail final : KsCoeffTail {
    const u32* perm;
    explicit KsPermTail(const u32* perm_) : KsCoeffTail(-1), perm(perm_) {}
    void launch(Context& c, int level, const u64* acc, long long s_acc, int acc_rpp, const u64* conv, long long s_conv, const KsOut& o,
                int nb, hipStream_t s) const override;
};
struct KsOut {
    enum Form { NTT, RESCALE, COEFF };
    u64* p;
    long long sp;
    const u64* base = nullptr;
    long long sbase = 0;
    int base_rpp = 0, base_polys = 0;
    Form form = NTT;
    KsRescale rs = {nullptr, 0};
    const u32* scatter = nullptr;
    const RotMacTerm* rmac = nullptr;
    const KsCoeffTail* tail = nullptr;
};
// the two recurring shapes: the switched polynomial pair added onto c0 of a ciphertext ct [2][L][N] (a rotation, a generic switch),
// or onto both polynomials of one (a relinearisation's (d0, d1), a slot sum's x).  `o`: the fields beyond p, sp and base
inline KsOut ks_onto(int base_polys, u64* p, long long sp, const u64* ct, long long sct, int L, KsOut o) {
    o.p = p, o.sp = sp, o.base = ct, o.sbase = sct, o.base_rpp = L, o.base_polys = base_polys;
    return o;
}
inline KsOut ks_onto_c0(u64* p, long long sp, const u64* ct, long long sct, int L, KsOut o = {}) { return ks_onto(1, p, sp, ct, sct, L, o); }
inline KsOut ks_onto_ct(u64* p, long long sp, const u64* ct, long long sct, int L, KsOut o = {}) { return ks_onto(2, p, sp, ct, sct, L, o); }

// The polynomial a tile switches, given once to decompose(): mac() and the extended MACs read it from the tile.
//   NTT      cx in the NTT domain; the decomposition takes it out
//   BOTH     the caller holds cx in the coefficient domain as well (BFV): the inverse transform is skipped
//   PRODUCT  cx = a1 * b1 of a tensor fold is never stored: the inverse transform forms it as it loads (the product prologue), and
//            the MAC takes its own digits and P * (d0, d1) from a and b (TensorFold)
//   COEFF    cx in the coefficient domain alone (BFV): the tile transforms it forward into L rows per item that it owns, in front
//            of its workspace (rows(c, level, COEFF) counts them) -- only the MAC's own-digit operand needs cx in the NTT domain
struct KsSource {
    enum Form { NTT, BOTH, PRODUCT, COEFF };
    Form form = NTT;
    const u64* ntt = nullptr;
    long long s_ntt = 0;
    const u64* coef = nullptr;
    long long s_coef = 0;
    const TensorFold* prod = nullptr;
    static KsSource of_ntt(const u64* cx, long long scx) { return {NTT, cx, scx}; }
    static KsSource of_both(const u64* cx, long long scx, const u64* cx_coef, long long s_coef) { return {BOTH, cx, scx, cx_coef, s_coef}; }
    static KsSource of_product(const TensorFold& tf) { return {PRODUCT, nullptr, 0, nullptr, 0, &tf}; }
    static KsSource of_coeff(const u64* cx_coef, long long s_coef) { return {COEFF, nullptr, 0, cx_coef, s_coef}; }
};

// One tile of a key switch: nb batch items on stream s, with the workspace laid out per batch item as
// cxi [L] | ext [beta][L+k] | acc [2][L+k] | conv [2][L] rows (a COEFF source: NTT(cx) [L] rows for every item in front of them).
// Whether the extension transform's second pass runs fused with the key MAC is decided here, once, so decompose() leaves the
// extended limbs in the state mac() reads them in.  Only a switch with one key per decomposition fuses (single_key); hoisted
// rotations -- several keys on one decomposition, whose residues are the same as if each rotation had been computed on its own --
// pass none and keep the two steps apart.
struct KsTile {
    Context& c;
    int level, L, T, beta, nb;
    hipStream_t s;
    const Key* key;   // fused: the one key mac() accepts
    bool fused;
    bool tail = false;   // plan_tail() said yes: decompose() leaves limb `level` to the stand-alone MAC, mac_rescale() follows
    u64 *cxn, *cxi, *ext, *acc, *conv;   // cxn: the rows of a COEFF source
    long long s_cxi, s_ext, s_acc, s_conv;
    KsSource src;

    static size_t rows(const Context& c, int level, KsSource::Form form = KsSource::NTT);   // workspace rows per batch item
    static size_t moddown_rows(int level) { return 2 * (size_t)(level + 1); }               // of moddown_ext's `conv`
    // tb (COEFF sources): the items the caller's workspace is laid out for, when its own rows follow the tile's (0: nb)
    KsTile(Context& c, int level, int nb, u64* ws, hipStream_t s, const Key* single_key = nullptr, KsSource::Form form = KsSource::NTT,
           int tb = 0);

    // steps 1-3: cx out of the NTT domain, every digit converted to the other limbs of Q u P, extended limbs back into the NTT
    // domain.  Fused: the limbs that take the fused kernel are left after the first pass (mac() runs the second).
    void decompose(const KsSource& source);
    // step 4: the gadget inner product of the digits with key k (both halves) -> acc, [2][L+k][N] over Q_level u P, NTT
    // domain; fused with the extension transform's second pass where decompose() stopped after the first one.  A PRODUCT
    // source folds the tensor product into the MAC.
    void mac(const Key& k);
    // step 4, extended form: the product leaves as the ROTATED EXTENDED ciphertext dst.out[h][tl][scatter[x]] (+)= sum(x) + (h == 0,
    // tl < L: P * base[tl][x]) in a buffer of the caller's (KsMacDst; never fused: the tile is made without a key)
    void mac_ext(const Key& k, const KsMacDst& dst);
    // the same for 2..4 keys in one launch, each into its own buffer (launch_ks_mac_multi)
    void mac_ext_multi(int n_keys, const KsMacMultiKey* keys, long long sout, const u64* base, long long sbase);
    void moddown(const KsOut& o) { moddown_of(acc, s_acc, o); }   // step 5
    // Steps 4 and 5 as one sequence, the merged rescale tail finished inside the fused key MAC: the Q part of the accumulator that
    // the fused kernel would write and the epilogue pass read back stays in registers.
    //   1. (decompose) limb l = level counts as an unfused target: its extension rows get the stand-alone second pass
    //   2. the fused P limbs (plain fused kernel) and k_ks_mac for the unfused targets and limb l -> acc's P rows, integer Q rows, row l
    //   3. ModDown's head as ever: P rows and row l out of the NTT domain, the two conversions, t = (INTT(acc_l) - conv_l) * P^-1
    //   4. the first pass of NTT(in_j), in_j = conv_j * P^-1 + lift_j(t), every limb j != l
    //   5. the fused kernel's tail variant on the FP64-engine Q limbs j != l: the digits, then the second pass of in_j for both
    //      polynomials, out_j = (sum * P^-1 - NTT(in_j)) * q_l^-1 straight into the rescaled ciphertext
    //   6. the integer-engine Q limbs j != l keep the epilogue pass: the second pass alone, on their rows
    // plan_tail(): the tile takes it -- fused, a tensor-fold product rescaled straight away (KsOut::RESCALE without base), FP64-engine
    // limbs fused alone, some FP64-engine Q limb below l, and Context::ks_tail_in_mac allows the ring.  Call it before decompose().
    bool plan_tail(const KsOut& o);
    void mac_rescale(const Key& k, const KsOut& o);
    // step 5 on an extended accumulator the caller holds ([2][L+k][N] per item; its P rows leave the NTT domain)
    void moddown_of(u64* ext_acc, long long s_ext_acc, const KsOut& o);
    // step 5 without a tile: `conv` is moddown_rows(level) rows per item of scratch
    static void moddown_ext(Context& c, int level, u64* ext_acc, long long s_ext_acc, u64* conv, const KsOut& o, int nb, hipStream_t s);
};

// a key switch with one key; ws: KsTile::rows(c, level, src.form) rows per item
void key_switch(Context& c, int level, const KsSource& src, const Key& key, const KsOut& o, int nb, u64* ws, hipStream_t s);

// The external product RLWE x RGSW: ct [2][L][N] in the coefficient domain (batch stride sct), the RGSW ciphertext the key pair (r0, r1):
//   acc = gadget_product(NTT(ct[0]), r0) + gadget_product(NTT(ct[1]), r1)   over Q_level u P, canonical;   o = ModDown(acc) (+ o.base)
// Both polynomials are decomposed as COEFF sources -- a dense ct (sct == 2 L N) as the 2 * nb rows of ONE launch sequence, a strided
// one as two sequences -- the two gadget products go into ONE accumulator and ONE ModDown follows.  The MAC is k_ks_mac_pair, or, with
// Context::rgsw_pair_mac == 0, launch_ks_mac twice through its extended output (identity index map, no base, the second call
// accumulating): the same words.  It is never the fused second-pass kernel, which takes one key.  o: KsOut::COEFF without a gathering
// tail; the tail (launch_moddown_final) reads o.base only at the points it writes, so o.p may be o.base, and ct has been consumed by the
// decompositions before the tail runs, so o.p may be ct.  ws: 2 * KsTile::rows(c, level, COEFF) rows per item.
void external_product(Context& c, int level, const u64* ct, long long sct, const Key& r0, const Key& r1, const KsOut& o, int nb, u64* ws,
                      hipStream_t s);

// the automorphism X -> X^g of a rotation as the SCATTER map of the key switch's last store: out[i] = in[perm_g[i]] is
// out[perm_{g^-1}[x]] = in[x] (the maps of g and g^-1 are inverse permutations).  rotation_scatter: null when the store cannot
// take it (unfused tails, LSA_ROT_SCATTER=0): the caller then permutes afterwards.
const u32* inverse_perm(Context& c, u64 g);
const u32* rotation_scatter(Context& c, u64 g);

// divide-and-round by the last prime of `level` (DivRoundByLastModulusNTT); ws: rescale_ws_rows rows per item
inline size_t rescale_ws_rows(int level, int polys) { return (size_t)polys * (1 + level); }
void rescale(Context& c, int level, int polys, const u64* in, long long sin, u64* out, long long sout, int nb, bool ntt_domain, u64* ws,
             hipStream_t s);

// ------------------------------------------------------------------------------------------------ tiling
int pick_tile(const Context& c, size_t rows_per_ct, int batch);

// Runs fn(nb, b0, ws, tb, stream) for every tile of `tb` ciphertexts.  Tiles alternate between the caller's stream and
// the context's auxiliary stream (each with its own workspace half): every kernel of the pipeline uses only part of the
// chip's VALU / HBM / latency budget, so two independent tiles in flight fill each other's gaps.
template <typename F>
void for_tiles(Context& c, size_t rows_per_ct, int batch, hipStream_t s, F&& fn) {
    if (batch <= 0) return;
    const int tb = pick_tile(c, rows_per_ct, batch);
    const int ntiles = ceil_div(batch, tb);
    const bool dual = c.dual_stream && ntiles >= 2;
    const size_t words = rows_per_ct * (size_t)c.n * tb;
    u64* ws = c.workspace(words * (dual ? 2 : 1), s);
    if (dual) c.fork_aux(s);
    for (int t = 0; t < ntiles; t++) {
        const int b0 = t * tb, nb = std::min(tb, batch - b0);
        const bool on_aux = dual && (t & 1);
        fn(nb, b0, ws + (on_aux ? words : 0), tb, on_aux ? c.aux_stream : s);
    }
    if (dual) c.join_aux(s);
}

}  // namespace lsa
