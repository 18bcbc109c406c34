// ops.hip — operator pipelines: the HEArithmeticOperator surface the reference's executors call
// (mega_ag_runners/gpu/mega_ag_executors_gpu.cu:71-426), built from the kernels in kernels.hip.
//
// Algorithms follow the CPU path the results must agree with (Lattigo v4, restated in oracle/ls_oracle.c):
//   key-switch  = per-digit exact ModUp (DecomposeSingleNTT) + gadget MAC + centred ModDown (ModDownQPtoQNTT)
//   CKKS rescale = divide-and-round by the last prime (DivRoundByLastModulusNTT)
//   rotate      = key-switch c1, add c0, then apply the automorphism (Evaluator.Automorphism)
//   BFV mult    = centred extension Q->QMul, tensor in Q u QMul, round(./Q), centred return to Q, times t
#include "layout_check.h"
#include "linear_transform.h"
#include "lsa_internal.h"
#include "plain_ops.h"
#include "tensor_sum.h"

namespace lsa {

static RowMap rm_seq(int count, int first = 0) {
    RowMap r;
    LSA_REQUIRE(count >= 1 && count <= LSA_MAX_PERIOD, "row map too long");
    r.period = count;
    for (int i = 0; i < count; i++) r.mod_of[i] = (unsigned char)(first + i);
    return r;
}

static int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------------------------------------ key switch
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
//   COEFF    coefficient domain, `base` given there (BFV).  coeff_gather: the coefficient-domain automorphism of a BFV rotation,
//            Context::coeff_perm(g), applied by the tail's loads (k_sub_mul_perm): p[row][x] = sign_x * value(pi_x).
//            slot_tail (base = x, both polynomials): one step of the BFV slot sum, the rotated c0 terms gathered by the tail
//            (k_bfv_slot_tail)
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
    const u32* coeff_gather = nullptr;
    const RotMacTerm* rmac = nullptr;
    const BfvSlotTail* slot_tail = nullptr;
};

// step 5, the division by P of a polynomial pair over Q_level u P (acc: [2][L+k][N] per batch item, NTT domain; its P rows --
// and, for the merged rescale, its last Q row -- are transformed in place), conv: 2L rows of scratch per batch item
static void ks_moddown(Context& c, int level, u64* acc, long long s_acc, u64* conv, const KsOut& o, int nb, hipStream_t s) {
    LSA_REQUIRE(!o.scatter || (c.fuse_tails && o.form == KsOut::NTT), "scattered ModDown store: fused tails, NTT-domain output");
    LSA_REQUIRE(!o.rmac || o.scatter, "rotate-and-MAC tail: needs the rotation's index map");
    LSA_REQUIRE(!o.coeff_gather || o.form == KsOut::COEFF, "gathered ModDown tail: coefficient-domain output");
    LSA_REQUIRE(!o.slot_tail || (o.form == KsOut::COEFF && !o.coeff_gather && o.base && o.base_polys == 2 && o.base_rpp == level + 1),
                "slot-sum ModDown tail: coefficient-domain output on a whole ciphertext");
    LSA_REQUIRE(o.form != KsOut::RESCALE || (c.fuse_tails && level >= 1 && ((o.base && o.base_polys == 2) || (!o.base && o.base_polys == 0))),
                "merged ModDown+rescale: unsupported shape");
    const bool coeff_out = o.form == KsOut::COEFF, rs = o.form == KsOut::RESCALE;
    const long long N = c.n;
    const int L = level + 1, np = c.np, T = L + np;
    const long long s_conv = 2LL * L * N;
    // 5. ModDown: P-part out of NTT, centred exact conversion P -> Q, back to NTT, (accQ - conv) * P^-1 (+ base).
    //    coeff_out (BFV: the result is wanted in the coefficient domain and `base` is given there): every row of acc leaves
    //    the NTT domain once and the tail runs on coefficients -- INTT((acc - NTT(conv)) * P^-1) == (INTT(acc) - conv) * P^-1
    //    residue for residue, 2(L+k) transforms instead of 2k + 2L + 2L.
    {
        RowMap rm;
        rm.period = 2 * T;
        for (int h = 0; h < 2; h++)
            for (int tl = 0; tl < T; tl++)
                rm.mod_of[h * T + tl] = tl >= L ? (unsigned char)c.p_mod(tl - L)
                                                : (coeff_out ? (unsigned char)tl
                                                             : (rs && tl == level ? (unsigned char)level : LSA_ROW_SKIP));
        launch_ntt(c, acc, acc, nb, s_acc, 2 * T, rm, true, s);
    }
    {
        std::vector<int> src, dst;
        BaseConvRows rows{};
        for (int i = 0; i < np; i++) {
            rows.src_row[i] = L + i;
            src.push_back(c.p_mod(i));
        }
        for (int j = 0; j < L; j++) {
            rows.dst_row[j] = j;
            dst.push_back(j);
        }
        const BaseConvPlan* k = c.baseconv(src, dst, true, rs);
        for (int h = 0; h < 2; h++)
            launch_baseconv(c, k, rows, acc + (size_t)h * T * N, conv + (size_t)h * L * N, nb, s_acc, s_conv, s);
    }
    if (coeff_out) {
        if (o.slot_tail)
            launch_bfv_slot_tail(c, level, *o.slot_tail, acc, s_acc, T, conv, s_conv, o.base, o.sbase, o.p, o.sp, nb, s);
        else if (o.coeff_gather)
            launch_moddown_final_perm(c, level, o.coeff_gather, acc, s_acc, T, conv, s_conv, o.base, o.sbase, o.base_rpp,
                                      o.base_polys, o.p, o.sp, nb, s);
        else
            launch_moddown_final(c, level, acc, s_acc, T, conv, s_conv, o.base, o.sbase, o.base_rpp, o.base_polys, o.p, o.sp, nb, s);
        return;
    }
    if (rs) {
        // base_polys == 0: the tensor fold -- P * base is already in acc's Q rows (TensorFold), so INTT(acc_l) * P^-1 carries
        // INTT(base_l) and the tails below run without base
        const int l = level;
        // t[h] = (INTT(acc[h][l]) - conv[h][l]) * P^-1 + INTT(base[h][l]) -> p[h][l].  base is the caller's scratch here
        // (the tensor output): its last limbs are transformed in place, nothing reads them in NTT form afterwards.
        if (o.base) {
            u64* base_rw = const_cast<u64*>(o.base);
            RowMap rb;
            rb.period = 1;
            rb.mod_of[0] = (unsigned char)l;
            rb.row0 = l;
            rb.row_step = o.base_rpp;
            launch_ntt(c, base_rw, base_rw, nb, o.sbase, o.sbase, 2, rb, true, s);
        }
        const unsigned char lm[1] = {(unsigned char)l};
        launch_sub_mul_general(c, 2, 1, lm, c.pinv_vec(level) + l, acc + (long long)l * N, s_acc, T, conv + (long long)l * N,
                               s_conv, L, o.base ? o.base + (long long)l * N : nullptr, o.sbase, o.base_rpp, o.base_polys,
                               o.p + (long long)l * N, o.sp, L, nb, s);
        // every other limb: in = conv_j*P^-1 + lift_j(t), out = (acc_j*P^-1 - NTT(in) + base_j) * q_l^-1
        RowMap rmo;
        rmo.period = 2 * L;
        for (int h = 0; h < 2; h++)
            for (int j = 0; j < L; j++) rmo.mod_of[h * L + j] = j == l ? LSA_ROW_SKIP : (unsigned char)j;
        NttFusion fb;
        fb.pro = 2;
        fb.epi = 2;
        fb.limbs = L;
        fb.ql_mod = l;
        fb.last = o.p + (long long)l * N;
        fb.last_stride = o.sp;
        fb.last_rpp = L;
        fb.a = acc;
        fb.a_stride = s_acc;
        fb.a_rpp = T;
        fb.base = o.base;
        fb.base_stride = o.sbase;
        fb.base_rpp = o.base_rpp;
        fb.base_polys = o.base_polys;
        fb.k = c.pinv_vec(level);
        fb.k2 = c.qlinv_vec(level);
        fb.out = o.rs.out;
        fb.out_stride = o.rs.sout;
        fb.out_rpp = level;
        launch_ntt(c, conv, conv, nb, s_conv, s_conv, 2 * L, rmo, false, s, &fb);
    } else if (c.fuse_tails) {
        // forward NTT of conv with the ModDown tail fused into its last-pass store: the transformed conv is consumed in
        // registers ((acc_Q - conv) * P^-1 + base) and never written
        NttFusion fz;
        fz.epi = 1;
        fz.limbs = L;
        fz.a = acc;
        fz.a_stride = s_acc;
        fz.a_rpp = T;
        fz.base = o.base;
        fz.base_stride = o.sbase;
        fz.base_rpp = o.base_rpp;
        fz.base_polys = o.base_polys;
        fz.k = c.pinv_vec(level);
        fz.out = o.p;
        fz.out_stride = o.sp;
        fz.out_rpp = L;
        fz.scatter = o.scatter;
        if (o.rmac) {
            fz.epi = 4;
            fz.pt = o.rmac->pt;
            fz.pt_stride = o.rmac->spt;
            fz.accumulate = o.rmac->accumulate;
        }
        launch_ntt(c, conv, conv, nb, s_conv, s_conv, 2 * L, rm_seq(L), false, s, &fz);
    } else {
        launch_ntt(c, conv, conv, nb, s_conv, 2 * L, rm_seq(L), false, s);
        launch_moddown_final(c, level, acc, s_acc, T, conv, s_conv, o.base, o.sbase, o.base_rpp, o.base_polys, o.p, o.sp, nb, s);
    }
}

// one key per decomposition (relinearisation, a single rotation, a generic switch): the extension transform's second pass
// and the key MAC run as one kernel where the shape allows (k_ntt_r16_ksmac) and some target limb takes it
bool ks_fuse_mac(const Context& c, int level, const Key& key) {
    const int L = level + 1, T = L + c.np, beta = ceil_div(L, c.np);
    if (!ks_fused_enabled(c) || !ks_fused_engines(c) || (c.fp64_ntt && !key.fp) || beta * T > LSA_MAX_PERIOD || T > 64) return false;
    for (int tl = 0; tl < T; tl++)
        if (ks_fused_limb(c, L, tl)) return true;
    return false;
}

// One tile of a key switch: nb batch items on stream s, with the workspace laid out per batch item as
// cxi [L] | ext [beta][L+k] | acc [2][L+k] | conv [2][L] rows.  Whether the extension transform's second pass runs fused with
// the key MAC is decided here, once, so decompose() leaves the extended limbs in the state mac() reads them in.  Only a switch
// with one key per decomposition fuses (single_key); hoisted rotations -- several keys on one decomposition, whose
// residues are the same as if each rotation had been computed on its own -- pass none and keep the two steps apart.
struct KsTile {
    Context& c;
    int level, L, T, beta, nb;
    hipStream_t s;
    const Key* key;   // fused: the one key mac() accepts
    bool fused;
    u64 *cxi, *ext, *acc, *conv;
    long long s_cxi, s_ext, s_acc, s_conv;

    static size_t rows(const Context& c, int level) {   // workspace rows per batch item
        LSA_REQUIRE(c.np >= 1, "key switching needs at least one special prime");
        const int L = level + 1, T = L + c.np, beta = ceil_div(L, c.np);
        return (size_t)L + (size_t)beta * T + 2 * (size_t)T + 2 * (size_t)L;
    }
    KsTile(Context& c_, int level_, int nb_, u64* ws, hipStream_t s_, const Key* single_key = nullptr)
        : c(c_), level(level_), nb(nb_), s(s_), key(single_key) {
        LSA_REQUIRE(c.np >= 1, "key switching needs at least one special prime");
        LSA_REQUIRE(level >= 0 && level < c.nq, "level out of range");
        const long long N = c.n;
        L = level + 1;
        T = L + c.np;
        beta = ceil_div(L, c.np);
        fused = key && ks_fuse_mac(c, level, *key);
        s_cxi = (long long)L * N;
        s_ext = (long long)beta * T * N;
        s_acc = 2LL * T * N;
        s_conv = 2LL * L * N;
        cxi = ws;
        ext = cxi + (size_t)nb * s_cxi;
        acc = ext + (size_t)nb * s_ext;
        conv = acc + (size_t)nb * s_acc;
    }

    // steps 1-3: cx out of the NTT domain, every digit converted to the other limbs of Q u P, extended limbs back into the NTT
    // domain.  cx_coef: the same polynomial in the coefficient domain if the caller has it (BFV): the inverse transform is
    // skipped.  prod (tensor fold, cx unused): cx = a1 * b1 is never stored, the inverse transform forms it as it loads (the
    // product prologue).  Fused: the limbs that take the fused kernel are left after the first pass (mac() runs the second).
    void decompose(const u64* cx, long long scx, const u64* cx_coef = nullptr, long long s_coef = 0, const TensorFold* prod = nullptr) {
        const long long N = c.n;
        const int np = c.np;
        // 1. cx out of the NTT domain
        if (prod) {
            LSA_REQUIRE(!cx_coef, "key switch: a product source has no coefficient-domain copy");
            NttFusion fz;
            fz.pro = 3;
            fz.limbs = L;
            fz.a = prod->a + prod->pa;   // the second polynomials a1, b1
            fz.a_stride = prod->sa;
            fz.a_rpp = (int)(prod->pa >> c.logn);
            fz.b = prod->b + prod->pb;
            fz.b_stride = prod->sb;
            fz.b_rpp = (int)(prod->pb >> c.logn);
            launch_ntt(c, cxi, cxi, nb, s_cxi, s_cxi, L, rm_seq(L), true, s, &fz);
        } else if (!cx_coef) {
            launch_ntt(c, cx, cxi, nb, scx, s_cxi, L, rm_seq(L), true, s);
        }
        const u64* conv_src = cx_coef ? cx_coef : cxi;
        const long long s_src = cx_coef ? s_coef : s_cxi;
        // 2. per digit: exact conversion of the digit's limbs to every other limb of Q u P.  A digit with ONE source limb q_s
        //    needs none: (Q_d/q_s)^-1 = 1, y = x, v = 0, every target row is x mod p_t -- the load of its extension transform
        //    lifts it (fz_pro = 4) and the rows are never stored in the coefficient domain (lsa_set_modup_lift(ctx, 0): converted as the others).
        //    v = 0 holds for the conversion as it is computed -- v = (int)RN(double(y) / double(q_s)) -- while q_s < 2^53: y and q_s
        //    are exact doubles and y / q_s <= 1 - 1/q_s < 1 - 2^-53 rounds below 1.  A larger q_s has residues next to q_s whose
        //    quotient rounds to 1.0 (the conversion then yields y - q_s): such a digit keeps the conversion kernel, residue for residue.
        const bool lift_on = c.modup_lift != 0;
        auto lifted = [&](int d) { return lift_on && std::min(d * np + np, L) - d * np == 1 && (c.T.mods[d * np].q >> 53) == 0; };
        bool any_lift = false, any_conv = false;
        for (int d = 0; d < beta; d++) {
            if (lifted(d)) {
                any_lift = true;
                continue;
            }
            any_conv = true;
            const int d0 = d * np, d1 = std::min(d0 + np, L);
            std::vector<int> src, dst;
            BaseConvRows rows{};
            for (int i = d0; i < d1; i++) {
                rows.src_row[i - d0] = i;
                src.push_back(i);
            }
            for (int tl = 0; tl < T; tl++) {
                if (tl >= d0 && tl < d1) continue;
                rows.dst_row[dst.size()] = d * T + tl;
                dst.push_back(c.qp_mod(L, tl));
            }
            launch_baseconv(c, c.baseconv(src, dst, false), rows, conv_src, ext, nb, s_src, s_ext, s);
        }
        // 3. extended limbs into the NTT domain (the digit's own limbs are taken from cx directly by the MAC)
        auto own = [&](int d, int tl) { return tl >= d * np && tl < std::min((d + 1) * np, L); };
        NttFusion lf;   // the lifted digits: digit d reads row d * np of conv_src (only read), modulus index d * np
        lf.pro = 4;
        lf.limbs = T;
        lf.last = conv_src;
        lf.last_stride = s_src;
        lf.last_rpp = np;
        lf.ql_mod = 0;
        if (beta * T <= LSA_MAX_PERIOD) {
            RowMap rm, rl;
            rm.period = rl.period = beta * T;
            for (int d = 0; d < beta; d++)
                for (int tl = 0; tl < T; tl++) {
                    const unsigned char m = own(d, tl) ? LSA_ROW_SKIP : (unsigned char)c.qp_mod(L, tl);
                    rm.mod_of[d * T + tl] = lifted(d) ? LSA_ROW_SKIP : m;
                    rl.mod_of[d * T + tl] = lifted(d) ? m : LSA_ROW_SKIP;
                }
            if (any_conv) launch_ntt(c, ext, ext, nb, s_ext, s_ext, beta * T, rm, false, s, nullptr, fused ? 1 : 3);
            if (any_lift) launch_ntt(c, ext, ext, nb, s_ext, s_ext, beta * T, rl, false, s, &lf, fused ? 1 : 3);
            if (!fused) return;
            // the target limbs that do not take the fused kernel get their second pass here (stand-alone MAC later)
            bool any = false;
            for (int i = 0; i < beta * T; i++) {
                rm.mod_of[i] = own(i / T, i % T) || ks_fused_limb(c, L, i % T) ? LSA_ROW_SKIP : (unsigned char)c.qp_mod(L, i % T);
                any |= rm.mod_of[i] != LSA_ROW_SKIP;
            }
            if (any) launch_ntt(c, ext, ext, nb, s_ext, s_ext, beta * T, rm, false, s, nullptr, 2);
            return;
        }
        for (int d = 0; d < beta; d++) {   // (never fused: ks_fuse_mac needs beta * T <= LSA_MAX_PERIOD)
            RowMap rm;
            rm.period = T;
            for (int tl = 0; tl < T; tl++) rm.mod_of[tl] = own(d, tl) ? LSA_ROW_SKIP : (unsigned char)c.qp_mod(L, tl);
            lf.last = conv_src + (size_t)d * np * N;   // (one digit per launch: polynomial 0 of the launch is digit d)
            lf.ql_mod = d * np;
            launch_ntt(c, ext + (size_t)d * T * N, ext + (size_t)d * T * N, nb, s_ext, s_ext, T, rm, false, s, lifted(d) ? &lf : nullptr);
        }
    }

    // step 4: the gadget inner product of the digits with key k (both halves) -> acc, [2][L+k][N] over Q_level u P, NTT
    // domain; fused with the extension transform's second pass where decompose() stopped after the first one.
    // fold: the tensor product folded into the MAC (TensorFold; the own digits come from its operands, cx is not read)
    void mac(const u64* cx, long long scx, const Key& k, const TensorFold* fold = nullptr) {
        if (!fused) {
            launch_ks_mac(c, level, cx, scx, ext, s_ext, k, acc, s_acc, nb, s, false, nullptr, nullptr, 0, fold);
            return;
        }
        LSA_REQUIRE(&k == key, "fused key MAC: the tile was planned for another key");
        LSA_REQUIRE(launch_ntt_ksmac(c, level, cx, scx, ext, s_ext, k, acc, s_acc, nb, s, fold), "fused key MAC: shape not covered");
        launch_ks_mac(c, level, cx, scx, ext, s_ext, k, acc, s_acc, nb, s, true, nullptr, nullptr, 0, fold);
    }

    void moddown(const KsOut& o) { ks_moddown(c, level, acc, s_acc, conv, o, nb, s); }   // step 5
};

// a key switch of cx (NTT domain) with one key
static void key_switch(Context& c, int level, const u64* cx, long long scx, const Key& key, const KsOut& o, int nb, u64* ws,
                       hipStream_t s) {
    KsTile t(c, level, nb, ws, s, &key);
    t.decompose(cx, scx);
    t.mac(cx, scx, key);
    t.moddown(o);
}

// the automorphism X -> X^g of a rotation as the SCATTER map of the key switch's last store: out[i] = in[perm_g[i]] is
// out[perm_{g^-1}[x]] = in[x] (the maps of g and g^-1 are inverse permutations).  Null when the store cannot take it
// (unfused tails, LSA_ROT_SCATTER=0): the caller then permutes afterwards.
static const u32* inverse_perm(Context& c, u64 g) {
    const u64 mask = 2 * (u64)c.n - 1;
    u64 inv = g;   // Newton iteration for the inverse modulo a power of two: doubles the correct low bits each step
    for (int i = 0; i < 6; i++) inv = (inv * (2 - g * inv)) & mask;
    LSA_REQUIRE(((inv * g) & mask) == 1, "Galois element without an inverse");
    return c.ntt_perm(inv);
}
static const u32* rotation_scatter(Context& c, u64 g) {
    return sw::rot_scatter() && c.fuse_tails ? inverse_perm(c, g) : nullptr;
}

// ------------------------------------------------------------------------------------------------ rescale
static size_t rescale_ws_rows(int level, int polys) { return (size_t)polys * (1 + level); }

static void rescale(Context& c, int level, int polys, const u64* in, long long sin, u64* out, long long sout, int nb,
                    bool ntt_domain, u64* ws, hipStream_t s) {
    LSA_REQUIRE(level >= 1 && level < c.nq, "rescale needs level >= 1");
    const long long N = c.n;
    const int L = level + 1;
    u64* last = ws;
    u64* tmp = last + (size_t)nb * polys * N;
    const long long s_last = (long long)polys * N, s_tmp = (long long)polys * level * N;
    std::vector<int> rows(polys);
    for (int p = 0; p < polys; p++) rows[p] = p * L + level;
    launch_copy_rows(c, in, sin, last, s_last, polys, rows.data(), nb, s);
    if (ntt_domain) {
        RowMap rm;
        rm.period = 1;
        rm.mod_of[0] = (unsigned char)level;
        launch_ntt(c, last, last, nb, s_last, polys, rm, true, s);
    }
    if (ntt_domain && c.fuse_tails) {
        // one forward NTT over the level limbs of every polynomial: its first-pass load derives the tile from the last limb
        // (centred remainder, reduced to the target prime), its last-pass store applies (c - t) * q_l^-1 -> out
        NttFusion fz;
        fz.pro = 1;
        fz.epi = 1;
        fz.limbs = level;
        fz.ql_mod = level;
        fz.last = last;
        fz.last_stride = s_last;
        fz.a = in;
        fz.a_stride = sin;
        fz.a_rpp = L;
        fz.k = c.qlinv_vec(level);
        fz.out = out;
        fz.out_stride = sout;
        fz.out_rpp = level;
        launch_ntt(c, tmp, tmp, nb, s_tmp, s_tmp, polys * level, rm_seq(level), false, s, &fz);
        return;
    }
    launch_rescale_prep(c, level, polys, last, s_last, tmp, s_tmp, nb, s);
    if (ntt_domain) launch_ntt(c, tmp, tmp, nb, s_tmp, polys * level, rm_seq(level), false, s);
    launch_rescale_final(c, level, polys, in, sin, tmp, s_tmp, out, sout, nb, s);
}

// ------------------------------------------------------------------------------------------------ tiling
static int pick_tile(const Context& c, size_t rows_per_ct, int batch) {
    if (c.tile_batch > 0) return std::min(c.tile_batch, batch);
    // measured on MI355X (profiles/r01/tile_sweep*.log): launches need >= ~2k workgroups each to fill 256 CUs (~16
    // ciphertexts per wave at N=2^16); past that the gain is the shrinking tail of each launch: +3 % (HMult) / +8 %
    // (rotate) from 19 to 64 ciphertexts, for 6.6 GiB of workspace out of 288.
    const size_t bytes_per_ct = rows_per_ct * (size_t)c.n * sizeof(u64);
    size_t tb = (8ull << 30) / std::max<size_t>(bytes_per_ct, 1);
    if (tb < 1) tb = 1;
    // the cap scales with 1/N (same work per launch): 64 at N=2^16, 256 at N=2^14 (BFV mult+relin +12 % over 64)
    const size_t cap = std::min<size_t>(512, std::max<size_t>(64, (64ull << 16) / (size_t)c.n));
    if (tb > cap) tb = cap;
    return (int)std::min<size_t>(tb, (size_t)batch);
}

// Runs fn(nb, b0, ws, tb, stream) for every tile of `tb` ciphertexts.  Tiles alternate between the caller's stream and
// the context's auxiliary stream (each with its own workspace half): every kernel of the pipeline uses only part of the
// chip's VALU / HBM / latency budget, so two independent tiles in flight fill each other's gaps.
template <typename F>
static void for_tiles(Context& c, size_t rows_per_ct, int batch, hipStream_t s, F&& fn) {
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

// ------------------------------------------------------------------------------------------------ argument checks
// The layout, overlap and argument contract of the first-generation entry points (include/lattisense_amd.h, "Layout and
// aliasing"), checked in the operators themselves so that the task dispatcher and the plan runners get it too.  Everything is
// decided on the host before a kernel or a copy is queued; every refusal is LSA_ERR_ARG with a message that begins with the entry
// point's name.  The span arithmetic is layout_check.h's.
namespace {
using layout::Span;

struct EntryCheck {
    const Context& c;
    std::string who;
    int level, batch;
    size_t N;
    // algo: LSA_ALGO_BFV / LSA_ALGO_CKKS, or -1 for an operator both schemes use; min_level: 1 for the operators that drop a limb
    EntryCheck(const Context& c_, const char* who_, int algo, int level_, int min_level, int batch_)
        : c(c_), who(who_), level(level_), batch(batch_), N((size_t)c_.n) {
        LSA_REQUIRE(algo < 0 || c.algo == algo, who + (algo == LSA_ALGO_BFV ? ": context is not BFV" : ": context is not CKKS"));
        LSA_REQUIRE(level >= min_level && level < c.nq,
                    who + ": level out of range (" + std::to_string(min_level) + ".." + std::to_string(c.nq - 1) + ")");
    }
    void polys(int polys) const {   // a plaintext or one polynomial, a ciphertext, a degree-2 ciphertext
        LSA_REQUIRE(polys >= 1 && polys <= 3, who + ": polys must be 1, 2 or 3");
    }
    void key(const Key& k, const char* what) const {
        LSA_REQUIRE(k.data != nullptr, who + ": " + what + " is null");
        LSA_REQUIRE(k.level >= level, who + ": " + what + " was exported at a lower level than the ciphertext");
    }
    // an operand of `words` words per batch item; shared_ok: a batch stride of 0 (one operand for the whole batch) is accepted
    Span operand(const u64* p, long long stride, size_t words, const char* what, bool shared_ok) const {
        LSA_REQUIRE(p != nullptr, who + ": " + what + " is null");
        const Span sp = layout::span_of(p, stride, words);
        LSA_REQUIRE(layout::stride_ok(sp, shared_ok), who + ": batch stride of " + what +
                                                          (shared_ok ? " below one operand (0: shared by the batch)" : " below one operand"));
        // the element-wise kernels move 16 bytes per lane at base + item * stride
        LSA_REQUIRE(layout::aligned16(sp), who + ": " + what + " must be 16-byte aligned with an even batch stride");
        return sp;
    }
    Span output(const u64* p, long long stride, size_t words, const char* what = "out") const { return operand(p, stride, words, what, false); }
    void apart(const Span& out, const Span& in, const char* what) const {
        LSA_REQUIRE(layout::apart(out, in, batch), who + ": the output overlaps " + what);
    }
    void same_or_apart(const Span& out, const Span& in, const char* what) const {
        LSA_REQUIRE(layout::same_or_apart(out, in, batch),
                    who + ": the output must be " + what + " itself (same pointer, same stride) or not overlap it");
    }
};
}  // namespace

// ================================================================================================ CKKS
void ckks_mult(Context& c, int level, const u64* a, const u64* b, u64* d3, int batch, long long sa, long long sb,
               long long sd, hipStream_t s) {
    const EntryCheck ck(c, "lsa_ckks_mult", LSA_ALGO_CKKS, level, 0, batch);
    if (batch <= 0) return;
    const size_t w = 2 * (size_t)(level + 1) * ck.N;
    const Span out = ck.output(d3, sd, w / 2 * 3, "d3");
    ck.apart(out, ck.operand(a, sa, w, "a", true), "a");
    ck.apart(out, ck.operand(b, sb, w, "b", true), "b");
    launch_tensor(c, a, b, d3, batch, sa, sb, sd, level + 1, rm_seq(level + 1), s);
}

void ckks_relin(Context& c, int level, const u64* d3, const Key& rlk, u64* out, int batch, long long sd, long long so,
                hipStream_t s) {
    const EntryCheck ck(c, "lsa_ckks_relin", LSA_ALGO_CKKS, level, 0, batch);
    ck.key(rlk, "the relinearisation key");
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    ck.apart(ck.output(out, so, 2 * (size_t)L * N), ck.operand(d3, sd, 3 * (size_t)L * N, "d3", false), "d3");
    for_tiles(c, KsTile::rows(c, level), batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        const u64* d = d3 + (size_t)b0 * sd;
        key_switch(c, level, d + 2LL * L * N, sd, rlk, {.p = out + (size_t)b0 * so, .sp = so, .base = d, .sbase = sd, .base_rpp = L, .base_polys = 2},
                   nb, ws, st);
    });
}

void ckks_rescale(Context& c, int level, int polys, const u64* in, u64* out, int batch, long long sin, long long sout,
                  hipStream_t s) {
    // (the output's rows sit at other offsets than the input's: an in-place call would store over rows still to be read)
    const EntryCheck ck(c, "lsa_ckks_rescale", LSA_ALGO_CKKS, level, 1, batch);
    ck.polys(polys);
    if (batch <= 0) return;
    ck.apart(ck.output(out, sout, (size_t)polys * level * ck.N), ck.operand(in, sin, (size_t)polys * (level + 1) * ck.N, "in", false), "in");
    for_tiles(c, rescale_ws_rows(level, polys), batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        rescale(c, level, polys, in + (size_t)b0 * sin, sin, out + (size_t)b0 * sout, sout, nb, true, ws, st);
    });
}

void ckks_rotate(Context& c, int level, const u64* in, u64 g, const Key& glk, u64* out, int batch, long long sin,
                 long long sout, hipStream_t s) {
    const EntryCheck ck(c, "lsa_ckks_rotate", LSA_ALGO_CKKS, level, 0, batch);
    ck.key(glk, "the Galois key");
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    const size_t ks_rows = KsTile::rows(c, level);
    const long long sp = 2LL * L * N;
    const Span sp_in = ck.operand(in, sin, 2 * (size_t)L * N, "in", false), sp_out = ck.output(out, sout, 2 * (size_t)L * N);
    // out == in item for item, or no common word: a partial overlap would let one tile store over what another still reads
    ck.same_or_apart(sp_out, sp_in, "in");
    // (an in-place rotation keeps the two-step form: the tail reads c0 from `in` while other workgroups already store)
    const bool apart = !layout::same(sp_out, sp_in);
    if (const u32* scatter = apart ? rotation_scatter(c, g) : nullptr) {
        // the permutation rides on the ModDown tail's store: no intermediate, no permutation kernel (2L reads + 2L writes less)
        for_tiles(c, ks_rows, batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
            const u64* ct = in + (size_t)b0 * sin;
            key_switch(c, level, ct + (long long)L * N, sin, glk,
                       {.p = out + (size_t)b0 * sout, .sp = sout, .base = ct, .sbase = sin, .base_rpp = L, .base_polys = 1, .scatter = scatter},
                       nb, ws, st);
        });
        return;
    }
    const u32* perm = c.ntt_perm(g);
    for_tiles(c, ks_rows + 2 * (size_t)L, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* p = ws + ks_rows * N * tb;
        const u64* ct = in + (size_t)b0 * sin;
        key_switch(c, level, ct + (long long)L * N, sin, glk, {.p = p, .sp = sp, .base = ct, .sbase = sin, .base_rpp = L, .base_polys = 1},
                   nb, ws, st);
        launch_permute_ntt(c, perm, p, sp, out + (size_t)b0 * sout, sout, 2 * L, nb, st);
    });
}

// rotations of the same ciphertexts by several Galois elements with ONE decomposition (hoisting); outs[i] = rotate(in, g[i]),
// each identical to ckks_rotate's result
void ckks_rotate_many(Context& c, int level, const u64* in, int n_rot, const u64* g, const Key* const* glk, u64* const* outs,
                      int batch, long long sin, long long sout, hipStream_t s) {
    const EntryCheck ck(c, "lsa_ckks_rotate_many", LSA_ALGO_CKKS, level, 0, batch);
    if (n_rot <= 0 || batch <= 0) return;
    LSA_REQUIRE(g && glk && outs, ck.who + ": null argument");
    const long long N = c.n;
    const int L = level + 1;
    const size_t ks_rows = KsTile::rows(c, level);
    const long long sp = 2LL * L * N;
    const Span sp_in = ck.operand(in, sin, 2 * (size_t)L * N, "in", false);
    std::vector<Span> sp_out(n_rot);
    std::vector<const u32*> perms(n_rot), scatters(n_rot);
    std::vector<int> order;   // the output that IS the input goes last: every other rotation still reads the intact ciphertext
    int in_place = -1;
    for (int i = 0; i < n_rot; i++) {
        LSA_REQUIRE(glk[i] != nullptr, ck.who + ": a Galois key is null");
        ck.key(*glk[i], "a Galois key");
        sp_out[i] = ck.output(outs[i], sout, 2 * (size_t)L * N, "an output");
        ck.same_or_apart(sp_out[i], sp_in, "in");
        for (int j = 0; j < i; j++) LSA_REQUIRE(layout::apart(sp_out[i], sp_out[j], batch), ck.who + ": two outputs overlap");
        const bool apart = !layout::same(sp_out[i], sp_in);
        if (apart) order.push_back(i);
        else in_place = i;   // (at most one: two of them would overlap each other)
    }
    if (in_place >= 0) order.push_back(in_place);
    for (int i = 0; i < n_rot; i++) {   // (table look-ups upload on first use: only after every argument is accepted)
        scatters[i] = i != in_place ? rotation_scatter(c, g[i]) : nullptr;
        perms[i] = scatters[i] ? nullptr : c.ntt_perm(g[i]);
    }
    for_tiles(c, ks_rows + 2 * (size_t)L, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* p = ws + ks_rows * N * tb;
        const u64* ct = in + (size_t)b0 * sin;
        KsTile t(c, level, nb, ws, st);
        t.decompose(ct + (long long)L * N, sin);
        for (int i : order) {
            t.mac(ct + (long long)L * N, sin, *glk[i]);
            if (scatters[i]) {   // the permutation rides on the ModDown tail's store
                t.moddown({.p = outs[i] + (size_t)b0 * sout, .sp = sout, .base = ct, .sbase = sin, .base_rpp = L, .base_polys = 1,
                           .scatter = scatters[i]});
                continue;
            }
            t.moddown({.p = p, .sp = sp, .base = ct, .sbase = sin, .base_rpp = L, .base_polys = 1});
            launch_permute_ntt(c, perms[i], p, sp, outs[i] + (size_t)b0 * sout, sout, 2 * L, nb, st);
        }
    });
}

// ---- extended ciphertexts: (c0, c1) times P over Q_level u P, [2][L+k][N] in the NTT domain -- what a key switch holds before
// its division by P.  Sums of them are exact, so a baby-step / giant-step linear transform divides once per giant step and
// once at the end instead of once per rotation ("double hoisting": Lattigo v4 ckks/linear_transform.go
// MultiplyByDiagMatrixBSGS over rlwe GadgetProductNoModDown / ModDownQPtoQNTT; bootstrap.hip, Eval::linear_transform).
void ckks_lift_ext(Context& c, int level, const u64* in, u64* out, int batch, long long sin, long long sout, hipStream_t s) {
    launch_permute_ext(c, level, nullptr, nullptr, 0, in, sin, 2, out, sout, false, batch, s);
}

// outs[i] = automorphism_g[i]( (P c0 + ks0, ks1) ), ks = gadget product of c1 with glk[i]; one decomposition for all
void ckks_rotate_many_ext(Context& c, int level, const u64* in, int n_rot, const u64* g, const Key* const* glk, u64* const* outs,
                          int batch, long long sin, long long sout, hipStream_t s, const u64* c1_coef, long long s_coef) {
    if (n_rot <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    const bool one_pass = sw::rot_scatter();   // the MAC writes the rotated extended ciphertext itself (LSA_ROT_SCATTER=0: MAC, then k_permute_ext)
    std::vector<const u32*> perms(n_rot);
    for (int i = 0; i < n_rot; i++) perms[i] = one_pass ? inverse_perm(c, g[i]) : c.ntt_perm(g[i]);
    for_tiles(c, KsTile::rows(c, level), batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        const u64* ct = in + (size_t)b0 * sin;
        KsTile t(c, level, nb, ws, st);
        t.decompose(ct + (long long)L * N, sin, c1_coef ? c1_coef + (size_t)b0 * s_coef : nullptr, s_coef);
        for (int i = 0; i < n_rot; i++) {
            if (one_pass) {
                launch_ks_mac(c, level, ct + (long long)L * N, sin, t.ext, t.s_ext, *glk[i], outs[i] + (size_t)b0 * sout, sout, nb, st,
                              false, perms[i], ct, sin);
                continue;
            }
            t.mac(ct + (long long)L * N, sin, *glk[i]);
            launch_permute_ext(c, level, perms[i], t.acc, t.s_acc, ct, sin, 1, outs[i] + (size_t)b0 * sout, sout, false, nb, st);
        }
    });
}

// out (+)= automorphism_g( (P c0 + ks0, ks1) ): one rotation without its division by P, optionally added to `out`.
// scatter_mac (and LSA_ROT_SCATTER not 0): the key MAC writes / adds the rotated extended ciphertext itself
// (out[perm[x]] (+)= mac(x) + P c0(x), as ckks_rotate_many_ext does for baby steps) -- no k_permute_ext pass over 2(L+k) limbs, but
// the extension transform's second pass cannot be fused with that MAC.  Otherwise decompose + MAC (fused where the shape
// allows) + k_permute_ext.  Same residues.
void ckks_rotate_ext(Context& c, int level, const u64* in, u64 g, const Key& glk, u64* out, bool accumulate, int batch,
                     long long sin, long long sout, hipStream_t s, bool scatter_mac) {
    const long long N = c.n;
    const int L = level + 1;
    if (scatter_mac && sw::rot_scatter()) {
        const u32* scatter = inverse_perm(c, g);
        for_tiles(c, KsTile::rows(c, level), batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
            const u64* ct = in + (size_t)b0 * sin;
            KsTile t(c, level, nb, ws, st);
            t.decompose(ct + (long long)L * N, sin);
            launch_ks_mac(c, level, ct + (long long)L * N, sin, t.ext, t.s_ext, glk, out + (size_t)b0 * sout, sout, nb, st, false, scatter,
                          ct, sin, nullptr, accumulate);
        });
        return;
    }
    const u32* perm = c.ntt_perm(g);
    for_tiles(c, KsTile::rows(c, level), batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        const u64* ct = in + (size_t)b0 * sin;
        KsTile t(c, level, nb, ws, st, &glk);
        t.decompose(ct + (long long)L * N, sin);
        t.mac(ct + (long long)L * N, sin, glk);
        launch_permute_ext(c, level, perm, t.acc, t.s_acc, ct, sin, 1, out + (size_t)b0 * sout, sout, accumulate, nb, st);
    });
}

// the rounded division by P: extended ciphertext -> ciphertext [2][L][N].  `in` is clobbered (its P rows leave the NTT domain).
void ckks_moddown_ext(Context& c, int level, u64* in, u64* out, int batch, long long sin, long long sout, hipStream_t s,
                      bool coeff_out) {
    const int L = level + 1;
    for_tiles(c, 2 * (size_t)L, batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        ks_moddown(c, level, in + (size_t)b0 * sin, sin, ws,
                   {.p = out + (size_t)b0 * sout, .sp = sout, .form = coeff_out ? KsOut::COEFF : KsOut::NTT}, nb, st);
    });
}

// (c0, c1) under s_in -> (c0 + ks0, ks1) under s_out with a generic switching key (bootstrapping's sparse-secret
// encapsulation keys swk_dts / swk_std, reference: custom_task.py:1989-1996): the rotation pipeline without the permutation
void ckks_switch_key(Context& c, int level, const u64* in, const Key& swk, u64* out, int batch, long long sin, long long sout,
                     hipStream_t s) {
    const long long N = c.n;
    const int L = level + 1;
    for_tiles(c, KsTile::rows(c, level), batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        const u64* ct = in + (size_t)b0 * sin;
        key_switch(c, level, ct + (long long)L * N, sin, swk,
                   {.p = out + (size_t)b0 * sout, .sp = sout, .base = ct, .sbase = sin, .base_rpp = L, .base_polys = 1}, nb, ws, st);
    });
}

// The relinearisation tail of a tile's degree-2 tensor d3 [3][L][N] (batch stride sd): out = (d0, d1) + KeySwitch(d2), rescaled when
// `with_rescale`.  r2: [2][L][N] per item, the unrescaled result (or the merged tail's scratch); sub: the key switch's and the
// rescale's rows
static void ckks_relin_tail(Context& c, int level, const u64* d3, long long sd, const Key& rlk, u64* out, long long so,
                            bool with_rescale, u64* r2, u64* sub, int nb, hipStream_t s) {
    const int L = level + 1;
    const long long sr = 2LL * L * c.n;
    const u64* d2 = d3 + 2LL * L * c.n;
    KsOut o{.p = r2, .sp = sr, .base = d3, .sbase = sd, .base_rpp = L, .base_polys = 2};
    const bool merged = with_rescale && c.fuse_tails;   // the merged ModDown + rescale tail
    if (!with_rescale) {
        o.p = out;
        o.sp = so;
    } else if (merged) {
        o.form = KsOut::RESCALE;
        o.rs = {out, so};
    }
    key_switch(c, level, d2, sd, rlk, o, nb, sub, s);
    if (with_rescale && !merged) rescale(c, level, 2, r2, sr, out, so, nb, true, sub, s);
}

void ckks_mult_relin_rescale(Context& c, int level, const u64* a, const u64* b, const Key& rlk, u64* out, int batch,
                             long long sa, long long sb, long long so, hipStream_t s) {
    ckks_mult_relin_rescale_rpp(c, level, a, b, rlk, out, batch, sa, sb, so, s, 0, 0);
}
// Tensor fold (fused tails; LSA_HMULT_FOLD=0 keeps the three steps apart).  d0, d1 and d2 = k_tensor's outputs are each read again by one consumer only, and each consumer can take them
// from a and b itself, residue for residue:
//   ModUp input  d2 = a1 b1                   (formed by the load of the decomposition's inverse transform, never stored)
//   MAC          own digit of Q target j: d2_j = a1_j b1_j, and acc'_j = acc_j + P * d_j  (d = (d0, d1), TensorFold)
//   ModDown      (acc'_j * P^-1 - NTT(in)) * q_l^-1 = (acc_j * P^-1 - NTT(in) + d_j) * q_l^-1;
//                INTT(acc'_l) * P^-1 = INTT(acc_l) * P^-1 + INTT(d_l)       (the merged tail with base_polys = 0)

// a_rpp / b_rpp: rows per polynomial of a / b when an operand sits at a higher level than `level` (0: level + 1) -- its leading
// rows ARE the operand at this level, so callers with operands at mixed levels (polynomial evaluation) need no copies
void ckks_mult_relin_rescale_rpp(Context& c, int level, const u64* a, const u64* b, const Key& rlk, u64* out, int batch,
                                 long long sa, long long sb, long long so, hipStream_t s, int a_rpp, int b_rpp) {
    const EntryCheck ck(c, "lsa_ckks_mult_relin_rescale", LSA_ALGO_CKKS, level, 1, batch);
    ck.key(rlk, "the relinearisation key");
    const long long N = c.n;
    const int L = level + 1;
    LSA_REQUIRE((a_rpp == 0 || a_rpp >= L) && (b_rpp == 0 || b_rpp >= L), ck.who + ": rows per polynomial below the limb count");
    if (batch <= 0) return;
    {   // an operand kept at a higher level spans its own rows per polynomial; a stride of 0 shares it with the whole batch
        const Span sp_out = ck.output(out, so, 2 * (size_t)level * N);
        ck.apart(sp_out, ck.operand(a, sa, 2 * (size_t)(a_rpp ? a_rpp : L) * N, "a", true), "a");
        ck.apart(sp_out, ck.operand(b, sb, 2 * (size_t)(b_rpp ? b_rpp : L) * N, "b", true), "b");
    }
    const bool fold = c.fuse_tails && sw::hmult_fold();
    const size_t r_d3 = (fold ? 0 : 3) * (size_t)L, r_r2 = 2 * (size_t)L;
    const size_t r_shared = std::max(KsTile::rows(c, level), rescale_ws_rows(level, 2));
    const long long sd = (long long)r_d3 * N, sr = 2LL * L * N;
    for_tiles(c, r_d3 + r_r2 + r_shared, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* d3 = ws;
        u64* r2 = d3 + r_d3 * N * tb;
        u64* sub = r2 + r_r2 * N * tb;
        if (fold) {
            const u64* ta = a + (size_t)b0 * sa;
            const u64* bt = b + (size_t)b0 * sb;
            const TensorFold tf{ta, bt, sa, sb, (long long)(a_rpp ? a_rpp : L) * N, (long long)(b_rpp ? b_rpp : L) * N};
            KsTile t(c, level, nb, sub, st, &rlk);
            t.decompose(nullptr, 0, nullptr, 0, &tf);
            t.mac(t.cxi, t.s_cxi, rlk, &tf);   // (the MAC takes the own digit from a and b: its cx is not read)
            t.moddown({.p = r2, .sp = sr, .form = KsOut::RESCALE, .rs = {out + (size_t)b0 * so, so}});
            return;
        }
        launch_tensor(c, a + (size_t)b0 * sa, b + (size_t)b0 * sb, d3, nb, sa, sb, sd, L, rm_seq(L), st, a_rpp, b_rpp);
        ckks_relin_tail(c, level, d3, sd, rlk, out + (size_t)b0 * so, so, true, r2, sub, nb, st);
    });
}

// ---- encrypted inner product: sum_i a_i (x) b_i with ONE relinearisation.  The degree-2 tensors are summed exactly (k_tensor_sum:
// every operand row read once, d3 written once), then the sum takes the key switch and the rescale of a single HMult.
// every argument error of the two entry points, before any work is queued; false: nothing to do (batch <= 0)
static bool dot_check(const Context& c, int level, const DotTerms& t, bool rescale, const u64* out, long long so, size_t wout, int batch) {
    LSA_REQUIRE(c.algo == LSA_ALGO_CKKS, "dot: context is not CKKS");
    LSA_REQUIRE(t.n >= 1, "dot: needs at least one term");
    LSA_REQUIRE(level >= 0 && level < c.nq, "dot: level out of range");
    LSA_REQUIRE(!rescale || level >= 1, "dot: rescale needs level >= 1");
    if (batch <= 0) return false;
    const int L = level + 1;
    const size_t N = (size_t)c.n;
    LSA_REQUIRE(t.as && t.sas && t.bs && t.sbs && out, "dot: null argument");
    LSA_REQUIRE(so >= (long long)wout, "dot: output stride below one result");
    auto operand = [&](const u64* p, long long stride, int rpp, const char* what) {
        LSA_REQUIRE(p != nullptr, std::string("dot: ") + what + " is null");
        LSA_REQUIRE(rpp >= L, std::string("dot: rows per polynomial of ") + what + " below level + 1");
        const size_t words = 2 * (size_t)rpp * N;
        LSA_REQUIRE(stride == 0 || stride >= (long long)words, std::string("dot: batch stride of ") + what + " below one ciphertext");
        LSA_REQUIRE(layout::apart(out, so, wout, p, stride, words, batch), std::string("dot: the output overlaps ") + what);
    };
    for (int i = 0; i < t.n; i++) {
        operand(t.as[i], t.sas[i], t.a_rpp && t.a_rpp[i] ? t.a_rpp[i] : L, "an operand");
        operand(t.bs[i], t.sbs[i], t.b_rpp && t.b_rpp[i] ? t.b_rpp[i] : L, "an operand");
    }
    if (t.addend) operand(t.addend, t.s_addend, L, "the addend");
    return true;
}

// the tile's summed tensor: launches of up to LSA_DOT_MAX_TERMS pairs, the later ones adding to d3; the addend rides in the first
static void dot_tensor(Context& c, int level, const DotTerms& t, int b0, u64* d3, long long sd, int nb, hipStream_t s) {
    const int L = level + 1;
    for (int i0 = 0; i0 < t.n; i0 += LSA_DOT_MAX_TERMS) {
        const int m = std::min(LSA_DOT_MAX_TERMS, t.n - i0);
        const u64 *a[LSA_DOT_MAX_TERMS], *b[LSA_DOT_MAX_TERMS];
        for (int i = 0; i < m; i++) {
            a[i] = t.as[i0 + i] + (size_t)b0 * t.sas[i0 + i];
            b[i] = t.bs[i0 + i] + (size_t)b0 * t.sbs[i0 + i];
        }
        const bool first = i0 == 0;
        launch_tensor_sum(c, m, a, t.sas + i0, t.a_rpp ? t.a_rpp + i0 : nullptr, b, t.sbs + i0, t.b_rpp ? t.b_rpp + i0 : nullptr,
                          first && t.addend ? t.addend + (size_t)b0 * t.s_addend : nullptr, t.s_addend, !first, d3, sd, nb, L, rm_seq(L), s);
    }
}

void ckks_mult_sum(Context& c, int level, const DotTerms& t, u64* d3, int batch, long long sd, hipStream_t s) {
    if (!dot_check(c, level, t, false, d3, sd, 3 * (size_t)(level + 1) * c.n, batch)) return;
    dot_tensor(c, level, t, 0, d3, sd, batch, s);
}

void ckks_dot(Context& c, int level, const DotTerms& t, const Key& rlk, u64* out, int batch, long long so, bool with_rescale,
              hipStream_t s) {
    if (!dot_check(c, level, t, with_rescale, out, so, 2 * (size_t)(with_rescale ? level : level + 1) * c.n, batch)) return;
    const long long N = c.n;
    const int L = level + 1;
    const size_t r_d3 = 3 * (size_t)L, r_r2 = 2 * (size_t)L;
    const size_t r_shared = std::max(KsTile::rows(c, level), rescale_ws_rows(level, 2));
    const long long sd = (long long)r_d3 * N;
    for_tiles(c, r_d3 + r_r2 + r_shared, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* d3 = ws;
        u64* r2 = d3 + r_d3 * N * tb;
        u64* sub = r2 + r_r2 * N * tb;
        dot_tensor(c, level, t, b0, d3, sd, nb, st);
        ckks_relin_tail(c, level, d3, sd, rlk, out + (size_t)b0 * so, so, with_rescale, r2, sub, nb, st);
    });
}

void drop_level(Context& c, int level, int polys, const u64* in, u64* out, int batch, long long sin, long long sout,
                hipStream_t s) {
    // scheme-agnostic (a row copy).  The second polynomial's rows move towards lower addresses while other workgroups still
    // read: in place is refused like any other overlap
    const EntryCheck ck(c, "lsa_drop_level", -1, level, 1, batch);
    ck.polys(polys);
    if (batch <= 0) return;
    ck.apart(ck.output(out, sout, (size_t)polys * level * ck.N), ck.operand(in, sin, (size_t)polys * (level + 1) * ck.N, "in", false), "in");
    std::vector<int> rows;
    for (int p = 0; p < polys; p++)
        for (int i = 0; i < level; i++) rows.push_back(p * (level + 1) + i);
    launch_copy_rows(c, in, sin, out, sout, (int)rows.size(), rows.data(), batch, s);
}

void poly_addsub(Context& c, int op, int level, int polys, const u64* a, const u64* b, u64* out, int batch, long long sa,
                 long long sb, long long so, hipStream_t s) {
    const EntryCheck ck(c, "lsa_poly_addsub", -1, level, 0, batch);
    LSA_REQUIRE(op >= 0 && op <= 2, ck.who + ": op must be 0 add, 1 sub, 2 neg");
    ck.polys(polys);
    if (batch <= 0) return;
    {   // element-wise: every lane reads its words before it stores them, so out may BE a or b (same pointer, same stride)
        const size_t w = (size_t)polys * (level + 1) * ck.N;
        const Span sp_out = ck.output(out, so, w);
        ck.same_or_apart(sp_out, ck.operand(a, sa, w, "a", true), "a");
        if (op != EW_NEG) ck.same_or_apart(sp_out, ck.operand(b, sb, w, "b", true), "b");   // (neg: b is ignored, null allowed)
    }
    launch_elementwise(c, (EwOp)op, a, b, out, batch, sa, sb, so, polys * (level + 1), rm_seq(level + 1), s);
}

// ================================================================================================ BFV
static int bfv_aux_limbs(const Context& c, int level) { return bfv_aux_count(c.T.mod.data(), level + 1, c.logn); }

// ---- BFV multiply: d3 = t * round(sum_i a_i (x) b_i / Q).  The operands are extended from Q_level to Q_level u the first M auxiliary
// primes, multiplied there (exact while the auxiliary basis holds the sum: tables.h), and the division by Q is one inverse transform
// and six exact base conversions.  bfv_mult is the one-term case; bfv_mult_sum / bfv_dot (below bfv_mult_relin) share every step.
// Folded (default; LSA_BFV_FOLD=0: the separate element-wise steps): the Q limbs are transformed straight from the operands into
// the extended buffer (no copy), and the two element-wise steps around the last conversion -- (aux - ext) * Q^-1 before it,
// * t after it -- live in its source load and its constants (Context::BaseConvFold)

namespace {
// workspace rows per ciphertext of a tile: g pairs of extended operands [2][L+M] each, the tensor [3][L+M], the converted rows [3][M]
size_t bfv_mult_rows(int L, int M, int g) { return (4 * (size_t)g + 3) * (size_t)(L + M) + 3 * (size_t)M; }

struct BfvBasis {   // Q_level u the first M auxiliary primes: row maps, conversion plans and constants, folded or not
    int L = 0, M = 0, T2 = 0;
    bool fold = false;
    RowMap rmT, rmAux;
    const BaseConvPlan *kQA = nullptr, *kAQ = nullptr, *kAQf = nullptr;
    BaseConvRows rQA{}, rAQ{};
    const u64 *kQinv = nullptr, *kT = nullptr;
    unsigned char lmA[LSA_MAX_PERIOD], lmQ[LSA_MAX_PERIOD];
    std::vector<int> sub_rows;
};

// the only place that builds them.  The cached constants are keyed by L and M: one context runs a level with M(1) for a single
// product and with M(m) > M(1) for a sum
BfvBasis bfv_basis(Context& c, const char* who, int level, int M, bool fold_on) {
    BfvBasis B;
    const int L = level + 1, T2 = L + M;
    LSA_REQUIRE(M >= 1 && M <= c.nmul && T2 <= LSA_MAX_PERIOD, std::string(who) + ": auxiliary basis too small");
    B.L = L, B.M = M, B.T2 = T2, B.fold = fold_on;
    std::vector<int> qmods, amods;
    B.rmT.period = T2;
    for (int i = 0; i < L; i++) {
        qmods.push_back(i);
        B.rmT.mod_of[i] = (unsigned char)i;
        B.rQA.src_row[i] = i, B.rAQ.dst_row[i] = i;
        B.lmQ[i] = (unsigned char)i;
    }
    for (int i = 0; i < M; i++) {
        amods.push_back(c.aux_mod(i));
        B.rmT.mod_of[L + i] = (unsigned char)c.aux_mod(i);
        B.rQA.dst_row[i] = i, B.rAQ.src_row[i] = i;
        B.lmA[i] = (unsigned char)c.aux_mod(i);
    }
    B.rmAux = B.rmT;   // the auxiliary rows only
    for (int i = 0; i < L; i++) B.rmAux.mod_of[i] = LSA_ROW_SKIP;
    std::vector<u64> qinv(M), tq(L);   // Q^-1 mod aux_i and t mod q_i
    for (int i = 0; i < M; i++) {
        const u64 p = c.T.mod[c.aux_mod(i)];
        u64 pr = 1;
        for (int l = 0; l < L; l++) pr = mul_mod_host(pr, c.T.mod[l] % p, p);
        qinv[i] = inv_mod(pr, p);
    }
    for (int i = 0; i < L; i++) tq[i] = c.t % c.T.mod[i];
    const std::string tag = std::to_string(L) + "m" + std::to_string(M);
    B.kQA = c.baseconv(qmods, amods, true);
    if (fold_on) {
        Context::BaseConvFold fold{"bfv_mul" + tag, qinv, tq};
        B.kAQf = c.baseconv(amods, qmods, true, false, &fold);
    } else {
        B.kAQ = c.baseconv(amods, qmods, true);
        B.kQinv = c.const_vec("bfv_qinv" + tag, amods, qinv);
        B.kT = c.const_vec("bfv_t" + tag, qmods, tq);
    }
    B.sub_rows.resize(M);
    for (int i = 0; i < M; i++) B.sub_rows[i] = i;
    return B;
}

// one operand into [2][T2][N] per item: the Q limbs transformed (folded: from where they are; else copied first), the auxiliary
// limbs by the centred exact extension, then transformed
void bfv_extend(Context& c, const BfvBasis& B, const u64* src, long long ss, u64* e, int nb, hipStream_t s) {
    const long long N = c.n;
    const int L = B.L, T2 = B.T2;
    const long long s_e = 2LL * T2 * N;
    for (int p = 0; p < 2; p++) {
        std::vector<int> rr(L);
        for (int i = 0; i < L; i++) rr[i] = p * L + i;
        if (B.fold) launch_ntt(c, src + (size_t)p * L * N, e + (size_t)p * T2 * N, nb, ss, s_e, L, rm_seq(L), false, s);
        else launch_copy_rows(c, src, ss, e + (size_t)p * T2 * N, s_e, L, rr.data(), nb, s);
        launch_baseconv(c, B.kQA, B.rQA, src + (size_t)p * L * N, e + ((size_t)p * T2 + L) * N, nb, ss, s_e, s);
    }
    launch_ntt(c, e, e, nb, s_e, 2 * T2, B.fold ? B.rmAux : B.rmT, false, s);
}

// d [3][T2][N] (NTT domain) -> o3 = t * round(d / Q) [3][L][N]; ext: [3][M][N] per item
void bfv_scale_down(Context& c, const BfvBasis& B, u64* d, u64* ext, u64* o3, long long so, int nb, hipStream_t s) {
    const long long N = c.n;
    const int L = B.L, M = B.M, T2 = B.T2;
    const long long s_d = 3LL * T2 * N, s_x = 3LL * M * N;
    launch_ntt(c, d, d, nb, s_d, 3 * T2, B.rmT, true, s);
    for (int k = 0; k < 3; k++) launch_baseconv(c, B.kQA, B.rQA, d + (size_t)k * T2 * N, ext + (size_t)k * M * N, nb, s_d, s_x, s);
    if (B.fold) {
        // out = t * conv_{A->Q}((aux - ext) * Q^-1): the subtraction on the conversion's source load, both factors in its constants
        for (int k = 0; k < 3; k++)
            launch_baseconv(c, B.kAQf, B.rAQ, d + ((size_t)k * T2 + L) * N, o3 + (size_t)k * L * N, nb, s_d, so, s, ext + (size_t)k * M * N,
                            s_x, B.sub_rows.data());
        return;
    }
    // aux part <- (aux - ext) * Q^-1     (= round(d/Q) in basis QMul), converted to Q, then * t
    launch_sub_mul_general(c, 3, M, B.lmA, B.kQinv, d + (size_t)L * N, s_d, T2, ext, s_x, M, nullptr, 0, 0, 0, d + (size_t)L * N, s_d,
                           T2, nb, s);
    for (int k = 0; k < 3; k++) launch_baseconv(c, B.kAQ, B.rAQ, d + ((size_t)k * T2 + L) * N, o3 + (size_t)k * L * N, nb, s_d, so, s);
    launch_sub_mul_general(c, 3, L, B.lmQ, B.kT, o3, so, L, nullptr, 0, 0, nullptr, 0, 0, 0, o3, so, L, nb, s);
}

#define LSA_BFV_DOT_CHUNK 4   // pairs extended per k_tensor_sum launch (measured, and why not more)

// the summed product of checked arguments, tile by tile: per group of the plan, chunks of g pairs extended and summed into the tensor
// (an operand shared by the batch once, a square once), one scale-down per group
void bfv_mult_sum_run(Context& c, const char* who, int level, const DotTerms& t, u64* d3, int batch, long long sd, hipStream_t s0) {
    const long long N = c.n;
    const int L = level + 1;
    const BfvDotPlan plan = bfv_dot_plan(c.T.mod.data(), c.nq, level, c.logn, t.n);
    const bool fold_on = sw::bfv_fold();
    // the groups' bases: a full group's and, where it differs, the shorter last group's
    std::vector<BfvBasis> bases;
    auto basis_of = [&](int m) -> const BfvBasis& {
        const int M = bfv_dot_aux_count(c.T.mod.data(), L, c.logn, m);
        for (const auto& B : bases)
            if (B.M == M) return B;
        bases.push_back(bfv_basis(c, who, level, M, fold_on));
        return bases.back();
    };
    bases.reserve(2);
    const int Mx = basis_of(std::min(t.n, plan.max_terms)).M;
    if (plan.n_groups > 1 && t.n % plan.max_terms) basis_of(t.n % plan.max_terms);
    // pairs per launch: the setting, at most one launch's and one group's terms, and no more than leaves the tile one product gets
    auto rows_of = [&](int g) { return bfv_mult_rows(L, Mx, g); };
    int g = std::min({c.bfv_dot_chunk > 0 ? c.bfv_dot_chunk : LSA_BFV_DOT_CHUNK, LSA_DOT_MAX_TERMS, t.n, plan.max_terms});
    const int tile1 = pick_tile(c, bfv_mult_rows(L, bfv_aux_limbs(c, level), 1), batch);
    while (g > 1 && pick_tile(c, rows_of(g), batch) < tile1) g--;
    for_tiles(c, rows_of(g), batch, s0, [&](int nb, int b0, u64* ws, int tb, hipStream_t s) {
        u64* o3 = d3 + (size_t)b0 * sd;
        for (int gi = 0, i0 = 0; gi < plan.n_groups; gi++) {
            const int m = std::min(plan.max_terms, t.n - i0);
            const BfvBasis& B = basis_of(m);
            const int T2 = B.T2;
            const long long s_e = 2LL * T2 * N, s_d = 3LL * T2 * N;
            const size_t slot = (size_t)tb * s_e;
            u64* e = ws;
            u64* d = e + 2 * (size_t)g * slot;
            u64* ext = d + (size_t)tb * s_d;
            for (int j0 = 0; j0 < m; j0 += g) {
                const int mm = std::min(g, m - j0);
                const u64 *pa[LSA_DOT_MAX_TERMS], *pb[LSA_DOT_MAX_TERMS];
                long long sa[LSA_DOT_MAX_TERMS], sb[LSA_DOT_MAX_TERMS];
                for (int j = 0; j < mm; j++) {
                    const int i = i0 + j0 + j;
                    // an operand shared by the batch (stride 0) is extended once and read by every item of the tensor
                    u64* ea = e + (size_t)(2 * j) * slot;
                    bfv_extend(c, B, t.as[i] + (size_t)b0 * t.sas[i], t.sas[i], ea, t.sas[i] ? nb : 1, s);
                    pa[j] = ea, sa[j] = t.sas[i] ? s_e : 0;
                    if (t.as[i] == t.bs[i] && t.sas[i] == t.sbs[i]) {   // a square
                        pb[j] = pa[j], sb[j] = sa[j];
                        continue;
                    }
                    u64* eb = e + (size_t)(2 * j + 1) * slot;
                    bfv_extend(c, B, t.bs[i] + (size_t)b0 * t.sbs[i], t.sbs[i], eb, t.sbs[i] ? nb : 1, s);
                    pb[j] = eb, sb[j] = t.sbs[i] ? s_e : 0;
                }
                // a group of one pair is a plain product (k_tensor); both kernels write canonical residues of the same values
                if (m == 1) launch_tensor(c, pa[0], pb[0], d, nb, sa[0], sb[0], s_d, T2, B.rmT, s);
                else launch_tensor_sum(c, mm, pa, sa, nullptr, pb, sb, nullptr, nullptr, 0, j0 > 0, d, s_d, nb, T2, B.rmT, s);
            }
            if (gi == 0) {
                bfv_scale_down(c, B, d, ext, o3, sd, nb, s);
            } else {   // a later group: scaled down on its own into the (now free) extension slots, then added in Q
                const long long st = 3LL * L * N;
                bfv_scale_down(c, B, d, ext, e, st, nb, s);
                launch_elementwise(c, EW_ADD, o3, e, o3, nb, sd, st, sd, 3 * L, rm_seq(L), s);
            }
            i0 += m;
        }
        if (t.addend)
            launch_elementwise(c, EW_ADD, o3, t.addend + (size_t)b0 * t.s_addend, o3, nb, sd, t.s_addend, sd, 2 * L, rm_seq(L), s);
    });
}
}  // namespace

void bfv_mult(Context& c, int level, const u64* a, const u64* b, u64* d3, int batch, long long sa, long long sb,
              long long sd, hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_mult", LSA_ALGO_BFV, level, 0, batch);
    LSA_REQUIRE(bfv_aux_limbs(c, level) <= c.nmul, ck.who + ": auxiliary basis too small");
    if (batch <= 0) return;
    {   // a stride of 0 shares an operand with the whole batch
        const size_t w = 2 * (size_t)(level + 1) * ck.N;
        const Span out = ck.output(d3, sd, w / 2 * 3, "d3");
        ck.apart(out, ck.operand(a, sa, w, "a", true), "a");
        ck.apart(out, ck.operand(b, sb, w, "b", true), "b");
    }
    const DotTerms one{1, &a, &sa, nullptr, &b, &sb, nullptr, nullptr, 0};   // the one-term sum: M(1) auxiliary primes, k_tensor
    bfv_mult_sum_run(c, "lsa_bfv_mult", level, one, d3, batch, sd, s);
}

// key switch of a coefficient-domain polynomial: NTT in, INTT out
// cx in the coefficient domain; p[h] = (h < base_polys ? base[h] : 0) + KeySwitch(cx)[h], all in the coefficient domain.
// Only the MAC's own-digit operand needs cx in the NTT domain; the decomposition starts from the coefficients the caller
// already has and the ModDown tail runs on coefficients (KsOut::COEFF).  Workspace: NTT(cx) [L] rows, then the tile's.
static void bfv_key_switch(Context& c, int level, const u64* cx, long long scx, const Key& key, const KsOut& o, int nb, u64* ws,
                           hipStream_t s) {
    const long long scxn = (long long)(level + 1) * c.n;
    KsTile t(c, level, nb, ws + (size_t)nb * scxn, s, &key);
    launch_ntt(c, cx, ws, nb, scx, scxn, level + 1, rm_seq(level + 1), false, s);
    t.decompose(ws, scxn, cx, scx);
    t.mac(ws, scxn, key);
    t.moddown(o);
}

void bfv_relin(Context& c, int level, const u64* d3, const Key& rlk, u64* out, int batch, long long sd, long long so,
               hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_relin", LSA_ALGO_BFV, level, 0, batch);
    ck.key(rlk, "the relinearisation key");
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    ck.apart(ck.output(out, so, 2 * (size_t)L * N), ck.operand(d3, sd, 3 * (size_t)L * N, "d3", false), "d3");
    for_tiles(c, KsTile::rows(c, level) + L, batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        const u64* d = d3 + (size_t)b0 * sd;
        bfv_key_switch(c, level, d + 2LL * L * N, sd, rlk,
                       {.p = out + (size_t)b0 * so, .sp = so, .base = d, .sbase = sd, .base_rpp = L, .base_polys = 2, .form = KsOut::COEFF},
                       nb, ws, st);
    });
}

// multiply + relinearise; the degree-2 tensor lives in the second arena so that the two pipelines' own arena use cannot overlap it
void bfv_mult_relin(Context& c, int level, const u64* a, const u64* b, const Key& rlk, u64* out, int batch, long long sa,
                    long long sb, long long so, hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_mult_relin", LSA_ALGO_BFV, level, 0, batch);
    ck.key(rlk, "the relinearisation key");
    if (batch <= 0) return;
    const size_t w = 2 * (size_t)(level + 1) * ck.N;
    const Span sp_out = ck.output(out, so, w);
    ck.apart(sp_out, ck.operand(a, sa, w, "a", true), "a");
    ck.apart(sp_out, ck.operand(b, sb, w, "b", true), "b");
    const long long sd = 3LL * (level + 1) * c.n;
    u64* d3 = c.workspace2((size_t)sd * batch, s);
    bfv_mult(c, level, a, b, d3, batch, sa, sb, sd, s);
    bfv_relin(c, level, d3, rlk, out, batch, sd, so, s);
}

// ---- BFV encrypted inner product: t * round(sum_i a_i (x) b_i / Q) with ONE scale-down and ONE relinearisation.  Only the
// extension of the operands and the tensor depend on the pair; the tensors are summed in Q u QMul (k_tensor_sum), where the sum is
// exact while the auxiliary basis holds it (tables.h bfv_dot_plan: groups of at most max_terms pairs, a group of m over the first
// M(m) auxiliary primes), and the inverse transform, the six conversions of the division by Q and the key switch run once.
// The extension, the tensor and the scale-down are shared with bfv_mult (bfv_mult_sum_run above it).
namespace {
// every argument error of the two entry points, before anything is queued; false: nothing to do (batch <= 0)
bool bfv_dot_check(const Context& c, int level, const DotTerms& t, const Key* rlk, bool with_relin, const u64* out, long long so,
                   int out_polys, int batch) {
    const EntryCheck ck(c, "bfv_dot", LSA_ALGO_BFV, level, 0, batch);
    LSA_REQUIRE(t.n >= 1, ck.who + ": needs at least one term");
    if (with_relin) {
        LSA_REQUIRE(rlk != nullptr, ck.who + ": the relinearisation key is null");
        ck.key(*rlk, "the relinearisation key");
    }
    if (batch <= 0) return false;
    LSA_REQUIRE(t.as && t.sas && t.bs && t.sbs, ck.who + ": null argument");
    const size_t w = 2 * (size_t)(level + 1) * ck.N;
    const Span sp_out = ck.output(out, so, w / 2 * out_polys, "the output");
    for (int i = 0; i < t.n; i++) {
        ck.apart(sp_out, ck.operand(t.as[i], t.sas[i], w, "an operand", true), "an operand");
        ck.apart(sp_out, ck.operand(t.bs[i], t.sbs[i], w, "an operand", true), "an operand");
    }
    if (t.addend) ck.apart(sp_out, ck.operand(t.addend, t.s_addend, w, "the addend", true), "the addend");
    return true;
}
}  // namespace

void bfv_mult_sum(Context& c, int level, const DotTerms& t, u64* d3, int batch, long long sd, hipStream_t s) {
    if (!bfv_dot_check(c, level, t, nullptr, false, d3, sd, 3, batch)) return;
    bfv_mult_sum_run(c, "bfv_dot", level, t, d3, batch, sd, s);
}

// the summed, scaled-down tensor lives in the second arena, as in bfv_mult_relin
void bfv_dot(Context& c, int level, const DotTerms& t, const Key* rlk, u64* out, int batch, long long so, hipStream_t s) {
    if (!bfv_dot_check(c, level, t, rlk, true, out, so, 2, batch)) return;
    const long long sd = 3LL * (level + 1) * c.n;
    u64* d3 = c.workspace2((size_t)sd * batch, s);
    bfv_mult_sum_run(c, "bfv_dot", level, t, d3, batch, sd, s);
    bfv_relin(c, level, d3, *rlk, out, batch, sd, so, s);
}

void bfv_rotate(Context& c, int level, const u64* in, u64 g, const Key& glk, u64* out, int batch, long long sin,
                long long sout, hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_rotate", LSA_ALGO_BFV, level, 0, batch);
    ck.key(glk, "the Galois key");
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    // always the two-step form (tail into the workspace, then the permutation): out == in item for item is safe, any other overlap
    // would let one tile store over what another still reads
    ck.same_or_apart(ck.output(out, sout, 2 * (size_t)L * N), ck.operand(in, sin, 2 * (size_t)L * N, "in", false), "in");
    const u32* perm = c.coeff_perm(g);
    const size_t ks_rows = KsTile::rows(c, level) + L;
    const long long sp = 2LL * L * N;
    for_tiles(c, ks_rows + 2 * (size_t)L, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* p = ws + ks_rows * N * tb;
        const u64* ct = in + (size_t)b0 * sin;
        bfv_key_switch(c, level, ct + (long long)L * N, sin, glk,   // p0 = c0 + ks0
                       {.p = p, .sp = sp, .base = ct, .sbase = sin, .base_rpp = L, .base_polys = 1, .form = KsOut::COEFF}, nb, ws, st);
        launch_permute_coeff(c, perm, p, sp, out + (size_t)b0 * sout, sout, 2 * L, rm_seq(L), nb, st);
    });
}

// rotations of the same ciphertexts by several Galois elements with ONE decomposition (hoisting); outs[i] = rotate(in, g[i]),
// each identical to bfv_rotate's result.  Per tile: c1 into the NTT domain once (the MAC's own-digit operand), the digits'
// conversions and extension transforms once from the coefficients; then per key the stand-alone MAC (several keys: the
// fused second pass + MAC does not apply) and the coefficient-domain ModDown, whose tail applies the automorphism by its
// loads and writes outs[i] directly (k_sub_mul_perm).  Two-step form (tail into the workspace, then k_permute) for an
// output that overlaps the input, for N > 2^14, with LSA_ROT_SCATTER=0 and with unfused tails.
void bfv_rotate_many(Context& c, int level, const u64* in, int n_rot, const u64* g, const Key* const* glk, u64* const* outs,
                     int batch, long long sin, long long sout, hipStream_t s) {
    LSA_REQUIRE(c.algo == LSA_ALGO_BFV, "context is not BFV");
    if (n_rot <= 0) return;
    if (n_rot == 1) {
        bfv_rotate(c, level, in, g[0], *glk[0], outs[0], batch, sin, sout, s);
        return;
    }
    LSA_REQUIRE(level >= 0 && level < c.nq, "level out of range");
    const long long N = c.n;
    const int L = level + 1;
    const size_t ks_rows = KsTile::rows(c, level) + L;
    const long long sp = 2LL * L * N;
    // the one-pass tail stages a limb in LDS (N <= 2^14); larger rings keep the two steps, which measured faster than gathering
    // from global memory
    const bool gather_on = sw::rot_scatter() && c.fuse_tails && c.logn <= LSA_PERM_LDS_MAX_LOGN;
    std::vector<const u32*> perms(n_rot);
    std::vector<bool> direct(n_rot);
    std::vector<int> order;   // an output that overlaps the input goes last: every other rotation still reads the intact c0
    int overlapping = -1;
    for (int i = 0; i < n_rot; i++) {
        const bool apart = layout::apart(outs[i], sout, 2 * (size_t)L * N, in, sin, 2 * (size_t)L * N, batch);
        perms[i] = c.coeff_perm(g[i]);
        direct[i] = apart && gather_on;
        if (apart) {
            order.push_back(i);
            continue;
        }
        LSA_REQUIRE(overlapping < 0, "bfv_rotate_many: at most one output may overlap the input");
        overlapping = i;
    }
    if (overlapping >= 0) order.push_back(overlapping);
    for_tiles(c, ks_rows + 2 * (size_t)L, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* cxn = ws;
        u64* p = ws + ks_rows * N * tb;
        const u64* ct = in + (size_t)b0 * sin;
        KsTile t(c, level, nb, ws + (size_t)nb * L * N, st);
        launch_ntt(c, ct + (long long)L * N, cxn, nb, sin, (long long)L * N, L, rm_seq(L), false, st);
        t.decompose(cxn, (long long)L * N, ct + (long long)L * N, sin);
        for (int i : order) {
            t.mac(cxn, (long long)L * N, *glk[i]);
            KsOut o{.p = p, .sp = sp, .base = ct, .sbase = sin, .base_rpp = L, .base_polys = 1, .form = KsOut::COEFF};
            if (direct[i]) {   // p0 = c0 + ks0 and the automorphism in one tail, straight into the output
                o.p = outs[i] + (size_t)b0 * sout;
                o.sp = sout;
                o.coeff_gather = perms[i];
                t.moddown(o);
                continue;
            }
            t.moddown(o);
            launch_permute_coeff(c, perms[i], p, sp, outs[i] + (size_t)b0 * sout, sout, 2 * L, rm_seq(L), nb, st);
        }
    });
}

// ---- BFV ct x pt_mul.  A pt_mul plaintext is the message lifted to Q, in the NTT domain and in Montgomery form (the
// reference frontend's BfvPlaintextMulNode); per poly and limb ct x pt = INTT(NTT(ct) . pt . 2^-64 mod q), Lattigo v4's
// mulPlaintextMul.  The Montgomery product rides on the store of the forward transform's last pass (fz_epi = 3, FZ bit 4);
// LSA_PTMUL_FUSED=0 runs the forward transform, k_mont_muladd and the inverse transform instead.  A MAC sums
// its terms in the NTT domain (canonical residues: the same values as a per-term multiply and adds) and runs one inverse
// transform per output; the partial sum is added after it, in the coefficient domain.
// out = NTT(ct) . pt . 2^-64 (+ out if acc) for nb ciphertexts; tmp receives the first pass of a two-pass transform (may be
// out, or ct, when acc is false)
static void ptmul_term(Context& c, int L, const u64* ct, long long sct, const u64* pt, long long spt, bool acc, u64* out,
                       long long so, u64* tmp, long long stmp, int nb, hipStream_t s) {
    const RowMap rm = rm_seq(L);
    if (sw::ptmul_fused()) {
        NttFusion fz;
        fz.epi = 3;
        fz.limbs = L;
        fz.a = pt;
        fz.a_stride = spt;
        fz.base = acc ? out : nullptr;
        fz.base_stride = so;
        fz.base_rpp = L;
        fz.out = out;
        fz.out_stride = so;
        fz.out_rpp = L;
        launch_ntt(c, ct, tmp, nb, sct, stmp, 2 * L, rm, false, s, &fz);
        return;
    }
    launch_ntt(c, ct, tmp, nb, sct, stmp, 2 * L, rm, false, s);
    launch_mont_muladd(c, tmp, stmp, pt, spt, acc ? out : nullptr, so, out, so, nb, 2, L, rm, s);
}

void bfv_mult_plain_mul(Context& c, int level, const u64* ct, const u64* pt, u64* out, int batch, long long sct, long long spt,
                        long long sout, hipStream_t s) {
    LSA_REQUIRE(c.algo == LSA_ALGO_BFV, "context is not BFV");
    LSA_REQUIRE(level >= 0 && level < c.nq, "level out of range");
    if (batch <= 0) return;
    const int L = level + 1;
    const size_t wct = 2 * (size_t)L * c.n, wpt = (size_t)L * c.n;
    LSA_REQUIRE((out == ct && sout == sct) || layout::apart(out, sout, wct, ct, sct, wct, batch),
                "bfv_mult_plain_mul: out must be ct or not overlap it");
    LSA_REQUIRE(layout::apart(out, sout, wct, pt, spt, wpt, batch), "bfv_mult_plain_mul: out overlaps the plaintexts");
    ptmul_term(c, L, ct, sct, pt, spt, false, out, sout, out, sout, batch, s);
    launch_ntt(c, out, out, batch, sout, 2 * L, rm_seq(L), true, s);
}

void bfv_mac_plain_mul(Context& c, int level, int n, const u64* const* cts, const long long* scts, const u64* const* pts,
                       const long long* spts, const u64* partial, long long spartial, u64* out, int batch, long long sout,
                       hipStream_t s) {
    LSA_REQUIRE(c.algo == LSA_ALGO_BFV, "context is not BFV");
    LSA_REQUIRE(level >= 0 && level < c.nq, "level out of range");
    LSA_REQUIRE(n >= 1, "bfv_mac_plain_mul: needs at least one term");
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    const size_t wct = 2 * (size_t)L * N, wpt = (size_t)L * N;
    // out holds the running sum while the terms are read: it may alias none of them
    for (int i = 0; i < n; i++) {
        LSA_REQUIRE(layout::apart(out, sout, wct, cts[i], scts[i], wct, batch), "bfv_mac_plain_mul: out overlaps a ciphertext");
        LSA_REQUIRE(layout::apart(out, sout, wct, pts[i], spts[i], wpt, batch), "bfv_mac_plain_mul: out overlaps a plaintext");
    }
    LSA_REQUIRE(!partial || layout::apart(out, sout, wct, partial, spartial, wct, batch), "bfv_mac_plain_mul: out overlaps the partial sum");
    // workspace: the first pass of terms 1.. (term 0 runs it in out)
    for_tiles(c, n > 1 ? 2 * (size_t)L : 0, batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        u64* o = out + (size_t)b0 * sout;
        for (int i = 0; i < n; i++)
            ptmul_term(c, L, cts[i] + (size_t)b0 * scts[i], scts[i], pts[i] + (size_t)b0 * spts[i], spts[i], i > 0, o, sout,
                       i == 0 ? o : ws, i == 0 ? sout : 2LL * L * N, nb, st);
        launch_ntt(c, o, o, nb, sout, 2 * L, rm_seq(L), true, st);
        if (partial)
            launch_elementwise(c, EW_ADD, o, partial + (size_t)b0 * spartial, o, nb, sout, spartial, sout, 2 * L, rm_seq(L), st);
    });
}

// ---- BFV rotate-and-MAC: out = sum_i rot_{g_i}(in) . pt_i (+ partial), the diagonal (Halevi-Shoup) matrix-vector product.
// Every output is bit-identical to bfv_rotate_many followed by bfv_mac_plain_mul on the same terms: the rotations never
// leave the NTT domain.  NTT(ModDown_coeff(x)) is the NTT-domain ModDown of NTT(x), residue for residue, and the NTT-domain
// automorphism is the scatter map of the ModDown store, so per rotation term only the 2k P rows of the key-switch
// accumulator are inverse-transformed and the 2L rows of its conversion forward-transformed (2(L+k) + 2L before); the
// rotated ciphertext is never written.  Per tile: NTT(c0) and NTT(c1) once, one decomposition; identity terms (g = 1) are
// a Montgomery product of NTT(ct); a rotation term is its key MAC and a ModDown whose last store applies the automorphism,
// the pt_mul product and the running sum (fz_epi = 4).  One inverse transform per output, then the partial sum.
// LSA_ROTMAC_FUSED=0, unfused tails and LSA_ROT_SCATTER=0 run each rotation term in two steps instead:
// the NTT-domain ModDown into the workspace (scattered, or k_permute after it), then k_mont_muladd.
void bfv_rotate_mac_plain_mul(Context& c, int level, const u64* in, int n, const u64* g, const Key* const* glk,
                              const u64* const* pts, const long long* spts, const u64* partial, long long spartial, u64* out,
                              int batch, long long sin, long long sout, hipStream_t s) {
    LSA_REQUIRE(c.algo == LSA_ALGO_BFV, "context is not BFV");
    LSA_REQUIRE(level >= 0 && level < c.nq, "level out of range");
    LSA_REQUIRE(n >= 1, "bfv_rotate_mac_plain_mul: needs at least one term");
    bool any_rot = false;
    for (int i = 0; i < n; i++) {
        LSA_REQUIRE((g[i] & 1) == 1 && g[i] < 2 * (u64)c.n, "bfv_rotate_mac_plain_mul: Galois element must be odd and < 2N");
        LSA_REQUIRE(pts[i] != nullptr, "bfv_rotate_mac_plain_mul: null plaintext");
        if (g[i] == 1) continue;
        LSA_REQUIRE(glk[i] != nullptr, "bfv_rotate_mac_plain_mul: a rotation term needs its key");
        any_rot = true;
    }
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    const size_t wct = 2 * (size_t)L * N, wpt = (size_t)L * N;
    // out holds the running sum while the input, the plaintexts and the partial sum are still read: it may alias none of them
    LSA_REQUIRE(layout::apart(out, sout, wct, in, sin, wct, batch), "bfv_rotate_mac_plain_mul: out overlaps the input");
    for (int i = 0; i < n; i++)
        LSA_REQUIRE(layout::apart(out, sout, wct, pts[i], spts[i], wpt, batch), "bfv_rotate_mac_plain_mul: out overlaps a plaintext");
    LSA_REQUIRE(!partial || layout::apart(out, sout, wct, partial, spartial, wct, batch),
                "bfv_rotate_mac_plain_mul: out overlaps the partial sum");
    const bool fused = sw::rotmac_fused() && c.fuse_tails && sw::rot_scatter();
    std::vector<const u32*> scatters(n, nullptr), perms(n, nullptr);
    for (int i = 0; i < n; i++) {
        if (g[i] == 1) continue;
        scatters[i] = rotation_scatter(c, g[i]);
        if (!scatters[i]) perms[i] = c.ntt_perm(g[i]);
    }
    const long long sct = 2LL * L * N;   // NTT(c0) | NTT(c1) per batch item in the workspace
    const size_t ks_rows = KsTile::rows(c, level);
    const size_t rows = 2 * (size_t)L + ks_rows + (fused ? 0 : 2 * (size_t)L);
    for_tiles(c, rows, batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        u64* ctn = ws;
        u64* sub = ctn + (size_t)nb * sct;
        u64* p = sub + (size_t)nb * ks_rows * N;   // two-step form: one rotated term, NTT domain
        const u64* ct = in + (size_t)b0 * sin;
        u64* o = out + (size_t)b0 * sout;
        KsTile t(c, level, nb, sub, st);
        launch_ntt(c, ct, ctn, nb, sin, sct, 2 * L, rm_seq(L), false, st);
        if (any_rot) t.decompose(ctn + L * N, sct, ct + (long long)L * N, sin);
        bool first = true;
        for (int i = 0; i < n; i++) {   // identity terms: no transform at all
            if (g[i] != 1) continue;
            launch_mont_muladd(c, ctn, sct, pts[i] + (size_t)b0 * spts[i], spts[i], first ? nullptr : o, sout, o, sout, nb, 2, L,
                               rm_seq(L), st);
            first = false;
        }
        for (int i = 0; i < n; i++) {
            if (g[i] == 1) continue;
            const u64* pt = pts[i] + (size_t)b0 * spts[i];
            t.mac(ctn + L * N, sct, *glk[i]);
            if (fused) {
                const RotMacTerm term{pt, spts[i], !first};
                t.moddown({.p = o, .sp = sout, .base = ctn, .sbase = sct, .base_rpp = L, .base_polys = 1, .scatter = scatters[i],
                           .rmac = &term});
            } else {
                t.moddown({.p = p, .sp = sct, .base = ctn, .sbase = sct, .base_rpp = L, .base_polys = 1, .scatter = scatters[i]});
                const u64* r = p;
                if (perms[i]) {   // no scattered store: the automorphism as a separate pass (conv is free again)
                    launch_permute_ntt(c, perms[i], p, sct, t.conv, t.s_conv, 2 * L, nb, st);
                    r = t.conv;
                }
                launch_mont_muladd(c, r, sct, pt, spts[i], first ? nullptr : o, sout, o, sout, nb, 2, L, rm_seq(L), st);
            }
            first = false;
        }
        launch_ntt(c, o, o, nb, sout, 2 * L, rm_seq(L), true, st);
        if (partial)
            launch_elementwise(c, EW_ADD, o, partial + (size_t)b0 * spartial, o, nb, sout, spartial, sout, 2 * L, rm_seq(L), st);
    });
}

void bfv_rescale(Context& c, int level, int polys, const u64* in, u64* out, int batch, long long sin, long long sout,
                 hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_rescale", LSA_ALGO_BFV, level, 1, batch);
    ck.polys(polys);
    if (batch <= 0) return;
    ck.apart(ck.output(out, sout, (size_t)polys * level * ck.N), ck.operand(in, sin, (size_t)polys * (level + 1) * ck.N, "in", false), "in");
    for_tiles(c, rescale_ws_rows(level, polys), batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        rescale(c, level, polys, in + (size_t)b0 * sin, sin, out + (size_t)b0 * sout, sout, nb, false, ws, st);
    });
}

// ================================================================================================ CKKS plaintext / constant operands
// Ciphertext (NTT domain, [2][level+1][N]) combined with something that is not encrypted: an encoded plaintext [level+1][N]
// (lsa_ckks_encode, linear_transform.hip) or a complex constant.  Every word is the oracle's (oracle/ckks_bootstrap.py
// Evaluator.mul_plain / add / mul_const / add_const / mul_by_i): canonical residues of exact modular products and sums, so the
// kernel that forms them is free -- plaintext products run on k_mac_plain, sums on k_elementwise, constants on k_cconst, which
// reads no plaintext at all (plain_ops.h).  A rescale is the existing ckks_rescale on the product, kept in the second arena.
namespace {

struct PlainCall {   // the checks every entry point shares; messages begin with the entry point's name
    const Context& c;
    std::string who;
    int level, batch, L;
    size_t wct, wpt;
    PlainCall(const Context& c_, const char* who_, int level_, int batch_, bool rescale) : c(c_), who(who_), level(level_), batch(batch_) {
        LSA_REQUIRE(c.algo == LSA_ALGO_CKKS, who + ": context is not CKKS");
        LSA_REQUIRE(level >= 0 && level < c.nq, who + ": level out of range");
        LSA_REQUIRE(!rescale || level >= 1, who + ": rescale needs level >= 1");
        L = level + 1;
        wct = 2 * (size_t)L * c.n;
        wpt = (size_t)L * c.n;
    }
    // the element-wise kernels move 16 bytes per lane at base + item * stride: every item has to start on a 16-byte boundary
    void aligned(const u64* p, long long stride, const char* what) const {
        LSA_REQUIRE(layout::aligned16(layout::span_of(p, stride, 0)),
                    who + ": " + what + " must be 16-byte aligned with an even batch stride");
    }
    void ciphertext(const u64* p, long long stride, const char* what) const {
        LSA_REQUIRE(p != nullptr, who + ": " + what + " is null");
        LSA_REQUIRE(stride >= (long long)wct, who + ": batch stride of " + what + " below one ciphertext");
        aligned(p, stride, what);
    }
    void plaintext(const u64* p, long long stride, const char* what) const {
        LSA_REQUIRE(p != nullptr, who + ": " + what + " is null");
        LSA_REQUIRE(stride == 0 || stride >= (long long)wpt, who + ": batch stride of " + what + " below one plaintext (0: shared by the batch)");
        aligned(p, stride, what);
    }
    // the output [2][level + 1 | level][N]: `same` (nullable) is the input it may coincide with when nothing is rescaled
    void output(const u64* out, long long so, bool rescale, const u64* same, long long s_same) const {
        LSA_REQUIRE(out != nullptr, who + ": out is null");
        const size_t wout = rescale ? 2 * (size_t)level * c.n : wct;
        LSA_REQUIRE(so >= (long long)wout, who + ": output stride below one result");
        aligned(out, so, "out");
        if (!same) return;
        if (rescale) LSA_REQUIRE(layout::apart(out, so, wout, same, s_same, wct, batch), who + ": out overlaps the ciphertexts (a rescaled result may not)");
        else LSA_REQUIRE((out == same && so == s_same) || layout::apart(out, so, wct, same, s_same, wct, batch), who + ": out must be ct or not overlap it");
    }
    void apart(const u64* out, long long so, bool rescale, const u64* p, long long sp, size_t words, const char* what) const {
        const size_t wout = rescale ? 2 * (size_t)level * c.n : wct;
        LSA_REQUIRE(layout::apart(out, so, wout, p, sp, words, batch), who + ": out overlaps " + what);
    }
};

// fn(dst, stride) writes the unrescaled result: into out, or into the second arena with ckks_rescale behind it
template <typename F>
void plain_finish(Context& c, int level, bool rescale, u64* out, long long so, int batch, hipStream_t s, F&& fn) {
    if (!rescale) {
        fn(out, so);
        return;
    }
    const long long st = 2LL * (level + 1) * c.n;
    u64* tmp = c.workspace2((size_t)st * batch, s);
    fn(tmp, st);
    ckks_rescale(c, level, 2, tmp, out, batch, st, so, s);
}

// The sign pattern of NTT(X^(N/2)), measured rather than assumed: the monomial goes through launch_ntt once per context, at every
// prime of the chain, and the host checks that each word is I_j = psi_j^(N/2) or q_j - I_j and that one bit of the index decides
// which -- the same bit, the same way round, at every limb.
const Context::CconstSelector& cconst_selector(Context& c, hipStream_t s) {
    if (c.cconst.bit >= 0) return c.cconst;
    const int nq = c.nq;
    const size_t N = (size_t)c.n;
    std::vector<u64> w((size_t)nq * N, 0);
    for (int j = 0; j < nq; j++) w[(size_t)j * N + N / 2] = 1;
    u64* d = c.workspace(w.size(), s);
    LSA_HIP(hipMemcpyAsync(d, w.data(), w.size() * sizeof(u64), hipMemcpyHostToDevice, s));
    launch_ntt(c, d, d, 1, (long long)w.size(), nq, rm_seq(nq), false, s);
    LSA_HIP(hipMemcpyAsync(w.data(), d, w.size() * sizeof(u64), hipMemcpyDeviceToHost, s));
    LSA_HIP(hipStreamSynchronize(s));
    auto internal = [](const std::string& m) { throw Error(LSA_ERR_INTERNAL, "complex constant: " + m); };
    std::vector<u64> I(nq);
    for (int j = 0; j < nq; j++) {
        I[j] = c.T.psi[((size_t)j * N + 1) * 2];   // psi^brv(1) = psi^(N/2)
        if (mul_mod_host(I[j], I[j], c.T.mod[j]) != c.T.mod[j] - 1) internal("psi^(N/2) is no square root of -1");
    }
    int pol = -1;
    if (w[0] == I[0]) pol = 0;
    else if (w[0] == c.T.mod[0] - I[0]) pol = 1;
    else internal("the transformed monomial holds a word that is not +-psi^(N/2)");
    for (int bit = 0; bit < c.logn; bit++) {
        bool ok = true;
        for (int j = 0; j < nq && ok; j++) {
            const u64 q = c.T.mod[j], plus = I[j], minus = q - I[j];
            const u64* row = w.data() + (size_t)j * N;
            for (size_t x = 0; x < N && ok; x++) ok = row[x] == ((int)((x >> bit) & 1) == pol ? plus : minus);
        }
        if (ok) {
            c.cconst.pol = pol;
            c.cconst.I = I;
            c.cconst.bit = bit;
            return c.cconst;
        }
    }
    internal("the sign of the transformed monomial is not a function of one index bit");
    return c.cconst;
}

struct Cplx64 {   // a complex constant as two rounded integers
    long long re = 0, im = 0;
};
Cplx64 cconst_round(double re, double im, double scale, const std::string& who) {
    LSA_REQUIRE(std::isfinite(re) && std::isfinite(im), who + ": constant not finite");
    LSA_REQUIRE(std::isfinite(scale) && scale > 0, who + ": scale must be positive");
    Cplx64 k;
    k.re = round_even(re * scale, who.c_str());
    k.im = round_even(im * scale, who.c_str());
    return k;
}

void cconst_run(Context& c, const PlainCall& pc, const Cplx64* alpha, const Cplx64* beta, const u64* ct, long long sct, u64* out,
                long long so, bool rescale, hipStream_t s) {
    LSA_REQUIRE(pc.L <= LSA_CCONST_MAX_LIMBS, pc.who + ": more than " + std::to_string(LSA_CCONST_MAX_LIMBS) + " limbs");
    const Context::CconstSelector& sel = cconst_selector(c, s);
    CconstLimb k[LSA_CCONST_MAX_LIMBS] = {};
    for (int j = 0; j < pc.L; j++) {
        const ModDev& m = c.T.mods[j];
        if (alpha) {
            const CconstPair p = cconst_pair(alpha->re, alpha->im, sel.I[j], m);
            k[j].k_plus = cconst_to_mont(p.plus, m);
            k[j].k_minus = cconst_to_mont(p.minus, m);
        }
        if (beta) {
            const CconstPair p = cconst_pair(beta->re, beta->im, sel.I[j], m);
            k[j].b_plus = p.plus;
            k[j].b_minus = p.minus;
        }
    }
    plain_finish(c, pc.level, rescale, out, so, pc.batch, s, [&](u64* dst, long long sd) {
        launch_cconst(c, alpha != nullptr, beta != nullptr, ct, sct, k, sel.bit, sel.pol, dst, sd, pc.L, pc.batch, s);
    });
}

}  // namespace

void ckks_mult_plain(Context& c, int level, const u64* ct, long long sct, const u64* pt, long long spt, u64* out, long long so,
                     int batch, bool rescale, hipStream_t s) {
    const PlainCall pc(c, "lsa_ckks_mult_plain", level, batch, rescale);
    if (batch <= 0) return;
    pc.ciphertext(ct, sct, "ct");
    pc.plaintext(pt, spt, "pt");
    pc.output(out, so, rescale, ct, sct);
    pc.apart(out, so, rescale, pt, spt, pc.wpt, "the plaintexts");
    plain_finish(c, level, rescale, out, so, batch, s, [&](u64* dst, long long sd) {
        launch_mac_plain(c, 1, &ct, &sct, &pt, &spt, nullptr, 0, dst, sd, batch, 2, pc.L, rm_seq(pc.L), s);
    });
}

void ckks_addsub_plain(Context& c, int op, int level, const u64* ct, long long sct, const u64* pt, long long spt, u64* out,
                       long long so, int batch, hipStream_t s) {
    const PlainCall pc(c, "lsa_ckks_addsub_plain", level, batch, false);
    LSA_REQUIRE(op == 0 || op == 1, pc.who + ": op must be 0 (add) or 1 (sub)");
    if (batch <= 0) return;
    pc.ciphertext(ct, sct, "ct");
    pc.plaintext(pt, spt, "pt");
    pc.output(out, so, false, ct, sct);
    pc.apart(out, so, false, pt, spt, pc.wpt, "the plaintexts");
    const int L = pc.L;
    launch_elementwise(c, op == 0 ? EW_ADD : EW_SUB, ct, pt, out, batch, sct, spt, so, L, rm_seq(L), s);
    if (out != ct) {   // c1 rides along
        std::vector<int> rows(L);
        for (int j = 0; j < L; j++) rows[j] = j;
        launch_copy_rows(c, ct + (size_t)L * c.n, sct, out + (size_t)L * c.n, so, L, rows.data(), batch, s);
    }
}

void ckks_mac_plain(Context& c, int level, int n, const u64* const* cts, const long long* scts, const u64* const* pts,
                    const long long* spts, const u64* addend, long long s_addend, u64* out, long long so, int batch, bool rescale,
                    hipStream_t s) {
    const PlainCall pc(c, "lsa_ckks_mac_plain", level, batch, rescale);
    LSA_REQUIRE(n >= 1, pc.who + ": needs at least one term");
    if (batch <= 0) return;
    LSA_REQUIRE(cts && scts && pts && spts, pc.who + ": null argument");
    pc.output(out, so, rescale, nullptr, 0);
    // out holds the running sum while later terms are read: it may alias none of them
    for (int i = 0; i < n; i++) {
        pc.ciphertext(cts[i], scts[i], "a ciphertext");
        pc.plaintext(pts[i], spts[i], "a plaintext");
        pc.apart(out, so, rescale, cts[i], scts[i], pc.wct, "a ciphertext");
        pc.apart(out, so, rescale, pts[i], spts[i], pc.wpt, "a plaintext");
    }
    if (addend) {
        pc.ciphertext(addend, s_addend, "the addend");
        pc.apart(out, so, rescale, addend, s_addend, pc.wct, "the addend");
    }
    plain_finish(c, level, rescale, out, so, batch, s, [&](u64* dst, long long sd) {
        for (int i0 = 0; i0 < n; i0 += LSA_MAC_MAX_TERMS) {   // later launches add to the sum so far
            const int m = std::min(LSA_MAC_MAX_TERMS, n - i0);
            launch_mac_plain(c, m, cts + i0, scts + i0, pts + i0, spts + i0, i0 ? dst : addend, i0 ? sd : s_addend, dst, sd, batch, 2,
                             pc.L, rm_seq(pc.L), s);
        }
    });
}

void ckks_mult_const(Context& c, int level, const u64* ct, long long sct, double re, double im, double const_scale, u64* out,
                     long long so, int batch, bool rescale, hipStream_t s) {
    const PlainCall pc(c, "lsa_ckks_mult_const", level, batch, rescale);
    const Cplx64 alpha = cconst_round(re, im, const_scale, pc.who);
    if (batch <= 0) return;
    pc.ciphertext(ct, sct, "ct");
    pc.output(out, so, rescale, ct, sct);
    cconst_run(c, pc, &alpha, nullptr, ct, sct, out, so, rescale, s);
}

void ckks_add_const(Context& c, int level, const u64* ct, long long sct, double re, double im, double ct_scale, u64* out,
                    long long so, int batch, hipStream_t s) {
    const PlainCall pc(c, "lsa_ckks_add_const", level, batch, false);
    const Cplx64 beta = cconst_round(re, im, ct_scale, pc.who);
    if (batch <= 0) return;
    pc.ciphertext(ct, sct, "ct");
    pc.output(out, so, false, ct, sct);
    cconst_run(c, pc, nullptr, &beta, ct, sct, out, so, false, s);
}

void ckks_affine_const(Context& c, int level, const u64* ct, long long sct, double re, double im, double const_scale, double add_re,
                       double add_im, double ct_scale, u64* out, long long so, int batch, bool rescale, hipStream_t s) {
    const PlainCall pc(c, "lsa_ckks_affine_const", level, batch, rescale);
    const Cplx64 alpha = cconst_round(re, im, const_scale, pc.who);
    LSA_REQUIRE(std::isfinite(ct_scale) && ct_scale > 0, pc.who + ": scale must be positive");
    const Cplx64 beta = cconst_round(add_re, add_im, ct_scale * const_scale, pc.who);   // the product's scale
    if (batch <= 0) return;
    pc.ciphertext(ct, sct, "ct");
    pc.output(out, so, rescale, ct, sct);
    cconst_run(c, pc, &alpha, &beta, ct, sct, out, so, rescale, s);
}

// ------------------------------------------------------------------------------------------------ CKKS slot sum
// out = sum_{i<count} rot(in, i*step) by the plan of slot_sum.h.  Per tile the steps run back to back: one decomposition of x's c1,
// the gadget products of the step's 1..4 keys written as rotated extended ciphertexts (launch_ks_mac with `scatter`: the words of
// ckks_rotate_ext) -- several keys in ONE k_ks_mac_multi launch, each into its own buffer, k_ext_sum joining them -- then
// x <- x + ModDown(NEXT sum) with x riding on the ModDown tail's base (base_polys = 2).  That store is index for index, so from
// the second step on x lives in `out` and is updated in place, and out == in is allowed.  The TAIL rotations gather in an extended
// accumulator that is divided once, after the last step.  All temporaries are the tile's workspace: the KsTile rows, up to three more
// extended ciphertexts for the keys of a multi-key launch beyond the first, and one for the tail.
SlotSumPlanHost slot_sum_plan_checked(int n_ring, long long step, int count, int radix) {
    try {
        return slot_sum_plan(n_ring, step, count, radix, LSA_SLOTSUM_DEFAULT_RADIX);
    } catch (const std::invalid_argument& e) {
        throw Error(LSA_ERR_ARG, e.what());
    }
}

SlotSum* slot_sum_create(Context& c, int level, long long step, int count, int radix) {
    LSA_REQUIRE(c.algo == LSA_ALGO_CKKS, "slot sum: context is not CKKS");
    LSA_REQUIRE(level >= 0 && level < c.nq, "slot sum: level out of range");
    auto p = std::make_unique<SlotSum>(c, level);
    p->plan = slot_sum_plan_checked(c.n, step, count, radix);
    LSA_REQUIRE(p->plan.steps.empty() || c.np >= 1, "slot sum: key switching needs at least one special prime");
    return p.release();
}

// What both slot-sum runners do before their tiles.  Every key of `elements` (the plan's, in the order a missing one is reported)
// is looked up and checked before anything is queued; then the operands; a plan without steps (count == 1, no row fold) is a
// copy; last the rotations' tables, element by element (table look-ups upload on first use: only after every argument is
// accepted): the NTT-domain scatter and, for the BFV gathering tail, the coefficient-domain permutation.
// run == false: nothing is left to do.
struct SlotSumCall {
    bool run = false;
    GaloisKeys key_of;   // the plan's keys alone, all present
    std::map<u64, const u32*> scatter_of, perm_of;
};
static SlotSumCall slot_sum_prologue(Context& c, const EntryCheck& ck, const SlotSumPlanHost& plan, const std::vector<u64>& elements,
                                     const GaloisKeys& glk, const u64* in, long long sin, u64* out, long long sout, int batch,
                                     bool gather, hipStream_t s) {
    SlotSumCall call;
    const std::vector<const Key*> keys = glk.resolve(elements, ck.who, [&](u64, const Key& k) { ck.key(k, "a Galois key"); });
    for (size_t i = 0; i < elements.size(); i++) call.key_of.insert(elements[i], keys[i]);
    if (batch <= 0) return call;
    const int L = ck.level + 1;
    const size_t w = 2 * (size_t)L * c.n;
    const Span sp_in = ck.operand(in, sin, w, "in", false), sp_out = ck.output(out, sout, w);
    ck.same_or_apart(sp_out, sp_in, "in");
    if (plan.steps.empty()) {
        if (layout::same(sp_out, sp_in)) return call;
        std::vector<int> rows(2 * L);
        for (int i = 0; i < 2 * L; i++) rows[i] = i;
        launch_copy_rows(c, in, sin, out, sout, 2 * L, rows.data(), batch, s);
        return call;
    }
    LSA_REQUIRE(!gather || c.logn <= LSA_PERM_LDS_MAX_LOGN, ck.who + ": the gathering tail needs N <= 2^14");
    for (u64 e : elements) {
        call.scatter_of[e] = inverse_perm(c, e);
        if (gather) call.perm_of[e] = c.coeff_perm(e);
    }
    call.run = true;
    return call;
}

void slot_sum_run(SlotSum& p, const u64* in, long long sin, u64* out, long long sout, int batch,
                  const GaloisKeys& glk, hipStream_t s) {
    Context& c = p.c;
    const int level = p.level;
    const EntryCheck ck(c, "lsa_ckks_slot_sum", LSA_ALGO_CKKS, level, 0, batch);
    std::vector<u64> by_rotation;   // a missing key is reported in the order of the plan's rotations
    for (int r : p.plan.rotations) by_rotation.push_back(galois_of_rotation(r, c.n));
    const SlotSumCall call = slot_sum_prologue(c, ck, p.plan, by_rotation, glk, in, sin, out, sout, batch, false, s);
    if (!call.run) return;
    const auto& key_of = call.key_of;
    const auto& scatter_of = call.scatter_of;
    const long long N = c.n;
    const int L = level + 1, T = L + c.np;
    const size_t ks_rows = KsTile::rows(c, level);
    const bool multi = p.multi_mac;
    // extended buffers beyond KsTile's acc: one per key of a multi-key launch that is neither the first NEXT key nor the first
    // TAIL key of the plan (the most any step needs), and the tail accumulator
    int n_more = 0;
    {
        bool live = false;
        for (const SlotSumStep& step : p.plan.steps) {
            int more = 0, next = 0;
            for (const SlotSumKey& k : step.keys) more += k.tail ? (live ? 1 : 0) : (next++ ? 1 : 0);
            for (const SlotSumKey& k : step.keys) live = live || k.tail;
            if (multi && step.keys.size() >= 2) n_more = std::max(n_more, more);
        }
    }
    const int n_extra = n_more + (p.plan.has_tail ? 1 : 0);
    for_tiles(c, ks_rows + (size_t)n_extra * 2 * T, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        KsTile t(c, level, nb, ws, st);
        const long long s_ext2 = t.s_acc;   // [2][T][N] per batch item, like t.acc
        u64* extra[LSA_SLOTSUM_MAX_KEYS];
        for (int i = 0; i < n_extra; i++) extra[i] = ws + (ks_rows * tb + (size_t)i * 2 * T * tb) * N;
        u64* tail = p.plan.has_tail ? extra[n_more] : nullptr;
        const u64* x = in + (size_t)b0 * sin;
        long long sx = sin;
        u64* o = out + (size_t)b0 * sout;
        bool tail_live = false;
        for (const SlotSumStep& step : p.plan.steps) {
            const u64* cx = x + (long long)L * N;
            t.decompose(cx, sx);
            const int nk = (int)step.keys.size();
            const bool one_launch = multi && nk >= 2;
            KsMacMultiKey mk[LSA_SLOTSUM_MAX_KEYS];
            bool add_to[LSA_SLOTSUM_MAX_KEYS];   // sequential form: the key's product is added to its destination
            const u64* next_more[LSA_SLOTSUM_MAX_KEYS];
            const u64* tail_more = nullptr;
            int n_next = 0, n_sum = 0, used = 0;
            for (int i = 0; i < nk; i++) {
                const SlotSumKey& k = step.keys[i];
                u64* dst;
                if (k.tail) {
                    add_to[i] = tail_live;
                    dst = !tail_live || !one_launch ? tail : extra[used++];
                    if (dst != tail) tail_more = dst;
                } else {
                    add_to[i] = n_next > 0;
                    dst = n_next == 0 || !one_launch ? t.acc : extra[used++];
                    if (dst != t.acc) next_more[n_sum++] = dst;
                    n_next++;
                }
                mk[i] = {key_of.at(k.g), scatter_of.at(k.g), dst};
            }
            if (one_launch) {
                launch_ks_mac_multi(c, level, cx, sx, t.ext, t.s_ext, nk, mk, s_ext2, x, sx, nb, st);
                if (n_sum) launch_ext_sum(c, level, n_sum, next_more, s_ext2, t.acc, s_ext2, true, nb, st);
                if (tail_more) launch_ext_sum(c, level, 1, &tail_more, s_ext2, tail, s_ext2, true, nb, st);
            } else {
                for (int i = 0; i < nk; i++)
                    launch_ks_mac(c, level, cx, sx, t.ext, t.s_ext, *mk[i].key, mk[i].out, s_ext2, nb, st, false, mk[i].scatter, x, sx, nullptr,
                                  add_to[i]);
            }
            for (int i = 0; i < nk; i++) tail_live = tail_live || step.keys[i].tail;
            t.moddown({.p = o, .sp = sout, .base = x, .sbase = sx, .base_rpp = L, .base_polys = 2});
            x = o;
            sx = sout;
        }
        if (tail_live) ks_moddown(c, level, tail, s_ext2, t.conv, {.p = o, .sp = sout, .base = x, .sbase = sx, .base_rpp = L, .base_polys = 2}, nb, st);
    });
}

// ------------------------------------------------------------------------------------------------ BFV slot sum
// out = sum_{i<count} rot_cols(y, i*step), y = in + rot_rows(in) if rows, by the plan of slot_sum.h on coefficient-domain
// ciphertexts.  Per tile and step, as bfv_rotate_many: c1 of x into the NTT domain once (the MAC's own-digit operand), the
// decomposition from the coefficients, one launch_ks_mac per key with the rotation's NTT-domain scatter -- the first NEXT key
// writes the tile's acc, later ones add to it, the TAIL key writes or adds to the extended tail accumulator -- then the
// coefficient-domain ModDown of the NEXT sum.  gather: the MACs add no P * c0; the tail (k_bfv_slot_tail) adds x and the rotated
// c0 terms, gathered from the c0 row in LDS, and collects the TAIL rotation's c0 term in tail_c0 [L][N]; after the last step
// out = x + (tail_c0, 0) + ModDown(tail).  plain: c0 is transformed too and enters the MACs as `base` (the CKKS form), the tails are
// launch_moddown_final with base = x.  ModDown(P z + a) = z + ModDown(a) residue for residue, so both give the same words.  x
// lives in `out` from the second step on and is updated in place.
SlotSumPlanHost bfv_slot_sum_plan_checked(int n_ring, long long step, int count, int radix, int rows) {
    try {
        return bfv_slot_sum_plan(n_ring, step, count, radix, rows, LSA_BFV_SLOTSUM_DEFAULT_RADIX);
    } catch (const std::invalid_argument& e) {
        throw Error(LSA_ERR_ARG, e.what());
    }
}

BfvSlotSum* bfv_slot_sum_create(Context& c, int level, long long step, int count, int radix, int rows) {
    LSA_REQUIRE(c.algo == LSA_ALGO_BFV, "lsa_bfv_slot_sum_create: context is not BFV");
    LSA_REQUIRE(level >= 0 && level < c.nq, "lsa_bfv_slot_sum_create: level out of range (0.." + std::to_string(c.nq - 1) + ")");
    auto p = std::make_unique<BfvSlotSum>(c, level);
    p->plan = bfv_slot_sum_plan_checked(c.n, step, count, radix, rows);
    LSA_REQUIRE(p->plan.steps.empty() || c.np >= 1, "lsa_bfv_slot_sum_create: key switching needs at least one special prime");
    return p.release();
}

void bfv_slot_sum_run(BfvSlotSum& p, const u64* in, long long sin, u64* out, long long sout, int batch,
                      const GaloisKeys& glk, hipStream_t s) {
    Context& c = p.c;
    const int level = p.level;
    const EntryCheck ck(c, "lsa_bfv_slot_sum", LSA_ALGO_BFV, level, 0, batch);
    const bool gather = p.gather;
    const SlotSumCall call = slot_sum_prologue(c, ck, p.plan, p.plan.galois, glk, in, sin, out, sout, batch, gather, s);
    if (!call.run) return;
    const auto& key_of = call.key_of;
    const auto& scatter_of = call.scatter_of;
    const auto& perm_of = call.perm_of;
    const long long N = c.n;
    const int L = level + 1, T = L + c.np;
    const bool has_tail = p.plan.has_tail;
    const size_t ks_rows = KsTile::rows(c, level);
    // per batch item: NTT(c1) | the KsTile rows | the extended tail accumulator | tail_c0 (gather) or NTT(c0) (plain)
    const size_t r_tail = has_tail ? 2 * (size_t)T : 0, r_last = gather ? (has_tail ? (size_t)L : 0) : (size_t)L;
    const long long sL = (long long)L * N;
    for_tiles(c, (size_t)L + ks_rows + r_tail + r_last, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* cxn = ws;
        u64* ks_ws = cxn + (size_t)L * N * tb;
        u64* tail = ks_ws + ks_rows * N * tb;
        u64* last = tail + r_tail * N * tb;   // tail_c0 or NTT(c0)
        KsTile t(c, level, nb, ks_ws, st);
        const long long s_ext2 = t.s_acc;   // [2][T][N] per batch item, like t.acc
        const u64* x = in + (size_t)b0 * sin;
        long long sx = sin;
        u64* o = out + (size_t)b0 * sout;
        bool tail_live = false;
        for (const SlotSumStep& step : p.plan.steps) {
            const u64* c1 = x + sL;
            launch_ntt(c, c1, cxn, nb, sx, sL, L, rm_seq(L), false, st);
            if (!gather) launch_ntt(c, x, last, nb, sx, sL, L, rm_seq(L), false, st);
            t.decompose(cxn, sL, c1, sx);
            BfvSlotTail bt;
            bool next_live = false;
            for (const SlotSumKey& k : step.keys) {
                const bool add_to = k.tail ? tail_live : next_live;
                launch_ks_mac(c, level, cxn, sL, t.ext, t.s_ext, *key_of.at(k.g), k.tail ? tail : t.acc, s_ext2, nb, st, false,
                              scatter_of.at(k.g), gather ? nullptr : last, sL, nullptr, add_to);
                if (k.tail) {
                    if (gather) {
                        bt.tail = perm_of.at(k.g);
                        bt.tail_c0 = last;
                        bt.s_tail = sL;
                        bt.tail_accumulate = tail_live;
                    }
                    tail_live = true;
                } else {
                    if (gather) bt.next[bt.n_next++] = perm_of.at(k.g);
                    next_live = true;
                }
            }
            t.moddown({.p = o, .sp = sout, .base = x, .sbase = sx, .base_rpp = L, .base_polys = 2, .form = KsOut::COEFF,
                       .slot_tail = gather ? &bt : nullptr});
            x = o;
            sx = sout;
        }
        if (tail_live) {
            BfvSlotTail bt;
            bt.addend = last;
            bt.s_addend = sL;
            ks_moddown(c, level, tail, s_ext2, t.conv,
                       {.p = o, .sp = sout, .base = x, .sbase = sx, .base_rpp = L, .base_polys = 2, .form = KsOut::COEFF,
                        .slot_tail = gather ? &bt : nullptr},
                       nb, st);
        }
    });
}

}  // namespace lsa
