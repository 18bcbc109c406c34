// key_switch.hip — the key switch (key_switch.h): the tile's decomposition, key MACs and ModDown, the rescale, the rotations'
// index maps and the tiling, built from the kernels in kernels.hip.  Algorithms follow the CPU path the results must agree with
// (Lattigo v4, restated in oracle/ls_oracle.c).
#include "key_switch.h"

namespace lsa {

RowMap rm_seq(int count, int first) {
    RowMap r;
    LSA_REQUIRE(count >= 1 && count <= LSA_MAX_PERIOD, "row map too long");
    r.period = count;
    for (int i = 0; i < count; i++) r.mod_of[i] = (unsigned char)(first + i);
    return r;
}

// ------------------------------------------------------------------------------------------------ key switch
// step 5, the division by P of a polynomial pair over Q_level u P (acc: [2][L+k][N] per batch item, NTT domain; its P rows --
// and, for the merged rescale, its last Q row -- are transformed in place), conv: 2L rows of scratch per batch item
// Its head, ks_moddown_head -- the inverse transforms and the conversion -- is the same for every output.  The merged rescale goes
// on with ks_rescale_head: t, then the fusion of the one forward transform of in_j that finishes it, which ks_moddown launches
// whole and KsTile::mac_rescale pass by pass around the key MAC's tail variant.
// The merged rescale with its head formed inside the conversion (Context::rescale_head_in_conv, lsa_set_rescale_head_in_conv):
// the conversion reads INTT(acc_l) (and INTT(base_l)), keeps t in registers and stores in_j = conv_j * P^-1 + lift_j(t) at
// conv[h][j], j != l (k_baseconv<.., HEAD>).  No k_sub_mul, conv_l and t are never written, and the forward transform of in_j
// starts with the plain first pass.  Same residues as the earlier sequence, which mode 0 (and mode 1 below N = 2^16) keeps.
static bool ks_head_in_conv(const Context& c, int level, const KsOut& o) {
    return o.form == KsOut::RESCALE && c.fuse_tails && level >= 1 && c.np <= LSA_BC_NARROW_SRC &&
           (c.rescale_head_in_conv == 2 || (c.rescale_head_in_conv == 1 && c.logn >= 16));
}
// the last limbs of base out of the NTT domain, in place.  base is the caller's scratch here (the tensor output): nothing reads
// these rows in NTT form afterwards.
static void ks_base_last_intt(Context& c, int level, const KsOut& o, int nb, hipStream_t s) {
    if (!o.base) return;
    u64* base_rw = const_cast<u64*>(o.base);
    RowMap rb;
    rb.period = 1;
    rb.mod_of[0] = (unsigned char)level;
    rb.row0 = level;
    rb.row_step = o.base_rpp;
    launch_ntt(c, base_rw, base_rw, nb, o.sbase, o.sbase, 2, rb, true, s);
}

static void ks_moddown_head(Context& c, int level, u64* acc, long long s_acc, u64* conv, const KsOut& o, int nb, hipStream_t s) {
    LSA_REQUIRE(!o.scatter || (c.fuse_tails && o.form == KsOut::NTT), "scattered ModDown store: fused tails, NTT-domain output");
    LSA_REQUIRE(!o.rmac || o.scatter, "rotate-and-MAC tail: needs the rotation's index map");
    LSA_REQUIRE(!o.tail || (o.form == KsOut::COEFF &&
                            (o.tail->base_polys < 0 || (o.base && o.base_polys == o.tail->base_polys && o.base_rpp == level + 1))),
                "ModDown tail hook: coefficient-domain output onto the base the tail states");
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
        const bool in_conv = ks_head_in_conv(c, level, o);
        const BaseConvPlan* k = c.baseconv(src, dst, true, rs, nullptr, in_conv);
        if (in_conv) {
            // (the plan's last target is l = level, unscaled: the row the head needs)
            ks_base_last_intt(c, level, o, nb, s);   // before the conversion reads INTT(base_l)
            for (int h = 0; h < 2; h++) {
                const BaseConvHead hd{acc + ((size_t)h * T + level) * N, s_acc,
                                      o.base && h < o.base_polys ? o.base + ((size_t)h * o.base_rpp + level) * N : nullptr, o.sbase,
                                      c.pinv_vec(level) + level};
                launch_baseconv(c, k, rows, acc + (size_t)h * T * N, conv + (size_t)h * L * N, nb, s_acc, s_conv, s, nullptr, 0, nullptr, &hd);
            }
            return;
        }
        for (int h = 0; h < 2; h++)
            launch_baseconv(c, k, rows, acc + (size_t)h * T * N, conv + (size_t)h * L * N, nb, s_acc, s_conv, s);
    }
}

static NttFusion ks_rescale_head(Context& c, int level, u64* acc, long long s_acc, u64* conv, const KsOut& o, int nb, hipStream_t s,
                                 RowMap& rmo);

static void ks_moddown(Context& c, int level, u64* acc, long long s_acc, u64* conv, const KsOut& o, int nb, hipStream_t s) {
    const bool coeff_out = o.form == KsOut::COEFF, rs = o.form == KsOut::RESCALE;
    const long long N = c.n;
    const int L = level + 1, T = L + c.np;
    const long long s_conv = 2LL * L * N;
    ks_moddown_head(c, level, acc, s_acc, conv, o, nb, s);
    if (coeff_out) {
        if (o.tail)
            o.tail->launch(c, level, acc, s_acc, T, conv, s_conv, o, nb, s);
        else
            launch_moddown_final(c, level, acc, s_acc, T, conv, s_conv, o.base, o.sbase, o.base_rpp, o.base_polys, o.p, o.sp, nb, s);
        return;
    }
    if (rs) {
        RowMap rmo;
        const NttFusion fb = ks_rescale_head(c, level, acc, s_acc, conv, o, nb, s, rmo);
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

// the merged rescale after the head: t into the last limbs of o.p, then the row map (rmo) and the fusion of the forward transform of
// in_j over every other limb (prologue: in_j = conv_j * P^-1 + lift_j(t); epilogue: out_j).  With the head formed inside the
// conversion (ks_head_in_conv) conv already holds in_j: no t, no prologue, the epilogue alone.
static NttFusion ks_rescale_head(Context& c, int level, u64* acc, long long s_acc, u64* conv, const KsOut& o, int nb, hipStream_t s,
                                 RowMap& rmo) {
    const long long N = c.n;
    const int L = level + 1, T = L + c.np;
    const long long s_conv = 2LL * L * N;
    // base_polys == 0: the tensor fold -- P * base is already in acc's Q rows (TensorFold), so INTT(acc_l) * P^-1 carries
    // INTT(base_l) and the tails below run without base
    const int l = level;
    // t[h] = (INTT(acc[h][l]) - conv[h][l]) * P^-1 + INTT(base[h][l]) -> p[h][l].  base is the caller's scratch here
    // (the tensor output): its last limbs are transformed in place, nothing reads them in NTT form afterwards.
    const bool in_conv = ks_head_in_conv(c, level, o);
    if (!in_conv) {
        ks_base_last_intt(c, level, o, nb, s);
        const unsigned char lm[1] = {(unsigned char)l};
        launch_sub_mul_general(c, 2, 1, lm, c.pinv_vec(level) + l, acc + (long long)l * N, s_acc, T, conv + (long long)l * N,
                               s_conv, L, o.base ? o.base + (long long)l * N : nullptr, o.sbase, o.base_rpp, o.base_polys,
                               o.p + (long long)l * N, o.sp, L, nb, s);
    }
    // every other limb: in = conv_j*P^-1 + lift_j(t), out = (acc_j*P^-1 - NTT(in) + base_j) * q_l^-1
    rmo.period = 2 * L;
    for (int h = 0; h < 2; h++)
        for (int j = 0; j < L; j++) rmo.mod_of[h * L + j] = j == l ? LSA_ROW_SKIP : (unsigned char)j;
    NttFusion fb;
    fb.pro = in_conv ? 0 : 2;
    fb.epi = 2;
    fb.limbs = L;
    fb.ql_mod = l;
    fb.last = in_conv ? nullptr : o.p + (long long)l * N;
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
    return fb;
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

size_t KsTile::rows(const Context& c, int level, KsSource::Form form) {
    LSA_REQUIRE(c.np >= 1, "key switching needs at least one special prime");
    const int L = level + 1, T = L + c.np, beta = ceil_div(L, c.np);
    return (form == KsSource::COEFF ? (size_t)L : 0) + (size_t)L + (size_t)beta * T + 2 * (size_t)T + 2 * (size_t)L;
}

KsTile::KsTile(Context& c_, int level_, int nb_, u64* ws, hipStream_t s_, const Key* single_key, KsSource::Form form, int tb)
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
    cxn = form == KsSource::COEFF ? ws : nullptr;
    cxi = cxn ? ws + (size_t)(tb ? tb : nb) * s_cxi : ws;
    ext = cxi + (size_t)nb * s_cxi;
    acc = ext + (size_t)nb * s_ext;
    conv = acc + (size_t)nb * s_acc;
}

void KsTile::decompose(const KsSource& source) {
    LSA_REQUIRE((source.form == KsSource::COEFF) == (cxn != nullptr), "key switch: the tile was laid out for another form of source");
    src = source;
    const long long N = c.n;
    const int np = c.np;
    if (src.form == KsSource::COEFF) {   // the MAC's own-digit operand, into the tile's own rows
        launch_ntt(c, src.coef, cxn, nb, src.s_coef, s_cxi, L, rm_seq(L), false, s);
        src.ntt = cxn;
        src.s_ntt = s_cxi;
    } else if (src.form == KsSource::PRODUCT) {   // (the MAC takes the own digit from a and b: its cx is not read)
        src.ntt = cxi;
        src.s_ntt = s_cxi;
    }
    const u64* cx_coef = src.coef;
    // 1. cx out of the NTT domain
    if (src.prod) {
        LSA_REQUIRE(!cx_coef, "key switch: a product source has no coefficient-domain copy");
        const TensorFold* prod = src.prod;
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
        launch_ntt(c, src.ntt, cxi, nb, src.s_ntt, s_cxi, L, rm_seq(L), true, s);
    }
    const u64* conv_src = cx_coef ? cx_coef : cxi;
    const long long s_src = cx_coef ? src.s_coef : s_cxi;
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
        std::vector<int> from, dst;
        BaseConvRows rows{};
        for (int i = d0; i < d1; i++) {
            rows.src_row[i - d0] = i;
            from.push_back(i);
        }
        for (int tl = 0; tl < T; tl++) {
            if (tl >= d0 && tl < d1) continue;
            rows.dst_row[dst.size()] = d * T + tl;
            dst.push_back(c.qp_mod(L, tl));
        }
        launch_baseconv(c, c.baseconv(from, dst, false), rows, conv_src, ext, nb, s_src, s_ext, s);
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
            const bool in_mac = ks_fused_limb(c, L, i % T) && !(tail && i % T == level);   // (tail: limb l goes to the stand-alone MAC)
            rm.mod_of[i] = own(i / T, i % T) || in_mac ? LSA_ROW_SKIP : (unsigned char)c.qp_mod(L, i % T);
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

void KsTile::mac(const Key& k) {
    LSA_REQUIRE(src.ntt, "key MAC: decompose() has not run on this tile");
    const TensorFold* fold = src.prod;
    if (!fused) {
        launch_ks_mac(c, level, src.ntt, src.s_ntt, ext, s_ext, k, {acc, s_acc}, nb, s, false, fold);
        return;
    }
    LSA_REQUIRE(&k == key && !tail, "fused key MAC: the tile was planned for another key or for mac_rescale()");
    LSA_REQUIRE(launch_ntt_ksmac(c, level, src.ntt, src.s_ntt, ext, s_ext, k, acc, s_acc, nb, s, fold), "fused key MAC: shape not covered");
    launch_ks_mac(c, level, src.ntt, src.s_ntt, ext, s_ext, k, {acc, s_acc}, nb, s, true, fold);
}

void KsTile::mac_ext(const Key& k, const KsMacDst& dst) {
    LSA_REQUIRE(src.ntt && !fused && dst.scatter, "extended key MAC: a decomposed, unfused tile and the rotation's index map");
    launch_ks_mac(c, level, src.ntt, src.s_ntt, ext, s_ext, k, dst, nb, s);
}

void KsTile::mac_ext_multi(int n_keys, const KsMacMultiKey* keys, long long sout, const u64* base, long long sbase) {
    LSA_REQUIRE(src.ntt && !fused, "extended key MAC: a decomposed, unfused tile");
    launch_ks_mac_multi(c, level, src.ntt, src.s_ntt, ext, s_ext, n_keys, keys, sout, base, sbase, nb, s);
}

void KsTile::moddown_of(u64* ext_acc, long long s_ext_acc, const KsOut& o) { ks_moddown(c, level, ext_acc, s_ext_acc, conv, o, nb, s); }

void KsTile::moddown_ext(Context& c, int level, u64* ext_acc, long long s_ext_acc, u64* conv, const KsOut& o, int nb, hipStream_t s) {
    ks_moddown(c, level, ext_acc, s_ext_acc, conv, o, nb, s);
}

bool KsTile::plan_tail(const KsOut& o) {
    const int mu = c.plan.pass[1].mu;   // (fused: a two-pass plan)
    tail = fused && c.ks_tail_in_mac != 0 && c.fuse_tails && level >= 1 && o.form == KsOut::RESCALE && !o.base && o.base_polys == 0 &&
           ks_fused_engines(c) == 2 && (mu == 8 || (mu == 7 && c.ks_tail_in_mac == 2));
    if (!tail) return false;
    tail = false;
    for (int j = 0; j < level; j++) tail |= ks_fused_limb(c, L, j);   // (a tile whose only FP64-engine Q limb is l has nothing to gain)
    return tail;
}

void KsTile::mac_rescale(const Key& k, const KsOut& o) {
    LSA_REQUIRE(src.ntt && fused && tail && &k == key, "tail in the key MAC: a decomposed tile planned for it and for this key");
    LSA_REQUIRE(o.form == KsOut::RESCALE && !o.base && o.base_polys == 0, "tail in the key MAC: a merged rescale without base");
    const TensorFold* fold = src.prod;
    // 2. the accumulator rows that ModDown's head reads
    LSA_REQUIRE(launch_ntt_ksmac(c, level, src.ntt, src.s_ntt, ext, s_ext, k, acc, s_acc, nb, s, fold, KS_FUSED_P), "fused key MAC: shape not covered");
    launch_ks_mac(c, level, src.ntt, src.s_ntt, ext, s_ext, k, {acc, s_acc}, nb, s, true, fold, level);
    // 3. the head
    ks_moddown_head(c, level, acc, s_acc, conv, o, nb, s);
    RowMap rmo;
    const NttFusion fb = ks_rescale_head(c, level, acc, s_acc, conv, o, nb, s, rmo);
    // 4. the first pass with the prologue alone (the prologue belongs to the first executed pass, the epilogue to the pass that
    //    stores final values: each transform launch here carries only the one its pass runs)
    //    (head formed inside the conversion: conv holds in_j, the plain first pass)
    NttFusion fp = fb;
    fp.epi = 0;
    launch_ntt(c, conv, conv, nb, s_conv, s_conv, 2 * L, rmo, false, s, fb.pro ? &fp : nullptr, 1);
    // 5. the digits and the tail of the FP64-engine Q limbs
    const KsTailOperands kt{conv, s_conv, o.rs.out, o.rs.sout};
    LSA_REQUIRE(launch_ntt_ksmac(c, level, src.ntt, src.s_ntt, ext, s_ext, k, acc, s_acc, nb, s, fold, KS_FUSED_Q_TAIL, &kt),
                "fused key MAC: tail shape not covered");
    // 6. the integer-engine limbs: the second pass alone with the epilogue, every FP64-engine row skipped
    for (int i = 0; i < 2 * L; i++)
        if (rmo.mod_of[i] != LSA_ROW_SKIP && c.fp_engine(rmo.mod_of[i])) rmo.mod_of[i] = LSA_ROW_SKIP;
    NttFusion fe = fb;
    fe.pro = 0;
    fe.last = nullptr;
    launch_ntt(c, conv, conv, nb, s_conv, s_conv, 2 * L, rmo, false, s, &fe, 2);
}

void key_switch(Context& c, int level, const KsSource& src, const Key& key, const KsOut& o, int nb, u64* ws, hipStream_t s) {
    KsTile t(c, level, nb, ws, s, &key, src.form);
    const bool tail = t.plan_tail(o);
    t.decompose(src);
    if (tail) {
        t.mac_rescale(key, o);
        return;
    }
    t.mac(key);
    t.moddown(o);
}

void external_product(Context& c, int level, const u64* ct, long long sct, const Key& r0, const Key& r1, const KsOut& o, int nb, u64* ws,
                      hipStream_t s) {
    if (nb <= 0) return;
    LSA_REQUIRE(o.form == KsOut::COEFF && !o.tail, "external product: a plain coefficient-domain output");
    const long long N = c.n;
    const int L = level + 1, T = L + c.np;
    const long long sL = (long long)L * N, s_acc = 2LL * T * N;
    const u64 *cx0, *cx1, *ext0, *ext1;
    long long scx, sext;
    u64 *acc, *conv;
    if (sct == 2 * sL) {   // polynomial h of item b is row 2b + h of one decomposition
        KsTile t(c, level, 2 * nb, ws, s, nullptr, KsSource::COEFF);
        t.decompose(KsSource::of_coeff(ct, sL));
        cx0 = t.src.ntt, cx1 = cx0 + t.s_cxi, scx = 2 * t.s_cxi;
        ext0 = t.ext, ext1 = t.ext + t.s_ext, sext = 2 * t.s_ext;
        acc = t.acc, conv = t.conv;   // (laid out for 2 * nb items: nb fit)
    } else {
        KsTile t0(c, level, nb, ws, s, nullptr, KsSource::COEFF);
        KsTile t1(c, level, nb, ws + KsTile::rows(c, level, KsSource::COEFF) * (size_t)N * nb, s, nullptr, KsSource::COEFF);
        t0.decompose(KsSource::of_coeff(ct, sct));
        t1.decompose(KsSource::of_coeff(ct + sL, sct));
        cx0 = t0.src.ntt, cx1 = t1.src.ntt, scx = t0.s_cxi;
        ext0 = t0.ext, ext1 = t1.ext, sext = t0.s_ext;
        acc = t0.acc, conv = t0.conv;
    }
    if (c.rgsw_pair_mac) {
        launch_ks_mac_pair(c, level, cx0, cx1, scx, ext0, ext1, sext, r0, r1, acc, s_acc, nb, s);
    } else {
        const u32* id = c.ntt_perm(1);   // the identity: the extended output as the plain accumulator
        launch_ks_mac(c, level, cx0, scx, ext0, sext, r0, {acc, s_acc, id}, nb, s);
        launch_ks_mac(c, level, cx1, scx, ext1, sext, r1, {acc, s_acc, id, nullptr, 0, true}, nb, s);
    }
    ks_moddown(c, level, acc, s_acc, conv, o, nb, s);
}

const u32* inverse_perm(Context& c, u64 g) {
    const u64 mask = 2 * (u64)c.n - 1;
    u64 inv = g;   // Newton iteration for the inverse modulo a power of two: doubles the correct low bits each step
    for (int i = 0; i < 6; i++) inv = (inv * (2 - g * inv)) & mask;
    LSA_REQUIRE(((inv * g) & mask) == 1, "Galois element without an inverse");
    return c.ntt_perm(inv);
}
const u32* rotation_scatter(Context& c, u64 g) {
    return sw::rot_scatter() && c.fuse_tails ? inverse_perm(c, g) : nullptr;
}

// ------------------------------------------------------------------------------------------------ rescale
void rescale(Context& c, int level, int polys, const u64* in, long long sin, u64* out, long long sout, int nb,
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
int pick_tile(const Context& c, size_t rows_per_ct, int batch) {
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

}  // namespace lsa
