// ops.hip — operator pipelines: the HEArithmeticOperator surface the reference's executors call
// (mega_ag_runners/gpu/mega_ag_executors_gpu.cu:71-426), built from the kernels in kernels.hip.
//
// Algorithms follow the CPU path the results must agree with (Lattigo v4, restated in oracle/ls_oracle.c):
//   key-switch  = key_switch.h: the tile (decomposition, key MACs, ModDown), the rescale and the tiling of a batch
//   CKKS rescale = divide-and-round by the last prime (DivRoundByLastModulusNTT)
//   rotate      = key-switch c1, add c0, then apply the automorphism (Evaluator.Automorphism)
//   BFV mult    = centred extension Q->QMul, tensor in Q u QMul, round(./Q), centred return to Q, times t
// The argument checks of the first-generation entry points are entry_check.h's; the slot sums' runners live in slot_sum.hip.
#include "entry_check.h"
#include "key_switch.h"
#include "linear_transform.h"
#include "plain_ops.h"
#include "tensor_sum.h"

namespace lsa {
namespace {
using layout::Span;
}

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
        key_switch(c, level, KsSource::of_ntt(d + 2LL * L * N, sd), rlk, ks_onto_ct(out + (size_t)b0 * so, so, d, sd, L), nb, ws, st);
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
            key_switch(c, level, KsSource::of_ntt(ct + (long long)L * N, sin), glk,
                       ks_onto_c0(out + (size_t)b0 * sout, sout, ct, sin, L, {.scatter = scatter}), nb, ws, st);
        });
        return;
    }
    const u32* perm = c.ntt_perm(g);
    for_tiles(c, ks_rows + 2 * (size_t)L, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* p = ws + ks_rows * N * tb;
        const u64* ct = in + (size_t)b0 * sin;
        key_switch(c, level, KsSource::of_ntt(ct + (long long)L * N, sin), glk, ks_onto_c0(p, sp, ct, sin, L), nb, ws, st);
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
    std::vector<const u32*> perms(n_rot), scatters(n_rot);
    for (int i = 0; i < n_rot; i++) {
        LSA_REQUIRE(glk[i] != nullptr, ck.who + ": a Galois key is null");
        ck.key(*glk[i], "a Galois key");
    }
    const int in_place = ck.rotate_many_outputs(sp_in, outs, n_rot, sout, 2 * (size_t)L * N);
    std::vector<int> order;   // the output that IS the input goes last: every other rotation still reads the intact ciphertext
    for (int i = 0; i < n_rot; i++)
        if (i != in_place) order.push_back(i);
    if (in_place >= 0) order.push_back(in_place);
    for (int i = 0; i < n_rot; i++) {   // (table look-ups upload on first use: only after every argument is accepted)
        scatters[i] = i != in_place ? rotation_scatter(c, g[i]) : nullptr;
        perms[i] = scatters[i] ? nullptr : c.ntt_perm(g[i]);
    }
    for_tiles(c, ks_rows + 2 * (size_t)L, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* p = ws + ks_rows * N * tb;
        const u64* ct = in + (size_t)b0 * sin;
        KsTile t(c, level, nb, ws, st);
        t.decompose(KsSource::of_ntt(ct + (long long)L * N, sin));
        for (int i : order) {
            t.mac(*glk[i]);
            if (scatters[i]) {   // the permutation rides on the ModDown tail's store
                t.moddown(ks_onto_c0(outs[i] + (size_t)b0 * sout, sout, ct, sin, L, {.scatter = scatters[i]}));
                continue;
            }
            t.moddown(ks_onto_c0(p, sp, ct, sin, L));
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
        const u64* c1 = ct + (long long)L * N;
        t.decompose(c1_coef ? KsSource::of_both(c1, sin, c1_coef + (size_t)b0 * s_coef, s_coef) : KsSource::of_ntt(c1, sin));
        for (int i = 0; i < n_rot; i++) {
            if (one_pass) {
                t.mac_ext(*glk[i], {.out = outs[i] + (size_t)b0 * sout, .sout = sout, .scatter = perms[i], .base = ct, .sbase = sin});
                continue;
            }
            t.mac(*glk[i]);
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
            t.decompose(KsSource::of_ntt(ct + (long long)L * N, sin));
            t.mac_ext(glk, {.out = out + (size_t)b0 * sout, .sout = sout, .scatter = scatter, .base = ct, .sbase = sin, .accumulate = accumulate});
        });
        return;
    }
    const u32* perm = c.ntt_perm(g);
    for_tiles(c, KsTile::rows(c, level), batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        const u64* ct = in + (size_t)b0 * sin;
        KsTile t(c, level, nb, ws, st, &glk);
        t.decompose(KsSource::of_ntt(ct + (long long)L * N, sin));
        t.mac(glk);
        launch_permute_ext(c, level, perm, t.acc, t.s_acc, ct, sin, 1, out + (size_t)b0 * sout, sout, accumulate, nb, st);
    });
}

// the rounded division by P: extended ciphertext -> ciphertext [2][L][N].  `in` is clobbered (its P rows leave the NTT domain).
void ckks_moddown_ext(Context& c, int level, u64* in, u64* out, int batch, long long sin, long long sout, hipStream_t s,
                      bool coeff_out) {
    for_tiles(c, KsTile::moddown_rows(level), batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        KsTile::moddown_ext(c, level, in + (size_t)b0 * sin, sin, ws,
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
        key_switch(c, level, KsSource::of_ntt(ct + (long long)L * N, sin), swk, ks_onto_c0(out + (size_t)b0 * sout, sout, ct, sin, L), nb, ws, st);
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
    KsOut o = ks_onto_ct(r2, sr, d3, sd, L);
    const bool merged = with_rescale && c.fuse_tails;   // the merged ModDown + rescale tail
    if (!with_rescale) {
        o.p = out;
        o.sp = so;
    } else if (merged) {
        o.form = KsOut::RESCALE;
        o.rs = {out, so};
    }
    key_switch(c, level, KsSource::of_ntt(d2, sd), rlk, o, nb, sub, s);
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
            key_switch(c, level, KsSource::of_product(tf), rlk, {.p = r2, .sp = sr, .form = KsOut::RESCALE, .rs = {out + (size_t)b0 * so, so}},
                       nb, sub, st);
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
    // the tensor kernel and the tails move 16 bytes per lane at base + item * stride
    LSA_REQUIRE(layout::aligned16(layout::span_of(out, so, wout)), "dot: the output must be 16-byte aligned with an even batch stride");
    auto operand = [&](const u64* p, long long stride, int rpp, const char* what) {
        LSA_REQUIRE(p != nullptr, std::string("dot: ") + what + " is null");
        LSA_REQUIRE(rpp >= L, std::string("dot: rows per polynomial of ") + what + " below level + 1");
        const size_t words = 2 * (size_t)rpp * N;
        LSA_REQUIRE(stride == 0 || stride >= (long long)words, std::string("dot: batch stride of ") + what + " below one ciphertext");
        LSA_REQUIRE(layout::aligned16(layout::span_of(p, stride, words)), std::string("dot: ") + what + " must be 16-byte aligned with an even batch stride");
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
    LSA_REQUIRE(rlk.data != nullptr && rlk.level >= level, "dot: the relinearisation key is missing or was exported at a lower level than the ciphertexts");
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

void bfv_relin(Context& c, int level, const u64* d3, const Key& rlk, u64* out, int batch, long long sd, long long so,
               hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_relin", LSA_ALGO_BFV, level, 0, batch);
    ck.key(rlk, "the relinearisation key");
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    ck.apart(ck.output(out, so, 2 * (size_t)L * N), ck.operand(d3, sd, 3 * (size_t)L * N, "d3", false), "d3");
    // the decomposition starts from the coefficients of d2 and the ModDown tail runs on coefficients (KsSource::COEFF, KsOut::COEFF)
    for_tiles(c, KsTile::rows(c, level, KsSource::COEFF), batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        const u64* d = d3 + (size_t)b0 * sd;
        key_switch(c, level, KsSource::of_coeff(d + 2LL * L * N, sd), rlk,
                   ks_onto_ct(out + (size_t)b0 * so, so, d, sd, L, {.form = KsOut::COEFF}), nb, ws, st);
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
    const size_t ks_rows = KsTile::rows(c, level, KsSource::COEFF);
    const long long sp = 2LL * L * N;
    for_tiles(c, ks_rows + 2 * (size_t)L, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* p = ws + ks_rows * N * tb;
        const u64* ct = in + (size_t)b0 * sin;
        key_switch(c, level, KsSource::of_coeff(ct + (long long)L * N, sin), glk,   // p0 = c0 + ks0
                   ks_onto_c0(p, sp, ct, sin, L, {.form = KsOut::COEFF}), nb, ws, st);
        launch_permute_coeff(c, perm, p, sp, out + (size_t)b0 * sout, sout, 2 * L, rm_seq(L), nb, st);
    });
}

// rotations of the same ciphertexts by several Galois elements with ONE decomposition (hoisting); outs[i] = rotate(in, g[i]),
// each identical to bfv_rotate's result.  Per tile: c1 into the NTT domain once (the MAC's own-digit operand), the digits'
// conversions and extension transforms once from the coefficients; then per key the stand-alone MAC (several keys: the
// fused second pass + MAC does not apply) and the coefficient-domain ModDown, whose tail applies the automorphism by its
// loads and writes outs[i] directly (k_sub_mul_perm).  Two-step form (tail into the workspace, then k_permute) for an
// output that is the input, for N > 2^14, with LSA_ROT_SCATTER=0 and with unfused tails.
void bfv_rotate_many(Context& c, int level, const u64* in, int n_rot, const u64* g, const Key* const* glk, u64* const* outs,
                     int batch, long long sin, long long sout, hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_rotate_many", LSA_ALGO_BFV, level, 0, batch);
    if (n_rot <= 0 || batch <= 0) return;
    LSA_REQUIRE(g && glk && outs, ck.who + ": null argument");
    const long long N = c.n;
    const int L = level + 1;
    const Span sp_in = ck.operand(in, sin, 2 * (size_t)L * N, "in", false);
    for (int i = 0; i < n_rot; i++) {
        LSA_REQUIRE(glk[i] != nullptr, ck.who + ": a Galois key is null");
        ck.key(*glk[i], "a Galois key");
    }
    // the rule of lsa_ckks_rotate_many: a partial overlap with the input would let one tile store over what another still reads
    const int in_place = ck.rotate_many_outputs(sp_in, outs, n_rot, sout, 2 * (size_t)L * N);
    if (n_rot == 1) {
        bfv_rotate(c, level, in, g[0], *glk[0], outs[0], batch, sin, sout, s);
        return;
    }
    const size_t ks_rows = KsTile::rows(c, level, KsSource::COEFF);
    const long long sp = 2LL * L * N;
    // the one-pass tail stages a limb in LDS (N <= 2^14); larger rings keep the two steps, which measured faster than gathering
    // from global memory
    const bool gather_on = sw::rot_scatter() && c.fuse_tails && c.logn <= LSA_PERM_LDS_MAX_LOGN;
    std::vector<const u32*> perms(n_rot);
    std::vector<bool> direct(n_rot);
    std::vector<int> order;   // the output that IS the input goes last: every other rotation still reads the intact c0
    for (int i = 0; i < n_rot; i++) {   // (table look-ups upload on first use: only after every argument is accepted)
        perms[i] = c.coeff_perm(g[i]);
        direct[i] = i != in_place && gather_on;
        if (i != in_place) order.push_back(i);
    }
    if (in_place >= 0) order.push_back(in_place);
    for_tiles(c, ks_rows + 2 * (size_t)L, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* p = ws + ks_rows * N * tb;
        const u64* ct = in + (size_t)b0 * sin;
        KsTile t(c, level, nb, ws, st, nullptr, KsSource::COEFF);
        t.decompose(KsSource::of_coeff(ct + (long long)L * N, sin));
        for (int i : order) {
            t.mac(*glk[i]);
            KsOut o = ks_onto_c0(p, sp, ct, sin, L, {.form = KsOut::COEFF});
            if (direct[i]) {   // p0 = c0 + ks0 and the automorphism in one tail, straight into the output
                const KsPermTail gathered(perms[i]);
                o.p = outs[i] + (size_t)b0 * sout;
                o.sp = sout;
                o.tail = &gathered;
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
    const EntryCheck ck(c, "lsa_bfv_mult_plain_mul", LSA_ALGO_BFV, level, 0, batch);
    if (batch <= 0) return;
    const int L = level + 1;
    const size_t wct = 2 * (size_t)L * c.n, wpt = (size_t)L * c.n;
    // the transforms load 16-byte pairs at base + item * stride; out == ct item for item is the in-place transform
    const Span sp_out = ck.output(out, sout, wct);
    ck.same_or_apart(sp_out, ck.operand(ct, sct, wct, "ct", false), "ct");
    ck.apart(sp_out, ck.operand(pt, spt, wpt, "pt", true), "the plaintexts");
    ptmul_term(c, L, ct, sct, pt, spt, false, out, sout, out, sout, batch, s);
    launch_ntt(c, out, out, batch, sout, 2 * L, rm_seq(L), true, s);
}

void bfv_mac_plain_mul(Context& c, int level, int n, const u64* const* cts, const long long* scts, const u64* const* pts,
                       const long long* spts, const u64* partial, long long spartial, u64* out, int batch, long long sout,
                       hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_mac_plain_mul", LSA_ALGO_BFV, level, 0, batch);
    LSA_REQUIRE(n >= 1, ck.who + ": needs at least one term");
    if (batch <= 0) return;
    LSA_REQUIRE(cts && scts && pts && spts, ck.who + ": null argument");
    const long long N = c.n;
    const int L = level + 1;
    const size_t wct = 2 * (size_t)L * N, wpt = (size_t)L * N;
    // out holds the running sum while the terms are read: it may alias none of them
    const Span sp_out = ck.output(out, sout, wct);
    for (int i = 0; i < n; i++) {
        ck.apart(sp_out, ck.operand(cts[i], scts[i], wct, "a ciphertext", false), "a ciphertext");
        ck.apart(sp_out, ck.operand(pts[i], spts[i], wpt, "a plaintext", true), "a plaintext");
    }
    if (partial) ck.apart(sp_out, ck.operand(partial, spartial, wct, "the partial sum", false), "the partial sum");
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
    const EntryCheck ck(c, "lsa_bfv_rotate_mac_plain_mul", LSA_ALGO_BFV, level, 0, batch);
    LSA_REQUIRE(n >= 1, ck.who + ": needs at least one term");
    LSA_REQUIRE(g && glk && pts && spts, ck.who + ": null argument");
    bool any_rot = false;
    for (int i = 0; i < n; i++) {
        LSA_REQUIRE((g[i] & 1) == 1 && g[i] < 2 * (u64)c.n, ck.who + ": Galois element must be odd and < 2N");
        if (g[i] == 1) continue;
        LSA_REQUIRE(glk[i] != nullptr, ck.who + ": a rotation term needs its key");
        ck.key(*glk[i], "a Galois key");
        any_rot = true;
    }
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    const size_t wct = 2 * (size_t)L * N, wpt = (size_t)L * N;
    // out holds the running sum while the input, the plaintexts and the partial sum are still read: it may alias none of them
    const Span sp_out = ck.output(out, sout, wct);
    ck.apart(sp_out, ck.operand(in, sin, wct, "in", false), "the input");
    for (int i = 0; i < n; i++) ck.apart(sp_out, ck.operand(pts[i], spts[i], wpt, "a plaintext", true), "a plaintext");
    if (partial) ck.apart(sp_out, ck.operand(partial, spartial, wct, "the partial sum", false), "the partial sum");
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
        if (any_rot) t.decompose(KsSource::of_both(ctn + L * N, sct, ct + (long long)L * N, sin));
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
            t.mac(*glk[i]);
            if (fused) {
                const RotMacTerm term{pt, spts[i], !first};
                t.moddown(ks_onto_c0(o, sout, ctn, sct, L, {.scatter = scatters[i], .rmac = &term}));
            } else {
                t.moddown(ks_onto_c0(p, sct, ctn, sct, L, {.scatter = scatters[i]}));
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

}  // namespace lsa
