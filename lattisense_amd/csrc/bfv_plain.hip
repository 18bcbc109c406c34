// bfv_plain.hip — a BFV ciphertext combined with a ring-t plaintext (lsa_bfv_addsub_plain / _plain_lift / _mult_plain; the task
// runtime's BFV ct +- ring-t nodes).  The per-word arithmetic is bfv_plain.h's; DESIGN.md 4.16 has the byte model.
//
//   k_bfv_addsub_plain  out = ct +- scaleUp(pt) (or scaleUp(pt) - ct) in ONE pass: a lane owns two adjacent coefficients of one
//                       batch item across all limbs.  It reads the two plaintext words once and forms the limb-independent
//                       u = (m [Q]_t + t/2) mod t once (k_lift_ringt forms it once per limb, with two 64-bit `%`); per limb it
//                       loads c0, adds or subtracts the scaled word and stores.  The other polynomials ride in the same launch:
//                       copied (op 0 / 1), negated (op 2), or left alone when the call works in place.  The scaled plaintext is
//                       never stored.
//   lift / multiply     the plaintext goes to pt_mul form through the encoder's transform (bfv_lift_rows), the product is
//                       bfv_mult_plain_mul's.
#include "bfv_plain.h"
#include "bfv_encode.h"
#include "entry_check.h"
#include "key_switch.h"
#include "tables.h"

namespace lsa {

namespace {

constexpr int TPB = 256;
constexpr int GROUP = 4;   // rows a lane has in flight: its loads are issued before the first store of the group

__device__ __forceinline__ ulonglong2 ld2(const u64* p) { return *reinterpret_cast<const ulonglong2*>(p); }
__device__ __forceinline__ void st2(u64* p, u64 x, u64 y) {
    ulonglong2 v;
    v.x = x;
    v.y = y;
    *reinterpret_cast<ulonglong2*>(p) = v;
}

struct BfvPlainArgs {
    const u64* ct;   // [batch][polys][L][N], coefficient domain
    const u64* pt;   // [batch][N] ring-t words (any 64-bit value); spt == 0: one plaintext for the batch
    u64* out;        // [batch][polys][L][N]; may be ct itself
    long long sct, spt, sout;
    const ModDev* mods;
    const u64* neg_tinv;   // -(t^-1) mod q_j, Montgomery form
    u64 t, trec, qmodt;    // trec = floor(2^64 / t), qmodt = Q_level mod t
    int L, polys, logn;
    int others;            // the polynomials after the first: 0 = not touched (in place, op 0 / 1), 1 = copied or negated
};

// grid: x = N / (2 TPB), y = batch; 16 B per lane and access.  The limb constants are uniform: scalar loads.
template <int OP>
__global__ __launch_bounds__(TPB) void k_bfv_addsub_plain(BfvPlainArgs g) {
    const int x = (blockIdx.x * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const ulonglong2 m = ld2(g.pt + b * g.spt + x);
    const BfvPlainWord w0 = bfv_plain_centre(m.x, g.t, g.trec, g.qmodt);
    const BfvPlainWord w1 = bfv_plain_centre(m.y, g.t, g.trec, g.qmodt);
    const u64* ct = g.ct + b * g.sct + x;
    u64* out = g.out + b * g.sout + x;
    for (int j0 = 0; j0 < g.L; j0 += GROUP) {
        ulonglong2 v[GROUP];
#pragma unroll
        for (int i = 0; i < GROUP; i++)
            if (j0 + i < g.L) v[i] = ld2(ct + ((long long)(j0 + i) << g.logn));
#pragma unroll
        for (int i = 0; i < GROUP; i++)
            if (j0 + i < g.L) {
                const ModDev md = g.mods[j0 + i];
                const u64 k = g.neg_tinv[j0 + i];
                st2(out + ((long long)(j0 + i) << g.logn), bfv_plain_word<OP>(v[i].x, bfv_plain_scale_up(w0, k, md), md.q),
                    bfv_plain_word<OP>(v[i].y, bfv_plain_scale_up(w1, k, md), md.q));
            }
    }
    if (!g.others) return;
    for (int p = 1; p < g.polys; p++) {
        const long long row0 = (long long)p * g.L;
        for (int j0 = 0; j0 < g.L; j0 += GROUP) {
            ulonglong2 v[GROUP];
#pragma unroll
            for (int i = 0; i < GROUP; i++)
                if (j0 + i < g.L) v[i] = ld2(ct + ((row0 + j0 + i) << g.logn));
#pragma unroll
            for (int i = 0; i < GROUP; i++)
                if (j0 + i < g.L) {
                    if (OP == 2) {
                        const u64 q = g.mods[j0 + i].q;
                        v[i].x = neg_mod(v[i].x, q);
                        v[i].y = neg_mod(v[i].y, q);
                    }
                    st2(out + ((row0 + j0 + i) << g.logn), v[i].x, v[i].y);
                }
        }
    }
}

// t below every modulus of the rows a lift of this form writes: the coefficient in [0, t) is then its own residue
void require_t_below(const Context& c, int level, int form, const std::string& who) {
    const int rows = bfv_pt_rows(c, level, form);
    LSA_REQUIRE(rows <= LSA_MAX_PERIOD, who + ": more rows than a transform launch takes");
    for (int j = 0; j < rows; j++)
        LSA_REQUIRE(c.t < c.T.mod[c.qp_mod(level + 1, j)], who + ": t must be below every modulus of the chain");
}

}  // namespace

void launch_bfv_addsub_plain(Context& c, int op, int level, int polys, const u64* ct, long long sct, const u64* pt, long long spt,
                             u64* out, long long sout, int batch, hipStream_t s) {
    if (batch <= 0) return;
    const int L = level + 1;
    LSA_REQUIRE(op >= 0 && op <= 2 && polys >= 2 && polys <= 3 && level >= 0 && level < c.nq, "bfv_addsub_plain: internal: bad shape");
    LSA_REQUIRE(c.t > 1 && c.t < (1ull << 32), "ring-t scale-up needs a plaintext modulus below 2^32");
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the elementwise kernels (need N >= 512)");
    BfvPlainArgs g{};
    g.ct = ct;
    g.pt = pt;
    g.out = out;
    g.sct = sct;
    g.spt = spt;
    g.sout = sout;
    g.mods = c.d_mods;
    g.t = c.t;
    g.trec = (u64)((((unsigned __int128)1) << 64) / c.t);
    u64 qm = 1 % c.t;
    std::vector<int> mods(L);
    std::vector<u64> v(L);
    for (int i = 0; i < L; i++) {
        qm = mul_mod_host(qm, c.T.mod[i] % c.t, c.t);
        mods[i] = i;
        v[i] = c.T.mod[i] - inv_mod(c.t % c.T.mod[i], c.T.mod[i]);
    }
    g.qmodt = qm;
    g.neg_tinv = c.const_vec("neg_tinv" + std::to_string(L), mods, v);   // the vector launch_lift_ringt caches, per level
    g.L = L;
    g.polys = polys;
    g.logn = c.logn;
    const bool in_place = out == ct && sout == sct;
    g.others = (in_place && op != 2) ? 0 : 1;
    // algorithmic bytes: the plaintext row once, c0 read and written, the other polynomials read and written unless left alone
    const double rows = 1.0 + 2.0 * L + (g.others ? 2.0 * (polys - 1) * L : 0.0);
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * rows * batch, s);
    const dim3 grid((unsigned)(c.n / (2 * TPB)), (unsigned)batch);
    if (op == 0) hipLaunchKernelGGL((k_bfv_addsub_plain<0>), grid, dim3(TPB), 0, s, g);
    else if (op == 1) hipLaunchKernelGGL((k_bfv_addsub_plain<1>), grid, dim3(TPB), 0, s, g);
    else hipLaunchKernelGGL((k_bfv_addsub_plain<2>), grid, dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

void bfv_addsub_plain(Context& c, int op, int level, const u64* ct, long long sct, const u64* pt, long long spt, u64* out,
                      long long sout, int batch, hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_addsub_plain", LSA_ALGO_BFV, level, 0, batch);
    LSA_REQUIRE(op >= 0 && op <= 2, ck.who + ": op must be 0 (ct + pt), 1 (ct - pt) or 2 (pt - ct)");
    LSA_REQUIRE(c.t > 1 && c.t < (1ull << 32), ck.who + ": the plaintext modulus t must be below 2^32");
    LSA_REQUIRE(c.n >= 2 * TPB, ck.who + ": ring degree too small for the elementwise kernels (need N >= 512)");
    const size_t w = 2 * (size_t)(level + 1) * c.n;
    const EntryCheck::Span so = ck.output(out, sout, w);
    ck.same_or_apart(so, ck.operand(ct, sct, w, "ct", false), "ct");
    ck.apart(so, ck.operand(pt, spt, (size_t)c.n, "pt", true), "the plaintexts");
    launch_bfv_addsub_plain(c, op, level, 2, ct, sct, pt, spt, out, sout, batch, s);
}

void bfv_plain_lift(Context& c, int level, int form, const u64* pt, long long spt, u64* out, long long sout, int batch,
                    hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_plain_lift", LSA_ALGO_BFV, level, 0, batch);
    LSA_REQUIRE(form == BFV_PT_MUL || form == BFV_PT_EXT, ck.who + ": form must be 1 (pt_mul) or 2 (extended)");
    require_t_below(c, level, form, ck.who);
    const size_t w = (size_t)bfv_pt_rows(c, level, form) * c.n;
    ck.apart(ck.output(out, sout, w), ck.operand(pt, spt, (size_t)c.n, "pt", true), "the plaintexts");
    bfv_lift_rows(c, level, form, pt, spt, out, sout, batch, s);
}

void bfv_mult_plain(Context& c, int level, const u64* ct, long long sct, const u64* pt, long long spt, u64* out, long long sout,
                    int batch, hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_mult_plain", LSA_ALGO_BFV, level, 0, batch);
    require_t_below(c, level, BFV_PT_MUL, ck.who);
    const int L = level + 1;
    const long long wpt = (long long)L * c.n;
    const size_t w = 2 * (size_t)wpt;
    const EntryCheck::Span so = ck.output(out, sout, w);
    ck.same_or_apart(so, ck.operand(ct, sct, w, "ct", false), "ct");
    ck.apart(so, ck.operand(pt, spt, (size_t)c.n, "pt", true), "the plaintexts");
    if (batch <= 0) return;
    if (spt == 0) {   // one plaintext: lifted once
        u64* lifted = c.workspace((size_t)wpt, s);
        bfv_lift_rows(c, level, BFV_PT_MUL, pt, 0, lifted, wpt, 1, s);
        bfv_mult_plain_mul(c, level, ct, lifted, out, batch, sct, 0, sout, s);
        return;
    }
    // per-item plaintexts: a tile's pt_mul rows in the workspace, then the tile's products
    for_tiles(c, (size_t)L, batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t st) {
        bfv_lift_rows(c, level, BFV_PT_MUL, pt + (size_t)b0 * spt, spt, ws, wpt, nb, st);
        bfv_mult_plain_mul(c, level, ct + (size_t)b0 * sct, ws, out + (size_t)b0 * sout, nb, sct, wpt, sout, st);
    });
}

}  // namespace lsa
