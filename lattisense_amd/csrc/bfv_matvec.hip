// bfv_matvec.hip — the BFV plaintext matrix x ciphertext vector product, the database scan of a PIR answer between lsa_bfv_expand and
// lsa_bfv_select (plan: bfv_matvec.h; semantics: include/lattisense_amd.h):
//   k_bfv_matvec<RB, ACC>   RB output rows from one read of the transformed query ciphertexts, both polynomials, 128-bit lazy sums
// and below it the runner: the tile's `cols` ciphertexts forward-transformed ONCE into the workspace, one launch of the kernel per
// column block over all rows, one inverse transform over the outputs, the partial added in the coefficient domain.  Every word equals
// bfv_mac_plain_mul (ops.hip) on row r's terms: both sum canonical residues mod q.
#include "bfv_matvec.h"
#include "entry_check.h"
#include "key_switch.h"
#include "ks_mac_pair.h"

namespace lsa {

namespace {

constexpr int TPB = 256;

__device__ __forceinline__ ulonglong2 ld2(const u64* p) { return *reinterpret_cast<const ulonglong2*>(p); }
__device__ __forceinline__ void st2(u64* p, u64 x, u64 y) {
    ulonglong2 v;
    v.x = x;
    v.y = y;
    *reinterpret_cast<ulonglong2*>(p) = v;
}

struct BfvMatvecArgs {
    const u64* ctn;   // the transformed ciphertexts of this column block: column c of item b at ctn + c * s_coln + b * sctn, [2][L][N]
    long long s_coln, sctn;
    const u64* pts;   // pt[r][c] of item b at pts + r * s_prow + c * s_pcol + b * spt, [L][N]; c counts from the block's first column
    long long s_prow, s_pcol, spt;
    u64* out;         // the NTT-domain sums: row r of item b at out + r * s_row + b * sout, [2][L][N]
    long long s_row, sout;
    const ModDev* mods;
    int logn, L, rows, cols, batch, n_rb;
};

// One workgroup = one 512-coefficient piece of one limb of one batch item and RB output rows, BOTH polynomials (they meet the same
// plaintext words); a thread owns the points x, x+1.  grid.x = pieces * n_rb * batch, the batch fastest and the row blocks next: the
// items that share a plaintext piece (spt == 0) and the row blocks that share a ciphertext piece run next to each other.
// Per column: 2 ciphertext and RB plaintext loads of 16 bytes, 4 RB products into RB x 2 x 2 128-bit sums; the next column's loads
// are issued before the current column is multiplied.  After every eighth column the sums are folded into canonical running residues
// (ks_mac_pair.h: 8 products of canonical residues stay below q * 2^64).  The plaintexts are in Montgomery form, so REDC of the sum
// is the sum of the products . 2^-64: the word k_mont_muladd and the fused transform store produce term by term.
// Rows past `rows` in the last block read the block's first row again (never past the database) and are not stored.
// ACC: the reduced sum is added to the canonical residue already in out (a later column block).
template <int RB, bool ACC>
__global__ __launch_bounds__(TPB) void k_bfv_matvec(BfvMatvecArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    unsigned w = blockIdx.x;
    const long long b = w % (unsigned)g.batch;
    w /= (unsigned)g.batch;
    const int r0 = (int)(w % (unsigned)g.n_rb) * RB;
    const int piece = (int)(w / (unsigned)g.n_rb);
    const int limb = piece / chunks;
    const int x = ((piece % chunks) * TPB + threadIdx.x) * 2;
    const ModDev m = g.mods[limb];
    const long long poff = ((long long)limb << g.logn) + x, pstep = (long long)g.L << g.logn;
    const int nr = min(RB, g.rows - r0);
    const u64* pc = g.ctn + b * g.sctn + poff;
    const u64* pp[RB];
#pragma unroll
    for (int i = 0; i < RB; i++) pp[i] = g.pts + b * g.spt + (long long)(r0 + (i < nr ? i : 0)) * g.s_prow + poff;
    u64 h[RB][2][2], l[RB][2][2], r[RB][2][2];
#pragma unroll
    for (int i = 0; i < RB; i++)
#pragma unroll
        for (int p = 0; p < 2; p++) h[i][p][0] = h[i][p][1] = l[i][p][0] = l[i][p][1] = r[i][p][0] = r[i][p][1] = 0;
    auto fold = [&]() {
#pragma unroll
        for (int i = 0; i < RB; i++)
#pragma unroll
            for (int p = 0; p < 2; p++)
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    r[i][p][k] = add_mod(r[i][p][k], csub(mont_redc_lazy(h[i][p][k], l[i][p][k], m.q, m.qinv), m.q), m.q);
                    h[i][p][k] = l[i][p][k] = 0;
                }
    };
    ulonglong2 cn0 = ld2(pc), cn1 = ld2(pc + pstep), wn[RB];
#pragma unroll
    for (int i = 0; i < RB; i++) wn[i] = ld2(pp[i]);
    for (int c = 0; c < g.cols; c++) {
        const ulonglong2 c0 = cn0, c1 = cn1;
        ulonglong2 wc[RB];
#pragma unroll
        for (int i = 0; i < RB; i++) wc[i] = wn[i];
        if (c + 1 < g.cols) {
            pc += g.s_coln;
            cn0 = ld2(pc);
            cn1 = ld2(pc + pstep);
#pragma unroll
            for (int i = 0; i < RB; i++) {
                pp[i] += g.s_pcol;
                wn[i] = ld2(pp[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < RB; i++) {
            mac128(h[i][0][0], l[i][0][0], c0.x, wc[i].x);
            mac128(h[i][0][1], l[i][0][1], c0.y, wc[i].y);
            mac128(h[i][1][0], l[i][1][0], c1.x, wc[i].x);
            mac128(h[i][1][1], l[i][1][1], c1.y, wc[i].y);
        }
        if (ks_pair_fold_after(c)) fold();
    }
    fold();
#pragma unroll
    for (int i = 0; i < RB; i++) {
        if (i < nr) {
#pragma unroll
            for (int p = 0; p < 2; p++) {
                u64* po = g.out + b * g.sout + (long long)(r0 + i) * g.s_row + p * pstep + poff;
                u64 v0 = r[i][p][0], v1 = r[i][p][1];
                if constexpr (ACC) {
                    const ulonglong2 v = ld2(po);
                    v0 = add_mod(v0, v.x, m.q);
                    v1 = add_mod(v1, v.y, m.q);
                }
                st2(po, v0, v1);
            }
        }
    }
}

template <int RB>
void launch_rb(const dim3& grid, bool acc, hipStream_t s, const BfvMatvecArgs& g) {
    if (acc) hipLaunchKernelGGL((k_bfv_matvec<RB, true>), grid, dim3(TPB), 0, s, g);
    else hipLaunchKernelGGL((k_bfv_matvec<RB, false>), grid, dim3(TPB), 0, s, g);
}

// one column block of one tile: out (+)= the block's NTT-domain sums for all rows
void launch_bfv_matvec(Context& c, int L, int row_block, BfvMatvecArgs g, bool acc, hipStream_t s) {
    g.mods = c.d_mods;
    g.logn = c.logn;
    g.L = L;
    g.n_rb = ceil_div(g.rows, row_block);
    const long long pieces = (long long)L * (c.n / (2 * TPB));
    const long long wgs = pieces * g.n_rb * g.batch;
    LSA_REQUIRE(wgs <= 0x7fffffffLL, "lsa_bfv_matvec_plain_mul: rows * batch: too many workgroups for one launch");
    // per item the block's ciphertexts once per row block and the sums written (read too when adding); the plaintexts once when the
    // batch shares them
    ProfScope ps(c, PROF_ELEMWISE,
                 8.0 * c.n * L * ((double)g.batch * (2.0 * g.cols * g.n_rb + 2.0 * g.rows * (acc ? 2 : 1)) +
                                  (double)g.rows * g.cols * (g.spt == 0 ? 1 : g.batch)), s);
    const dim3 grid((unsigned)wgs);
    switch (row_block) {
    case 1: launch_rb<1>(grid, acc, s, g); break;
    case 2: launch_rb<2>(grid, acc, s, g); break;
    case 4: launch_rb<4>(grid, acc, s, g); break;
    case 8: launch_rb<8>(grid, acc, s, g); break;
    default: LSA_REQUIRE(false, "lsa_bfv_matvec_plain_mul: no kernel for this row block");
    }
    LSA_HIP(hipGetLastError());
}

typedef layout::u128 u128;
u128 U(long long v) { return (u128)(unsigned long long)v; }

}  // namespace

BfvMatvecPlanHost bfv_matvec_plan_checked(int n_ring, int level_limbs, int rows, int cols, int batch, size_t workspace_bytes,
                                          int row_block, int col_block) {
    try {
        return bfv_matvec_plan(n_ring, level_limbs, rows, cols, batch, workspace_bytes, row_block, col_block);
    } catch (const std::invalid_argument& e) {
        throw Error(LSA_ERR_ARG, e.what());
    }
}

void bfv_matvec_plain_mul(Context& c, int level, int rows, int cols, const BfvMatvecLayout& a, int batch, hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_matvec_plain_mul", LSA_ALGO_BFV, level, 0, batch);
    LSA_REQUIRE(rows >= 1, ck.who + ": rows must be >= 1");
    LSA_REQUIRE(cols >= 1, ck.who + ": cols must be >= 1");
    LSA_REQUIRE(c.n >= 2 * TPB, ck.who + ": ring degree too small (need N >= 512)");
    const long long N = c.n;
    const int L = level + 1;
    const size_t wct = 2 * (size_t)L * N, wpt = (size_t)L * N;
    const int nbatch = batch > 1 ? batch : 1;
    const layout::Span sp_ct = ck.operand(a.cts, a.sct, wct, "cts", false);
    const layout::Span sp_pt = ck.operand(a.pts, a.spt, wpt, "pts", true);
    const layout::Span sp_out = ck.output(a.out, a.sout, wct);
    // an index stride is even and spans the batch it strides over: the items of two indices do not interleave
    auto index_stride = [&](long long st, const layout::Span& item, const char* what) {
        LSA_REQUIRE((st & 1) == 0, ck.who + ": " + what + " must be even");
        const u128 need = item.stride == 0 ? (u128)item.words : (u128)(unsigned)nbatch * U(item.stride);
        LSA_REQUIRE(st > 0 && U(st) >= need, ck.who + ": " + what + " is a stride below the batch it spans");
    };
    index_stride(a.s_col, sp_ct, "s_col");
    index_stride(a.s_row, sp_out, "s_row");
    // the database is only read: its rows and columns may nest either way round (a per-item database is usually [b][r][c]), each
    // stride at least one plaintext
    auto pt_stride = [&](long long st, const char* what) {
        LSA_REQUIRE((st & 1) == 0, ck.who + ": " + what + " must be even");
        LSA_REQUIRE(st > 0 && U(st) >= (u128)wpt, ck.who + ": " + what + " is a stride below one plaintext");
    };
    pt_stride(a.s_prow, "s_prow");
    pt_stride(a.s_pcol, "s_pcol");
    layout::Span sp_pa{};
    if (a.partial) {
        sp_pa = ck.operand(a.partial, a.spartial, wct, "partial", false);
        index_stride(a.s_partial_row, sp_pa, "s_partial_row");
    }
    LSA_REQUIRE((long long)rows * nbatch <= 0x7fffffffLL, ck.who + ": rows * batch does not fit a batch");
    LSA_REQUIRE((long long)cols * nbatch <= 0x7fffffffLL, ck.who + ": cols * batch does not fit a batch");
    if (batch <= 0) return;
    {   // out shares no word with an input: disjoint hulls settle the usual case, interleaved ones are walked index by index
        const u128 out_lo = sp_out.base, out_hi = out_lo + 8 * (U(a.s_row) * (unsigned)(rows - 1) + U(a.sout) * (unsigned)(batch - 1) + wct);
        auto hull_apart = [&](u128 lo, u128 hi) { return hi <= out_lo || out_hi <= lo; };
        const u128 ct_lo = sp_ct.base, ct_hi = ct_lo + 8 * (U(a.s_col) * (unsigned)(cols - 1) + U(a.sct) * (unsigned)(batch - 1) + wct);
        if (!hull_apart(ct_lo, ct_hi))
            for (int r = 0; r < rows; r++)
                for (int j = 0; j < cols; j++)
                    ck.apart(layout::span_of(a.out + r * a.s_row, a.sout, wct), layout::span_of(a.cts + j * a.s_col, a.sct, wct), "cts");
        const u128 pt_lo = sp_pt.base,
                   pt_hi = pt_lo + 8 * (U(a.s_prow) * (unsigned)(rows - 1) + U(a.s_pcol) * (unsigned)(cols - 1) + U(a.spt) * (unsigned)(batch - 1) + wpt);
        LSA_REQUIRE(hull_apart(pt_lo, pt_hi), ck.who + ": the output overlaps pts (their hulls must be apart)");
        if (a.partial) {
            const u128 pa_lo = sp_pa.base,
                       pa_hi = pa_lo + 8 * (U(a.s_partial_row) * (unsigned)(rows - 1) + U(a.spartial) * (unsigned)(batch - 1) + wct);
            if (!hull_apart(pa_lo, pa_hi))
                for (int r = 0; r < rows; r++)
                    for (int q = 0; q < rows; q++)
                        ck.apart(layout::span_of(a.out + r * a.s_row, a.sout, wct),
                                 layout::span_of(a.partial + q * a.s_partial_row, a.spartial, wct), "partial");
        }
    }
    const BfvMatvecPlanHost plan =
        bfv_matvec_plan_checked(c.n, L, rows, cols, batch, BFV_MATVEC_WORKSPACE_BYTES, c.matvec_row_block, c.matvec_col_block);
    const RowMap rm = rm_seq(L);
    const long long wl = (long long)wct;
    for_tiles(c, plan.workspace_rows, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        const bool whole = nb == batch;   // one tile: b0 == 0, tb == batch
        const long long s_coln = wl * tb;
        u64* o = a.out + (size_t)b0 * a.sout;
        for (int j = 0; j < plan.n_col_blocks; j++) {
            const int c0 = plan.col_begin(j), nc = plan.col_count(j);
            const u64* src = a.cts + (long long)c0 * a.s_col + (size_t)b0 * a.sct;
            if (whole && U(a.s_col) == (u128)(unsigned)batch * U(a.sct)) {   // dense index-major: the block's nc * batch items are one batch
                launch_ntt(c, src, ws, nc * batch, a.sct, wl, 2 * L, rm, false, st);
            } else {
                for (int k = 0; k < nc; k++) launch_ntt(c, src + (long long)k * a.s_col, ws + (long long)k * s_coln, nb, a.sct, wl, 2 * L, rm, false, st);
            }
            BfvMatvecArgs g{};
            g.ctn = ws, g.s_coln = s_coln, g.sctn = wl;
            g.pts = a.pts + (long long)c0 * a.s_pcol + (long long)b0 * a.spt;
            g.s_prow = a.s_prow, g.s_pcol = a.s_pcol, g.spt = a.spt;
            g.out = o, g.s_row = a.s_row, g.sout = a.sout;
            g.rows = rows, g.cols = nc, g.batch = nb;
            launch_bfv_matvec(c, L, plan.row_block, g, j > 0, st);
        }
        const bool dense_out = whole && U(a.s_row) == (u128)(unsigned)batch * U(a.sout);
        if (dense_out) launch_ntt(c, o, o, rows * batch, a.sout, 2 * L, rm, true, st);
        else
            for (int r = 0; r < rows; r++) launch_ntt(c, o + (long long)r * a.s_row, o + (long long)r * a.s_row, nb, a.sout, 2 * L, rm, true, st);
        if (!a.partial) return;
        const u64* pa = a.partial + (size_t)b0 * a.spartial;
        if (dense_out && U(a.s_partial_row) == (u128)(unsigned)batch * U(a.spartial)) {
            launch_elementwise(c, EW_ADD, o, pa, o, rows * batch, a.sout, a.spartial, a.sout, 2 * L, rm, st);
        } else {
            for (int r = 0; r < rows; r++)
                launch_elementwise(c, EW_ADD, o + (long long)r * a.s_row, pa + (long long)r * a.s_partial_row, o + (long long)r * a.s_row, nb,
                                   a.sout, a.spartial, a.sout, 2 * L, rm, st);
        }
    });
}

}  // namespace lsa
