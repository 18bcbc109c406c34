// bfv_matvec.h — the plan of the BFV plaintext matrix x ciphertext vector product (lsa_bfv_matvec_plain_mul; semantics:
// include/lattisense_amd.h):  out[r] = INTT( sum_{c < cols} NTT(ct[c]) . pt[r][c] . 2^-64 )  for r < rows.  Pure C++17, host only: no
// device, no context (lsa_bfv_matvec_plan, tests/cpp/test_bfv_matvec.cpp).
//
// The runner transforms the `cols` query ciphertexts once into the workspace, 2 * level_limbs rows per column and batch item.  When all
// columns of one item do not fit `workspace_bytes`, the columns are cut into blocks of `col_block`; every block is one launch of
// k_bfv_matvec over all row blocks, the first writing the NTT-domain sums and the later ones adding to them.  A workgroup of the kernel
// sums `row_block` output rows from one read of the transformed ciphertext; the last row block of a `rows` that is no multiple of it
// masks its rows.  The batch is cut into tiles of as many items as fit the workspace next to each other.
#pragma once
#include <cstddef>
#include <stdexcept>
#include <string>

namespace lsa {

constexpr int BFV_MATVEC_ROW_BLOCK_MAX = 8;
// Measured on an MI355X (profiles/r29): two rows per workgroup win or tie at every shape whose grid fills
// the chip (102 VGPRs, 4 waves per SIMD; four and eight rows run at 2 and 1 waves and lose by 5-50 %); a grid below
// BFV_MATVEC_MIN_WORKGROUPS workgroups is short of parallelism instead and takes one row per workgroup.
constexpr int BFV_MATVEC_ROW_BLOCK_DEFAULT = 2;
constexpr long long BFV_MATVEC_MIN_WORKGROUPS = 1024;   // 4 per CU
// the budget the runner plans with: the one pick_tile() sizes a tile by
constexpr size_t BFV_MATVEC_WORKSPACE_BYTES = (size_t)8 << 30;

struct BfvMatvecPlanHost {
    int rows = 0, cols = 0, batch = 0;
    int row_block = 0;       // RB: output rows per workgroup, 1, 2, 4 or 8
    int n_row_blocks = 0;    // ceil(rows / row_block): a dimension of one launch's grid, not a launch each
    int col_block = 0;       // columns transformed and multiplied per launch
    int n_col_blocks = 0;    // ceil(cols / col_block)
    int tile_batch = 0;      // batch items whose col_block columns fit the workspace together, <= batch
    int n_tiles = 0;         // ceil(batch / tile_batch)
    int n_launches = 0;      // launches of k_bfv_matvec of one call: n_tiles * n_col_blocks
    size_t workspace_rows = 0;   // rows of N words per batch item: col_block * 2 * level_limbs
    // column block j covers [col_begin(j), col_begin(j) + col_count(j))
    int col_begin(int j) const { return j * col_block; }
    int col_count(int j) const { return cols - j * col_block < col_block ? cols - j * col_block : col_block; }
    int row_count(int i) const { return rows - i * row_block < row_block ? rows - i * row_block : row_block; }
};

inline bool bfv_matvec_row_block_legal(int rb) { return rb == 0 || rb == 1 || rb == 2 || rb == 4 || rb == 8; }

// force_row_block / force_col_block: lsa_set_bfv_matvec_block's values, 0 = the default.  A forced col_block is cut to `cols` and to
// what the workspace holds.  Throws std::invalid_argument; the message begins "lsa_bfv_matvec" and names the argument.
inline BfvMatvecPlanHost bfv_matvec_plan(int n_ring, int level_limbs, int rows, int cols, int batch, size_t workspace_bytes,
                                         int force_row_block = 0, int force_col_block = 0) {
    const std::string who = "lsa_bfv_matvec_plan: ";
    if (n_ring < 512 || (n_ring & (n_ring - 1)) != 0 || n_ring > (1 << 20))
        throw std::invalid_argument(who + "n_ring must be a power of two, 512 .. 2^20");
    if (level_limbs < 1 || level_limbs > 256) throw std::invalid_argument(who + "level_limbs must be 1 .. 256");
    if (rows < 1) throw std::invalid_argument(who + "rows must be >= 1");
    if (cols < 1) throw std::invalid_argument(who + "cols must be >= 1");
    if (batch < 1) throw std::invalid_argument(who + "batch must be >= 1");
    if (!bfv_matvec_row_block_legal(force_row_block)) throw std::invalid_argument(who + "row_block must be 0, 1, 2, 4 or 8");
    if (force_col_block < 0) throw std::invalid_argument(who + "col_block must be >= 0");
    const size_t col_bytes = 2 * (size_t)level_limbs * (size_t)n_ring * 8;   // one transformed ciphertext
    const size_t fit = workspace_bytes / col_bytes;
    if (fit < 1) throw std::invalid_argument(who + "workspace_bytes: the workspace does not hold one transformed ciphertext");
    BfvMatvecPlanHost p;
    p.rows = rows, p.cols = cols, p.batch = batch;
    int rb = force_row_block ? force_row_block : BFV_MATVEC_ROW_BLOCK_DEFAULT;
    if (!force_row_block) {
        while (rb > 1 && rb / 2 >= rows) rb /= 2;   // no wider than the smallest block that holds all rows
        const long long pieces = (long long)level_limbs * (n_ring / 512);
        if (pieces * ((rows + rb - 1) / rb) * batch < BFV_MATVEC_MIN_WORKGROUPS) rb = 1;
    }
    p.row_block = rb;
    p.n_row_blocks = (rows + rb - 1) / rb;
    size_t cb = (size_t)cols;
    if (force_col_block > 0 && (size_t)force_col_block < cb) cb = (size_t)force_col_block;
    if (fit < cb) cb = fit;
    p.col_block = (int)cb;
    p.n_col_blocks = (cols + p.col_block - 1) / p.col_block;
    size_t tb = fit / cb;
    if (tb > (size_t)batch) tb = (size_t)batch;
    p.tile_batch = (int)tb;
    p.n_tiles = (batch + p.tile_batch - 1) / p.tile_batch;
    p.workspace_rows = cb * 2 * (size_t)level_limbs;
    const long long launches = (long long)p.n_tiles * p.n_col_blocks;
    if (launches > 0x7fffffffLL) throw std::invalid_argument(who + "batch * cols: too many launches for this workspace");
    p.n_launches = (int)launches;
    return p;
}

}  // namespace lsa
