// Host program for lattisense_amd/csrc/bfv_matvec.h (tests/test_bfv_matvec_host.py builds it with -fsanitize=address,undefined): the
// plan of the plaintext matrix x ciphertext vector product for every rows, cols <= 40, a few batches and workspace sizes and every
// forced block -- the column blocks cover the columns exactly once, the row blocks the rows, a tile's columns fit the workspace, the
// launches are tiles x column blocks -- and the refusals.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../lattisense_amd/csrc/bfv_matvec.h"

using namespace lsa;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond);     \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static void plans() {
    const int n_ring = 2048, limbs = 3;
    const size_t col_bytes = 2 * (size_t)limbs * n_ring * 8;
    const size_t spaces[] = {col_bytes, col_bytes + 8, 3 * col_bytes, 7 * col_bytes - 8, 16 * col_bytes, 100 * col_bytes, BFV_MATVEC_WORKSPACE_BYTES};
    const int batches[] = {1, 3, 16};
    const int rbs[] = {0, 1, 2, 4, 8};
    const int cbs[] = {0, 1, 4, 16, 17, 1000};
    for (int rows = 1; rows <= 40; rows++)
        for (int cols = 1; cols <= 40; cols++)
            for (size_t space : spaces)
                for (int batch : batches)
                    for (int rb : rbs)
                        for (int cb : cbs) {
                            const BfvMatvecPlanHost p = bfv_matvec_plan(n_ring, limbs, rows, cols, batch, space, rb, cb);
                            CHECK(p.rows == rows && p.cols == cols && p.batch == batch);
                            // the row blocks: a legal width, the forced one if any, never wider than needed by default
                            CHECK(p.row_block == 1 || p.row_block == 2 || p.row_block == 4 || p.row_block == 8);
                            if (rb) CHECK(p.row_block == rb);
                            else {   // two rows where that still leaves the chip its workgroups, else one
                                const long long wgs2 = (long long)limbs * (n_ring / 512) * ((rows + 1) / 2) * batch;
                                CHECK(p.row_block == (rows >= 2 && wgs2 >= BFV_MATVEC_MIN_WORKGROUPS ? 2 : 1));
                            }
                            std::vector<int> row_seen(rows, 0);
                            for (int i = 0; i < p.n_row_blocks; i++) {
                                CHECK(p.row_count(i) >= 1 && p.row_count(i) <= p.row_block);
                                for (int r = 0; r < p.row_count(i); r++) row_seen[i * p.row_block + r]++;
                            }
                            for (int r = 0; r < rows; r++) CHECK(row_seen[r] == 1);
                            // the column blocks cover the columns exactly once, in order
                            CHECK(p.col_block >= 1 && p.col_block <= cols);
                            if (cb) CHECK(p.col_block <= cb);
                            std::vector<int> col_seen(cols, 0);
                            int next = 0;
                            for (int j = 0; j < p.n_col_blocks; j++) {
                                CHECK(p.col_begin(j) == next && p.col_count(j) >= 1 && p.col_count(j) <= p.col_block);
                                for (int k = 0; k < p.col_count(j); k++) col_seen[p.col_begin(j) + k]++;
                                next += p.col_count(j);
                            }
                            CHECK(next == cols);
                            for (int k = 0; k < cols; k++) CHECK(col_seen[k] == 1);
                            // a tile fits; a larger block or one more item would not, unless cols, the forced block or the batch stops it
                            CHECK(p.workspace_rows == (size_t)p.col_block * 2 * limbs);
                            CHECK(p.tile_batch >= 1 && p.tile_batch <= batch);
                            CHECK((size_t)p.tile_batch * p.col_block * col_bytes <= space);
                            const int want_cb = cb ? (cb < cols ? cb : cols) : cols;
                            if (p.col_block < want_cb) CHECK((size_t)(p.col_block + 1) * col_bytes > space);
                            if (p.tile_batch < batch) CHECK((size_t)(p.tile_batch + 1) * p.col_block * col_bytes > space);
                            CHECK(p.n_tiles == (batch + p.tile_batch - 1) / p.tile_batch);
                            CHECK(p.n_launches == p.n_tiles * p.n_col_blocks);
                        }
    // the budget of the runner holds whole shapes of the benchmark in one block
    const BfvMatvecPlanHost big = bfv_matvec_plan(16384, 8, 1024, 256, 16, BFV_MATVEC_WORKSPACE_BYTES);
    CHECK(big.col_block == 256 && big.n_col_blocks == 1 && big.tile_batch == 16 && big.n_launches == 1 && big.row_block == BFV_MATVEC_ROW_BLOCK_DEFAULT);
    const BfvMatvecPlanHost cut = bfv_matvec_plan(65536, 16, 4, 1024, 2, BFV_MATVEC_WORKSPACE_BYTES);   // 16 MiB a column: 512 fit
    CHECK(cut.col_block == 512 && cut.n_col_blocks == 2 && cut.tile_batch == 1 && cut.n_launches == 4);
    std::printf("ok plan\n");
}

static bool refused(int n_ring, int limbs, int rows, int cols, int batch, size_t space, int rb, int cb, const char* needle) {
    try {
        bfv_matvec_plan(n_ring, limbs, rows, cols, batch, space, rb, cb);
    } catch (const std::invalid_argument& e) {
        const std::string m = e.what();
        return m.rfind("lsa_bfv_matvec", 0) == 0 && m.find(needle) != std::string::npos;
    }
    return false;
}

static void refusals() {
    const size_t ok = (size_t)1 << 30;
    CHECK(refused(256, 3, 4, 4, 1, ok, 0, 0, "n_ring"));
    CHECK(refused(3000, 3, 4, 4, 1, ok, 0, 0, "n_ring"));
    CHECK(refused(2048, 0, 4, 4, 1, ok, 0, 0, "level_limbs"));
    CHECK(refused(2048, 3, 0, 4, 1, ok, 0, 0, "rows"));
    CHECK(refused(2048, 3, 4, -1, 1, ok, 0, 0, "cols"));
    CHECK(refused(2048, 3, 4, 4, 0, ok, 0, 0, "batch"));
    CHECK(refused(2048, 3, 4, 4, 1, ok, 3, 0, "row_block"));
    CHECK(refused(2048, 3, 4, 4, 1, ok, 16, 0, "row_block"));
    CHECK(refused(2048, 3, 4, 4, 1, ok, 0, -1, "col_block"));
    CHECK(refused(2048, 3, 4, 4, 1, 2 * 3 * 2048 * 8 - 8, 0, 0, "workspace_bytes"));   // one word short of one column
    CHECK(refused(2048, 3, 4, 4, 1, 0, 0, 0, "workspace_bytes"));
    CHECK(bfv_matvec_plan(2048, 3, 4, 4, 1, 2 * 3 * 2048 * 8).col_block == 1);
    std::printf("ok refusals\n");
}

int main() {
    plans();
    refusals();
    return 0;
}
