"""CPU restatement of the BFV plaintext matrix x ciphertext vector product (include/lattisense_amd.h: lsa_bfv_matvec_plain_mul) on the
oracle, the expression tests/test_gpu_bfv_ptmul.py::_want_mac states with every query ciphertext transformed once:
  out[r] = INTT( sum_c NTT(ct[c]) . pt[r][c] . 2^-64 )  (+ partial[r])
per polynomial and limb, built from Oracle.ntt, Oracle.vec and Oracle.intt.  The plan is restated here as well (plan_of)."""
import numpy as np

ROW_BLOCK_DEFAULT = 2
MIN_WORKGROUPS = 1024


def plan_of(n_ring, limbs, rows, cols, batch, workspace_bytes):
    """(row_block, col_block, launches, workspace_rows) of lsa_bfv_matvec_plan"""
    fit = workspace_bytes // (2 * limbs * n_ring * 8)
    assert fit >= 1
    rb = ROW_BLOCK_DEFAULT
    while rb > 1 and rb // 2 >= rows:
        rb //= 2
    if limbs * (n_ring // 512) * -(-rows // rb) * batch < MIN_WORKGROUPS:
        rb = 1
    cb = min(cols, fit)
    tile = min(batch, fit // cb)
    return rb, cb, -(-batch // tile) * -(-cols // cb), cb * 2 * limbs


def minv(q):
    return np.uint64(pow(2 ** 64, -1, int(q)))


def pt_mul_of(o, L, coeffs):
    """the pt_mul plaintext [L][N] of a polynomial with coefficients in [0, t): the coefficient as it is at every modulus, NTT domain,
    Montgomery form (form 1 of lsa_bfv_encode / lsa_bfv_plain_lift)"""
    c = np.asarray(coeffs, dtype=np.uint64)
    return np.stack([o.vec("mul", j, o.ntt(j, c), np.full(o.n, np.uint64(2 ** 64 % int(o.q[j])), dtype=np.uint64)) for j in range(L)])


def transform(o, L, cts):
    """cts [cols][2][L][N] coefficient domain -> their forward transforms, once each"""
    cts = np.asarray(cts, dtype=np.uint64)
    return np.stack([np.stack([np.stack([o.ntt(j, ct[pl, j]) for j in range(L)]) for pl in range(2)]) for ct in cts])


def descale(o, L, pts):
    """pts [rows][cols][L][N] pt_mul plaintexts -> pt . 2^-64 mod q, once each (shared by the batch items of a shared database)"""
    pts = np.asarray(pts, dtype=np.uint64)
    out = np.empty_like(pts)
    for j in range(L):
        r = np.full(o.n, minv(o.q[j]), dtype=np.uint64)
        for a in range(pts.shape[0]):
            for c in range(pts.shape[1]):
                out[a, c, j] = o.vec("mul", j, pts[a, c, j], r)
    return out


def matvec_ntt(o, L, ctn, ptd, partial=None):
    """ctn = transform(cts), ptd = descale(pts) -> out [rows][2][L][N], coefficient domain"""
    rows, cols = ptd.shape[:2]
    assert ctn.shape[0] == cols
    out = np.empty((rows, 2, L, o.n), dtype=np.uint64)
    for r in range(rows):
        for pl in range(2):
            for j in range(L):
                acc = np.zeros(o.n, dtype=np.uint64)
                for c in range(cols):
                    acc = o.vec("add", j, acc, o.vec("mul", j, ctn[c, pl, j], ptd[r, c, j]))
                v = o.intt(j, acc)
                out[r, pl, j] = o.vec("add", j, v, np.asarray(partial[r][pl, j], dtype=np.uint64)) if partial is not None else v
    return out


def matvec(o, L, cts, pts, partial=None):
    """cts [cols][2][L][N], pts [rows][cols][L][N], partial [rows][2][L][N] or None -> [rows][2][L][N]"""
    return matvec_ntt(o, L, transform(o, L, cts), descale(o, L, pts), partial)
