"""CPU restatement of the BFV slot sum (lattisense_amd/csrc/slot_sum.h and slot_sum.hip bfv_slot_sum_run), twice:

slot_sum        the words as include/lattisense_amd.h fixes them: every limb of the ciphertext into the NTT domain, the steps on
                oracle/ckks_bootstrap.py's rotate_ext, add_ext, moddown and add exactly as tests/slot_sum_model.py slot_sum states
                them (the row step is rotate_ext with g = 2N-1), the result back into the coefficient domain;
slot_sum_coeff  the device's gathering form on Oracle primitives: only c1 enters the NTT domain, the gadget products are rotated
                and summed without P * c0, the division by P runs on coefficients, and x and the rotated c0 terms are added there.

ModDown(P z + a) = z + ModDown(a) residue for residue, so the two agree word for word (tests/test_bfv_slot_sum_api.py)."""
import numpy as np

from oracle.ckks_bootstrap import Ct, ExtCt


def steps_of(n_ring, step, count, radix=4, rows=0):
    """[[(Galois element, "tail" | "next"), ...], ...]: one list per step (one decomposition), the TAIL key first; with rows the
    row step (the key of 2N-1, NEXT) comes before the column steps"""
    h, m = n_ring // 2, 2 * n_ring
    s, n = step % h, count
    steps = [[(m - 1, "next")]] if rows else []
    while n > 1:
        rots = []
        if n % 2:
            rots.append(((n - 1) * s % h, "tail"))
            n -= 1
        if radix == 4 and n % 4 == 0:
            rots += [(i * s % h, "next") for i in (1, 2, 3)]
            s, n = 4 * s % h, n // 4
        else:
            rots.append((s, "next"))
            s, n = 2 * s % h, n // 2
        assert all(r for r, _ in rots), "a planned rotation is a multiple of N/2"
        steps.append([(pow(5, r, m), d) for r, d in rots])
    return steps


def galois_elements_of(n_ring, step, count, radix=4, rows=0):
    return sorted({g for keys in steps_of(n_ring, step, count, radix, rows) for g, _ in keys})


def make_evaluator(oracle, client, key_level):
    """an oracle.ckks_bootstrap.Evaluator without its relinearisation key (the slot sum needs none); works over a BFV Oracle too"""
    from oracle.ckks_bootstrap import Evaluator
    ev = Evaluator.__new__(Evaluator)
    ev.o, ev.c, ev.klvl, ev.n = oracle, client, key_level, oracle.n
    ev.glk, ev.counts = {}, {"rotate": 0, "mult": 0, "mul_plain": 0}
    return ev


def rotate_ext_g(ev, a, g):
    """Evaluator.rotate_ext for a Galois element instead of a column rotation: automorphism_g of (P c0 + ks0, ks1)"""
    L = a.level + 1
    acc = ev.o.gadget_product(a.level, a.data[1], ev._key(g), ev.klvl)
    c0p = ev.lift_ext(a).data[0]
    for j in range(L):
        acc[0, j] = ev.o.vec("add", j, acc[0, j], c0p[j])
    out = np.stack([np.stack([ev.o.automorph_ntt(g, acc[pl, tl]) for tl in range(acc.shape[1])]) for pl in range(2)])
    return ExtCt(out, a.level, a.scale)


def _each_limb(o, data, fn):
    return np.stack([np.stack([fn(j, data[pl, j]) for j in range(data.shape[1])]) for pl in range(data.shape[0])])


def slot_sum(ev, ct, level, step, count, radix=4, rows=0):
    """ct: [2][level+1][N] coefficient domain -> the same shape.  The words of the header."""
    x, tail = Ct(_each_limb(ev.o, np.asarray(ct), ev.o.ntt), level, 1.0), None
    for keys in steps_of(ev.n, step, count, radix, rows):
        nxt = None
        for g, dest in keys:
            e = rotate_ext_g(ev, x, g)
            if dest == "tail":
                tail = e if tail is None else ev.add_ext(tail, e)
            else:
                nxt = e if nxt is None else ev.add_ext(nxt, e)
        x = ev.add(x, ev.moddown(nxt))
    if tail is not None:
        x = ev.add(x, ev.moddown(tail))
    return _each_limb(ev.o, x.data, ev.o.intt)


def _moddown_coeff(ev, level, acc):
    """[2][T][N] over Q_level u P, NTT domain -> [2][L][N] coefficients: every row out of the NTT domain once, the P rows
    converted (centred) to Q, (acc_Q - conv) * P^-1"""
    o = ev.o
    L, T = level + 1, acc.shape[1]
    pidx, qidx = [o.nq + i for i in range(o.np_)], list(range(L))
    out = np.empty((2, L, o.n), dtype=np.uint64)
    for pl in range(2):
        co = [o.intt(ev._mi(level, tl), acc[pl, tl]) for tl in range(T)]
        conv = o.baseconv(pidx, qidx, np.stack(co[L:]), True)
        for j in range(L):
            q, pm = o.mod[j], 1
            for pp in o.p:
                pm = pm * (pp % q) % q
            out[pl, j] = o.vec("mul", j, o.vec("sub", j, co[j], conv[j]), np.full(o.n, pow(pm, -1, q), dtype=np.uint64))
    return out


def slot_sum_coeff(ev, ct, level, step, count, radix=4, rows=0):
    """the gathering form: x stays in the coefficient domain; per step NTT(c1) is decomposed once, each key's gadget product is
    rotated in the NTT domain WITHOUT P * c0, the NEXT sum is divided in the coefficient domain and x and the rotated c0 terms join
    there; the TAIL products gather in an extended accumulator and their c0 terms in tail_c0, divided and added after the last step"""
    o = ev.o
    L = level + 1
    x = np.array(ct, dtype=np.uint64)

    def add_rows(a, b, mi_of):
        return np.stack([np.stack([o.vec("add", mi_of(tl), a[pl, tl], b[pl, tl]) for tl in range(a.shape[1])]) for pl in range(2)])

    tail, tail_c0 = None, None
    for keys in steps_of(ev.n, step, count, radix, rows):
        c1n = np.stack([o.ntt(j, x[1, j]) for j in range(L)])
        nxt, c0_terms = None, []
        for g, dest in keys:
            prod = o.gadget_product(level, c1n, ev._key(g), ev.klvl)
            prod = np.stack([np.stack([o.automorph_ntt(g, prod[pl, tl]) for tl in range(prod.shape[1])]) for pl in range(2)])
            rot_c0 = np.stack([o.automorph_coeff(j, g, x[0, j]) for j in range(L)])
            if dest == "tail":
                tail = prod if tail is None else add_rows(tail, prod, lambda tl: ev._mi(level, tl))
                tail_c0 = rot_c0 if tail_c0 is None else np.stack([o.vec("add", j, tail_c0[j], rot_c0[j]) for j in range(L)])
            else:
                nxt = prod if nxt is None else add_rows(nxt, prod, lambda tl: ev._mi(level, tl))
                c0_terms.append(rot_c0)
        x = add_rows(x, _moddown_coeff(ev, level, nxt), lambda j: j)
        for r in c0_terms:
            x[0] = np.stack([o.vec("add", j, x[0, j], r[j]) for j in range(L)])
    if tail is not None:
        x = add_rows(x, _moddown_coeff(ev, level, tail), lambda j: j)
        x[0] = np.stack([o.vec("add", j, x[0, j], tail_c0[j]) for j in range(L)])
    return x


def plain_slot_sum(values, n_ring, step, count, rows, t):
    """the slot sum of the 2 x N/2 slot matrix mod t: values[0 : N/2] is row 0, values[N/2 :] row 1"""
    h = n_ring // 2
    v = np.asarray(values, dtype=np.int64).reshape(2, h)
    y = (v + v[::-1]) if rows else v
    out = np.zeros_like(y)
    for i in range(count):
        out = (out + np.roll(y, -i * step, axis=1)) % t
    return out.reshape(-1) % t
