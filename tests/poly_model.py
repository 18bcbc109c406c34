"""CPU restatement of the polynomial evaluator (lattisense_amd/csrc/poly_eval.hip) over
oracle.ckks_bootstrap.Evaluator: the Paterson-Stockmeyer plan (counts only: `plan`) and its evaluation (`evaluate`), which takes
the device plan's integer constants when given (then both sides do integer arithmetic only) and computes its own otherwise.

Recursion (k = ceil(log2(len)), b = log_baby, L = level of u):
  powers   P_1 = u, P_j = P_ceil(j/2) (x) P_floor(j/2), level L - ceil(log2 j); only those a node or a needed power uses.
           monomial: ev.mul.  Chebyshev even: 2 P_a^2 - 1.  Chebyshev odd: rescale(2 relin(P_a (x) P_c) - K u), K = round(s_a s_c / s_u).
  rec(c, level_out, scale_out): a node of degree < 2^b whose powers (non-zero coefficients) sit at level >= level_out + 1 is a
           LEAF: rescale(sum_j K_j P_j[rows <= level_out + 1]) + round(c_0 scale_out), K_j = round(c_j (scale_out q / s_j)).
           Otherwise hi * P_half + lo (Chebyshev: the oracle's fold-back); an all-zero hi: rec(lo); a constant hi: the one-term
           leaf hi_0 P_half instead of a multiplication; a constant lo: add_const.
"""
import numpy as np

from oracle.ckks_bootstrap import Ct

MAX_OUT, MAX_SRC = 8, 15      # outputs / sources of one leaf launch


def _clog2(x):
    return (x - 1).bit_length()


def _shape(v):
    return 2 if any(x != 0.0 for x in v[1:]) else (1 if v[0] != 0.0 else 0)


def pad(coeffs):
    k = max(1, _clog2(len(coeffs)))
    c = np.zeros(1 << k)
    c[: len(coeffs)] = np.asarray(coeffs, dtype=np.float64)
    return c, k


def split(c, basis):
    half = len(c) // 2
    if basis == "chebyshev":
        hi = np.zeros(half)
        lo = np.array(c[:half], dtype=np.float64)
        hi[0] = c[half]
        for j in range(1, half):                  # T_{half+j} = 2 T_half T_j - T_{half-j}
            hi[j] = 2 * c[half + j]
            lo[half - j] -= c[half + j]
        return hi, lo
    return np.array(c[half:], dtype=np.float64), np.array(c[:half], dtype=np.float64)


class Structure:
    """the tree, the leaf jobs and the needed powers of one (coefficients, b); level arithmetic relative to L = 0"""

    def __init__(self, coeffs, basis, b):
        self.c, self.k = pad(coeffs)
        assert _shape(self.c) == 2, "degree 0"
        self.basis, self.b = basis, b
        self.jobs, self.nodes, self.needed, self.mults = [], [], set(), 0
        self.mult_levels = []                      # level of every multiplication, relative to the level of u
        self.root = self.rec(self.c, -self.k)
        for j in range(len(self.c) - 1, 1, -1):
            if j in self.needed:
                self.needed |= {(j + 1) // 2, j // 2}
        self.needed.discard(1)
        self.mults += len(self.needed)
        self.mult_levels += [min(self.plevel((j + 1) // 2), self.plevel(j // 2)) for j in sorted(self.needed)]
        self.groups = []
        by_level = {}
        for i, job in enumerate(self.jobs):
            by_level.setdefault(job["level"], []).append(i)
        for level in sorted(by_level):
            cur, src = [], []
            for i in by_level[level]:
                new = src + [j for j, _ in self.jobs[i]["terms"] if j not in src]
                if cur and (len(cur) == MAX_OUT or len(new) > MAX_SRC):
                    self.groups.append(cur)
                    cur, new = [], [j for j, _ in self.jobs[i]["terms"]]
                cur, src = cur + [i], new
            self.groups.append(cur)

    @staticmethod
    def plevel(j):
        return -_clog2(j)

    def rec(self, c, level_out):
        deg = max(j for j in range(len(c)) if c[j] != 0.0)
        if deg < (1 << self.b) and all(c[j] == 0.0 or self.plevel(j) >= level_out + 1 for j in range(1, deg + 1)):
            terms = [(j, float(c[j])) for j in range(1, deg + 1) if c[j] != 0.0]
            self.needed |= {j for j, _ in terms}
            self.jobs.append({"level": level_out, "terms": terms, "c0": float(c[0])})
            return ("job", len(self.jobs) - 1)
        assert len(c) > 2
        half = len(c) // 2
        hi, lo = split(c, self.basis)
        sh, sl = _shape(hi), _shape(lo)
        if sh == 0:
            return self.rec(lo, level_out)
        assert self.plevel(half) >= level_out + 1
        self.needed.add(half)
        node = {"half": half, "level": level_out, "hi": None, "lo": None, "hi_is_product": sh == 1, "lo_const": None}
        self.nodes.append(node)
        idx = len(self.nodes) - 1
        if sh == 1:
            self.jobs.append({"level": level_out, "terms": [(half, float(hi[0]))], "c0": 0.0})
            node["hi"] = ("job", len(self.jobs) - 1)
        else:
            node["hi"] = self.rec(hi, level_out + 1)
            self.mults += 1
            self.mult_levels.append(level_out + 1)
        if sl == 1:
            node["lo_const"] = float(lo[0])
        elif sl == 2:
            node["lo"] = self.rec(lo, level_out)
        return ("node", idx)


def plan(coeffs, basis="chebyshev", log_baby=0, interval=False):
    """{depth, log_baby, mults, leaves, leaf_launches}: what lsa_poly_plan reports"""
    _, k = pad(coeffs)
    if log_baby:
        st = Structure(coeffs, basis, min(log_baby, k))
    else:
        st = min((Structure(coeffs, basis, b) for b in range(1, min(4, k) + 1)), key=lambda s: (s.mults, s.b))
    return {"depth": k + (1 if interval else 0), "log_baby": st.b, "mults": st.mults, "leaves": len(st.jobs),
            "leaf_launches": len(st.groups)}


def binary_splitting_mults(k):
    """ciphertext multiplications of oracle.ckks_bootstrap.eval_chebyshev / eval_monomial for 2^k dense coefficients"""
    return (1 << (k - 1)) + k - 2


class _Constants:
    def __init__(self, given):
        self.given, self.pos, self.own = given, 0, []

    def take(self, computed):
        computed = int(computed)
        self.own.append(computed)
        if self.given is None:
            return computed
        v = self.given[self.pos]
        self.pos += 1
        return v


def _lincomb(ev, level, terms, consts):
    """sum K * ct[rows <= level] over (K, ct) pairs, limb by limb"""
    acc = None
    for kk, ct in terms:
        d = ev.mul_int(ev.drop(ct, level), kk)
        acc = d if acc is None else Ct(ev.add(Ct(acc.data, level, 1.0), Ct(d.data, level, 1.0)).data, level, 1.0)
    return acc.data


def _add_int(ev, ct, k):
    d = ct.data.copy()
    for j in range(ct.level + 1):
        d[0, j] = ev.o.vec("add", j, d[0, j], ev._const(k, j))
    return Ct(d, ct.level, ct.scale)


def evaluate(ev, x, coeffs, basis="chebyshev", interval=(-1, 1), scale_out=None, log_baby=0, constants=None):
    """(result Ct, every integer constant in the plan's order); x: Ct at the input level and scale"""
    q = lambda lvl: float(ev.q(lvl))
    K = _Constants(constants)
    has_interval = tuple(interval) != (-1, 1)
    b = plan(coeffs, basis, log_baby, has_interval)["log_baby"]
    st = Structure(coeffs, basis, b)
    u = x
    if has_interval:
        a, bb = float(interval[0]), float(interval[1])
        cs = q(x.level)
        t = ev.mul_int(x, K.take(round(2.0 / (bb - a) * cs)))
        t = ev.rescale(Ct(t.data, t.level, x.scale * cs))
        u = _add_int(ev, t, K.take(round(-(a + bb) / (bb - a) * t.scale)))
    L = u.level
    assert L - st.k >= 0
    P = {1: u}
    for j in sorted(st.needed):
        pa, pc = P[(j + 1) // 2], P[j // 2]
        if basis == "monomial":
            P[j] = ev.mul(pa, pc)
        elif j % 2 == 0:
            sq = ev.mul(pa, pa)
            P[j] = _add_int(ev, ev.mul_int(sq, 2), K.take(round(-1.0 * sq.scale)))
        else:
            lam = min(pa.level, pc.level)
            d3 = ev.o.ckks_mult(lam, ev.drop(pa, lam).data, ev.drop(pc, lam).data)
            prod = Ct(ev.o.ckks_relin(lam, d3, ev.rlk, ev.klvl), lam, pa.scale * pc.scale)
            ev.counts["mult"] += 1
            kk = K.take(round(pa.scale * pc.scale / u.scale))
            diff = _lincomb(ev, lam, [(2, prod), (-kk, u)], K)
            P[j] = ev.rescale(Ct(diff, lam, prod.scale))
        assert P[j].level == L + Structure.plevel(j)
    # target scales, top down
    level_out = L - st.k
    top_scale = float(scale_out) if scale_out else q(level_out + 1)

    def assign(v, sc):
        if v is None:
            return
        if v[0] == "job":
            st.jobs[v[1]]["scale"] = sc
            return
        n = st.nodes[v[1]]
        n["scale"] = sc
        assign(n["hi"], sc if n["hi_is_product"] else sc * q(L + n["level"] + 1) / P[n["half"]].scale)
        assign(n["lo"], sc)
    assign(st.root, top_scale)
    out = []
    for job in st.jobs:
        lam, sc = L + job["level"], job["scale"]
        terms = [(K.take(round(cj * (sc * q(lam + 1) / P[j].scale))), P[j]) for j, cj in job["terms"]]
        r = ev.rescale(Ct(_lincomb(ev, lam + 1, terms, K), lam + 1, sc * q(lam + 1)))
        r = Ct(r.data, lam, sc)
        if job["c0"] != 0.0:
            r = _add_int(ev, r, K.take(round(job["c0"] * sc)))
        out.append(r)
    for n in st.nodes:
        if n["lo_const"] is not None:
            n["k0"] = K.take(round(n["lo_const"] * n["scale"]))

    def run(v):
        if v[0] == "job":
            return out[v[1]]
        n = st.nodes[v[1]]
        prod = run(n["hi"])
        if not n["hi_is_product"]:
            prod = ev.mul(prod, P[n["half"]])
        prod = Ct(prod.data, prod.level, n["scale"])
        if n["lo_const"] is not None:
            prod = _add_int(ev, prod, n["k0"])
        return ev.add(prod, run(n["lo"])) if n["lo"] is not None else prod
    y = run(st.root)
    assert y.level == level_out
    return Ct(y.data, y.level, top_scale), K.own
