"""CKKS polynomial evaluation on the device (lsa_poly_* / lsa_ckks_poly_eval, lattisense_amd/csrc/poly_eval.hip) against the CPU.
With log_baby = 1 the operator must reproduce the frozen oracle (oracle/ckks_bootstrap.py eval_chebyshev / eval_monomial, which
computes its own constants) word for word; for every other plan it must reproduce tests/poly_model.py, the restatement of the
Paterson-Stockmeyer recursion over the oracle's operators, which is handed the plan's integer constants so that both sides do
integer arithmetic only.  The plan's constants are compared with the model's own (at most one unit apart), its counts with the
model's planner, the message with numpy's chebval / polyval by the project's criterion (mean precision >= 10 bits), on one-pass,
whole-limb and two-pass rings, with both NTT engines and under every switch the operator's path reads.

Input scales sit at the size of the chain's primes (2^45 on the headline chain, 2^40 on the bootstrap chain's): a power's scale
is s^2 / q, so any other choice drifts by a factor that doubles with every squaring.

Measured on an MI355X box: the module takes about 25 s, most of it the oracle's walk at N = 2^16."""
import numpy as np
import pytest

from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

SWITCHES = ({"LSA_HMULT_FOLD": "0"}, {"LSA_KS_FUSED": "0"}, {"LSA_KSMAC_XCD": "0"})


def _chain(name):
    from lattisense_amd import params
    if name == "headline":                    # 13 Q limbs of the FP64 engine (q ~ 2^45 but q_0) + 4 P
        P = params.CKKS_DEFAULT[65536]
        return P["q"][:13], P["p"], float(2 ** 45)
    if name == "ceiling":                     # N = 2^13: every Q and P prime within 2^23 of 2^61 (tests/boundary.py)
        from tests.boundary import ceiling_chain
        C = ceiling_chain(1 << 13, 6, 2)
        return C["q"], C["p"], float(2 ** 61)
    B = params.CKKS_BOOTSTRAP_65536           # a 60-bit prime and 40-bit ones with 60/61-bit special primes: integer engine
    return B["q"][:8], B["p"], float(2 ** 40)


class Rig:
    def __init__(self, log_n, chain, seed):
        from lattisense_amd.device import ALGO_CKKS, DeviceContext
        from oracle.ckks_bootstrap import Evaluator
        from oracle.client import Client
        from oracle.pyoracle import Oracle
        self.q, self.p, self.scale = _chain(chain)
        self.N = 1 << log_n
        self.top = len(self.q) - 1
        self.o = Oracle(self.N, self.q, self.p, 0)
        self.c = Client(self.o, seed=seed)
        self.ctx = DeviceContext(ALGO_CKKS, self.N, self.q, self.p)
        self.ev = Evaluator(self.o, self.c, self.top)          # generates the relinearisation key
        self.rlk = self.ctx.upload_key(self.ev.rlk, self.top)


def _reference(basis, coeffs, x, interval):
    a, b = interval
    u = (2 * x - a - b) / (b - a)
    if basis == "chebyshev":
        return np.polynomial.chebyshev.chebval(u, coeffs)
    return np.polynomial.polynomial.polyval(u, coeffs)


def _check(rig, coeffs, basis, log_baby, level=None, interval=(-1, 1), scale_out=None, batch=1, pin=False, env_variants=(),
           fp64_variants=(1,), monkeypatch=None, seed=0, chunk_mib=0):
    """device == restatement (== frozen oracle when `pin`) word for word; counts, constants, message; switch variants.
    chunk_mib: one more run under lsa_set_ntt_chunk_mib, the same words (every batch item of `got` was held to the restatement)"""
    from lattisense_amd.device import PolynomialPlan
    from oracle.ckks_bootstrap import Ct, eval_chebyshev, eval_monomial
    from oracle.client import mean_precision_bits
    from tests import poly_model as pm
    N, c, ctx, ev = rig.N, rig.c, rig.ctx, rig.ev
    level = rig.top if level is None else level
    has_interval = tuple(interval) != (-1, 1)
    plan = PolynomialPlan(ctx, coeffs, level, rig.scale, basis=basis, interval=interval, scale_out=scale_out, log_baby=log_baby)
    want_plan = pm.plan(coeffs, basis, log_baby, has_interval)
    got_plan = {"depth": plan.depth, "log_baby": plan.log_baby, "mults": plan.mults, "leaves": plan.leaves,
                "leaf_launches": plan.leaf_launches}
    assert got_plan == want_plan
    assert plan.level_in == level and plan.level_out == level - plan.depth
    assert plan.scale_out == (float(scale_out) if scale_out else float(rig.o.mod[plan.level_out + 1]))
    rng = np.random.default_rng(500 + seed)
    half_width = (interval[1] - interval[0]) / 2.0
    zs = [rng.uniform(-1, 1, N // 2) * half_width + (interval[0] + interval[1]) / 2.0 + 0j for _ in range(batch)]
    cts = np.stack([c.ckks_encrypt(z, level, rig.scale) for z in zs])
    xin = ctx.upload(cts)
    shape = (batch, 2, plan.level_out + 1, N)
    got = ctx.download(plan.run(xin, batch, rig.rlk), shape)
    consts = plan.constants()
    assert len(consts) == plan.n_constants
    for b in range(batch):
        x = Ct(cts[b], level, rig.scale)
        mults_before = ev.counts["mult"]
        want, own = pm.evaluate(ev, x, coeffs, basis, interval, scale_out, log_baby, constants=consts)
        assert ev.counts["mult"] - mults_before == plan.mults
        assert want.data.shape == got[b].shape
        assert np.array_equal(got[b], want.data), "batch item %d differs from the restatement" % b
        assert len(own) == len(consts)
        worst = max(abs(a - k) for a, k in zip(own, consts))
        assert worst <= 1, "a plan constant is %d units from the independently computed one" % worst
        if pin:
            frozen = (eval_chebyshev if basis == "chebyshev" else eval_monomial)(ev, x, np.asarray(coeffs, dtype=np.float64))
            assert frozen.level == plan.level_out and frozen.scale == plan.scale_out
            assert np.array_equal(got[b], frozen.data), "batch item %d differs from the frozen oracle" % b
        re, _ = mean_precision_bits(_reference(basis, coeffs, zs[b], interval), c.ckks_decrypt(got[b], plan.scale_out))
        print("%s %d terms log_baby %d: %d multiplications, %d leaves in %d launches, precision %.1f bits"
              % (basis, len(coeffs), plan.log_baby, plan.mults, plan.leaves, plan.leaf_launches, re))
        assert re >= 10, re
    for fp in fp64_variants:
        for env in ({},) + tuple(env_variants):
            if fp == 1 and not env:
                continue
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            ctx.set_fp64_ntt(fp)
            alt = ctx.download(plan.run(xin, batch, rig.rlk), shape)
            ctx.set_fp64_ntt(1)
            for k in env:
                monkeypatch.delenv(k)
            assert np.array_equal(alt, got), (env, fp)
    if chunk_mib:
        ctx.set_ntt_chunk_mib(chunk_mib)
        try:
            alt = ctx.download(plan.run(xin, batch, rig.rlk), shape)
        finally:
            ctx.set_ntt_chunk_mib(0)
        assert np.array_equal(alt, got), ("ntt chunk", chunk_mib)
    info = got_plan
    plan.close()
    return info


def _dense(rng, n):
    return rng.uniform(-1, 1, n) / n


@pytest.mark.parametrize("basis", ["chebyshev", "monomial"])
def test_log_baby_1_is_the_frozen_oracle(basis):
    """dense random coefficients of 4, 8, 32 terms: the oracle computes its own constants, so this pins them too"""
    need_gpu()
    from tests import poly_model as pm
    rig = Rig(12, "headline", 71)
    rng = np.random.default_rng(11)
    for n in (4, 8, 32):
        info = _check(rig, _dense(rng, n), basis, 1, pin=True, seed=n)
        k = n.bit_length() - 1
        assert info["mults"] == pm.binary_splitting_mults(k) and info["leaves"] == n // 2


CASES = [
    ("dense16", lambda r: _dense(r, 16), {}, (0, 3)),
    ("dense32", lambda r: _dense(r, 32), {}, (0, 2, 3, 4)),
    ("dense64", lambda r: _dense(r, 64), {}, (0, 3, 4)),
    ("degree40", lambda r: _dense(r, 41), {}, (0, 2, 3, 4)),
    ("odd31", lambda r: np.where(np.arange(32) % 2 == 1, _dense(r, 32), 0.0), {}, (0, 3)),
    ("upper_half_zero", lambda r: np.concatenate([_dense(r, 16), np.zeros(16)]), {}, (0, 3)),
    ("interval", lambda r: _dense(r, 16), {"interval": (-8, 8)}, (0, 3)),
    ("scale_out", lambda r: _dense(r, 16), {"scale_out": 2.0 ** 38}, (0, 2)),
    ("batch3", lambda r: _dense(r, 32), {"batch": 3}, (3,)),
]


@pytest.mark.parametrize("basis", ["chebyshev", "monomial"])
@pytest.mark.parametrize("name,make,kw,babies", CASES, ids=[c[0] for c in CASES])
def test_new_ground_against_the_restatement(basis, name, make, kw, babies, monkeypatch):
    """N = 2^12 on the headline chain at level 12; the first log_baby of every case also runs under the switches and on the
    integer NTT engine"""
    need_gpu()
    rig = Rig(12, "headline", 72)
    coeffs = make(np.random.default_rng(len(name)))
    for i, b in enumerate(babies):
        _check(rig, coeffs, basis, b, env_variants=SWITCHES if i == 0 else (), fp64_variants=(1, 0) if i == 0 else (1,),
               monkeypatch=monkeypatch, seed=b, **kw)


def test_planner_choice_beats_binary_splitting_on_the_device():
    need_gpu()
    from tests import poly_model as pm
    rig = Rig(12, "headline", 73)
    rng = np.random.default_rng(13)
    info = _check(rig, _dense(rng, 64), "chebyshev", 0, seed=1)
    assert info["mults"] == 18 and info["mults"] < pm.binary_splitting_mults(6) == 36


@pytest.mark.parametrize("log_n", [13, 14])
def test_whole_limb_rings(log_n, monkeypatch):
    """N = 2^13 / 2^14: whole-limb transform plans; batch 3 in tiles of 2 (uneven last tile), once more with the two-pass
    transforms cut into 1 MiB chunks"""
    need_gpu()
    rig = Rig(log_n, "headline", 60 + log_n)
    rng = np.random.default_rng(log_n)
    rig.ctx.set_tile_batch(2)
    _check(rig, _dense(rng, 32), "chebyshev", 3, batch=3, env_variants=SWITCHES, fp64_variants=(1, 0), monkeypatch=monkeypatch, seed=1,
           chunk_mib=1)
    rig.ctx.set_tile_batch(0)
    _check(rig, _dense(rng, 32), "monomial", 0, env_variants=SWITCHES[:1], monkeypatch=monkeypatch, seed=2)


def test_two_pass_ring(monkeypatch):
    """N = 2^16 on the headline chain, 32 terms, log_baby = 3: odd Chebyshev powers 3, 5, 7 and grouped leaves on a two-pass ring"""
    need_gpu()
    rig = Rig(16, "headline", 81)
    rng = np.random.default_rng(16)
    _check(rig, _dense(rng, 32), "chebyshev", 3, env_variants=SWITCHES, fp64_variants=(1, 0), monkeypatch=monkeypatch, seed=3)


def test_bootstrap_chain_primes(monkeypatch):
    """the first 8 primes of the bootstrap chain (60-bit q_0, 60/61-bit special primes: integer engine, unfused key MAC), 8 terms"""
    need_gpu()
    rig = Rig(13, "bootstrap8", 82)
    rng = np.random.default_rng(17)
    _check(rig, _dense(rng, 8), "chebyshev", 0, env_variants=SWITCHES, fp64_variants=(1, 0), monkeypatch=monkeypatch, seed=4)
    _check(rig, _dense(rng, 8), "monomial", 3, seed=5)
    _check(rig, _dense(rng, 8), "chebyshev", 1, pin=True, seed=6)


def test_ceiling_chain(monkeypatch):
    """N = 2^13, six Q limbs and two special primes at the 61-bit ceiling, scale 2^61: the moduli of k_poly_lincomb, of the
    tensor and of the key switch at the ceiling (the constants are the plan's, not worst-case residues)"""
    need_gpu()
    rig = Rig(13, "ceiling", 83)
    rng = np.random.default_rng(18)
    _check(rig, _dense(rng, 8), "chebyshev", 0, env_variants=SWITCHES, fp64_variants=(1, 0), monkeypatch=monkeypatch, seed=7)
    _check(rig, _dense(rng, 8), "monomial", 1, pin=True, seed=8)


def test_batch_positions_and_strides():
    """the same ciphertext at two batch positions gives the same words; padded batch strides are honoured"""
    need_gpu()
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import PolynomialPlan
    rig = Rig(12, "headline", 74)
    rng = np.random.default_rng(5)
    N, lvl = rig.N, 8
    plan = PolynomialPlan(rig.ctx, _dense(rng, 16), lvl, rig.scale, log_baby=3)
    lo = plan.level_out + 1
    za, zb = [rng.uniform(-1, 1, N // 2) + 0j for _ in range(2)]
    a, b = rig.c.ckks_encrypt(za, lvl, rig.scale), rig.c.ckks_encrypt(zb, lvl, rig.scale)
    got = rig.ctx.download(plan.run(rig.ctx.upload(np.stack([a, b, a])), 3, rig.rlk), (3, 2, lo, N))
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1])
    pad, L = 3 * N, lvl + 1
    xin = np.zeros((2, 2 * L * N + pad), dtype=np.uint64)
    xin[0, : 2 * L * N], xin[1, : 2 * L * N] = a.ravel(), b.ravel()
    out = rig.ctx.alloc(2 * (2 * lo * N + pad))
    check(lib().lsa_ckks_poly_eval(rig.ctx.h, plan.h, rig.ctx.upload(xin).ptr, out.ptr, 2, 2 * L * N + pad, 2 * lo * N + pad, rig.rlk,
                                   rig.ctx.stream))
    strided = rig.ctx.download(out, (2, 2 * lo * N + pad))
    assert np.array_equal(strided[0, : 2 * lo * N].reshape(2, lo, N), got[0])
    assert np.array_equal(strided[1, : 2 * lo * N].reshape(2, lo, N), got[1])
    plan.close()


def test_argument_errors_and_missing_key():
    need_gpu()
    from lattisense_amd import params
    from lattisense_amd._native import LsaError
    from lattisense_amd.device import ALGO_BFV, DeviceContext, PolynomialPlan
    rig = Rig(12, "headline", 75)
    rng = np.random.default_rng(6)
    ctx, N = rig.ctx, rig.N
    good = _dense(rng, 16)

    def fails(fn, needle="poly"):
        with pytest.raises(LsaError) as e:
            fn()
        assert e.value.code == 1, e.value
        assert needle in str(e.value), e.value
    fails(lambda: PolynomialPlan(ctx, good, 3, rig.scale), "levels")                      # depth 4 from level 3
    fails(lambda: PolynomialPlan(ctx, good, 4, rig.scale, interval=(-2, 2)), "levels")    # the interval costs one more
    fails(lambda: PolynomialPlan(ctx, good, 13, rig.scale), "level out of range")
    fails(lambda: PolynomialPlan(ctx, [0.5], 12, rig.scale), "degree 0")
    fails(lambda: PolynomialPlan(ctx, [0.5, 0.0, 0.0], 12, rig.scale), "degree 0")
    fails(lambda: PolynomialPlan(ctx, good, 12, rig.scale, log_baby=5), "log_baby")
    fails(lambda: PolynomialPlan(ctx, good, 12, rig.scale, interval=(1, -1)), "interval")
    fails(lambda: PolynomialPlan(ctx, good * 1e12, 12, rig.scale), "out of range")        # a constant beyond 2^62
    B = params.BFV_DEFAULT[8192]
    bfv = DeviceContext(ALGO_BFV, 8192, B["q"], B["p"], B["t"])
    fails(lambda: PolynomialPlan(bfv, good, 0, rig.scale), "CKKS")
    bfv.close()
    plan = PolynomialPlan(ctx, good, 12, rig.scale)
    ct = rig.c.ckks_encrypt(rng.uniform(-1, 1, N // 2) + 0j, 12, rig.scale)
    xin = ctx.upload(ct[None])
    shape = (1, 2, plan.level_out + 1, N)
    ref = ctx.download(plan.run(xin, 1, rig.rlk), shape)
    fails(lambda: plan.run(xin, 1, None), "relinearisation key")
    low = ctx.upload_key(rig.c.gen_relin_key(5), 5)
    fails(lambda: plan.run(xin, 1, low), "relinearisation key")                           # a key below the input level
    fails(lambda: plan.run(xin, 1, rig.rlk, out=xin), "overlaps")
    assert np.array_equal(ctx.download(plan.run(xin, 1, rig.rlk), shape), ref)            # the context and the plan stay usable
    sentinel = ctx.upload(np.full(2 * (plan.level_out + 1) * N, 7, dtype=np.uint64))
    plan.run(xin, 0, rig.rlk, out=sentinel)                                               # batch <= 0: a no-op
    assert np.all(ctx.download(sentinel, (2 * (plan.level_out + 1) * N,)) == 7)
    plan.close()
