"""CKKS linear transform on the device (lsa_lt_* / lsa_ckks_linear_transform, lattisense_amd/csrc/linear_transform.hip) against
its oracle (oracle/ckks_bootstrap.py linear_transform).  The plan's encoded diagonals are handed to the oracle, after which
both sides do integer arithmetic only: the result must be identical word for word, for every plan shape (no split, one 8 x 8
block, blocked in one or both directions, giant steps only, sparse packing), on one-pass, whole-limb and two-pass rings, with
both NTT engines and under every switch.  The message is checked with the project's criterion (mean precision >= 10 bits) and
the encoder against the oracle's own encoder.

Measured on an MI355X box: the module takes about a minute, most of it the oracle's walk at N = 2^16."""
import numpy as np
import pytest

from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

D40 = float(2 ** 40)


def _chain(name):
    from lattisense_amd import params
    if name == "headline":                    # 13 Q limbs of the FP64 engine (q < 2^47 but q_0) + 4 P
        P = params.CKKS_DEFAULT[65536]
        return P["q"][:13], P["p"]
    if name == "ceiling":                     # N = 2^13: every Q and P prime within 2^23 of 2^61 (tests/boundary.py)
        from tests.boundary import ceiling_chain
        C = ceiling_chain(1 << 13, 4, 2)
        return C["q"], C["p"]
    B = params.CKKS_BOOTSTRAP_65536           # 60- and 61-bit primes next to 40-bit ones: integer engine, unfused key MAC
    return B["q"][:8], B["p"]


class Rig:
    def __init__(self, log_n, chain, seed):
        from lattisense_amd.device import ALGO_CKKS, DeviceContext
        from oracle.ckks_bootstrap import Evaluator
        from oracle.client import Client
        from oracle.pyoracle import Oracle
        self.q, self.p = _chain(chain)
        self.N = 1 << log_n
        self.top = len(self.q) - 1
        self.o = Oracle(self.N, self.q, self.p, 0)
        self.c = Client(self.o, seed=seed)
        self.ctx = DeviceContext(ALGO_CKKS, self.N, self.q, self.p)
        self.ev = Evaluator.__new__(Evaluator)          # no relinearisation key needed
        self.ev.o, self.ev.c, self.ev.klvl, self.ev.n = self.o, self.c, self.top, self.N
        self.ev.glk, self.ev.counts = {}, {"rotate": 0, "mult": 0, "mul_plain": 0}
        self.dev_keys = {}

    def keys_for(self, elements):
        for e in elements:
            if e not in self.ev.glk:
                self.ev.glk[e] = self.c.gen_galois_key(e, self.top)
            if e not in self.dev_keys:
                self.dev_keys[e] = self.ctx.upload_key(self.ev.glk[e], self.top)
        return {e: self.dev_keys[e] for e in elements}


def _diags(rng, index, period):
    d = len(index)
    return {k: (rng.uniform(-1, 1, period) + 1j * rng.uniform(-1, 1, period)) / d for k in index}


def _reduced(diags, period):
    return {k % period: v for k, v in diags.items()}


def _check(rig, level, diags, period, ratio=2.0, double_hoist=True, rescale=True, batch=1, n1=None, env_variants=(),
           monkeypatch=None, fp64_variants=(1,), seed=0, chunk_mib=0):
    """device == oracle word for word; the switch variants == the default run; message precision; returns the plan's info.
    chunk_mib: one more run under lsa_set_ntt_chunk_mib, the same words (every batch item of `got` was held to the oracle)"""
    from lattisense_amd.device import LinearTransformPlan
    from oracle.ckks_bootstrap import Ct, apply_plain, linear_transform, rotations_of
    from oracle.client import galois_element_for_col_rotation, mean_precision_bits
    N, o, c, ctx, ev = rig.N, rig.o, rig.c, rig.ctx, rig.ev
    plan = LinearTransformPlan(ctx, level, diags, log_slots=period.bit_length() - 1, ratio=ratio, double_hoist=double_hoist)
    red = _reduced(diags, period)
    assert plan.diagonals == sorted(red) and plan.period == period and plan.level == level
    if n1 is not None:
        assert plan.n1 == n1                                          # through lsa_lt_info
    assert plan.rows == level + 1 + (len(rig.p) if double_hoist and len(red) >= 3 else 0)
    assert plan.pt_scale == float(o.mod[level])
    want_rot = rotations_of(red, period, ratio)
    assert plan.galois_elements == sorted(galois_element_for_col_rotation(r, N) for r in want_rot)
    glk = rig.keys_for(plan.galois_elements)
    rng = np.random.default_rng(1000 + seed)
    zs = [rng.uniform(-1, 1, period) + 1j * rng.uniform(-1, 1, period) for _ in range(batch)]
    cts = np.stack([c.ckks_encrypt(np.tile(z, (N // 2) // period), level, D40) for z in zs])
    xin = ctx.upload(cts)
    lo = level if rescale else level + 1
    got = ctx.download(plan.run(xin, batch, glk, rescale=rescale), (batch, 2, lo, N))
    plains = plan.oracle_plains()
    before = set(ev.glk)
    for b in range(batch):
        want = linear_transform(ev, Ct(cts[b], level, D40), red, ratio, plains=plains, rescale=rescale, n_slots=period,
                                double_hoist=double_hoist)
        assert want.data.shape == got[b].shape
        assert np.array_equal(got[b], want.data), "batch item %d differs from the oracle" % b
        scale = D40 * plan.pt_scale / (float(o.mod[level]) if rescale else 1.0)
        re, im = mean_precision_bits(apply_plain(red, zs[b]), c.ckks_decrypt(got[b], scale)[:period])
        assert re >= 10 and im >= 10, (re, im)
    assert set(ev.glk) == before                                      # the oracle run needed no other key
    for fp in fp64_variants:
        for env in env_variants:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            ctx.set_fp64_ntt(fp)
            alt = ctx.download(plan.run(xin, batch, glk, rescale=rescale), (batch, 2, lo, N))
            ctx.set_fp64_ntt(1)
            for k in env:
                monkeypatch.delenv(k)
            assert np.array_equal(alt, got), (env, fp)
    if chunk_mib:
        ctx.set_ntt_chunk_mib(chunk_mib)
        try:
            alt = ctx.download(plan.run(xin, batch, glk, rescale=rescale), (batch, 2, lo, N))
        finally:
            ctx.set_ntt_chunk_mib(0)
        assert np.array_equal(alt, got), ("ntt chunk", chunk_mib)
    info = (plan.n1, plan.rows)
    plan.close()
    return info


SWITCHES = ({}, {"LSA_ROT_SCATTER": "0"}, {"LSA_LT_BLOCKED_MAC": "0"}, {"LSA_LT_GIANT_SCATTER": "0"}, {"LSA_LT_GIANT_SCATTER": "1"})


def test_one_pass_ring_every_shape(monkeypatch):
    """N = 2^12 on the headline chain at level 12"""
    need_gpu()
    rig = Rig(12, "headline", 21)
    rng = np.random.default_rng(2)
    P = 1 << 11
    lvl = 12
    _check(rig, lvl, _diags(rng, [0, 5], P), P, env_variants=SWITCHES, monkeypatch=monkeypatch, seed=1)            # no split
    _check(rig, lvl, _diags(rng, range(-3, 4), P), P, env_variants=SWITCHES, monkeypatch=monkeypatch, fp64_variants=(1, 0), seed=2)
    _check(rig, lvl, _diags(rng, range(-3, 4), P), P, rescale=False, seed=3)
    _check(rig, lvl, _diags(rng, range(-3, 4), P), P, double_hoist=False, env_variants=SWITCHES, monkeypatch=monkeypatch, seed=4)
    _check(rig, lvl, _diags(rng, range(64), P), P, n1=8, env_variants=SWITCHES, monkeypatch=monkeypatch, seed=5)    # 8 x 8: one launch
    _check(rig, lvl, _diags(rng, range(0, 2017, 32), P), P, env_variants=SWITCHES[1:3], monkeypatch=monkeypatch, seed=6)   # giant steps only
    _check(rig, 1, _diags(rng, range(-3, 4), P), P, env_variants=SWITCHES, monkeypatch=monkeypatch, seed=7)        # level 1: one digit


def test_wide_matrices_blocked_inner_sums(monkeypatch):
    """0..199: 16 babies x 13 giants at ratio 2 (blocked in both directions), 8 x 25 at ratio 1 (blocked in one); double- and
    single-hoisted; LSA_LT_BLOCKED_MAC=0 gives the same words"""
    need_gpu()
    rig = Rig(12, "headline", 22)
    rng = np.random.default_rng(3)
    P = 1 << 11
    d = _diags(rng, range(200), P)
    _check(rig, 12, d, P, ratio=2.0, n1=16, env_variants=SWITCHES, monkeypatch=monkeypatch, fp64_variants=(1, 0), seed=1)
    _check(rig, 12, d, P, ratio=1.0, n1=8, env_variants=SWITCHES[2:3], monkeypatch=monkeypatch, seed=2)
    _check(rig, 12, d, P, ratio=2.0, n1=16, double_hoist=False, rescale=False, env_variants=SWITCHES[2:3], monkeypatch=monkeypatch, seed=3)


def test_sparse_packing(monkeypatch):
    """log_slots = log2(N) - 3: diagonals of period N/8 tiled over the N/2 slots, index arithmetic modulo the period"""
    need_gpu()
    rig = Rig(12, "headline", 23)
    rng = np.random.default_rng(4)
    P = 1 << 9
    _check(rig, 12, _diags(rng, range(-5, 40), P), P, env_variants=SWITCHES[1:], monkeypatch=monkeypatch, seed=1)
    _check(rig, 12, _diags(rng, [0, -1], P), P, seed=2)


@pytest.mark.parametrize("log_n", [13, 14])
def test_whole_limb_rings(log_n, monkeypatch):
    """N = 2^13 / 2^14: whole-limb and seven-stage transform plans; batch 3 in tiles of 2 (uneven last tile), once more with the
    two-pass transforms cut into 1 MiB chunks (at 13 + 4 limbs: every item a chunk)"""
    need_gpu()
    rig = Rig(log_n, "headline", 30 + log_n)
    rng = np.random.default_rng(log_n)
    P = rig.N // 2
    rig.ctx.set_tile_batch(2)
    _check(rig, 12, _diags(rng, range(-3, 4), P), P, batch=3, env_variants=SWITCHES, monkeypatch=monkeypatch, fp64_variants=(1, 0), seed=1,
           chunk_mib=1)
    rig.ctx.set_tile_batch(0)
    if log_n == 14:
        _check(rig, 5, _diags(rng, range(200), P), P, n1=16, env_variants=SWITCHES[2:3], monkeypatch=monkeypatch, seed=2)
    else:
        _check(rig, 12, _diags(rng, range(64), P), P, n1=8, env_variants=SWITCHES[1:2], monkeypatch=monkeypatch, seed=2)


def test_ceiling_chain(monkeypatch):
    """N = 2^13, four Q limbs and two special primes at the 61-bit ceiling, plaintexts at the scale q_3: the moduli of
    k_mac_plain_multi, the scattering key MAC and the extended ModDown at the ceiling (the plaintext words are encoder outputs,
    not worst-case residues)"""
    need_gpu()
    rig = Rig(13, "ceiling", 61)
    rng = np.random.default_rng(61)
    P = rig.N // 2
    _check(rig, 3, _diags(rng, range(-3, 4), P), P, env_variants=SWITCHES, monkeypatch=monkeypatch, seed=61)
    _check(rig, 3, _diags(rng, range(64), P), P, n1=8, double_hoist=False, seed=62)


@pytest.mark.parametrize("chain,level,index", [("headline", 12, list(range(64))), ("headline", 12, list(range(200))),
                                                ("headline", 1, list(range(-3, 4))), ("bootstrap8", 7, list(range(-3, 4)))],
                         ids=["headline-l12-dense64", "headline-l12-dense200", "headline-l1-band", "bootstrap-primes-l7-band"])
def test_two_pass_ring(chain, level, index, monkeypatch):
    """N = 2^16 (k_ntt_r16; the fused key MAC on the headline chain, the integer engine and the unfused MAC on the bootstrap
    chain's primes): the scattering key MAC, k_permute_ext, the multi-sum kernel and the extended ModDown against the oracle
    on a two-pass ring"""
    need_gpu()
    rig = Rig(16, chain, 40 + level)
    rng = np.random.default_rng(level)
    P = rig.N // 2
    _check(rig, level, _diags(rng, index, P), P, n1=16 if len(index) == 200 else None, env_variants=SWITCHES[1:], monkeypatch=monkeypatch,
           fp64_variants=(1, 0) if level == 1 else (1,), seed=level)


def test_batch_position_independence_and_strides():
    """the same ciphertext at two batch positions gives the same words; padded batch strides are honoured"""
    need_gpu()
    import ctypes
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import LinearTransformPlan
    rig = Rig(12, "headline", 24)
    rng = np.random.default_rng(5)
    N, P, lvl = rig.N, 1 << 11, 6
    L = lvl + 1
    plan = LinearTransformPlan(rig.ctx, lvl, _diags(rng, range(20), P))
    glk = rig.keys_for(plan.galois_elements)
    za, zb = [rng.uniform(-1, 1, P) + 1j * rng.uniform(-1, 1, P) for _ in range(2)]
    a, b = rig.c.ckks_encrypt(za, lvl, D40), rig.c.ckks_encrypt(zb, lvl, D40)
    got = rig.ctx.download(plan.run(rig.ctx.upload(np.stack([a, b, a])), 3, glk), (3, 2, lvl, N))
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1])
    solo = rig.ctx.download(plan.run(rig.ctx.upload(b[None]), 1, glk), (1, 2, lvl, N))
    assert np.array_equal(solo[0], got[1])
    pad = 3 * N
    xin = np.zeros((2, 2 * L * N + pad), dtype=np.uint64)
    xin[0, : 2 * L * N], xin[1, : 2 * L * N] = a.ravel(), b.ravel()
    out = rig.ctx.alloc(2 * (2 * lvl * N + pad))
    elts = (ctypes.c_uint64 * len(glk))(*glk.keys())
    keys = (ctypes.c_void_p * len(glk))(*[k.value for k in glk.values()])
    xdev = rig.ctx.upload(xin)
    check(lib().lsa_ckks_linear_transform(rig.ctx.h, plan.h, xdev.ptr, out.ptr, 2, 2 * L * N + pad, 2 * lvl * N + pad,
                                          1, len(glk), elts, keys, rig.ctx.stream))
    strided = rig.ctx.download(out, (2, 2 * lvl * N + pad))
    assert np.array_equal(strided[0, : 2 * lvl * N].reshape(2, lvl, N), got[0])
    assert np.array_equal(strided[1, : 2 * lvl * N].reshape(2, lvl, N), got[1])
    plan.close()


def test_argument_errors_and_missing_key():
    need_gpu()
    import ctypes
    from lattisense_amd import params
    from lattisense_amd._native import LsaError, check, lib
    from lattisense_amd.device import ALGO_BFV, DeviceContext, LinearTransformPlan
    rig = Rig(12, "headline", 25)
    rng = np.random.default_rng(6)
    ctx, N, P, lvl = rig.ctx, rig.N, 1 << 11, 4
    good = _diags(rng, range(10), P)

    def fails(fn, needle=None):
        with pytest.raises(LsaError) as e:
            fn()
        assert e.value.code == 1, e.value
        if needle:
            assert needle in str(e.value), e.value
    fails(lambda: LinearTransformPlan(ctx, 13, good))                                  # level out of range
    fails(lambda: LinearTransformPlan(ctx, -1, good))
    fails(lambda: LinearTransformPlan(ctx, lvl, _diags(rng, [0, 1], 1 << 12), log_slots=12))   # log_slots > log2(N) - 1
    fails(lambda: LinearTransformPlan(ctx, lvl, {3: good[3], 3 + P: good[4]}), "repeats")       # duplicate after reduction
    fails(lambda: LinearTransformPlan(ctx, lvl, good, pt_scale=2.0 ** 70), "out of range")      # encodes beyond 2^62
    B = params.BFV_DEFAULT[8192]
    bfv = DeviceContext(ALGO_BFV, 8192, B["q"], B["p"], B["t"])
    fails(lambda: LinearTransformPlan(bfv, 0, _diags(rng, [0, 1], 1 << 12)), "CKKS")
    bfv.close()
    plan = LinearTransformPlan(ctx, lvl, good)
    glk = rig.keys_for(plan.galois_elements)
    ct = rig.c.ckks_encrypt(rng.uniform(-1, 1, P) + 0j, lvl, D40)
    xin = ctx.upload(ct[None])
    ref = ctx.download(plan.run(xin, 1, glk), (1, 2, lvl, N))
    missing = plan.galois_elements[-1]
    fails(lambda: plan.run(xin, 1, {e: k for e, k in glk.items() if e != missing}), str(missing))
    assert np.array_equal(ctx.download(plan.run(xin, 1, glk), (1, 2, lvl, N)), ref)    # the context and the plan stay usable
    fails(lambda: plan.run(xin, 1, glk, out=xin), "overlaps")
    sentinel = ctx.upload(np.full(2 * lvl * N, 7, dtype=np.uint64))
    plan.run(xin, 0, glk, out=sentinel)                                                # batch <= 0: a no-op
    assert np.all(ctx.download(sentinel, (2 * lvl * N,)) == 7)
    other = Rig(12, "headline", 26)
    elts = (ctypes.c_uint64 * 1)(0)
    keys = (ctypes.c_void_p * 1)(None)
    with pytest.raises(LsaError) as e:
        check(lib().lsa_ckks_linear_transform(other.ctx.h, plan.h, xin.ptr, sentinel.ptr, 1, 2 * (lvl + 1) * N, 2 * lvl * N, 1, 0, elts,
                                              keys, None))
    assert e.value.code == 1
    plan.close()


def test_encoder_against_the_oracles_own():
    """every coefficient of every encoded diagonal within 2^-30 of the encoding scale of the oracle's own encoding of
    rot_{-giant}(d_k), tiled (the tolerance tests/test_gpu_bootstrap.py states for the bootstrap constants), and one integer
    polynomial across the rows; with and without the special-prime rows, dense and sparse packing, a caller's own scale"""
    need_gpu()
    from lattisense_amd.device import LinearTransformPlan
    rig = Rig(12, "headline", 27)
    rng = np.random.default_rng(7)
    o, ev, N = rig.o, rig.ev, rig.N
    for period, index, dh, pt_scale in ((1 << 11, range(20), True, 0), (1 << 9, range(-4, 9), True, 2.0 ** 35), (1 << 11, range(20), False, 0),
                                        (1 << 11, [0, 7], True, 0)):
        lvl = 5
        diags = _reduced(_diags(rng, index, period), period)
        plan = LinearTransformPlan(rig.ctx, lvl, diags, pt_scale=pt_scale, double_hoist=dh)
        scale = pt_scale or float(o.mod[lvl])
        assert plan.pt_scale == scale
        got = plan.oracle_plains()
        for k in plan.diagonals:
            giant = (k // plan.n1) * plan.n1 if plan.n1 else 0
            z = np.tile(np.roll(diags[k], giant), (N // 2) // period)
            ext = plan.rows > lvl + 1
            want = ev.encode_ext(z, lvl, scale) if ext else ev.encode(z, lvl, scale)
            assert got[k].shape == want.shape
            deltas = []
            for row in sorted({0, lvl, plan.rows - 1}):
                j = ev._mi(lvl, row)
                q = o.mod[j]
                dd = (o.intt(j, got[k][row]).astype(object) - o.intt(j, want[row]).astype(object)) % q
                deltas.append(np.array([int(x) - q if int(x) > q // 2 else int(x) for x in dd], dtype=np.float64))
            assert all(np.array_equal(deltas[0], x) for x in deltas[1:]), k
            assert np.max(np.abs(deltas[0])) / scale < 2.0 ** -30, k
        plan.close()


def test_bootstrap_matrix_through_the_operator():
    """The first CoeffsToSlots matrix of a bootstrap plan at N = 2^13 (whole-limb transforms, 25 Q + 5 P, level 24) through the
    public operator.  Both plans encode with the same code, but the diagonal VALUES differ in their last bits (the bootstrap
    plan composes its FFT layers in C++, this test in numpy), so each side is compared with the oracle on its own plaintexts:
    the operator's result equals the oracle transform with the operator plan's plaintexts, the two plans agree on indices, split
    and rotations, and their plaintexts agree to 2^-30 of the scale."""
    need_gpu()
    from lattisense_amd import params
    from lattisense_amd.device import ALGO_CKKS, BootstrapPlan, DeviceContext, LinearTransformPlan
    from oracle.ckks_bootstrap import Ct, Evaluator, linear_transform, merged_matrices
    from oracle.client import Client, galois_element_for_col_rotation
    from oracle.pyoracle import Oracle
    B = params.CKKS_BOOTSTRAP_65536
    N = 1 << 13
    n = N // 2
    o = Oracle(N, B["q"], B["p"], 0)
    c = Client(o, seed=61, hamming=32)
    ctx = DeviceContext(ALGO_CKKS, N, B["q"], B["p"])
    top = len(B["q"]) - 1
    bplan = BootstrapPlan(ctx, in_scale=D40, out_scale=D40)
    lvl, n1, ks, bplains = bplan.matrix(0)
    assert lvl == top
    mat = merged_matrices(n, 4, True)[0]
    diags = {k: v / (2.0 * n * 16) for k, v in mat.items()}          # the factor the plan folds into its first matrix (K = 16)
    assert sorted(diags) == ks
    plan = LinearTransformPlan(ctx, lvl, diags)
    assert plan.n1 == n1 and plan.diagonals == ks and plan.rows == lvl + 1 + len(B["p"])
    assert set(plan.galois_elements) <= set(bplan.galois_elements)
    plains = plan.oracle_plains()
    ev = Evaluator.__new__(Evaluator)
    ev.o, ev.c, ev.klvl, ev.n, ev.glk, ev.counts = o, c, top, N, {}, {"rotate": 0, "mult": 0, "mul_plain": 0}
    worst = 0.0
    for k in ks:
        assert plains[k].shape == bplains[k].shape
        for row in (0, plan.rows - 1):
            j = ev._mi(lvl, row)
            q = o.mod[j]
            dd = (o.intt(j, plains[k][row]).astype(object) - o.intt(j, bplains[k][row]).astype(object)) % q
            worst = max(worst, max(abs(int(x) - q if int(x) > q // 2 else int(x)) for x in dd) / float(o.mod[lvl]))
    print("operator plan vs bootstrap plan plaintexts: worst coefficient difference %.3g of the scale" % worst)
    assert worst < 2.0 ** -30
    ev.glk = {e: c.gen_galois_key(e, top) for e in plan.galois_elements}
    glk = {e: ctx.upload_key(kk, top) for e, kk in ev.glk.items()}
    rng = np.random.default_rng(62)
    z = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    ct = c.ckks_encrypt(z, lvl, D40)
    got = ctx.download(plan.run(ctx.upload(ct[None]), 1, glk), (1, 2, lvl, N))[0]
    want = linear_transform(ev, Ct(ct, lvl, D40), diags, 2.0, plains=plains, rescale=True, n_slots=n, double_hoist=True)
    assert np.array_equal(got, want.data)
    assert sorted(ev.glk) == sorted(galois_element_for_col_rotation(r, N) for r in
                                    {k % n1 for k in ks} | {(k // n1) * n1 for k in ks} if r)
    plan.close()
    bplan.close()
