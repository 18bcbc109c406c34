"""Key switch with the ModUp of a single-limb digit lifted by the load of its extension transform (NttPassArgs::fz_pro == 4,
key_switch.hip KsTile::decompose) instead of a base-conversion launch.  The lift changes which kernel produces the digit's extension
rows, never a residue: every output is compared bit for bit with lsa_set_modup_lift(ctx, 0) (the conversion kernel, same context) and
with the CPU oracle, at the smallest shapes that reach each kernel the prologue lives in -- the single-pass and the staged
two-pass k_ntt_pass, the 7- and 8-stage k_ntt_r16 first passes, k_ntt_r8x3 behind a lifted first pass -- with the key MAC fused
and apart, FP64- and integer-engine targets, NTT- and coefficient-domain (BFV) sources.  The CPU replay of the same code is
tests/test_emulate_ntt_lift.py."""
import numpy as np
import pytest

from lattisense_amd import params
from tests.gpu_util import env, need_gpu

pytestmark = pytest.mark.gpu

G1, G2 = 5, 25   # Galois elements of the rotations


def _rand(rng, mods, shape, n):
    out = np.empty((*shape, len(mods), n), dtype=np.uint64)
    for i, m in enumerate(mods):
        out[..., i, :] = rng.integers(0, m, size=(*shape, n), dtype=np.uint64)
    return out


def _top(mods, shape, n):
    """every residue q - 1"""
    out = np.empty((*shape, len(mods), n), dtype=np.uint64)
    for i, m in enumerate(mods):
        out[..., i, :] = m - 1
    return out


def _single_source_plans(ctx):
    return [pl for pl in ctx.baseconv_plans() if pl[0] == 1]


def _both(ctx, run, want, tag, lifts=None, strict=True):
    """run(): the operator's output as an array.  default == lsa_set_modup_lift(ctx, 0) == oracle.
    lifts (the first operator a context runs at a level, which is the one that makes the level's conversion plans): which
    path ran, read from the base-conversion plans -- the run with the lift off makes the single-source plans of the level's
    single-limb digits exactly when the default run lifted them (lifts), and none otherwise; strict (several special primes,
    so ModDown is no single-source conversion): the default run made no single-source plan at all"""
    n0 = len(_single_source_plans(ctx))
    got = run()
    n1 = len(_single_source_plans(ctx))
    ctx.set_modup_lift(0)
    try:
        old = run()
    finally:
        ctx.set_modup_lift(1)
    n2 = len(_single_source_plans(ctx))
    assert np.array_equal(got, old), ("lift differs from the conversion kernel",) + tag
    assert np.array_equal(got, want), ("lift differs from the oracle",) + tag
    if lifts is not None:
        assert (n2 > n1) == lifts, ("which path ran", n0, n1, n2) + tag
        assert not strict or n1 == n0, ("the default path made a single-source conversion", n0, n1) + tag


def _ckks(n, q, p, levels, batch, seed, ops=("hmult", "rotate"), tiles=(0,), top=False, fused_off=False, fp64=True):
    """levels: {level: whether a digit of that level has one source limb below 2^53, i.e. one that is lifted}; top: the last batch
    item is filled with q - 1"""
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    rng = np.random.default_rng(seed)
    klvl = max(levels)
    np_ = len(p)
    beta = (klvl + 1 + np_ - 1) // np_
    o = Oracle(n, q, p, 0)
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    try:
        if not fp64:
            ctx.set_fp64_ntt(0)
        raw = {g: _rand(rng, q[: klvl + 1] + p, (beta, 2), n) for g in (0, G1, G2)}   # 0: the relinearisation key
        keys = {g: ctx.upload_key(k, klvl) for g, k in raw.items()}
        for lvl, single in levels.items():
            L = lvl + 1
            assert any(min(d + np_, L) - d == 1 and not q[d] >> 53 for d in range(0, L, np_)) == single, (L, np_)
            A = _rand(rng, q[:L], (batch, 2), n)
            B = _rand(rng, q[:L], (batch, 2), n)
            if top:
                A[batch - 1], B[batch - 1] = _top(q[:L], (2,), n), _top(q[:L], (2,), n)
            da, db = ctx.upload(A), ctx.upload(B)
            path = [single]   # checked on the level's first operator
            with env(LSA_KS_FUSED="0" if fused_off else None):
                for tile in tiles:
                    ctx.set_tile_batch(tile)
                    tag = (n, lvl, tile, fused_off, fp64)
                    if "hmult" in ops:
                        want = np.stack([o.ckks_mult_relin_rescale(lvl, A[i], B[i], raw[0], klvl) for i in range(batch)])
                        _both(ctx, lambda: ctx.download(ctx.ckks_mult_relin_rescale(lvl, da, db, keys[0], batch), want.shape), want,
                              ("hmult",) + tag, path.pop() if path else None, np_ > 1)
                    if "rotate" in ops:
                        want = np.stack([o.ckks_rotate(lvl, A[i], G1, raw[G1], klvl) for i in range(batch)])
                        _both(ctx, lambda: ctx.download(ctx.ckks_rotate(lvl, da, G1, keys[G1], batch), want.shape), want,
                              ("rotate",) + tag, path.pop() if path else None, np_ > 1)
                    if "rotate_many" in ops:
                        want = np.stack([np.stack([o.ckks_rotate(lvl, A[i], g, raw[g], klvl) for i in range(batch)]) for g in (G1, G2)])

                        def many():
                            outs = ctx.ckks_rotate_many(lvl, da, {g: keys[g] for g in (G1, G2)}, batch)
                            return np.stack([ctx.download(outs[g], want.shape[1:]) for g in (G1, G2)])
                        _both(ctx, many, want, ("rotate_many",) + tag, path.pop() if path else None, np_ > 1)
                ctx.set_tile_batch(0)
    finally:
        ctx.close()


def test_case1_n12_single_pass_every_digit_lifted():
    need_gpu()
    C = params.CKKS_DEFAULT[4096]
    _ckks(1 << 12, C["q"], C["p"], {1: True}, 2, 9012)


def test_case2_n13_staged_two_pass_levels_1_and_5():
    need_gpu()
    C = params.CKKS_DEFAULT[8192]
    _ckks(1 << 13, C["q"], C["p"], {1: True, 5: True}, 2, 9013)


def test_case3_n14_k2_odd_and_even_level_hoisted():
    """7-stage first pass; L = 5 lifts its last digit, L = 6 is the control without one; rotate_many keeps the extension
    transform's passes together (unfused)"""
    need_gpu()
    C = params.CKKS_DEFAULT[16384]
    q, p = C["q"][:6], C["p"]
    assert len(p) == 2
    _ckks(1 << 14, q, p, {4: True, 5: False}, 2, 9014, ops=("hmult", "rotate", "rotate_many"))


def test_case4_n16_headline_digit_shape_tiles_and_top_residues():
    """L = 13, k = 4: digits of 4, 4, 4 and 1 limbs, the fused key MAC behind the lifted first pass, FP64-engine Q targets and
    integer-engine P targets; the default tile and a tile batch of 1; the second item is filled with q - 1"""
    need_gpu()
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    C = params.CKKS_DEFAULT[65536]
    q, p = C["q"][:13], C["p"][:4]
    _ckks(1 << 16, q, p, {12: True}, 2, 9016, tiles=(0, 1), top=True)
    # which path ran: a fresh context under the default builds no single-source conversion, set_modup_lift(0) builds one
    rng = np.random.default_rng(9116)
    ctx = DeviceContext(ALGO_CKKS, 1 << 16, q, p)
    try:
        k = ctx.upload_key(_rand(rng, q + p, (4, 2), 1 << 16), 12)
        da = ctx.upload(_rand(rng, q, (1, 2), 1 << 16))
        ctx.ckks_rotate(12, da, G1, k, 1)
        ctx.sync()
        assert not _single_source_plans(ctx)
        ctx.set_modup_lift(0)
        ctx.ckks_rotate(12, da, G1, k, 1)
        ctx.sync()
        assert _single_source_plans(ctx)
    finally:
        ctx.close()


@pytest.mark.parametrize("fp64", [True, False])
def test_case5_n16_unfused_key_mac_and_integer_engine(fp64):
    need_gpu()
    C = params.CKKS_DEFAULT[65536]
    _ckks(1 << 16, C["q"][:13], C["p"][:4], {12: True}, 1, 9216, ops=("hmult",), fused_off=True, fp64=fp64)


def test_case6_n17_nine_stage_second_pass():
    """the generated N = 2^17 chain (k = 5) at L = 6: digits of 5 and 1 limbs, k_ntt_r8x3 reads what the lifted first pass wrote"""
    need_gpu()
    C = params.ckks_n17_chain()
    q, p = C["q"][:6], C["p"]
    assert len(p) == 5
    _ckks(C["n"], q, p, {5: True}, 1, 9017, ops=("hmult",))


def bfv_lift_chain(n):
    """k = 2, five Q limbs: digits of 2, 2 and 1 limbs, the last one a 50-bit prime (below 2^53: lifted); FP64- and integer-engine
    targets, 61-bit special primes (every prime of BFV_DEFAULT[16384] is above 2^53: its single-limb digits keep the conversion)"""
    q = (params.ntt_primes_below(58, n, 1) + params.ntt_primes_below(47, n, 1) + params.ntt_primes_below(57, n, 2) +
         params.ntt_primes_below(50, n, 1))
    return q, params.ntt_primes_below(61, n, 2)


def test_case7_bfv_n14_coefficient_domain_source():
    """BFV starts the key switch from coefficients: the lift reads the caller's buffer (bfv_rotate: the input ciphertext's second
    polynomial; bfv_mult_relin: the product's third).  k = 2 at L = 5 on bfv_lift_chain"""
    need_gpu()
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.pyoracle import Oracle
    n, t = 1 << 14, 65537
    q, p = bfv_lift_chain(n)
    lvl = klvl = len(q) - 1
    batch = 2
    assert len(set(q + p)) == 7 and len(p) == 2 and (lvl + 1) % 2 == 1 and not q[lvl] >> 53
    rng = np.random.default_rng(9714)
    beta = (klvl + 1 + len(p) - 1) // len(p)
    o = Oracle(n, q, p, t)
    ctx = DeviceContext(ALGO_BFV, n, q, p, t)
    try:
        assert ctx.moduli == o.mod
        raw = {g: _rand(rng, q[: klvl + 1] + p, (beta, 2), n) for g in (0, G1)}
        keys = {g: ctx.upload_key(k, klvl) for g, k in raw.items()}
        A = _rand(rng, q[: lvl + 1], (batch, 2), n)
        B = _rand(rng, q[: lvl + 1], (batch, 2), n)
        A[1, :, lvl], B[1, :, lvl] = q[lvl] - 1, q[lvl] - 1   # the lifted limb's largest residue in every coefficient
        da, db = ctx.upload(A), ctx.upload(B)
        want = np.stack([o.bfv_rotate(lvl, A[i], G1, raw[G1], klvl) for i in range(batch)])
        _both(ctx, lambda: ctx.download(ctx.bfv_rotate(lvl, da, G1, keys[G1], batch), want.shape), want, ("bfv_rotate",), True)
        want = np.stack([o.bfv_mult_relin(lvl, A[i], B[i], raw[0], klvl) for i in range(batch)])
        _both(ctx, lambda: ctx.download(ctx.bfv_mult_relin(lvl, da, db, keys[0], batch), want.shape), want, ("bfv_mult_relin",))
    finally:
        ctx.close()


def test_case8_n12_source_limb_of_61_bits_keeps_the_conversion():
    """one special prime, so every digit has one limb: q_1 (41 bits) is lifted, q_0 (61 bits) is not -- the conversion computes
    v = (int)RN(double(y) / double(q_s)), which is 1 for residues next to a q_s of 2^53 or more, and the lift would give
    y mod p_t where the conversion gives y - q_s.  The second item is filled with q - 1."""
    need_gpu()
    B = params.CKKS_BOOTSTRAP_65536
    q, p = B["q"][:2], B["p"][:1]
    assert q[0] >> 53 and not q[1] >> 53
    _ckks(1 << 12, q, p, {1: True}, 2, 9112, top=True)
