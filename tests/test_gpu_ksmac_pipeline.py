"""The fused second pass + key MAC (k_ntt_r16_ksmac) with its twiddles cached in LDS once per workgroup (ntt_r16.h, "twiddles once
per workgroup").  That changes where a transform's twiddles come from, never a residue: every output is compared bit for bit with
the CPU oracle, and HMult + relinearise + rescale under tail mode 0 (lsa_set_ks_tail_in_mac) with the default mode, at the
smallest shapes at which each branch of the loop exists -- batch 3 in tiles of 2, five or fewer Q limbs:

  N = 2^15: the smallest ring whose second pass has eight stages (one radix-16 group of private twiddles); eight tiles per limb
  N = 2^14: seven stages (two radix-8 groups)
  N = 2^17: nine stages (the loop as it was)"""
import numpy as np
import pytest

from lattisense_amd import params
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

BATCH, TILE = 3, 2
C16 = params.CKKS_DEFAULT[65536]
Q, P = C16["q"], C16["p"]
CHAINS = {
    # every limb on the FP64 engine.  Level 4: digits of 2, 2 and 1 limbs, l the lifted single-limb digit, the P limbs on the
    # non-tail launch, four tail limbs (the XCD deal is on); level 3: three tail limbs (deal off), l inside a two-limb digit;
    # level 1: one digit -- no foreign digit, the tail's transforms are the workgroup's first
    "fp": (Q[1:6], Q[6:8]),
    # integer-engine q_0 and P limbs: the fused launch covers only part of the limbs
    "mixed": (Q[0:5], P[:2]),
}


def _rand(rng, mods, shape, n):
    out = np.empty((*shape, len(mods), n), dtype=np.uint64)
    for i, m in enumerate(mods):
        out[..., i, :] = rng.integers(0, m, size=(*shape, n), dtype=np.uint64)
    return out


class Rig:
    def __init__(self, n, chain, seed, batch=BATCH, tile=TILE):
        from lattisense_amd.device import ALGO_CKKS, DeviceContext
        from oracle.pyoracle import Oracle
        self.n, (self.q, self.p) = n, CHAINS[chain] if isinstance(chain, str) else chain
        self.batch = batch
        self.klvl = len(self.q) - 1
        rng = np.random.default_rng(seed)
        beta = -(-(self.klvl + 1) // len(self.p))
        self.o = Oracle(n, self.q, self.p, 0)
        self.ctx = DeviceContext(ALGO_CKKS, n, self.q, self.p)
        self.ctx.set_tile_batch(tile)
        self.raw = _rand(rng, self.q + self.p, (beta, 2), n)
        self.key = self.ctx.upload_key(self.raw, self.klvl)
        self.A = _rand(rng, self.q, (batch, 2), n)
        self.B = _rand(rng, self.q, (batch, 2), n)
        self.g = int(pow(5, 77, 2 * n))
        self.dev, self.want_mul, self.want_rot = {}, {}, {}

    def close(self):
        self.ctx.close()

    def operands(self, level):
        if level not in self.dev:
            L = level + 1
            self.dev[level] = (self.ctx.upload(self.A[:, :, :L]), self.ctx.upload(self.B[:, :, :L]))
        return self.dev[level]

    def oracle_mul(self, level):
        """computed once per level, shared by every variant, never written"""
        if level not in self.want_mul:
            L = level + 1
            w = np.stack([self.o.ckks_mult_relin_rescale(level, np.ascontiguousarray(self.A[i, :, :L]),
                                                         np.ascontiguousarray(self.B[i, :, :L]), self.raw, self.klvl)
                          for i in range(self.batch)])
            w.setflags(write=False)
            self.want_mul[level] = w
        return self.want_mul[level]

    def oracle_rot(self, level):
        if level not in self.want_rot:
            L = level + 1
            w = np.stack([self.o.ckks_rotate(level, np.ascontiguousarray(self.A[i, :, :L]), self.g, self.raw, self.klvl)
                          for i in range(self.batch)])
            w.setflags(write=False)
            self.want_rot[level] = w
        return self.want_rot[level]

    def mul(self, level, mode, batch=None):
        """one HMult + relinearise + rescale under lsa_set_ks_tail_in_mac(mode); None: the context's default"""
        batch = self.batch if batch is None else batch
        da, db = self.operands(level)
        if mode is not None:
            self.ctx.set_ks_tail_in_mac(mode)
        try:
            out = self.ctx.ckks_mult_relin_rescale(level, da, db, self.key, batch)
            self.ctx.sync()
        finally:
            if mode is not None:
                self.ctx.set_ks_tail_in_mac(1)
        return self.ctx.download(out, (batch, 2, level, self.n))

    def check_mul(self, level, mode, tag, batch=None):
        batch = self.batch if batch is None else batch
        got, old = self.mul(level, mode, batch), self.mul(level, 0, batch)
        assert np.array_equal(got, old), ("differs from tail mode 0", tag)
        assert np.array_equal(got, self.oracle_mul(level)[:batch]), ("differs from the oracle", tag)

    def check_rot(self, level, tag, batch=None):
        batch = self.batch if batch is None else batch
        got = self.ctx.download(self.ctx.ckks_rotate(level, self.operands(level)[0], self.g, self.key, batch), (batch, 2, level + 1, self.n))
        assert np.array_equal(got, self.oracle_rot(level)[:batch]), ("rotate differs from the oracle", tag)


_RIGS = {}


def _rig(n, chain):
    need_gpu()
    if (n, chain) not in _RIGS:
        _RIGS[(n, chain)] = Rig(n, chain, n.bit_length() * 100 + len(chain))
    return _RIGS[(n, chain)]


def teardown_module(module):
    for r in _RIGS.values():
        r.close()
    _RIGS.clear()


# ------------------------------------------------------------------------------------------------ N = 2^15
@pytest.mark.parametrize("chain,level", [("fp", 4), ("fp", 3), ("fp", 1), ("mixed", 4)])
def test_n15_hmult(chain, level):
    _rig(1 << 15, chain).check_mul(level, None, (chain, level))


@pytest.mark.parametrize("chain", ["fp", "mixed"])
def test_n15_rotate(chain):
    """no fold: the own digit is read from the ciphertext, the non-tail kernel runs for every limb, the own digit is the first, a
    middle and the last digit across the Q targets, the P targets have none"""
    _rig(1 << 15, chain).check_rot(4, chain)


@pytest.mark.parametrize("chain", ["fp", "mixed"])
@pytest.mark.parametrize("variant", ["batch_1", "dual_stream"])
def test_n15_variants(chain, variant):
    from lattisense_amd._native import check, lib
    r = _rig(1 << 15, chain)
    try:
        if variant == "dual_stream":
            check(lib().lsa_set_dual_stream(r.ctx.h, 1))
        batch = 1 if variant == "batch_1" else None
        r.check_mul(4, None, (chain, variant), batch=batch)
        r.check_rot(4, (chain, variant), batch=batch)
    finally:
        check(lib().lsa_set_dual_stream(r.ctx.h, 0))


# ------------------------------------------------------------------------------------------------ N = 2^14
@pytest.mark.parametrize("chain", ["fp", "mixed"])
def test_n14_hmult_tail_modes_2_and_0(chain):
    _rig(1 << 14, chain).check_mul(4, 2, chain)


@pytest.mark.parametrize("chain", ["fp", "mixed"])
def test_n14_rotate(chain):
    _rig(1 << 14, chain).check_rot(4, chain)


# ------------------------------------------------------------------------------------------------ N = 2^17: the loop as it was
def test_n17_hmult_and_rotate():
    """three Q limbs and two special primes, all on the FP64 engine: the nine-stage kernel carries every target limb"""
    need_gpu()
    C = params.ckks_n17_chain()
    r = Rig(C["n"], (C["q"][1:4], C["q"][4:6]), 1700, batch=2, tile=2)
    try:
        assert all(m < (1 << 47) for m in r.q + r.p)
        r.check_mul(2, None, "2^17")
        r.check_rot(2, "2^17")
    finally:
        r.close()
