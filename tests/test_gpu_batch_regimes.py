"""Oracle parity of the key-switch family at the batches the benchmark and the task runtime run, where the launch arithmetic that
depends on the batch alone takes the branches a batch of 1..7 never reaches.  The reference is always
oracle.pyoracle.Oracle (through oracle/ckks_bootstrap.py's Evaluator for the plan operators); comparisons between modes are extra.

  a  N = 2^12, 5 Q + 2 P, batch 39 / 76   stand-alone key MAC, 37 groups of 2 / 3 items with a last group of one
  b  N = 2^16, 6 Q + 2 P, integer engine  batch 5 in groups of 3 and 2 on a two-pass ring
  c  N = 2^14, fused second pass + MAC    prime batch 37 in one tile: the XCD deal's slot % batch, its tail and rescale-head modes
  d  N = 2^12 / 2^14, batch cap + 1       pick_tile's automatic split with a last tile of one
  e  N = 2^12 slot sum / linear transform the slot-sum copy of the grouping; k_mac_plain_multi's batch map at batch 11
  f  BFV, N = 2^12, batch 39              the same key MAC behind the BFV extension and scale-down
  g  stride 2^32 + 2 W words              item 1 lies 32 GiB behind item 0: beyond 32-bit bytes and 32-bit words, signed or not
  h  the headline shape, batch 48 / 64    one tile whose workspace passes 4 GiB

A large batch is drawn from K distinct ciphertexts (tests/ks_groups.py spread): the oracle runs K times, computed once per rig
and shared by its variants, and EVERY batch position is compared word for word with its source's result.  Each case asserts,
from the restated launch arithmetic of tests/ks_groups.py, that its shape is in the regime it claims: a change to the constants
makes the case fail instead of silently losing its coverage."""
import ctypes

import numpy as np
import pytest

from lattisense_amd import params
from tests import ks_groups
from tests.gpu_util import need_gpu, rand_ct
from tests.layout_util import SENT, invoke, last_error

pytestmark = pytest.mark.gpu

C16 = params.CKKS_DEFAULT[65536]
Q, P = C16["q"], C16["p"]
PROF_KSMAC = 2
GIB = 1 << 30


def _rand_key(rng, mods, beta, n):
    key = np.empty((beta, 2, len(mods), n), dtype=np.uint64)
    for j, m in enumerate(mods):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, n), dtype=np.uint64)
    return key


def _free_gib():
    import torch
    return torch.cuda.mem_get_info()[0] / GIB


class Rig:
    """One context, its oracle, one uniform key at the top level, a batch of `batch` operand pairs drawn from `k` distinct ones
    (k == batch: every item distinct), oracle results computed once per distinct pair, shared and never written."""

    def __init__(self, algo, n, q, p, t, level, batch, k, seed, g=None, pick=None):
        from lattisense_amd.device import DeviceContext
        from oracle.pyoracle import Oracle
        self.n, self.q, self.p, self.level, self.batch, self.k = n, list(q), list(p), level, batch, k
        self.klvl = len(q) - 1
        self.L = level + 1
        self.T = self.L + len(p)
        rng = np.random.default_rng(seed)
        self.o = Oracle(n, q, p, t)
        self.ctx = DeviceContext(algo, n, q, p, t)
        self.ctx.set_tile_batch(0)
        self.raw = _rand_key(rng, self.q + self.p, -(-(self.klvl + 1) // len(p)), n)
        self.key = self.ctx.upload_key(self.raw, self.klvl)
        self.src_a, self.src_b = rand_ct(rng, q[: self.L], 2, n, k), rand_ct(rng, q[: self.L], 2, n, k)
        if pick is None:
            pick = np.arange(batch) if k == batch else ks_groups.spread(rng, np.arange(k), batch)[1]
        self.pick = np.asarray(pick)
        assert len(set(self.pick.tolist())) == k and (batch == 1 or self.pick[0] != self.pick[-1])
        self.g = int(pow(5, 77, 2 * n)) if g is None else g      # the Galois element of "rot"
        self._dev, self._want = {}, {}

    def close(self):
        self._dev.clear()
        self.ctx.close()

    def dev(self, name):
        """the batch of operand `name` ("a", "b", "d3") on the device, uploaded once"""
        if name not in self._dev:
            src = {"a": lambda: self.src_a, "b": lambda: self.src_b, "d3": lambda: self.want("d3")}[name]()
            self._dev[name] = self.ctx.upload(src[self.pick])
        return self._dev[name]

    def want(self, op):
        """the oracle's result for each of the k distinct operand pairs"""
        if op not in self._want:
            o, lvl, kl = self.o, self.level, self.klvl
            fn = {"mul": lambda a, b: o.ckks_mult_relin_rescale(lvl, a, b, self.raw, kl),
                  "rot": lambda a, b: o.ckks_rotate(lvl, a, self.g, self.raw, kl),
                  "d3": lambda a, b: o.ckks_mult(lvl, a, b),
                  "bfv_mul": lambda a, b: o.bfv_mult_relin(lvl, a, b, self.raw, kl),
                  "bfv_rot": lambda a, b: o.bfv_rotate(lvl, a, self.g, self.raw, kl)}.get(op)
            if op == "relin":
                w = np.stack([o.ckks_relin(lvl, d, self.raw, kl) for d in self.want("d3")])
            else:
                w = np.stack([fn(self.src_a[i], self.src_b[i]) for i in range(self.k)])
            w.setflags(write=False)
            self._want[op] = w
        return self._want[op]

    def run(self, op, batch=None):
        """the device's words for the first `batch` items"""
        ctx, lvl, n = self.ctx, self.level, self.n
        batch = self.batch if batch is None else batch
        if op == "mul":
            return ctx.download(ctx.ckks_mult_relin_rescale(lvl, self.dev("a"), self.dev("b"), self.key, batch), (batch, 2, lvl, n))
        if op == "rot":
            return ctx.download(ctx.ckks_rotate(lvl, self.dev("a"), self.g, self.key, batch), (batch, 2, self.L, n))
        if op == "relin":
            return ctx.download(ctx.ckks_relin(lvl, self.dev("d3"), self.key, batch), (batch, 2, self.L, n))
        if op == "bfv_mul":
            return ctx.download(ctx.bfv_mult_relin(lvl, self.dev("a"), self.dev("b"), self.key, batch), (batch, 2, self.L, n))
        assert op == "bfv_rot"
        return ctx.download(ctx.bfv_rotate(lvl, self.dev("a"), self.g, self.key, batch), (batch, 2, self.L, n))

    def held(self, op, tag, batch=None, got=None):
        """every batch position against its source's oracle result; the message names the positions and rows that differ, and
        whether a wrong item is another source's result (an item that read a neighbour's data)"""
        got = self.run(op, batch) if got is None else got
        want, bad = self.want(op), []
        for b in range(got.shape[0]):
            w = want[self.pick[b]]
            if not np.array_equal(got[b], w):
                rows = np.argwhere((got[b] != w).any(axis=-1)).tolist()
                other = [i for i in range(self.k) if np.array_equal(got[b], want[i])]
                bad.append((b, int(self.pick[b]), rows[:6], other))
        assert not bad, "%s %s: %d of %d items differ from the oracle; (item, source, [poly, row]s, equals source): %s" % (
            op, tag, len(bad), got.shape[0], bad[:8])
        return got

    def mac_gx(self):
        return ks_groups.mac_gx(self.n, self.T)


def _ckks(n, q, p, level, batch, k, seed, **kw):
    from lattisense_amd.device import ALGO_CKKS
    need_gpu()
    return Rig(ALGO_CKKS, n, q, p, 0, level, batch, k, seed, **kw)


def _regime(gx, batch, groups=None):
    got = ks_groups.ks_mac_groups(gx, batch)
    assert ks_groups.short_last_group(gx, batch), (gx, batch, got)
    assert groups is None or got[0] == groups, (gx, batch, got)
    return got


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("batch", [39, 76])
def test_a_standalone_mac_groups_with_a_last_group_of_one(batch, monkeypatch):
    """a one-pass ring has no fused kernel: every target limb goes through k_ks_mac, gx = 7 * 8 = 56 -> 37 groups"""
    r = _ckks(1 << 12, Q[:5], P[:2], 4, batch, 4, 1200 + batch)
    try:
        _, bpt, gy = _regime(r.mac_gx(), batch, groups=37)
        assert r.mac_gx() == 56 and bpt == {39: 2, 76: 3}[batch] and batch - (gy - 1) * bpt == 1
        assert not r.ctx.key_switch_fused(r.level, r.key)
        folded = r.held("mul", "folded")
        monkeypatch.setenv("LSA_HMULT_FOLD", "0")
        assert np.array_equal(r.held("mul", "LSA_HMULT_FOLD=0"), folded)
        monkeypatch.delenv("LSA_HMULT_FOLD")
        scattered = r.held("rot", "scatter")
        monkeypatch.setenv("LSA_ROT_SCATTER", "0")
        assert np.array_equal(r.held("rot", "LSA_ROT_SCATTER=0"), scattered)
        monkeypatch.delenv("LSA_ROT_SCATTER")
        r.held("relin", "")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ b
def test_b_two_pass_ring_groups_of_three_and_two():
    """N = 2^16 on the integer engine: no fused kernel, gx = 8 * 128 = 1024 -> 2 groups, items (0 1 2) (3 4); every item distinct"""
    r = _ckks(1 << 16, Q[:6], P[:2], 5, 5, 5, 1605)
    try:
        r.ctx.set_fp64_ntt(0)
        assert r.mac_gx() == 1024 and _regime(1024, 5) == (2, 3, 2)
        assert not r.ctx.key_switch_fused(r.level, r.key)
        r.held("mul", "")
        r.held("rot", "")
    finally:
        r.ctx.set_fp64_ntt(1)
        r.close()


# ------------------------------------------------------------------------------------------------ c
C_CHAINS = {"fp": (Q[1:6], Q[6:8]), "mixed": (Q[0:5], P[:2])}     # the chains of tests/test_gpu_ksmac_pipeline.py


@pytest.mark.parametrize("chain", ["fp", "mixed"])
def test_c_fused_mac_prime_batch_in_one_tile(chain, monkeypatch):
    """N = 2^14, level 4, batch 37 in one automatic tile: k_ntt_r16_ksmac's slot % batch and (slot / batch) * 8 + (w & 7) at a
    batch that divides nothing, with the merged rescale tail inside the MAC (mode 2) and without (0), the rescale head inside
    ModDown's conversion (2) and without (0); chain fp once more with the XCD deal off"""
    q, p = C_CHAINS[chain]
    r = _ckks(1 << 14, q, p, 4, 37, 4, 1437 + len(chain))
    ctx = r.ctx
    try:
        assert ks_groups.auto_tile(r.n, ks_groups.hmult_rows(4, 2, False), 37) == 37                 # one tile
        assert ctx.key_switch_fused(r.level, r.key)
        # the deal needs a launch's limbs x the 4 tiles of a limb to be a multiple of the 8 XCDs.  Limbs below 2^47 take the fused
        # kernel.  fp: 5 Q + 2 P of them -- on for the tail launch (4 Q limbs) and the P launch, off for the single launch of 7
        # (tail mode 0, the rotation); mixed: 4 Q of them -- on for the single launch of 4, off for the tail launch of 3
        fq, fp = sum(m < 1 << 47 for m in q), sum(m < 1 << 47 for m in p)
        assert (fq, fp) == {"fp": (5, 2), "mixed": (4, 0)}[chain]
        first = None
        for tail, head in [(2, 2), (0, 0), (2, 0), (0, 2), (1, 1)]:
            ctx.set_ks_tail_in_mac(tail)
            ctx.set_rescale_head_in_conv(head)
            got = r.held("mul", (chain, "tail", tail, "head", head))
            first = got if first is None else first
            assert np.array_equal(got, first), (tail, head)
        r.held("rot", chain)
        if chain == "fp":
            monkeypatch.setenv("LSA_KSMAC_XCD", "0")
            ctx.set_ks_tail_in_mac(2)
            ctx.set_rescale_head_in_conv(2)
            assert np.array_equal(r.held("mul", "LSA_KSMAC_XCD=0"), first)
            r.held("rot", "LSA_KSMAC_XCD=0")
    finally:
        ctx.set_ks_tail_in_mac(1)
        ctx.set_rescale_head_in_conv(1)
        r.close()


# ------------------------------------------------------------------------------------------------ d
def _mac_launches(ctx, fn):
    from lattisense_amd._native import lib
    L = lib()
    assert L.lsa_profile_begin(ctx.h, 1) == 0
    try:
        out = fn()
        ctx.sync()
    finally:
        assert L.lsa_profile_end(ctx.h) == 0
    n = ctypes.c_longlong()
    assert L.lsa_profile_read(ctx.h, PROF_KSMAC, None, None, None, ctypes.byref(n)) == 0
    return out, n.value


@pytest.mark.parametrize("log_n,cap", [(12, 512), (14, 256)])
def test_d_automatic_tiles_with_a_last_tile_of_one(log_n, cap):
    """batch = cap + 1 under lsa_set_tile_batch(0): pick_tile cuts it into a full tile and a tile of one.  The key-MAC launches
    (profiler kind 2) are exactly twice those of the same call at batch = cap, on one stream and on two."""
    from lattisense_amd._native import check, lib
    n = 1 << log_n
    r = _ckks(n, Q[:3], P[:2], 2, cap + 1, 4, 1300 + log_n)
    try:
        rows_hmult = ks_groups.hmult_rows(2, 2, False)            # the larger of the two operators' workspaces
        assert ks_groups.tile_cap(n) == cap
        assert ks_groups.auto_tile(n, rows_hmult, cap + 1) == cap and ks_groups.auto_tile(n, rows_hmult, cap) == cap
        for dual in (0, 1):
            check(lib().lsa_set_dual_stream(r.ctx.h, dual))
            for op in ("mul", "rot"):
                whole, n_whole = _mac_launches(r.ctx, lambda: r.run(op))
                r.held(op, ("dual", dual, "batch", cap + 1), got=whole)
                one, n_one = _mac_launches(r.ctx, lambda: r.run(op, cap))
                r.held(op, ("dual", dual, "batch", cap), got=one)
                assert n_one >= 1 and n_whole == 2 * n_one, (op, dual, n_whole, n_one)
    finally:
        check(lib().lsa_set_dual_stream(r.ctx.h, 0))
        r.close()


# ------------------------------------------------------------------------------------------------ e
def test_e_slot_sum_multi_key_mac_groups():
    """lsa_ckks_slot_sum at N = 2^12, 5 Q + 2 P, batch 39 drawn from 4 ciphertexts: launch_ks_mac_multi's copy of the grouping
    (gx = 56: groups of 2 with a last group of one), two, three and four keys per launch, against tests/slot_sum_model.py; the
    single-key launches give the same words"""
    need_gpu()
    from lattisense_amd.device import ALGO_CKKS, DeviceContext, SlotSumPlan
    from oracle.ckks_bootstrap import Ct, Evaluator
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    from tests.slot_sum_model import slot_sum, steps_of
    n, q, p, level, batch, k = 1 << 12, Q[:5], P[:2], 4, 39, 4
    _regime(ks_groups.mac_gx(n, level + 1 + len(p)), batch, groups=37)
    o = Oracle(n, q, p, 0)
    c = Client(o, seed=39)
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    ev = Evaluator.__new__(Evaluator)
    ev.o, ev.c, ev.klvl, ev.n = o, c, level, n
    ev.glk, ev.counts = {}, {"rotate": 0, "mult": 0, "mul_plain": 0}
    rng = np.random.default_rng(3912)
    scale = float(2 ** 40)
    src = np.stack([c.ckks_encrypt(rng.uniform(-1, 1, n // 2) + 1j * rng.uniform(-1, 1, n // 2), level, scale) for _ in range(k)])
    items, pick = ks_groups.spread(rng, src, batch)
    xin = ctx.upload(items)
    try:
        for count, radix in ((5, 4), (7, 4), (12, 4)):
            plan = SlotSumPlan(ctx, level, 1, count, radix)
            assert max(len(s) for s in steps_of(n, 1, count, radix)) == {5: 4, 7: 2, 12: 3}[count]
            for e in plan.galois_elements:
                if e not in ev.glk:
                    ev.glk[e] = c.gen_galois_key(e, level)
            glk = {e: ctx.upload_key(ev.glk[e], level) for e in plan.galois_elements}
            want = [slot_sum(ev, Ct(ct, level, scale), 1, count, radix).data for ct in src]
            plan.multi_mac = True
            got = ctx.download(plan.run(xin, batch, glk), (batch, 2, level + 1, n))
            bad = [b for b in range(batch) if not np.array_equal(got[b], want[pick[b]])]
            assert not bad, ("multi-key MAC: items differ from the model", count, radix, bad)
            plan.multi_mac = False
            assert np.array_equal(ctx.download(plan.run(xin, batch, glk), (batch, 2, level + 1, n)), got), (count, radix)
            plan.close()
            for h in glk.values():
                ctx.destroy_key(h)
    finally:
        ctx.close()


def test_e_linear_transform_multi_mac_batch_map(monkeypatch):
    """lsa_ckks_linear_transform at N = 2^12 with 24 diagonals (more than 8, one k_mac_plain_multi launch over all inner sums)
    at batch 11, every item distinct and held to the oracle: slot % batch and (slot / batch) * 8 + (w & 7) with the XCD deal
    (the piece count 4 * 8 is a multiple of 8), blockIdx.x % batch under LSA_MACM_NO_XCD=1"""
    from tests.test_gpu_ckks_lt import Rig as LtRig, _check, _diags
    need_gpu()
    rig = LtRig(12, "headline", 1112)
    try:
        period = 1 << 11
        assert rig.N // 512 == 8                             # pieces per limb: any limb count gives a multiple of 8
        d = _diags(np.random.default_rng(11), range(24), period)
        n1, _ = _check(rig, 3, d, period, batch=11, env_variants=({"LSA_MACM_NO_XCD": "1"},), monkeypatch=monkeypatch, seed=11)
        assert 2 <= n1 < 24                                  # split into baby and giant steps: the inner sums are the multi-MAC's
    finally:
        rig.ctx.close()


# ------------------------------------------------------------------------------------------------ f
BFV_CHAINS = {
    # the issue's chain: 2 Q + 1 P, three target limbs (gx = 24: one item per group at batch 39)
    "default_n4096": (params.BFV_DEFAULT[4096]["q"], params.BFV_DEFAULT[4096]["p"], params.BFV_DEFAULT[4096]["t"]),
    # 5 Q + 2 P of the N = 2^14 set: seven target limbs, the grouping of case a (groups of 2, a last group of one)
    "q5_p2": (params.BFV_DEFAULT[16384]["q"][:5], params.BFV_DEFAULT[16384]["p"], params.BFV_DEFAULT[16384]["t"]),
}


@pytest.mark.parametrize("chain", list(BFV_CHAINS))
def test_f_bfv_mult_relin_and_rotate(chain):
    from lattisense_amd.device import ALGO_BFV
    need_gpu()
    q, p, t = BFV_CHAINS[chain]
    r = Rig(ALGO_BFV, 1 << 12, q, p, t, len(q) - 1, 39, 4, 4039 + len(q))
    try:
        assert r.ctx.moduli == r.o.mod                       # the same auxiliary basis on both sides
        if chain == "q5_p2":
            _regime(r.mac_gx(), 39, groups=37)
        else:
            assert ks_groups.ks_mac_groups(r.mac_gx(), 39) == (39, 1, 39)
        r.held("bfv_mul", chain)
        r.held("bfv_rot", chain)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ g
GUARD = 512                                                 # words: a 4 KiB sentinel window before and after each item


class FarField:
    """Two items of up to `room` words inside ONE allocation shared with other fields, item b at word off + b * stride.  Only the
    windows [item - GUARD, item + room + GUARD) are ever written or read."""

    def __init__(self, ctx, buf, off, stride, room):
        self.ctx, self.buf, self.off, self.stride, self.room = ctx, buf, off, stride, room

    @property
    def ptr(self):
        return self.buf.ptr + 8 * self.off

    def _window(self, b):
        return self.buf.ptr + 8 * (self.off + b * self.stride - GUARD), 2 * GUARD + self.room

    def fill(self, data=None):
        """both windows: sentinels, with item b's payload data[b] at its place"""
        from lattisense_amd._native import check, lib
        for b in range(2):
            ptr, words = self._window(b)
            img = np.full(words, SENT, dtype=np.uint64)
            if data is not None:
                flat = np.ascontiguousarray(data[b], dtype=np.uint64).reshape(-1)
                img[GUARD:GUARD + flat.size] = flat
            check(lib().lsa_memcpy_h2d(self.ctx.h, ptr, img.ctypes.data, img.nbytes, self.ctx.stream))
        self.ctx.sync()

    def check(self, what, data=None):
        """both windows hold data[b] (nothing: sentinels) at the item and sentinels everywhere else"""
        from lattisense_amd._native import check, lib
        for b in range(2):
            ptr, words = self._window(b)
            got = np.empty(words, dtype=np.uint64)
            check(lib().lsa_memcpy_d2h(self.ctx.h, got.ctypes.data, ptr, got.nbytes, self.ctx.stream))
            self.ctx.sync()
            size = 0
            if data is not None:
                flat = np.ascontiguousarray(data[b], dtype=np.uint64).reshape(-1)
                size = flat.size
                assert np.array_equal(got[GUARD:GUARD + size], flat), "%s: item %d differs from the oracle" % (what, b)
            assert (got[:GUARD] == SENT).all(), "%s: the window before item %d was written" % (what, b)
            assert (got[GUARD + size:] == SENT).all(), "%s: the window behind item %d was written" % (what, b)


def test_g_items_32_gib_apart():
    """N = 2^12, 3 Q + 1 P, level 2, batch 2; a, b and out interleaved in one allocation with the stride 2^32 + 2 W words for all
    three (W: the largest item, the 3 (level + 1) N words of lsa_ckks_mult's output): item 1 of each lies 32 GiB behind item 0,
    beyond 2^32 bytes, 2^31 words and 2^32 words.  Raw C calls; both payloads equal the oracle, every sentinel window stays."""
    need_gpu()
    free = _free_gib()
    if free < 40:
        pytest.skip("%.1f GiB of device memory free, the 32 GiB stride needs 40" % free)
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    n, q, p, lvl, batch = 1 << 12, Q[:3], P[:1], 2, 2
    L = lvl + 1
    W = 3 * L * n
    stride = (1 << 32) + 2 * W
    slot = W + 2 * GUARD
    assert stride % 2 == 0 and 8 * stride > 1 << 32 and stride > 1 << 32 and slot % 2 == 0
    rng = np.random.default_rng(3232)
    o = Oracle(n, q, p, 0)
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    buf = None
    try:
        ctx.set_tile_batch(0)
        raw = _rand_key(rng, list(q) + list(p), 3, n)
        key = ctx.upload_key(raw, lvl)
        g = int(pow(5, 77, 2 * n))
        A, B = rand_ct(rng, q, 2, n, batch), rand_ct(rng, q, 2, n, batch)
        buf = ctx.alloc(stride + 3 * slot)
        fa, fb, fo = (FarField(ctx, buf, i * slot + GUARD, stride, W) for i in range(3))
        fa.fill(A)
        fb.fill(B)

        def vec(op, x, y):
            return np.stack([np.stack([o.vec(op, j, x[pl, j], y[pl, j]) for j in range(L)]) for pl in range(2)])
        cases = [
            ("lsa_poly_addsub", dict(op=0, polys=2), lambda x, y: vec("add", x, y)),
            ("lsa_poly_addsub", dict(op=1, polys=2), lambda x, y: vec("sub", x, y)),
            ("lsa_ckks_mult", {}, lambda x, y: o.ckks_mult(lvl, x, y)),
            ("lsa_ckks_rescale", dict(polys=2), lambda x, y: o.ckks_rescale(lvl, x)),
            ("lsa_ckks_rotate", dict(g=g, key=key), lambda x, y: o.ckks_rotate(lvl, x, g, raw, lvl)),
            ("lsa_ckks_mult_relin_rescale", dict(key=key), lambda x, y: o.ckks_mult_relin_rescale(lvl, x, y, raw, lvl)),
        ]
        for name, extra, fn in cases:
            fo.fill()
            a = dict(ptrs=[fa.ptr, fb.ptr], strides=[stride, stride], out=fo.ptr, so=stride, batch=batch, level=lvl)
            a.update(extra)
            assert invoke(name, ctx.h, a, ctx.stream) == 0, (name, last_error())
            ctx.sync()
            tag = "%s %s" % (name, extra.get("op", ""))
            fo.check(tag + ": output", [fn(A[b], B[b]) for b in range(batch)])
            fa.check(tag + ": a", A)
            fb.check(tag + ": b", B)
    finally:
        if buf is not None:
            buf.free()
        ctx.close()


# ------------------------------------------------------------------------------------------------ h
H_LEVEL, H_K = 12, 3
_H = {}


def _headline():
    """13 Q + 4 P at N = 2^16, level 12: 64 items drawn from 3 distinct pairs so that the first 48 also use every source and
    end on another source than they start with; three full-size oracle runs per operator, shared by both batches"""
    need_gpu()
    if "rig" not in _H:
        free = _free_gib()
        if free < 16:
            pytest.skip("%.1f GiB of device memory free, the headline tile needs 16" % free)
        rng = np.random.default_rng(4800)
        while True:
            pick = ks_groups.spread(rng, np.arange(H_K), 64)[1]
            if pick[47] != pick[0] and len(set(pick[:48].tolist())) == H_K:
                break
        _H["rig"] = _ckks(1 << 16, Q[:13], P, H_LEVEL, 64, H_K, 4801, g=5, pick=pick)
    return _H["rig"]


def teardown_module(module):
    if "rig" in _H:
        _H.pop("rig").close()


def _headline_rows(fold):
    """workspace rows per ciphertext of lsa_ckks_mult_relin_rescale and of the rotation's key switch"""
    return ks_groups.hmult_rows(H_LEVEL, 4, fold), ks_groups.ks_tile_rows(H_LEVEL, 4)


def test_h_headline_batch_48_in_one_tile(monkeypatch):
    """batch 48 under lsa_set_tile_batch(0) (cap 64: one tile).  The tile's workspace is 48 x rows x N x 8 bytes: 5.18e9 bytes with
    the tensor product as a kernel of its own (LSA_HMULT_FOLD=0, 206 rows: 6.4 GiB at the cap of 64, where pick_tile's
    comment has 6.6), beyond 2^32; the folded form (167 rows, 4.20e9) and the rotation (141 rows, 3.55e9) stay just below it at 48 and
    pass it at 64 (the next test).  HMult + relinearise + rescale in both forms and the rotation by 5, every position against
    the oracle."""
    r = _headline()
    n = r.n
    (rows_unfolded, ks_rows), rows_folded = _headline_rows(False), _headline_rows(True)[0]
    assert (rows_unfolded, rows_folded, ks_rows) == (206, 167, 141)
    assert ks_groups.auto_tile(n, rows_unfolded, 48) == 48
    assert 48 * rows_unfolded * n * 8 > 1 << 32 and 64 * rows_unfolded * n * 8 == int(6.4375 * GIB)
    folded = r.held("mul", "batch 48, folded", batch=48)
    monkeypatch.setenv("LSA_HMULT_FOLD", "0")
    assert np.array_equal(r.held("mul", "batch 48, LSA_HMULT_FOLD=0", batch=48), folded)
    monkeypatch.delenv("LSA_HMULT_FOLD")
    del folded
    r.held("rot", "batch 48, rotation by 5", batch=48)


def test_h_headline_batch_64_the_full_tile():
    """the cap itself, the tile bench.py runs: one tile of 64, whose workspace is 5.60e9 bytes (folded HMult) and 4.73e9 (rotation),
    both beyond 2^32; the same three oracle results"""
    r = _headline()
    n = r.n
    rows_folded, ks_rows = _headline_rows(True)
    assert ks_groups.tile_cap(n) == 64 and ks_groups.auto_tile(n, rows_folded, 64) == 64
    assert 64 * ks_rows * n * 8 > 1 << 32 and 64 * rows_folded * n * 8 > 1 << 32
    r.held("mul", "batch 64, folded")
    r.held("rot", "batch 64, rotation by 5")
