"""CKKS bootstrapping on the rings whose transforms take two passes (or the whole-limb plan), bit for bit against the oracle
program: the method of tests/test_gpu_bootstrap.py::test_bootstrap_bit_exact_against_the_oracle_program (the device plan's
floating-point constants go to oracle.ckks_bootstrap.Bootstrapper, both sides use the same keys, np.array_equal on the
refreshed ciphertext, the reference's >= 10-bit precision assertion, unittests/test_gpu_ckks.cpp:763-781, on the device
result) at N = 2^13 .. 2^16, where that file stops at 2^11 and so never leaves the one-pass kernel.  Chain:
params.CKKS_BOOTSTRAP_65536 (25 Q + 5 P; q0 and P are integer-engine limbs, the 40-bit limbs FP64-engine ones, so both
engines and both k_ntt_r16_ksmac<MU, FP> launches run).

Which ring reaches which kernels (make_ntt_plan, ntt_r16_shape_ok, ntt_launch_r16):

| N    | plan                                                                    | kernels reached                                                                 |
|------|-------------------------------------------------------------------------|---------------------------------------------------------------------------------|
| 2^13 | default: whole-limb, chosen per launch; `LSA_NTT_WIDE=0`: 6 + 7 stages  | `k_ntt_pass<..,512>`; staged first pass + `k_ntt_r16<1,.,7>`, `ksmac<7,.>`      |
| 2^14 | default: whole-limb per launch; `LSA_NTT_WIDE=0`: 7 + 7                 | `k_ntt_pass<..,1024>`; `k_ntt_r16<0,0,7>`, `<1,.,7>`, `ksmac<7,.>`              |
| 2^15 | 7 + 8                                                                   | `k_ntt_r16<0,0,7>`, `<1,.,8>`, `ksmac<8,.>`                                     |
| 2^16 | 8 + 8                                                                   | `k_ntt_r16<0,.,8>` incl. the `<0,1,8>` prologue, `<1,.,8>`, `ksmac<8,.>`        |

What the program runs beyond the single operators other files test: mod_raise (inverse NTT at level 0, launch_lift_ringt to
25 limbs, forward NTT of 2 x 25 rows), ckks_switch_key at level 0 with a level-0 key and at the top level with
np = 5 / beta = 5 / 30 target limbs (swk_dts, swk_std), conj, mul_by_i, mul_int_add_const / launch_add_const, the SubSum
rotations of sparse packing, and EvalMod's 44 multiplications, many of which read the leading rows of a higher-level operand,
with a batch of 2m.

The oracle is the cost.  One `Bootstrapper.bootstrap` of one ciphertext on one CPU thread of the development machine, the
plan's plaintexts handed to it (encoding them itself, as a bare `Bootstrapper(ev)` does, roughly doubles the time: 39.9 s at
2^13), construction and key generation not counted: 2.2 s at N = 2^10, 21.4 s at 2^13, 42.0 s at 2^14, 99.4 s at 2^15 with
encapsulation; the three-step prefix at 2^16 with encapsulation 18.5 s per ciphertext (17 s of it the first matrix).  Key
generation: 5.6 s (29 keys, 2^13), 11 s (2^14), 28 s (2^15), about 1.4 s per key at 2^16.
One oracle replay serves every device configuration of a ring (the device constants are asserted equal across them), so
a switch costs a device run, not an oracle run."""
import numpy as np
import pytest

from tests.gpu_util import env, need_gpu

pytestmark = pytest.mark.gpu

D = float(2 ** 40)
_CASES = {}        # (log_n, log_slots, encapsulate) -> the oracle side of a ring: built once, shared by its device configurations


class _Case:
    """keys, ciphertexts and (lazily, per batch position) the oracle's refreshed ciphertexts of one ring"""

    def __init__(self, log_n, log_slots, encapsulate, seed, batch=2):
        from lattisense_amd import params
        from oracle.ckks_bootstrap import Evaluator
        from oracle.client import Client
        from oracle.pyoracle import Oracle
        self.B = B = params.CKKS_BOOTSTRAP_65536
        self.log_n, self.log_slots, self.N = log_n, log_slots, 1 << log_n
        self.ns = (1 << log_slots) if log_slots else self.N // 2
        self.top = len(B["q"]) - 1
        self.o = Oracle(self.N, B["q"], B["p"], 0)
        # encapsulation: dense main secret, ephemeral secret of Hamming weight 32; else a sparse main secret
        self.c = Client(self.o, seed=seed, hamming=None if encapsulate else 32)
        self.ev = Evaluator(self.o, self.c, self.top)
        self.dts = self.std = None
        if encapsulate:
            sparse = Client(self.o, seed=seed + 1, hamming=32)
            self.dts = self.c.gen_switching_key(self.c.s_ntt, sparse.s_ntt, 0)
            self.std = self.c.gen_switching_key(sparse.s_ntt, self.c.s_ntt, self.top)
        rng = np.random.default_rng(seed + 2)
        self.zs = [rng.uniform(-1, 1, self.ns) + 1j * rng.uniform(-1, 1, self.ns) for _ in range(batch)]      # different messages
        self.cts = np.stack([self.c.ckks_encrypt(np.tile(z, (self.N // 2) // self.ns), 0, D) for z in self.zs])
        self.keys = None
        self.constants = None
        self.want = {}

    def galois_keys(self, elements):
        if self.keys is None:
            self.keys = {e: self.c.gen_galois_key(e, self.top) for e in elements}
            self.ev.glk = dict(self.keys)          # both sides rotate with the same keys
        assert sorted(self.keys) == sorted(elements)
        return self.keys

    def same_constants(self, plan):
        """the oracle is fed the FIRST device configuration's constants; every later one must have made the same integers"""
        plains, cheb = plan.oracle_plains(), plan.chebyshev()
        if self.constants is None:
            self.constants = (plains, cheb, plan.double_hoist)
            return
        p0, c0, dh0 = self.constants
        assert dh0 == plan.double_hoist and np.array_equal(c0, cheb) and sorted(p0) == sorted(plains)
        for key in p0:
            assert sorted(p0[key]) == sorted(plains[key]), key
            for k in p0[key]:
                assert np.array_equal(p0[key][k], plains[key][k]), (key, k)

    def bootstrapper(self):
        from oracle.ckks_bootstrap import Bootstrapper, SparseBootstrapper
        plains, cheb, dh = self.constants
        cfg = dict(out_scale=D, plains=plains, coeffs=cheb, double_hoist=dh)
        return SparseBootstrapper(self.ev, self.log_slots, **cfg) if self.log_slots else Bootstrapper(self.ev, **cfg)

    def oracle(self, b):
        from oracle.ckks_bootstrap import Ct
        if b not in self.want:
            w = self.bootstrapper().bootstrap(Ct(self.cts[b], 0, D), self.top, self.dts, self.std)
            assert w.scale == D
            self.want[b] = w
        return self.want[b]


def _release(case):
    """after a ring's last configuration: its keys and plaintexts (gigabytes at N = 2^15) need not outlive it"""
    for key in [k for k, v in _CASES.items() if v is case]:
        del _CASES[key]


def _case(log_n, log_slots=0, encapsulate=False):
    key = (log_n, log_slots, encapsulate)
    if key not in _CASES:
        _CASES[key] = _Case(log_n, log_slots, encapsulate, seed=100 * log_n + log_slots)
    return _CASES[key]


def _device(case, positions=None):
    """one device bootstrap of the case's ciphertexts (all of them, or the listed batch positions) in a context of its own:
    made here, so under the caller's CONTEXT / PLAN switches"""
    from lattisense_amd.device import ALGO_CKKS, BootstrapPlan, DeviceContext
    ctx = DeviceContext(ALGO_CKKS, case.N, case.B["q"], case.B["p"])
    try:
        plan = BootstrapPlan(ctx, in_scale=D, out_scale=D, log_slots=case.log_slots)
        assert plan.out_level == 9 and plan.out_scale == D and plan.sparse == bool(case.log_slots)
        keys = case.galois_keys(plan.galois_elements)
        case.same_constants(plan)
        rlk = ctx.upload_key(case.ev.rlk, case.top)
        glk = {e: ctx.upload_key(k, case.top) for e, k in keys.items()}
        kd = ctx.upload_key(case.dts, 0) if case.dts is not None else None
        ks = ctx.upload_key(case.std, case.top) if case.std is not None else None
        cts = case.cts if positions is None else case.cts[list(positions)]
        out = plan.run(ctx.upload(cts), len(cts), rlk, glk, kd, ks)
        got = ctx.download(out, (len(cts), 2, plan.out_level + 1, case.N))
        plan.close()
        return got
    finally:
        ctx.close()


def _precise(case, b, got):
    from oracle.client import mean_precision_bits
    re, im = mean_precision_bits(case.zs[b], case.c.ckks_decrypt(got, D)[: case.ns])
    print("N=2^%d position %d: mean precision %.1f / %.1f bits" % (case.log_n, b, re, im))
    assert re >= 10 and im >= 10, (b, re, im)


_FULL = [(13, None, None), (13, "0", None), (13, "0", "LSA_BT_NO_MULTI_MAC"), (13, None, "LSA_MACM_NO_XCD"), (14, None, None), (14, "0", None)]


@pytest.mark.parametrize("log_n,wide,extra", _FULL)
def test_full_replay_whole_limb_and_two_pass_plans(log_n, wide, extra):
    """Sparse main secret, no encapsulation, device batch 2 with two different ciphertexts, the oracle replays both.
    LSA_NTT_WIDE is a CONTEXT switch: unset, the whole-limb kernel is chosen per launch; "0", every transform takes two passes.
    extra: the two A/B switches of the plaintext multi-MAC (LSA_BT_NO_MULTI_MAC: one k_mac_plain launch per giant step;
    LSA_MACM_NO_XCD: the multi-MAC's workgroups without the XCD deal), CALL lifetime, set for the run: the same program, so the
    same oracle replay holds them."""
    need_gpu()
    case = _case(log_n)
    with env(**{"LSA_NTT_WIDE": wide, **({extra: "1"} if extra else {})}):
        got = _device(case)
    for b in range(2):
        want = case.oracle(b)
        assert want.level == 9
        assert np.array_equal(got[b], want.data), (log_n, wide, extra, b)
        _precise(case, b, got[b])
    assert sorted(case.ev.glk) == sorted(case.keys)          # the oracle program needed no key beyond the plan's
    if (log_n, wide, extra) == [f for f in _FULL if f[0] == log_n][-1]:
        _release(case)


@pytest.mark.parametrize("scatter", [True, False])
def test_full_replay_n15_with_encapsulation(scatter):
    """Dense main secret, swk_dts at level 0, swk_std at the top level; device batch 2 with two different ciphertexts.  The
    oracle replays batch position 1 (a stride or batch-index slip shows at a non-zero position); position 0 gets the precision
    assertion and must equal a second device run of that ciphertext alone at batch 1.
    The extra case at this ring is LSA_ROT_SCATTER=0 rather than LSA_BT_DOUBLE_HOIST=0: the permutation form of every rotation
    (k_permute_ext / k_permute after the MAC / ModDown) computes the same program, so it is held to the oracle replay already
    made, at the price of a device run; without double hoisting the program itself changes and the oracle (about 200 s) would
    have to replay it again."""
    need_gpu()
    case = _case(15, encapsulate=True)
    with env(LSA_ROT_SCATTER=None if scatter else "0"):
        got = _device(case)
        alone = _device(case, positions=(0,))
    want = case.oracle(1)
    assert want.level == 9
    assert np.array_equal(got[1], want.data), scatter
    assert np.array_equal(got[0], alone[0]), scatter
    assert not np.array_equal(got[0], got[1])
    _precise(case, 0, got[0])
    _precise(case, 1, got[1])
    assert sorted(case.ev.glk) == sorted(case.keys)
    if not scatter:
        _release(case)


def test_sparse_packing_on_a_two_pass_ring():
    """SparseBootstrapper at N = 2^13 with LSA_NTT_WIDE=0, 2^9 slots: SubSum runs log N - 1 - log_slots = 3 rotations"""
    need_gpu()
    case = _case(13, log_slots=9)
    with env(LSA_NTT_WIDE="0"):
        got = _device(case)
    for b in range(2):
        want = case.oracle(b)
        assert want.level == 9
        assert np.array_equal(got[b], want.data), b
        _precise(case, b, got[b])
    assert sorted(case.ev.glk) == sorted(case.keys)
    _release(case)


def test_n16_checkpointed_prefix_then_the_full_run():
    """N = 2^16, the reference's parameter set (main secret of Hamming weight 192, ephemeral one of 32, both switching keys), batch
    2.  A full oracle bootstrap is too slow here, so the LSA_BT_STOP diagnostic (CALL lifetime) returns the device's
    intermediates of steps 1 (mul_int), 2 (switch to the sparse secret + mod_raise) and 3 (switch back + the first CoeffsToSlots
    matrix at level 24), which are compared with the oracle's (tests/bootstrap_replay.py) at both batch positions; then the
    switch is unset and the full run gets the reference's precision assertion."""
    need_gpu()
    from lattisense_amd import params
    from lattisense_amd.device import ALGO_CKKS, BootstrapPlan, DeviceContext
    from oracle.ckks_bootstrap import Bootstrapper, Ct, Evaluator, rotations_of
    from oracle.client import Client, galois_element_for_col_rotation, mean_precision_bits
    from oracle.pyoracle import Oracle
    from tests.bootstrap_replay import emitted, limb_equality, steps
    B = params.CKKS_BOOTSTRAP_65536
    N, top, batch = 1 << 16, len(B["q"]) - 1, 2
    o = Oracle(N, B["q"], B["p"], 0)
    c, sparse = Client(o, seed=1616, hamming=192), Client(o, seed=1617, hamming=32)
    ctx = DeviceContext(ALGO_CKKS, N, B["q"], B["p"])
    try:
        plan = BootstrapPlan(ctx, in_scale=D, out_scale=D)
        assert plan.out_level == 9 and not plan.sparse and len(plan.galois_elements) == 48
        ev = Evaluator(o, c, top)
        rlk = ctx.upload_key(ev.rlk, top)
        # the oracle's prefix rotates by the first matrix's baby and giant steps only: those keys stay on the host (157 MB each),
        # the others go to the device and are dropped
        _, _, ks0, plains0 = plan.matrix(0)
        bt = Bootstrapper(ev, out_scale=D, plains={("cts", 0): plains0}, coeffs=plan.chebyshev(), double_hoist=plan.double_hoist)
        assert sorted(bt.cts[0]) == sorted(ks0)
        prefix = {galois_element_for_col_rotation(r, N) for r in rotations_of(bt.cts[0], N // 2)}
        assert prefix <= set(plan.galois_elements)
        glk = {}
        for e in plan.galois_elements:
            k = c.gen_galois_key(e, top)
            glk[e] = ctx.upload_key(k, top)
            if e in prefix:
                ev.glk[e] = k
        dts = c.gen_switching_key(c.s_ntt, sparse.s_ntt, 0)
        std = c.gen_switching_key(sparse.s_ntt, c.s_ntt, top)
        kd, ks = ctx.upload_key(dts, 0), ctx.upload_key(std, top)
        rng = np.random.default_rng(1618)
        zs = [rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2) for _ in range(batch)]
        cts = np.stack([c.ckks_encrypt(z, 0, D) for z in zs])
        dev_in = ctx.upload(cts)
        shape = (batch, 2, plan.out_level + 1, N)
        got = {}
        for step in (1, 2, 3):
            with env(LSA_BT_STOP=str(step)):
                got[step] = ctx.download(plan.run(dev_in, batch, rlk, glk, kd, ks), shape)
        for b in range(batch):
            for step, name, want in steps(bt, Ct(cts[b], 0, D), top, dts, std):
                lv, wd = emitted(want, plan.out_level)
                assert (lv, want.level) == {1: (0, 0), 2: (9, 24), 3: (9, 23)}[step]
                # `emit` returns only the first out_level + 1 = 10 limbs of an intermediate, so limbs 10..24 of the mod_raise
                # output (step 2) are never compared directly.  Step 3 holds them: the key switch back to the main secret and
                # the key switches inside the first matrix decompose ALL 25 limbs and convert every digit into every target
                # limb, so a wrong word in limbs 10..24 of step 2 changes limbs 0..9 of step 3.
                assert np.array_equal(got[step][b][:, : lv + 1], wd), (b, step, name, limb_equality(got[step][b], wd, lv))
                if step == 3:
                    break
        assert sorted(ev.glk) == sorted(prefix)               # the prefix needed exactly the first matrix's keys
        full = ctx.download(plan.run(dev_in, batch, rlk, glk, kd, ks), shape)          # LSA_BT_STOP unset again
        assert not np.array_equal(full[0], got[3][0])
        for b in range(batch):
            re, im = mean_precision_bits(zs[b], c.ckks_decrypt(full[b], D))
            print("N=2^16 bootstrap, position %d: level 0 -> %d, mean precision %.1f / %.1f bits" % (b, plan.out_level, re, im))
            assert re >= 10 and im >= 10
        plan.close()
    finally:
        ctx.close()
