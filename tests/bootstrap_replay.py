"""The oracle's side of the device bootstrap's step numbering (LSA_BT_STOP, lattisense_amd/csrc/bootstrap.hip bootstrap_run):
ONE statement of "step k of the device program = this oracle value", shared by tools/bt_debug.py and
tests/test_gpu_bootstrap_two_pass.py.

    step                      dense packing                      sparse packing
    1                         mul_int                            mul_int
    2                         mod_raise (after swk_dts)          mod_raise (after swk_dts)
    3 .. 2 + M                cts0 .. (swk_std first)            cts0 .. (swk_std, then SubSum, first); M = cts_depth - 1
    then                      u_re, u_im, y_re, y                u, y          (M = cts_depth for dense packing)
    (no number)               out: the refreshed ciphertext      out

`steps` is a generator: a caller that needs a prefix only pays for the prefix.  The values are built from the same oracle
operators, in the same order, as Bootstrapper.bootstrap / SparseBootstrapper.bootstrap (tests/test_oracle_bootstrap.py holds
the two walks to each other)."""
import numpy as np

from oracle.ckks_bootstrap import Ct, SparseBootstrapper, eval_mod, linear_transform


def steps(bt, ct, top, swk_dts=None, swk_std=None):
    """yields (step, name, Ct); step is the LSA_BT_STOP number, None for the final output"""
    ev = bt.ev
    sparse = isinstance(bt, SparseBootstrapper)
    pl = bt.plains or {}
    assert ct.level == 0
    q0 = ev.q(0)
    c = max(1, int(round(q0 / (bt.mr * ct.scale))))
    d1 = ct.scale * c
    x = ev.mul_int(ct, c)
    yield 1, "mul_int", x
    if swk_dts is not None:
        x = bt.key_switch(x, swk_dts, 0)
    x = Ct(bt.mod_raise(x, top), top, float(q0))
    yield 2, "mod_raise", x
    if swk_std is not None:
        x = bt.key_switch(x, swk_std, top)
    step = 2
    if sparse:
        ns = bt.ns
        for i in range(bt.log_slots, ev.n.bit_length() - 2):          # SubSum
            x = ev.add(x, ev.rotate(x, 1 << i))
    for i, m in enumerate(bt.cts):
        x = linear_transform(ev, x, m, n_slots=ns if sparse else None, plains=pl.get(("cts", i)), double_hoist=bt.double_hoist)
        step += 1
        yield step, "cts%d" % i, x
    if sparse:
        a = linear_transform(ev, x, bt.p1, rescale=False, n_slots=2 * ns, plains=pl.get(("p1",)), double_hoist=bt.double_hoist)
        b = linear_transform(ev, ev.conj(x), bt.p2, rescale=False, n_slots=2 * ns, plains=pl.get(("p2",)), double_hoist=bt.double_hoist)
        u = ev.rescale(ev.add(a, b))
        yield step + 1, "u", u
        y = eval_mod(ev, u, bt.K, bt.r, bt.coeffs, bt.asin, bt.sine_deg)
        yield step + 2, "y", y
    else:
        xc = ev.conj(x)
        u_re = ev.add(x, xc)
        yield step + 1, "u_re", u_re
        u_im = ev.mul_by_i(ev.sub(x, xc), -1)
        yield step + 2, "u_im", u_im
        y_re = eval_mod(ev, u_re, bt.K, bt.r, bt.coeffs, bt.asin, bt.sine_deg)
        y_im = eval_mod(ev, u_im, bt.K, bt.r, bt.coeffs, bt.asin, bt.sine_deg)
        yield step + 3, "y_re", y_re
        y = ev.add(y_re, ev.mul_by_i(y_im, 1))
        yield step + 4, "y", y
    natural = y.scale * 2 * np.pi * d1 / q0
    stc = list(bt.stc)
    if bt.out_scale is not None:
        kappa = bt.out_scale / natural
        stc[0] = {k: d * kappa for k, d in stc[0].items()}
        natural = bt.out_scale
    for i, m in enumerate(stc):
        period = None if not sparse else 2 * ns if i == 0 else ns
        y = linear_transform(ev, y, m, n_slots=period, plains=pl.get(("stc", i)), double_hoist=bt.double_hoist)
    yield None, "out", Ct(y.data, y.level, natural)


def emitted(want, out_level):
    """what the device returns for a stopped step: the first out_level + 1 limbs of the intermediate (rows past a lower level
    repeat its last limb: never compared)"""
    lv = min(want.level, out_level)
    return lv, want.data[:, : lv + 1]


def limb_equality(got, want, lv):
    """[poly][limb] equality vector of a stopped step: names the limb that differs"""
    return [[bool(np.array_equal(got[p, j], want[p, j])) for j in range(lv + 1)] for p in range(2)]
