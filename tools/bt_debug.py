"""Step-by-step comparison of the device bootstrap with the oracle program (LSA_BT_STOP diagnostic of bootstrap.hip); the
oracle's value of each device step comes from tests/bootstrap_replay.py, which tests/test_gpu_bootstrap_two_pass.py shares.
usage: bt_debug.py [log_n [log_slots]]      (log_slots: sparse packing)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from lattisense_amd import params
from lattisense_amd.device import ALGO_CKKS, DeviceContext, BootstrapPlan
from oracle.client import Client, mean_precision_bits
from oracle.pyoracle import Oracle
from oracle.ckks_bootstrap import Bootstrapper, Ct, Evaluator, SparseBootstrapper, bsgs_split
from tests.bootstrap_replay import emitted, limb_equality, steps

B = params.CKKS_BOOTSTRAP_65536
log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 10
log_slots = int(sys.argv[2]) if len(sys.argv) > 2 else 0
N = 1 << log_n
ns = (1 << log_slots) if log_slots else N // 2
o = Oracle(N, B["q"], B["p"], 0)
c = Client(o, seed=21, hamming=32)
ctx = DeviceContext(ALGO_CKKS, N, B["q"], B["p"])
top = len(B["q"]) - 1
D = float(2 ** 40)
plan = BootstrapPlan(ctx, in_scale=D, out_scale=D, log_slots=log_slots)
ev = Evaluator(o, c, top)
rlk = ctx.upload_key(ev.rlk, top)
keys = {e: c.gen_galois_key(e, top) for e in plan.galois_elements}
ev.glk = dict(keys)      # the oracle must rotate with the SAME keys (fresh ones differ in their noise)
glk = {e: ctx.upload_key(k, top) for e, k in keys.items()}
rng = np.random.default_rng(1)
z = rng.uniform(-1, 1, ns) + 1j * rng.uniform(-1, 1, ns)
ct0 = c.ckks_encrypt(np.tile(z, (N // 2) // ns), 0, D)
cfg = dict(out_scale=D, plains=plan.oracle_plains(), coeffs=plan.chebyshev(), double_hoist=plan.double_hoist)
bt = SparseBootstrapper(ev, log_slots, **cfg) if plan.sparse else Bootstrapper(ev, **cfg)
dev_in = ctx.upload(ct0[None])
for step, name, want in steps(bt, Ct(ct0, 0, D), top):
    if step is None:
        os.environ.pop("LSA_BT_STOP", None)
    else:
        os.environ["LSA_BT_STOP"] = str(step)
    out = plan.run(dev_in, 1, rlk, glk)
    got = ctx.download(out, (1, 2, plan.out_level + 1, N))[0]
    lv, wd = emitted(want, plan.out_level)
    ok = np.array_equal(got[:, : lv + 1], wd)
    print(step, name, "level", want.level, "MATCH" if ok else "DIFF", limb_equality(got, wd, lv))
    if not ok:
        zw = c.ckks_decrypt(wd, want.scale)
        zg = c.ckks_decrypt(got[:, : lv + 1], want.scale)
        print("decrypt want/got agree bits:", mean_precision_bits(zw, zg), "| first slots", zw[:2], zg[:2])
        if name.startswith("cts"):
            lvm, n1, ks, _ = plan.matrix(step - 3)
            print("device matrix level", lvm, "n1", n1, "ks", ks)
            print("oracle n1", bsgs_split(ks, ns), "oracle ks", sorted(bt.cts[step - 3]))
        break
