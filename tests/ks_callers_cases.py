"""The case table of tests/test_gpu_ks_callers.py and tools/record_ks_callers.py: one seeded call of every entry point that reaches a
key-switch tile (lattisense_amd/csrc/key_switch.h KsTile), and what is kept of it -- the SHA-256 of the output words and, for each
of the five profiler kinds, the launches and the algorithmic bytes of the call (lsa_profile_begin(ctx, 1) / lsa_profile_read).
Nothing here judges a word: the golden file holds what the library itself produced at the commit the file was recorded at, and
the test asks for equality.

Shapes, the smallest at which each path exists:
  ckks12  N = 2^12, four Q limbs and the special primes of the headline chain: single-pass transforms, one digit, never fused
  ckks14  N = 2^14, five Q and two P limbs of the headline chain's 46-bit primes: two-pass transforms, FP64 target limbs, so a
          single-key switch runs the fused second pass + key MAC; three digits, the last of one limb (the ModUp lift)
  bfv12   N = 2^12, the three Q limbs and one special prime of BFV_DEFAULT[8192]
  bfv14   N = 2^14 (the largest ring with the gathering tails), five Q and two P limbs of BFV_DEFAULT[16384]
Batch 3 in tiles of 2: a full tile and a ragged one.  Operands and keys are uniform residues; every case draws from its own seed."""
import contextlib
import ctypes
import hashlib
import zlib

import numpy as np

from tests.gpu_util import env, rand_ct

BATCH, TILE = 3, 2
KINDS = 5                                                  # NTT pass, base conversion, key MAC, tensor, other element-wise
SETTINGS = {"default": dict(fuse=1, dual=0), "unfused_tails": dict(fuse=0, dual=0), "dual_stream": dict(fuse=1, dual=1)}


def _lib():
    from lattisense_amd._native import lib
    return lib()


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


class Rig:
    """one context at its top level; keys are made on first use and kept"""

    def __init__(self, name, algo, n, q, p, t=0):
        from lattisense_amd.device import DeviceContext
        self.name, self.n, self.q, self.p = name, n, list(q), list(p)
        self.level = len(self.q) - 1
        self.L = len(self.q)
        self.ctx = DeviceContext(algo, n, q, p, t)
        self._keys, self.plans = {}, {}

    def key(self, what):
        """the key of a Galois element, or "rlk"/"swk": uniform residues seeded by its name"""
        if what not in self._keys:
            rng = np.random.default_rng(_seed(self.name, "key", what))
            beta = -(-self.L // len(self.p))
            raw = np.empty((beta, 2, self.L + len(self.p), self.n), dtype=np.uint64)
            for j, m in enumerate(self.q + self.p):
                raw[:, :, j, :] = rng.integers(0, m, size=(beta, 2, self.n), dtype=np.uint64)
            self._keys[what] = self.ctx.upload_key(raw, self.level)
        return self._keys[what]

    def keys(self, elements):
        return {g: self.key(g) for g in elements}

    def rng(self, case):
        return np.random.default_rng(_seed(self.name, case))

    def ct(self, rng, polys=2, limbs=None):
        return rand_ct(rng, self.q[: limbs or self.L], polys, self.n, BATCH)

    @contextlib.contextmanager
    def settings(self, fuse, dual):
        L, h = _lib(), self.ctx.h
        try:
            assert L.lsa_set_tile_batch(h, TILE) == 0 and L.lsa_set_dual_stream(h, dual) == 0 and L.lsa_set_fuse_tails(h, fuse) == 0
            yield
        finally:
            assert L.lsa_set_tile_batch(h, 0) == 0 and L.lsa_set_dual_stream(h, 0) == 0 and L.lsa_set_fuse_tails(h, 1) == 0

    def close(self):
        for p in self.plans.values():
            p.close()
        for k in self._keys.values():
            self.ctx.destroy_key(k)
        self.plans, self._keys = {}, {}
        self.ctx.close()


def make_rig(name):
    from lattisense_amd import params
    from lattisense_amd.device import ALGO_BFV, ALGO_CKKS
    H = params.CKKS_DEFAULT[65536]
    if name == "ckks12":
        return Rig(name, ALGO_CKKS, 1 << 12, H["q"][:4], H["p"])
    if name == "ckks14":
        return Rig(name, ALGO_CKKS, 1 << 14, H["q"][1:6], H["q"][6:8])
    if name == "bfv12":
        B = params.BFV_DEFAULT[8192]
        return Rig(name, ALGO_BFV, 1 << 12, B["q"], B["p"], B["t"])
    B = params.BFV_DEFAULT[16384]
    return Rig(name, ALGO_BFV, 1 << 14, B["q"][:5], B["p"], B["t"])


# ---- the cases.  case(rig) -> make; make() uploads fresh operands and returns (call, outputs): call() queues the one library call,
# outputs() the device buffers it wrote, in a fixed order.  Plans are made once per rig, outside the profiled call.
def _rotations(rig):
    n = rig.n
    return [5, pow(5, 3, 2 * n), 2 * n - 1]


def _words(rig, polys=2, limbs=None):
    return polys * (limbs or rig.L) * rig.n


def _relin(entry):
    def case(rig):
        def make():
            from lattisense_amd._native import check
            ctx = rig.ctx
            d3 = ctx.upload(rig.ct(rig.rng(entry), 3))
            out = ctx.alloc(BATCH * _words(rig))
            fn = getattr(_lib(), "lsa_" + entry)
            return (lambda: check(fn(ctx.h, rig.level, d3.ptr, rig.key("rlk"), out.ptr, BATCH, _words(rig, 3), _words(rig), ctx.stream)),
                    lambda: [(out, BATCH * _words(rig))])
        return make
    return case


def _rotate(entry, in_place):
    def case(rig):
        def make():
            from lattisense_amd._native import check
            ctx, w = rig.ctx, _words(rig)
            x = ctx.upload(rig.ct(rig.rng(entry)))
            out = x if in_place else ctx.alloc(BATCH * w)
            fn = getattr(_lib(), "lsa_" + entry)
            return (lambda: check(fn(ctx.h, rig.level, x.ptr, 5, rig.key(5), out.ptr, BATCH, w, w, ctx.stream)), lambda: [(out, BATCH * w)])
        return make
    return case


def _rotate_many(entry):
    """three rotations; the second output is the input itself"""
    def case(rig):
        def make():
            from lattisense_amd._native import check
            ctx, w, g = rig.ctx, _words(rig), _rotations(rig)
            x = ctx.upload(rig.ct(rig.rng(entry)))
            outs = [ctx.alloc(BATCH * w), x, ctx.alloc(BATCH * w)]
            els = (ctypes.c_uint64 * 3)(*g)
            hk = (ctypes.c_void_p * 3)(*[rig.key(e).value for e in g])
            po = (ctypes.c_void_p * 3)(*[o.ptr for o in outs])
            fn = getattr(_lib(), "lsa_" + entry)
            return (lambda: check(fn(ctx.h, rig.level, x.ptr, 3, els, hk, po, BATCH, w, w, ctx.stream)), lambda: [(o, BATCH * w) for o in outs])
        return make
    return case


def _ckks_mult_relin_rescale(rig):
    def make():
        ctx, rng = rig.ctx, rig.rng("mrr")
        a, b = ctx.upload(rig.ct(rng)), ctx.upload(rig.ct(rng))
        out = ctx.alloc(BATCH * _words(rig, 2, rig.level))
        return (lambda: ctx.ckks_mult_relin_rescale(rig.level, a, b, rig.key("rlk"), BATCH, out=out), lambda: [(out, BATCH * _words(rig, 2, rig.level))])
    return make


def _ckks_dot(rig):
    def make():
        ctx, rng = rig.ctx, rig.rng("dot")
        a, b = [ctx.upload(rig.ct(rng)) for _ in range(2)], [ctx.upload(rig.ct(rng)) for _ in range(2)]
        out = ctx.alloc(BATCH * _words(rig, 2, rig.level))
        return (lambda: ctx.ckks_dot(rig.level, a, b, rig.key("rlk"), BATCH, rescale=True, out=out), lambda: [(out, BATCH * _words(rig, 2, rig.level))])
    return make


def _ckks_lt(giant_scatter):
    """four diagonals split 2 x 2: one baby-step rotation (rotate_many_ext), one giant step (rotate_ext), two divisions (moddown_ext)"""
    def case(rig):
        from lattisense_amd.device import LinearTransformPlan
        if "lt" not in rig.plans:
            rng = rig.rng("lt_plan")
            rig.plans["lt"] = LinearTransformPlan(rig.ctx, rig.level, {k: rng.uniform(-1, 1, 8) + 1j * rng.uniform(-1, 1, 8) for k in range(4)}, ratio=1.0)
        plan = rig.plans["lt"]
        assert plan.n1 == 2 and len(plan.diagonals) == 4 and plan.double_hoist

        def make():
            ctx = rig.ctx
            x = ctx.upload(rig.ct(rig.rng("lt")))
            out = ctx.alloc(BATCH * _words(rig, 2, rig.level))
            glk = rig.keys(plan.galois_elements)

            def call():
                with env(LSA_LT_GIANT_SCATTER="1" if giant_scatter else "0"):   # read per call; the library has no setter for it
                    plan.run(x, BATCH, glk, rescale=True, out=out)
            return call, lambda: [(out, BATCH * _words(rig, 2, rig.level))]
        return make
    return case


def _ckks_slot_sum(multi_mac):
    """count 13, radix 4: a step of four keys (three NEXT, one TAIL), a step of two, and the tail's division"""
    def case(rig):
        from lattisense_amd.device import SlotSumPlan
        if "slot_sum" not in rig.plans:
            rig.plans["slot_sum"] = SlotSumPlan(rig.ctx, rig.level, 3, 13, 4)
        plan = rig.plans["slot_sum"]
        # more key MACs than steps: some step has two keys or more; one division more than steps: the plan has a tail
        assert plan.keyswitches > plan.steps >= 1 and plan.moddowns == plan.steps + 1

        def make():
            ctx = rig.ctx
            x = ctx.upload(rig.ct(rig.rng("slot_sum")))
            out = ctx.alloc(BATCH * _words(rig))
            glk = rig.keys(plan.galois_elements)

            def call():
                plan.multi_mac = multi_mac
                plan.run(x, BATCH, glk, out=out)
            return call, lambda: [(out, BATCH * _words(rig))]
        return make
    return case


def _pt_mul(rig, rng):
    return rand_ct(rng, rig.q, 1, rig.n, BATCH)


def _bfv_rotate_mac(rig):
    def make():
        ctx, rng = rig.ctx, rig.rng("rotmac")
        x = ctx.upload(rig.ct(rng))
        g = _rotations(rig)[:2]
        terms = [(1, None, ctx.upload(_pt_mul(rig, rng)))] + [(e, rig.key(e), ctx.upload(_pt_mul(rig, rng))) for e in g]
        box = []
        return (lambda: box.append(ctx.bfv_rotate_mac_plain_mul(rig.level, x, terms, BATCH)), lambda: [(box[-1], BATCH * _words(rig))])
    return make


def _bfv_lt(rig):
    from lattisense_amd.device import BfvLinearTransformPlan
    if "bfv_lt" not in rig.plans:
        rng = rig.rng("bfv_lt_plan")
        rig.plans["bfv_lt"] = BfvLinearTransformPlan(rig.ctx, rig.level, {k: rng.integers(0, rig.ctx.t, (2, 8), dtype=np.uint64) for k in (0, 1, 2, 5)})
        rig.plans["bfv_lt"]._handle()
    plan = rig.plans["bfv_lt"]
    assert len(plan.diagonals) == 4

    def make():
        ctx = rig.ctx
        x = ctx.upload(rig.ct(rig.rng("bfv_lt")))
        out = ctx.alloc(BATCH * _words(rig))
        glk = rig.keys(plan.galois_elements)
        return (lambda: plan.run(x, BATCH, glk, out=out), lambda: [(out, BATCH * _words(rig))])
    return make


def _bfv_slot_sum(gather):
    """rows = 1 and count 13: the row step, then the column steps with TAIL keys.  gather: the library's default on these rings,
    the ModDown tail gathering the rotated c0 terms; off: the plain form, c0 transformed too and riding through the MACs as P * c0"""
    def case(rig):
        from lattisense_amd.device import BfvSlotSumPlan
        name = "bfv_slot_sum" if gather else "bfv_slot_sum_plain"
        if name not in rig.plans:
            rig.plans[name] = BfvSlotSumPlan(rig.ctx, rig.level, 3, 13, 4, rows=1)
            rig.plans[name].gather = gather
        plan = rig.plans[name]
        assert plan.keyswitches > plan.steps >= 2 and plan.moddowns == plan.steps + 1

        def make():
            ctx = rig.ctx
            x = ctx.upload(rig.ct(rig.rng("bfv_slot_sum")))
            out = ctx.alloc(BATCH * _words(rig))
            glk = rig.keys(plan.galois_elements)

            def call():
                plan.run(x, BATCH, glk, out=out)
                assert plan.gather_in_force() == gather
            return call, lambda: [(out, BATCH * _words(rig))]
        return make
    return case


CKKS_CASES = {
    "relin": _relin("ckks_relin"),
    "rotate": _rotate("ckks_rotate", False),
    "rotate_in_place": _rotate("ckks_rotate", True),
    "rotate_many": _rotate_many("ckks_rotate_many"),
    "mult_relin_rescale": _ckks_mult_relin_rescale,
    "dot_rescale": _ckks_dot,
    "lt_giant_permute": _ckks_lt(False),
    "lt_giant_scatter": _ckks_lt(True),
    "slot_sum": _ckks_slot_sum(False),
    "slot_sum_multi_mac": _ckks_slot_sum(True),
}
BFV_CASES = {
    "relin": _relin("bfv_relin"),
    "rotate": _rotate("bfv_rotate", False),
    "rotate_many": _rotate_many("bfv_rotate_many"),
    "rotate_mac_plain_mul": _bfv_rotate_mac,
    "lt": _bfv_lt,
    "slot_sum": _bfv_slot_sum(True),
    "slot_sum_plain": _bfv_slot_sum(False),
}
RIGS = {"ckks12": CKKS_CASES, "ckks14": CKKS_CASES, "bfv12": BFV_CASES, "bfv14": BFV_CASES}
CASE_IDS = [(r, c, s) for r, cases in RIGS.items() for c in cases for s in SETTINGS]


def golden_key(rig, case, setting):
    return "%s/%s/%s" % (rig, case, setting)


def measure(rig, case, setting):
    """{"sha256", "launched" [KINDS], "bytes" [KINDS]} of one call of `case` on `rig` under `setting`"""
    L, ctx = _lib(), rig.ctx
    with rig.settings(**SETTINGS[setting]):
        make = RIGS[rig.name][case](rig)
        call, _ = make()
        call()                                             # first use: permutation tables, conversion plans, the arenas
        ctx.sync()
        call, outputs = make()
        assert L.lsa_profile_begin(ctx.h, 1) == 0
        try:
            call()
            ctx.sync()
        finally:
            assert L.lsa_profile_end(ctx.h) == 0
        launched, nbytes = [], []
        for kind in range(KINDS):
            by, n = ctypes.c_double(), ctypes.c_longlong()
            assert L.lsa_profile_read(ctx.h, kind, None, ctypes.byref(by), None, ctypes.byref(n)) == 0
            assert by.value == int(by.value)               # computed from shapes: an integer in a double
            launched.append(n.value)
            nbytes.append(int(by.value))
        sha = hashlib.sha256()
        for buf, words in outputs():
            sha.update(ctx.download(buf, (words,)).tobytes())
    return {"sha256": sha.hexdigest(), "launched": launched, "bytes": nbytes}
