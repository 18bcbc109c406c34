"""A task-graph builder for tests: writes the mega_ag.json of a task directory by hand, so that a test can put a graph at the
edge of a load-time rewrite (TaskGraph::fuse_accumulations / fuse_mult_relin_rescale / fuse_rotate_mac), of the bucket
signature, of gather's stride test, of the rotation hoisting and of release_inputs; the frontend only ever emits graphs
that meet or miss those preconditions cleanly.

Test infrastructure, data only.  Field names and defaults are those of tests/golden/tasks/*/mega_ag.json; the `parameter`
block is copied from a committed fixture (CKKS: ckks_n4096_cmc_relin_rescale, BFV: bfv_n4096_cmp_mul; N = 4096, t = 65537).
The loader reads nothing but mega_ag.json, so that is all `write` produces.

    g = Graph("CKKS")
    x, y, k = g.ct(2), g.ct(2), g.rlk(2)
    z = g.rescale(g.relin(g.mult(x, y), k))
    g.output(z)
    g.write(tmp_path)

Every constructor returns the index of a datum.  Data constructors make task inputs (in the order they are called, unless
`set_inputs` says otherwise); node constructors make the result datum from the operands' level and degree, as the frontend
does.  `index=` fixes a datum's index, `at=` a compute node's (the runtime orders the nodes of a level, and so its buckets,
by compute index), `id=` / `node_id=` the names; what is not given is numbered upwards and named at random.
"""
import json
import os
import random
import string

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMETER_FIXTURE = {"CKKS": "ckks_n4096_cmc_relin_rescale", "BFV": "bfv_n4096_cmp_mul"}
PLAIN_TYPES = ("pt", "pt_ringt", "pt_mul")


def fixture_parameter(algorithm):
    path = os.path.join(ROOT, "tests", "golden", "tasks", PARAMETER_FIXTURE[algorithm], "mega_ag.json")
    with open(path) as f:
        return json.load(f)["parameter"]


class Graph:
    def __init__(self, algorithm, name="Acc task", seed=0):
        assert algorithm in PARAMETER_FIXTURE
        self.algorithm = algorithm
        self.name = name
        self.parameter = fixture_parameter(algorithm)
        self.data = {}        # index -> fields, in creation order
        self.compute = {}     # index -> fields, in creation order
        self.inputs = []
        self.outputs = []
        self._rng = random.Random(seed)

    # ------------------------------------------------------------------------------------------------ helpers
    @property
    def bfv(self):
        return self.algorithm == "BFV"

    @property
    def n(self):
        return self.parameter["n"]

    def _name(self):
        return "".join(self._rng.choice(string.ascii_lowercase) for _ in range(12))

    def _datum(self, fields, index, is_input):
        if index is None:
            index = max(self.data, default=-1) + 1
        assert index not in self.data, "datum index %d used twice" % index
        self.data[index] = fields
        if is_input:
            self.inputs.append(index)
        return index

    def _ct_fields(self, level, degree, id):
        return {"id": id or self._name(), "type": "ct3" if degree == 2 else "ct", "level": level, "degree": degree,
                "is_ntt": not self.bfv, "is_mform": False, "poly1_rns_sp_decomped": False}

    def _key_fields(self, type, id, level):
        return {"id": id, "type": type, "level": level, "degree": 1, "is_ntt": True, "is_mform": True,
                "sp_level": len(self.parameter["p"]) - 1}

    def kind(self, d):
        return self.data[d]["type"]

    def level(self, d):
        return self.data[d]["level"]

    def degree(self, d):
        return self.data[d]["degree"]

    # ------------------------------------------------------------------------------------------------ data (task inputs)
    def ct(self, level, degree=1, id=None, index=None):
        return self._datum(self._ct_fields(level, degree, id), index, True)

    def pt(self, level, id=None, index=None):
        """a full plaintext at the ciphertext's level (CKKS: NTT domain; BFV: coefficient domain)"""
        return self._datum({"id": id or self._name(), "type": "pt", "level": level, "degree": 0, "is_ntt": not self.bfv,
                            "is_mform": False}, index, True)

    def pt_ringt(self, id=None, index=None):
        """a ring-t plaintext: one limb, declared at level 0 whatever the ciphertext's level"""
        return self._datum({"id": id or self._name(), "type": "pt_ringt", "level": 0, "degree": 0, "is_ntt": False,
                            "is_mform": False}, index, True)

    def pt_mul(self, level, id=None, index=None):
        """a plaintext lifted to Q, in the NTT domain and Montgomery form"""
        return self._datum({"id": id or self._name(), "type": "pt_mul", "level": level, "degree": 0, "is_ntt": True,
                            "is_mform": True}, index, True)

    def rlk(self, level, index=None):
        return self._datum(self._key_fields("rlk", "rlk_ntt", level), index, True)

    def glk(self, element, level, index=None):
        row = element == 2 * self.n - 1
        f = self._key_fields("glk", "glk_ntt_row" if row else "glk_ntt_col_%d" % element, level)
        f["galois_element"] = element
        return self._datum(f, index, True)

    def set_inputs(self, order):
        assert sorted(order) == sorted(self.inputs)
        self.inputs = list(order)

    def output(self, d):
        self.outputs.append(d)
        return d

    # ------------------------------------------------------------------------------------------------ compute nodes
    def _node(self, type, inputs, level, degree, index, at, id, node_id, **extra):
        out = self._datum(self._ct_fields(level, degree, id), index, False)
        if at is None:
            at = max(self.compute, default=-1) + 1
        assert at not in self.compute, "compute index %d used twice" % at
        self.compute[at] = {"id": node_id or self._name(), "type": type, "inputs": list(inputs), "outputs": [out], **extra}
        return out

    def _same_shape(self, type, inputs, kw):
        a = inputs[0]
        return self._node(type, inputs, self.level(a), self.degree(a), **kw)

    @staticmethod
    def _kw(index=None, at=None, id=None, node_id=None):
        return {"index": index, "at": at, "id": id, "node_id": node_id}

    def add(self, a, b=None, **kw):
        return self._same_shape("add", [a] if b is None else [a, b], self._kw(**kw))

    def sub(self, a, b=None, **kw):
        return self._same_shape("sub", [a] if b is None else [a, b], self._kw(**kw))

    def neg(self, a, **kw):
        return self._same_shape("neg", [a], self._kw(**kw))

    def mult(self, a, b=None, **kw):
        """ct x ct (one operand: a square) -> degree 2; ct x plaintext, on either side -> the ciphertext's shape"""
        ins = [a] if b is None else [a, b]
        cts = [d for d in ins if self.kind(d) not in PLAIN_TYPES]
        if len(cts) == len(ins):
            return self._node("mult", ins, self.level(a), 2, **self._kw(**kw))
        return self._node("mult", ins, self.level(cts[0]), self.degree(cts[0]), **self._kw(**kw))

    def relin(self, a, key, **kw):
        return self._node("relin", [a, key], self.level(a), 1, **self._kw(**kw))

    def rescale(self, a, **kw):
        return self._node("rescale", [a], self.level(a) - 1, self.degree(a), **self._kw(**kw))

    def drop_level(self, a, level, **kw):
        return self._node("drop_level", [a], level, self.degree(a), **self._kw(**kw))

    def rotate_col(self, a, key, step=None, **kw):
        if step is None:   # the element is 5^step mod 2N
            e, step = self.data[key]["galois_element"], 0
            while pow(5, step, 2 * self.n) != e:
                step += 1
        return self._node("rotate_col", [a, key], self.level(a), 1, **self._kw(**kw), step=step)

    def rotate_row(self, a, key, **kw):
        return self._node("rotate_row", [a, key], self.level(a), 1, **self._kw(**kw))

    def _pt_type(self, pts, pt_type):
        if pt_type is not None:
            return pt_type
        return {"pt": "pt", "pt_ringt": "pt_ringt", "pt_mul": ""}[self.kind(pts[0])]

    def cmp_sum(self, cts, pts, pt_type=None, **kw):
        """sum_i cts[i] * pts[i]"""
        assert len(cts) == len(pts)
        return self._node("cmp_sum", list(cts) + list(pts), self.level(cts[0]), self.degree(cts[0]), **self._kw(**kw),
                          sum_cnt=len(cts), pt_type=self._pt_type(pts, pt_type))

    def cmpac_sum(self, cts, partial, pts, pt_type=None, **kw):
        """partial + sum_i cts[i] * pts[i]"""
        assert len(cts) == len(pts)
        return self._node("cmpac_sum", list(cts) + [partial] + list(pts), self.level(cts[0]), self.degree(cts[0]),
                          **self._kw(**kw), sum_cnt=len(cts), pt_type=self._pt_type(pts, pt_type))

    def reverse_compute_order(self):
        """the same nodes with the compute indices mirrored: every level's buckets form in the opposite order"""
        top = max(self.compute)
        self.compute = {top - k: v for k, v in self.compute.items()}

    # ------------------------------------------------------------------------------------------------ output
    def to_json(self):
        return {"name": self.name, "algorithm": self.algorithm,
                "data": {str(k): v for k, v in self.data.items()},
                "compute": {str(k): v for k, v in self.compute.items()},
                "inputs": list(self.inputs), "outputs": list(self.outputs), "offline_inputs": [],
                "parameter": self.parameter}

    def write(self, path):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "mega_ag.json"), "w") as f:
            json.dump(self.to_json(), f, indent=4)
        return str(path)
