"""Generates the BFV rotate-and-MAC task fixtures under tests/golden/tasks/ with the reference's Python frontend.

Like tools/gen_ptmul_fixtures.py it runs only where the reference frontend is importable, writes plain JSON data
(mega_ag.json + task_signature.json per task) and only ADDS directories: node ids are random, so an existing fixture is
never regenerated (tests pin its contents).  Every graph is a diagonal matrix-vector product: advanced_rotate_cols /
rotate_rows of one ciphertext X, then ct_pt_mult_accumulate over X and its rotations with pt_mul plaintexts
(BfvPlaintextMulNode).  The load-time peephole TaskGraph::fuse_rotate_mac rewrites them into FUSED_ROTATE_MAC nodes.
"""
import os
import shutil
import sys

REF = "/root/reference"
sys.path.insert(0, REF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from frontend.custom_task import *  # noqa: E402,F401,F403
from lattisense_amd import params as P  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tasks")


def emit(name, inputs, outputs):
    d = os.path.join(OUT, name)
    if os.path.exists(d):
        print("kept (exists):", name)
        return
    os.makedirs(d)
    process_custom_task(input_args=inputs, offline_input_args=[], output_args=outputs, output_instruction_path=d,
                        fpga_acc=False)
    for f in os.listdir(d):   # keep only the two files the runtime reads
        if f not in ("mega_ag.json", "task_signature.json"):
            p = os.path.join(d, f)
            shutil.rmtree(p) if os.path.isdir(p) else os.remove(p)
    print("wrote:", name)


def bfv_param(n, nq):
    D = P.BFV_DEFAULT[16384]
    return BfvParam.create_custom_param(n=n, q=D["q"][:nq], p=D["p"], t=D["t"])


def main():
    # X and its column rotations by 1, 2, 3 at level 2: the frontend emits mult(X, p_0), a 2-term and a 1-term cmpac_sum
    set_fhe_param(bfv_param(4096, 4))
    x = BfvCiphertextNode("x", level=2)
    rs = advanced_rotate_cols(x, [1, 2, 3])
    ps = [BfvPlaintextMulNode(f"p_{i}", level=2) for i in range(4)]
    z = ct_pt_mult_accumulate([x] + rs, ps)
    emit("bfv_n4096_rotmac4", [Argument("x", x), Argument("ps", ps)], [Argument("zs", [z])])

    # a row rotation and a column rotation of X, the partial sum an independent input ciphertext
    set_fhe_param(bfv_param(4096, 4))
    x = BfvCiphertextNode("x", level=2)
    y = BfvCiphertextNode("y", level=2)
    rr = rotate_rows(x)
    rc = advanced_rotate_cols(x, [5])[0]
    ps = [BfvPlaintextMulNode(f"p_{i}", level=2) for i in range(2)]
    z = ct_pt_mult_accumulate_add_ct_slice([rr, rc, y], ps)
    emit("bfv_n4096_rotmac_row_partial", [Argument("x", x), Argument("y", y), Argument("ps", ps)], [Argument("zs", [z])])

    # one rotated ciphertext is also a task output: not private, the peephole leaves the graph alone
    set_fhe_param(bfv_param(4096, 4))
    x = BfvCiphertextNode("x", level=2)
    rs = advanced_rotate_cols(x, [1, 2])
    ps = [BfvPlaintextMulNode(f"p_{i}", level=2) for i in range(2)]
    z = ct_pt_mult_accumulate_slice(rs, ps)
    emit("bfv_n4096_rotmac_shared", [Argument("x", x), Argument("ps", ps)], [Argument("zs", [z]), Argument("r", [rs[0]])])

    # default N = 16384 parameters at the top level: X plus 19 column rotations (a 16-term cmp_sum and a chained cmpac_sum)
    B = P.BFV_DEFAULT[16384]
    set_fhe_param(BfvParam.create_custom_param(n=16384, q=B["q"], p=B["p"], t=B["t"]))
    lv = len(B["q"]) - 1
    x = BfvCiphertextNode("x", level=lv)
    rs = advanced_rotate_cols(x, list(range(1, 20)))
    ps = [BfvPlaintextMulNode(f"p_{i}", level=lv) for i in range(20)]
    z = ct_pt_mult_accumulate([x] + rs, ps)
    emit("bfv_n16384_rotmac20", [Argument("x", x), Argument("ps", ps)], [Argument("zs", [z])])


if __name__ == "__main__":
    main()
