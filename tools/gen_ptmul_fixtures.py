"""Generates the BFV pt_mul task fixtures under tests/golden/tasks/ with the reference's Python frontend.

Like tools/gen_task_fixtures.py it runs only where the reference frontend is importable and writes plain JSON data
(mega_ag.json + task_signature.json per task).  It only ADDS directories: node ids are random, so an existing fixture is
never regenerated (tests pin its contents).  pt_mul plaintexts (BfvPlaintextMulNode) are NTT-domain, Montgomery-form
residues at the ciphertext's level; the graphs follow the reference's BFV_cmp_mul test and ct_pt_mult_accumulate.
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
    # 4 x ct * pt_mul at level 2; the last one written pt_mul * ct
    set_fhe_param(bfv_param(4096, 4))
    xs = [BfvCiphertextNode(f"x_{i}", level=2) for i in range(4)]
    ys = [BfvPlaintextMulNode(f"y_{i}", level=2) for i in range(4)]
    zs = [mult(xs[i], ys[i], f"z_{i}") if i < 3 else mult(ys[i], xs[i], f"z_{i}") for i in range(4)]
    emit("bfv_n4096_cmp_mul", [Argument("xs", xs), Argument("ys", ys)], [Argument("zs", zs)])

    # 3-term dot product: the frontend emits mult(c_0, p_0) and a 2-term cmpac_sum over it
    set_fhe_param(bfv_param(4096, 4))
    cs = [BfvCiphertextNode(f"c_{i}", level=2) for i in range(3)]
    ps = [BfvPlaintextMulNode(f"p_{i}", level=2) for i in range(3)]
    z = ct_pt_mult_accumulate(cs, ps)
    emit("bfv_n4096_cmpac_mul", [Argument("cs", cs), Argument("ps", ps)], [Argument("zs", [z])])

    # 20 terms on the default N = 16384 parameters at the top level: a 16-term cmp_sum and a 4-term cmpac_sum
    B = P.BFV_DEFAULT[16384]
    set_fhe_param(BfvParam.create_custom_param(n=16384, q=B["q"], p=B["p"], t=B["t"]))
    lv = len(B["q"]) - 1
    cs = [BfvCiphertextNode(f"c_{i}", level=lv) for i in range(20)]
    ps = [BfvPlaintextMulNode(f"p_{i}", level=lv) for i in range(20)]
    z = ct_pt_mult_accumulate(cs, ps)
    emit("bfv_n16384_cmpac_mul20", [Argument("cs", cs), Argument("ps", ps)], [Argument("zs", [z])])

    # a MAC that mixes pt_mul and ring-t plaintexts: refused at bind time
    set_fhe_param(bfv_param(4096, 4))
    cs = [BfvCiphertextNode(f"c_{i}", level=2) for i in range(3)]
    ps = [BfvPlaintextMulNode("p_0", level=2), BfvPlaintextRingtNode("p_1"), BfvPlaintextMulNode("p_2", level=2)]
    z = ct_pt_mult_accumulate(cs, ps)
    emit("bfv_n4096_cmpac_mixed_unsupported", [Argument("cs", cs), Argument("ps", ps)], [Argument("zs", [z])])


if __name__ == "__main__":
    main()
