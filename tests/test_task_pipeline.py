"""CPU-only: the pipeline planner (lattisense_amd/csrc/task_pipeline.h) -- the independent subgraphs of a task graph grouped into
the chunks that lattisense_amd/csrc/shard_plan.h deals out to shards -- on committed graphs, under AddressSanitizer + UBSan
(tests/cpp/test_task_pipeline.cpp holds the properties: chunk count, every node once and at its level, keys shared, no datum in
two chunks, stores in one level, the byte threshold, nothing to plan for a small graph or for a single subgraph)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lattisense_amd", "csrc")


def test_pipeline_plan_properties(tmp_path):
    exe = str(tmp_path / "test_task_pipeline")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_task_pipeline.cpp"), os.path.join(CSRC, "task_graph.cpp"), "-o", exe])
    many = os.path.join(ROOT, "tests", "golden", "tasks_bench", "bfv_n16384_l3_cmc_relin_x256", "mega_ag.json")
    few = os.path.join(ROOT, "tests", "golden", "tasks", "ckks_n4096_cmc_relin_rescale", "mega_ag.json")
    one = os.path.join(ROOT, "tests", "golden", "tasks", "ckks_n4096_cmpac", "mega_ag.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LSA_")}   # the loader reads LSA_NO_GRAPH_FUSION
    out = subprocess.run([exe, many, few, one], capture_output=True, text=True, timeout=120,
                         env=dict(env, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert "OK task_pipeline" in out.stdout, out.stdout
