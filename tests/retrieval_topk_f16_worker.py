"""Runs the dyadic cases of tests/test_gpu_retrieval_topk.py against the library OCTMAE_LIB selects (a process binds one library:
octcubem_amd/_lib.py) and writes what passed to --out as JSON.  tests/test_gpu_retrieval_topk.py starts it with the half-operand build
before its own process touches the GPU.

As tests/multitask_f16_worker.py: the session already runs more than a dozen helper processes beside itself from the moment the
collection ends, and a GPU takes a bounded number of processes at once.  So this one is started with them but opens the GPU only when
its test asks for the result: it reads one line from stdin first -- nothing that touches the GPU is imported before that -- and from
then on runs under a time limit of its own (SIGALRM ends the process)."""
import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
LIMIT_S = 240

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if not sys.stdin.readline():                           # the parent went away without asking
        sys.exit(2)
    signal.alarm(LIMIT_S)

    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))     # runs beside the test session
    from octcubem_amd import _lib, ops
    from tests import test_gpu_retrieval_topk as T

    passed = []
    for case in T.DYADIC_CASES:
        T.check_dyadic(*case)
        passed.append(list(case))
    torch.cuda.synchronize()
    with open(a.out, "w") as f:
        json.dump({"lib": os.path.basename(_lib.LIB_PATH), "lp_is_f16": bool(ops.LP_IS_F16), "passed": passed}, f)
