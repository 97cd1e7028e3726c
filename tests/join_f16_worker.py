"""Runs WORKER_CASES of tests/test_gpu_join.py against the library OCTMAE_LIB selects (a process binds one library:
octcubem_amd/_lib.py) and writes the raw results to --out (npz).  tests/test_gpu_join.py starts it with the half-operand build."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(min(8, os.cpu_count() or 1))       # runs beside the test session

from octcubem_amd import _lib, ops  # noqa: E402
from tests import test_gpu_join as T  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    res = T.worker_results()
    torch.cuda.synchronize()
    res["meta"] = np.asarray(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "lp_is_f16": bool(ops.LP_IS_F16)}))
    np.savez(a.out, **res)
