"""Runs KERNEL_CHECKS of tests/test_gpu_recompute.py against the library OCTMAE_LIB selects (a process binds one library:
octcubem_amd/_lib.py) and writes which ran and which failed to --out (json).  tests/test_gpu_recompute.py starts it with the half-operand
build."""
import argparse
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

torch.set_num_threads(min(8, os.cpu_count() or 1))       # runs beside the test session

from octcubem_amd import _lib, ops  # noqa: E402
from tests import test_gpu_recompute as T  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    ran, failed = [], {}
    for name, fn in T.KERNEL_CHECKS.items():
        ran.append(name)
        try:
            fn()
            torch.cuda.synchronize()
        except AssertionError:
            failed[name] = traceback.format_exc()[-1500:]
    with open(a.out, "w") as f:
        json.dump({"lib": os.path.basename(_lib.LIB_PATH), "lp_is_f16": bool(ops.LP_IS_F16), "ran": ran, "failed": failed}, f)
