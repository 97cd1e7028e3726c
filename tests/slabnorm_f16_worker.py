"""Runs the checks of tests/test_gpu_slabnorm_kernels.py against the library OCTMAE_LIB selects (a process binds one library:
octcubem_amd/_lib.py) and writes a one-line summary to --out (json).  tests/test_gpu_slabnorm_kernels.py starts it with the
half-operand build; a failed check ends it with a traceback and a non-zero status."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

torch.set_num_threads(min(8, os.cpu_count() or 1))       # runs beside the test session

from octcubem_amd import _lib, ops  # noqa: E402
from tests import test_gpu_slabnorm_kernels as T  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rep = T.run_all_checks()
    torch.cuda.synchronize()
    with open(a.out, "w") as f:
        json.dump({"lib": os.path.basename(_lib.LIB_PATH), "lp_is_f16": bool(ops.LP_IS_F16), "cases": len(rep)}, f)
