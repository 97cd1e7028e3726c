"""python tests/f16_worker.py --call tests.test_gpu_x:function --out PATH

The half-build worker of the GPU tests: calls one function of a test module against the library OCTMAE_LIB selects (a process binds one
library: octcubem_amd/_lib.py) and writes what it returns to --out.  The function returns a JSON-able dict, written as JSON, or a dict
of numpy arrays, written as npz (--out ends in .npz); either carries which library ran ("lib", "lp_is_f16": top-level keys of the JSON,
a JSON string under "meta" in the npz), which the parent checks.  A failed check ends the worker with a traceback and a non-zero
status.  tests/children.py starts it, gated and under a time limit."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--call", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()

    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))       # runs beside the test session
    from octcubem_amd import _lib, ops

    module, function = a.call.split(":")
    res = getattr(importlib.import_module(module), function)()
    torch.cuda.synchronize()
    meta = {"lib": os.path.basename(_lib.LIB_PATH), "lp_is_f16": bool(ops.LP_IS_F16)}
    if a.out.endswith(".npz"):
        import numpy as np
        np.savez(a.out, meta=np.asarray(json.dumps(meta)), **res)
    else:
        with open(a.out, "w") as f:
            json.dump({**meta, **res}, f)
