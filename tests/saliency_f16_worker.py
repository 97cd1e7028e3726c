"""Runs the scatter, patch-embed and model-parity checks of tests/test_gpu_saliency.py against the library OCTMAE_LIB selects (a process
binds one library: octcubem_amd/_lib.py) and writes what it measured to --out as JSON.  tests/test_gpu_saliency.py starts it with the
half-operand build before its own process touches the GPU.

The session already runs a dozen helper processes beside itself from the moment the collection ends (tests/test_gpu_comm.py, the other
half-build workers), and a GPU takes a bounded number of processes at once.  So this one is started with them but opens the GPU only
when tests/test_gpu_saliency.py releases it, after those have ended: it reads one line from stdin first -- nothing that touches the GPU
is imported before that -- and from then on runs under a time limit of its own (SIGALRM ends the process)."""
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
    if not sys.stdin.readline():                         # the parent went away without asking
        sys.exit(2)
    signal.alarm(LIMIT_S)

    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))   # runs beside the test session
    from octcubem_amd import _lib, ops
    from tests import test_gpu_saliency as T

    ops.ATTN_BWD_FUSED_MIN_FILL = 0.0                    # as tests/conftest.py sets it for every GPU test
    res = {"lib": os.path.basename(_lib.LIB_PATH), "lp_is_f16": bool(ops.LP_IS_F16)}
    res["scatter_cases"] = sum(T.check_scatter(*geom) for geom in T.SCATTER_GEOM) + T.check_scatter_past_the_grid_cap()
    res["patch_embed"] = {f"{kind} {ids}": T.check_patch_embed(kind, ids) for kind in ("3d", "2d") for ids in (False, True)}
    res["parity"] = {v: T.measure_model_parity(v)[0] for v in ("native", "flash_compat", "flash_blocks", "vit2d")}
    torch.cuda.synchronize()
    with open(a.out, "w") as f:
        json.dump(res, f)
