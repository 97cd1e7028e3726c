#!/usr/bin/env python3
"""Generate tests/golden/losses_small.npz from the REAL reference (build container only; the reference never travels to a GPU box).

    python tools/gen_golden_losses.py [--reference DIR]

What runs from the reference's own source: ``WeightedLabelSmoothingCrossEntropy`` (OCTCube/util/WeightedLabelSmoothingCrossEntropy.py),
forward and backward on the CPU in float32; it needs only torch.  Cases, each stored as ``<name>/x`` (logits), ``<name>/t`` (one-hot
targets with all-zero rows), ``<name>/loss`` and ``<name>/grad`` (d loss / d logits), with ``<name>/smoothing``:
  c3_one    3 classes, 6 rows, one all-zero row        c10_one    10 classes, 8 rows, one all-zero row
  c3_some   3 classes, 6 rows, three all-zero rows     c10_some   10 classes, 8 rows, five all-zero rows
  c3_all    3 classes, 6 rows, every row zero          c10_all    10 classes, 8 rows, every row zero
  c10_none  10 classes, 8 rows, no zero row, smoothing 0.2
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CASES = [("c3_one", 3, 6, (4,), 0.1), ("c3_some", 3, 6, (0, 2, 5), 0.1), ("c3_all", 3, 6, tuple(range(6)), 0.1),
         ("c10_one", 10, 8, (0,), 0.1), ("c10_some", 10, 8, (1, 2, 4, 6, 7), 0.1), ("c10_all", 10, 8, tuple(range(8)), 0.1),
         ("c10_none", 10, 8, (), 0.2)]


def load_reference(ref_root):
    path = os.path.join(ref_root, "OCTCube", "util", "WeightedLabelSmoothingCrossEntropy.py")
    spec = importlib.util.spec_from_file_location("ref_weighted_ls_ce", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.WeightedLabelSmoothingCrossEntropy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "losses_small.npz"))
    a = ap.parse_args()
    Ref = load_reference(a.reference)
    out = {"cases": np.array([c[0] for c in CASES])}
    for k, (name, C, n, zero_rows, smoothing) in enumerate(CASES):
        g = torch.Generator().manual_seed(100 + k)
        x = (torch.randn(n, C, generator=g) * 2.0).requires_grad_(True)
        t = torch.zeros(n, C)
        t[torch.arange(n), torch.randint(0, C, (n,), generator=g)] = 1.0
        t[list(zero_rows)] = 0.0
        loss = Ref(smoothing)(x, t)
        loss.backward()
        out[name + "/x"] = x.detach().numpy()
        out[name + "/t"] = t.numpy()
        out[name + "/loss"] = loss.detach().numpy()
        out[name + "/grad"] = x.grad.numpy()
        out[name + "/smoothing"] = np.float64(smoothing)
        print(f"{name}: loss {float(loss.detach()):.8f}  |grad| {float(x.grad.norm()):.6f}  valid rows {n - len(zero_rows)}")
    np.savez(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
