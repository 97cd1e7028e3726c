"""Writes tests/golden/metrics_multitask_small.npz by calling the REFERENCE's own functions (build container only):

    python tools/gen_golden_multitask.py [--check]

``misc_measures_multi_task``, ``multi_label_target_to_multi_task_target`` and ``multi_task_loss`` (with the reference's
``WeightedLabelSmoothingCrossEntropy``, smoothing 0.1) of OCTCube/engine_finetune.py run on three small seeded multi-task problems
(tests/test_cpu_multitask.py: golden_problem regenerates the inputs and checks that no population is degenerate), and the five
scipy / scikit-learn calls of the regression block of its ``evaluate`` (:648-653) on two seeded regression problems
(tests/test_cpu_regression_report.py: regression_problem) -- once on the float32 vectors the reference gathers, and once on the same
values as float64 (``*_f64``: the libraries keep the input's precision, so only these show what a float64 restatement must reach).
The file holds the inputs' CRC-32 and the expected values only.  The module is imported under the shims of
tools/gen_golden_metrics.py; scikit-learn and scipy must be installed (their versions are recorded).  Data only: no text of the
reference is copied.  --check recomputes and compares instead of writing."""
import argparse
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PATH = os.path.join(ROOT, "tests", "golden", "metrics_multitask_small.npz")
REGRESSION = ("pearsonr", "r2", "explained_variance", "mse", "mae")


def regression_values(pred, target):
    """The reference's five calls, in its argument order."""
    from scipy.stats import pearsonr
    from sklearn.metrics import explained_variance_score, mean_absolute_error, mean_squared_error, r2_score
    return np.array([pearsonr(pred, target)[0], r2_score(target, pred), explained_variance_score(target, pred),
                     mean_squared_error(target, pred), mean_absolute_error(target, pred)], dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    import torch
    from gen_golden_metrics import reference_engine
    from tests import test_cpu_multitask as T
    from tests import test_cpu_regression_report as G
    ref, version = reference_engine()
    assert version != "absent", "scikit-learn is needed: every value here comes from it"
    import scipy
    from util.WeightedLabelSmoothingCrossEntropy import WeightedLabelSmoothingCrossEntropy
    d = {"sklearn_version": np.array(version), "scipy_version": np.array(scipy.__version__)}
    for k in range(T.N_GOLDEN):
        y, logits, kind = T.golden_problem(k)
        d[f"crc_{k}"] = np.array(T.crc(y, logits), dtype=np.int64)
        with contextlib.redirect_stdout(io.StringIO()):           # the function prints its result
            res = ref.misc_measures_multi_task(y, logits.copy(), threshold=0.5, multi_task_type=kind)
        for half in ("macro", "classwise"):
            for key, v in res[half].items():
                d[f"{half}_{k}/{key}"] = np.asarray(v, dtype=np.float64)
        tm, w = ref.multi_label_target_to_multi_task_target(torch.from_numpy(y))
        d[f"target_mt_{k}"], d[f"weight_{k}"] = tm.numpy(), w.numpy()
        loss = ref.multi_task_loss(torch.from_numpy(logits.copy()), torch.from_numpy(y), WeightedLabelSmoothingCrossEntropy(0.1), kind)
        d[f"loss_{k}"] = np.array(float(loss), dtype=np.float64)
    for k in range(G.N_REGRESSION):
        pred, target = G.regression_problem(k)
        assert pred.dtype == target.dtype == np.float32
        d[f"reg_crc_{k}"] = np.array(T.crc(pred, target), dtype=np.int64)
        d[f"reg_{k}"] = regression_values(pred, target)
        d[f"reg_f64_{k}"] = regression_values(pred.astype(np.float64), target.astype(np.float64))
    if a.check:
        g = np.load(PATH)
        bad = [key for key in d if not key.endswith("_version") and not np.array_equal(g[key], d[key], equal_nan=True)]
        print("differs: " + ", ".join(bad) if bad else f"{PATH}: equal (scikit-learn {version}, scipy {scipy.__version__})")
        sys.exit(1 if bad else 0)
    np.savez_compressed(PATH, **d)
    print(f"{PATH}: {T.N_GOLDEN} + {G.N_REGRESSION} problems, scikit-learn {version}, scipy {scipy.__version__}, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
