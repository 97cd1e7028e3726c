"""Writes tests/golden/metrics_small.npz by calling the REFERENCE's own metric functions (build container only):

    python tools/gen_golden_metrics.py [--check]

``misc_measures`` and ``misc_measures_multi_label`` of the reference's OCTCube/engine_finetune.py run on three small seeded problems
(tests/test_cpu_metrics.py: golden_problem regenerates the inputs; the file holds their CRC-32 and the expected values only).  The module
is imported under the oracle harness's stubs (oracle/gen_golden.py: install_shims, plus timm.data / timm.utils / pycm as
oracle/gen_golden_finetune.py adds them).  The reference's functions call scikit-learn: where it is installed its values are what the
file records (``sklearn_version``); where it is not, the file holds ``misc_measures`` alone (``sklearn_version`` = "absent") and the
test pins only that.  Data only: no text of the reference is copied.  --check recomputes and compares instead of writing."""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OC = "/root/reference/OCTCube"
PATH = os.path.join(ROOT, "tests", "golden", "metrics_small.npz")
MEASURES = ("acc", "sensitivity", "specificity", "precision", "G", "F1", "mcc", "balanced_acc")


def reference_engine():
    from oracle.gen_golden import install_shims
    install_shims()
    td = types.ModuleType("timm.data"); tu = types.ModuleType("timm.utils"); pycm = types.ModuleType("pycm")
    td.Mixup = type("Mixup", (), {})
    tu.accuracy = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("not used"))
    pycm.__all__ = []
    sys.modules.update({"timm.data": td, "timm.utils": tu, "pycm": pycm})
    sys.modules["timm"].data = td; sys.modules["timm"].utils = tu
    try:
        import sklearn
        version = sklearn.__version__
    except ImportError:
        version = "absent"
        sk = types.ModuleType("sklearn"); skm = types.ModuleType("sklearn.metrics")
        skm.__getattr__ = lambda name: (lambda *a, **k: (_ for _ in ()).throw(RuntimeError("scikit-learn is not installed")))
        sk.metrics = skm
        sys.modules.update({"sklearn": sk, "sklearn.metrics": skm})
    for name in ("matplotlib", "matplotlib.pyplot", "scipy", "scipy.stats"):     # imported by the module, not used by the two functions
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.__getattr__ = lambda attr: None
            sys.modules[name] = m
    sys.path.insert(0, OC)
    cwd = os.getcwd()
    os.chdir(OC)
    try:
        import engine_finetune as ref_engine
    finally:
        os.chdir(cwd)
    return ref_engine, version


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    from tests import test_cpu_metrics as T
    ref, version = reference_engine()
    d = {"sklearn_version": np.array(version)}
    for k in range(T.N_GOLDEN):
        true_idx, pred_idx, num_class, y_true, y_prob = T.golden_problem(k)
        d[f"crc_{k}"] = np.array(T.crc(true_idx, pred_idx, y_true, y_prob), dtype=np.int64)
        ovr = T.one_vs_rest(true_idx, pred_idx, num_class)
        if version != "absent":
            from sklearn.metrics import multilabel_confusion_matrix
            assert np.array_equal(ovr, multilabel_confusion_matrix(true_idx, pred_idx, labels=list(range(num_class))))
        d[f"ovr_{k}"] = ovr
        d[f"measures_{k}"] = np.array([float(v) for v in ref.misc_measures(ovr)], dtype=np.float64)
        if version == "absent":
            continue
        res = ref.misc_measures_multi_label(y_true, y_prob, threshold=0.5)
        for half in ("macro", "classwise"):
            for key, v in res[half].items():
                d[f"{half}_{k}/{key}"] = np.asarray(v, dtype=np.float64)
    if a.check:
        g = np.load(PATH)
        bad = [key for key in d if key != "sklearn_version" and not np.array_equal(g[key], d[key], equal_nan=True)]
        print("differs: " + ", ".join(bad) if bad else f"{PATH}: equal (scikit-learn {version})")
        sys.exit(1 if bad else 0)
    np.savez_compressed(PATH, **d)
    print(f"{PATH}: {T.N_GOLDEN} problems, scikit-learn {version}, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
