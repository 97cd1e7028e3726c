"""Writes tests/golden/retrieval_small.npz by calling the REFERENCE's own retrieval metrics (build container only):

    python tools/gen_golden_retrieval.py [--check]

``get_metrics`` and ``get_corrected_metrics`` of the reference's retinal-COEM/src/training/train_retclip.py and ``get_metrics_3modalities``
of train_retclip_3modalities.py run on three small seeded problems (tests/test_cpu_retrieval.py: golden_problem regenerates the inputs; the
file holds their CRC-32 and the expected values only).  The two modules are imported under stubs for what they import and these functions
do not use (open_clip, the training package's distributed / zero_shot / precision, wandb); scikit-learn's recall_score is the real one.
Before anything is recorded the tool asserts that no two scores of a row, scaled or not, lie within MIN_GAP of each other (and, where the sign is used, of 0): the
reference's argsort leaves the order of ties open and its f32 sigmoid threshold passes a sliver below 0, and the fixture must depend on
neither.  Data only: no text of the reference is copied.  --check recomputes and compares instead of writing."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = "/root/reference/retinal-COEM/src"
PATH = os.path.join(ROOT, "tests", "golden", "retrieval_small.npz")


def reference_modules():
    import sklearn
    oc = types.ModuleType("open_clip")
    oc.__getattr__ = lambda name: type(name, (), {})
    pkg = types.ModuleType("training")
    pkg.__path__ = [os.path.join(SRC, "training")]
    sys.modules.update({"open_clip": oc, "training": pkg})
    for sub, names in (("distributed", ("is_master",)), ("zero_shot", ("zero_shot_eval",)), ("precision", ("get_autocast",))):
        m = types.ModuleType(f"training.{sub}")
        for nm in names:
            setattr(m, nm, lambda *a, **k: (_ for _ in ()).throw(RuntimeError("not used")))
        sys.modules[f"training.{sub}"] = m
    return importlib.import_module("training.train_retclip"), importlib.import_module("training.train_retclip_3modalities"), sklearn.__version__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    from tests import test_cpu_retrieval as T
    two, three, version = reference_modules()
    t = lambda x: torch.from_numpy(np.asarray(x))
    d = {"sklearn_version": np.array(version)}
    for k in range(T.N_GOLDEN):
        p = T.golden_problem(k)
        d[f"crc_{k}"] = np.array(T.crc(p), dtype=np.int64)
        if k == 0:
            pairs = [(p["image"], p["text"], p["logit_scale"])]
            res = two.get_metrics(t(p["image"]), t(p["text"]), t(p["logit_scale"]))
        elif k == 1:
            pairs = [(p["image"], p["text1"], p["logit_scale"]), (p["image"], p["text2"], p["logit_scale1"]),
                     (p["text1"], p["text2"], p["logit_scale2"])]
            res = three.get_metrics_3modalities(t(p["image"]), t(p["text1"]), t(p["text2"]), t(p["logit_scale"]), t(p["logit_scale1"]),
                                                t(p["logit_scale2"]), t(p["w1"]), t(p["w2"]))
        else:
            last = sorted({l: i for i, l in enumerate(p["labels"])}.values())
            pairs = [(p["image"], p["text"][last], p["logit_scale"])]
            full = p["image"].astype(np.float64) @ p["text"].astype(np.float64).T        # the recall threshold sees every pair
            assert np.abs(full).min() > T.MIN_GAP, (k, np.abs(full).min())
            res = two.get_corrected_metrics(t(p["image"]), t(p["text"]), t(p["logit_scale"]), list(p["labels"]))
        for x, y, scale in pairs:
            s = x.astype(np.float64) @ y.astype(np.float64).T
            for m in (s, s.T) if k < 2 else (s,):
                assert T.row_gap(m) > T.MIN_GAP and T.row_gap(m * float(scale)) > T.MIN_GAP, (k, T.row_gap(m))
        for key, v in res.items():
            d[f"p{k}/{key}"] = np.asarray(float(v), dtype=np.float64)
    if a.check:
        g = np.load(PATH)
        bad = [key for key in d if key != "sklearn_version" and not np.array_equal(g[key], d[key])]
        bad += [key for key in g.files if key not in d]
        print("differs: " + ", ".join(bad) if bad else f"{PATH}: equal (scikit-learn {version})")
        sys.exit(1 if bad else 0)
    np.savez_compressed(PATH, **d)
    print(f"{PATH}: {T.N_GOLDEN} problems, scikit-learn {version}, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
