"""Writes tests/golden/eval3mod_small.npz by calling the REFERENCE's own validation loops (build container only):

    python tools/gen_golden_eval3mod.py [--check]

``evaluate`` of the reference's retinal-COEM/src/training/train_retclip_3modalities.py (multimodal_type 'oct_faf_ir') and ``evaluate`` of
train_retclip.py ('oct_ir') run on the CPU on the seeded problem of tests/test_cpu_eval3mod.py (``problem`` regenerates the inputs; the file
holds their CRC-32 and the returned values only), once with ``correct_label`` 0 and once with 1.  The two modules are imported under stubs
for what they import, as tools/gen_golden_retrieval.py does, except that here the loops do call some of it: ``is_master`` is true,
``zero_shot_eval`` returns {}, ``get_autocast`` gives a null context, ``get_cast_dtype`` gives None (no input cast) and
``convert_modalities_idx_to_flag`` -- which the reference imports from a module it does not ship -- turns the loader's flags into a
float32 tensor.  The model is the test's ``Echo``: the batches hold the seeded, normalised features themselves.  ``save_logs`` is off:
the reference's saving block names variables it never defines.

Before anything is recorded the tool asserts, as tools/gen_golden_retrieval.py does, that no two scores of a row, scaled or not, lie
within MIN_GAP of each other on all three products and their transposes -- for ``correct_label`` 1 with the second of the two bit-copied
IR rows left out of the IR products, and with both copies absent (w1 = 0), so that no REPORTED rank touches the tie the copies make: the
reference's argsort leaves the order of ties open and the fixture must not depend on it.  It also asserts that every one of the six
directions keeps at least one present sample.  The 'oct_ir' loop ranks without a filter and is recorded on the copy-free features, with
both values of ``correct_label``.  Data only: no text of the reference is copied.  --check recomputes and compares instead of writing."""
import argparse
import contextlib
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = "/root/reference/retinal-COEM/src"
PATH = os.path.join(ROOT, "tests", "golden", "eval3mod_small.npz")


def reference_modules():
    import sklearn  # noqa: F401  (the modules import recall_score)
    oc = types.ModuleType("open_clip")
    oc.get_cast_dtype = lambda precision: None
    oc.convert_modalities_idx_to_flag = lambda m: torch.as_tensor(m).to(torch.float32)
    oc.__getattr__ = lambda name: type(name, (), {})
    pkg = types.ModuleType("training")
    pkg.__path__ = [os.path.join(SRC, "training")]
    sys.modules.update({"open_clip": oc, "training": pkg})
    for sub, name, fn in (("distributed", "is_master", lambda args, local=False: True), ("zero_shot", "zero_shot_eval", lambda *a, **k: {}),
                          ("precision", "get_autocast", lambda precision: contextlib.nullcontext)):
        m = types.ModuleType(f"training.{sub}")
        setattr(m, name, fn)
        sys.modules[f"training.{sub}"] = m
    return importlib.import_module("training.train_retclip"), importlib.import_module("training.train_retclip_3modalities")


def assert_gaps(T, G, p, cl):
    keep_ir = np.ones(T.N, dtype=bool)
    if cl:
        assert p["w1"][list(T.COPY)].max() == 0 and T.COPY[0] < T.BATCHES[0] > T.COPY[1]
        keep_ir[T.COPY[1]] = False
    everything = np.ones(T.N, dtype=bool)
    for x, kx, y, ky, scale in ((p["image"], everything, p["ir"], keep_ir, T.SCALES[0]), (p["image"], everything, p["faf"], everything, T.SCALES[1]),
                                (p["ir"], keep_ir, p["faf"], everything, T.SCALES[2])):
        if cl and (kx is keep_ir or ky is keep_ir):
            kx = ky = keep_ir                      # the copy leaves rows and columns alike: a square problem without it
        s = x[kx].astype(np.float64) @ y[ky].astype(np.float64).T
        for m in (s, s.T):
            assert G.row_gap(m) > G.MIN_GAP and G.row_gap(m * float(scale)) > G.MIN_GAP, (cl, G.row_gap(m))
    for w in (p["w1"], p["w2"], p["w1"] * p["w2"]):
        assert (w > 0).any()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    from tests import test_cpu_eval3mod as T
    from tests import test_cpu_retrieval as G
    two, three = reference_modules()
    d = {}
    for cl in (0, 1):
        p = T.problem(cl)
        assert_gaps(T, G, p, cl)
        d[f"crc_{cl}"] = np.array(T.crc(p), dtype=np.int64)
        runs = (("three", three, "oct_faf_ir", p), ("oct_ir", two, "oct_ir", T.problem(0)))
        for prefix, module, mm, q in runs:
            data = {"val": types.SimpleNamespace(dataloader=T.loader(q))}
            with contextlib.redirect_stdout(open(os.devnull, "w")):
                res = module.evaluate(T.Echo(), data, 2, T.eval_args(mm, cl))
            assert len(res) == (33 if prefix == "three" else 13), sorted(res)
            for key, v in res.items():
                d[f"{prefix}{cl}/{key}"] = np.asarray(float(v), dtype=np.float64)
    if a.check:
        g = np.load(PATH)
        bad = [key for key in d if not np.array_equal(g[key], d[key])]
        bad += [key for key in g.files if key not in d]
        print("differs: " + ", ".join(bad) if bad else f"{PATH}: equal")
        sys.exit(1 if bad else 0)
    np.savez_compressed(PATH, **d)
    print(f"{PATH}: {len(d)} entries, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
