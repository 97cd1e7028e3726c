"""GPU: the validation loops of the dict-batch recipes end to end (coem.evaluate_3modalities, coem.evaluate_multimodal) on a tiny
three-tower model -- 13 samples in dict batches of 5, 5 and 3 with presence flags that include zeros.

``val_loss`` is held against tests/eval3mod_ref.py (float64) on the model's own features within 1e-6 * max(1, |want|), the limit of
tests/test_gpu_retrieval.py::test_evaluate_end_to_end: float32 log-sum-exps of 3 or 5 logits on features that are given.  The ranks
are held with that test's ``bounds`` / ``stable_preds`` check: the inputs must leave no rank open within the f32 bound (asserted), so the
positions are known exactly and the filtered summaries must EQUAL ``retrieval_ref.rank_metrics``."""
import json
import math
import os
import types
from functools import partial

import numpy as np
import pytest
import torch

from tests import eval3mod_ref as E
from tests import retrieval_ref as R
from tests import test_gpu_retrieval as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
BATCHES = (5, 5, 3)
N = sum(BATCHES)
# [modality][sample]: every sample has its OCT volume; IR and FAF are absent here and there, sample 6 lacks both
FLAGS = ([1] * N, [1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1], [1, 0, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1, 0])
DIRECTIONS = (("image_to_text1", 0, 1, "w1"), ("text1_to_image", 1, 0, "w1"), ("image_to_text2", 0, 2, "w2"), ("text2_to_image", 2, 0, "w2"),
              ("text1_to_text2", 1, 2, "w12"), ("text2_to_text1", 2, 1, "w12"))


class ThreeTowerCLIP(torch.nn.Module):
    """ThreeTowerCLIP of tests/test_gpu_coem_loop.py, restated"""

    def __init__(self, visual, ir, faf):
        super().__init__()
        self.visual, self.text, self.text2 = visual, ir, faf
        self.logit_scale = torch.nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self.logit_scale1 = torch.nn.Parameter(torch.ones([]) * math.log(20.0))
        self.logit_scale2 = torch.nn.Parameter(torch.ones([]) * math.log(5.5))

    def forward(self, image, ir, faf):
        f = lambda t, x: torch.nn.functional.normalize(t(x).float(), dim=-1)
        return (f(self.visual, image), f(self.text, ir), f(self.text2, faf), self.logit_scale.exp(), self.logit_scale1.exp(),
                self.logit_scale2.exp())


def tiny_three(seed):
    from octcubem_amd import models_vit, models_vit_st
    torch.manual_seed(seed)
    kw = dict(mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    m3 = models_vit_st.VisionTransformer(num_frames=6, t_patch_size=3, img_size=64, patch_size=16, in_chans=1, num_classes=64, embed_dim=128,
                                         depth=2, num_heads=2, sep_pos_embed=True, cls_embed=True, global_pool=True, dropout=0.0, **kw)
    m2 = [models_vit.VisionTransformer(img_size=64, patch_size=16, in_chans=3, num_classes=64, embed_dim=128, depth=2, num_heads=2,
                                       qkv_bias=True, global_pool=True, **kw) for _ in range(2)]
    for m in [m3] + m2:
        torch.nn.init.normal_(m.head.weight, std=0.2)                         # a projection that spreads the samples
    return ThreeTowerCLIP(m3, *m2).to(DEV)


def dict_loader():
    g = torch.Generator().manual_seed(8)
    vol = torch.rand(N, 1, 6, 64, 64, generator=g) * torch.linspace(0.2, 3.0, N).view(N, 1, 1, 1, 1)
    ir = torch.randn(N, 3, 64, 64, generator=g) + torch.linspace(-1.5, 1.5, N).view(N, 1, 1, 1)
    faf = torch.randn(N, 3, 64, 64, generator=g) * torch.linspace(0.5, 2.0, N).view(N, 1, 1, 1) + torch.linspace(1.0, -1.0, N).view(N, 1, 1, 1)
    out, i = [], 0
    for bsz in BATCHES:
        sl = slice(i, i + bsz)
        flags = [torch.tensor(f[sl]) for f in FLAGS]
        out.append(({"oct": vol[sl], "ir": ir[sl], "f2_faf": faf[sl]}, ([f"s{k}" for k in range(i, i + bsz)], [0] * bsz, flags, None)))
        i += bsz
    return out


def eval_args(tmp, mm="oct_faf_ir", **kw):
    base = dict(device=DEV, val_frequency=1, epochs=4, save_logs=True, checkpoint_path=str(tmp), save_retrieval_results=True,
                multimodal_type=mm, return_metainfo=False, correct_label=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


def test_three_modality_loop_end_to_end(tmp_path):
    from octcubem_amd import coem
    model = tiny_three(23)
    loader = dict_loader()
    data = {"val": types.SimpleNamespace(dataloader=loader)}
    scalars = []
    tb = types.SimpleNamespace(add_scalar=lambda name, val, step: scalars.append((name, val, step)))
    args = eval_args(tmp_path)
    got = coem.evaluate_3modalities(model, data, 2, args, tb_writer=tb)
    assert not model.training and got["epoch"] == 2 and got["num_samples"] == N and len(got) == 33
    # the same features, batch by batch
    outs = []
    with torch.no_grad():
        for x, _ in loader:
            outs.append([o.cpu().numpy() for o in model(x["oct"].to(DEV), x["ir"].to(DEV), x["f2_faf"].to(DEV))])
    w = {"w1": np.asarray(FLAGS[1], dtype=np.float32), "w2": np.asarray(FLAGS[2], dtype=np.float32)}
    w["w12"] = w["w1"] * w["w2"]
    assert all((v > 0).any() and (v == 0).any() for v in w.values())
    ref_batches, i = [], 0
    for o, bsz in zip(outs, BATCHES):
        ref_batches.append(tuple(o[:3]) + tuple(float(s) for s in o[3:]) + (w["w1"][i:i + bsz], w["w2"][i:i + bsz]))
        i += bsz
    want = E.val_loss(ref_batches)
    print(f"val_loss {got['val_loss']!r} / {want!r}")
    assert abs(got["val_loss"] - want) <= 1e-6 * max(1.0, abs(want))
    assert abs(E.val_loss(ref_batches, text_pair_weight="w1w2") - want) > 1e-4            # the w1-only text pair shows on this data too
    feats = [np.concatenate([o[k] for o in outs]) for k in range(3)]
    diag = np.arange(N)
    for name, a, b, wk in DIRECTIONS:
        lo, hi, s, _ = T.bounds(feats[a], feats[b], diag)
        assert np.array_equal(lo, hi), f"{name}: the inputs leave a rank open within the f32 bound"
        assert np.array_equal(lo, R.stable_preds(s))
        for key, v in R.rank_metrics(name, lo[w[wk] > 0]).items():
            assert got[key] == v, (key, got[key], v)
    # the files
    lines = open(os.path.join(str(tmp_path), "results.jsonl")).read().splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == got
    assert sorted(scalars) == sorted((f"val/{k}", v, 2) for k, v in got.items())
    z = np.load(os.path.join(str(tmp_path), "retrieval_results_2.npz"))
    assert set(z.files) == {"image_features", "text1_features", "text2_features", "t_weight1", "t_weight2", "logit_scale"}
    for key, f in zip(("image_features", "text1_features", "text2_features"), feats):
        assert z[key].shape == (N, 64) and np.array_equal(z[key], f)
    assert np.array_equal(z["t_weight1"], w["w1"]) and np.array_equal(z["t_weight2"], w["w2"])
    assert z["logit_scale"].shape == (3, 3) and np.array_equal(z["logit_scale"][0], np.asarray(outs[0][3:], dtype=np.float32))
    # the same inside autocast, and from the per-direction kernel; not due -> {}
    args.save_logs = False
    with torch.autocast("cuda", dtype=torch.float16):
        again = coem.evaluate_3modalities(model, data, 4, args)
    assert again["epoch"] == 4 and abs(again["val_loss"] - got["val_loss"]) <= 1e-6
    assert without(again, "epoch", "val_loss") == without(got, "epoch", "val_loss")
    calls = []
    from octcubem_amd import ops
    prev = ops.KTIMER
    ops.KTIMER = types.SimpleNamespace(launch=lambda kind, flops, nbytes, fn, exec_flops=None: (calls.append(kind), fn()))
    try:
        on = coem.evaluate_3modalities(model, data, 2, args, pair_ranks=True)
        n_on = (calls.count("retrieval_pair_ranks"), calls.count("retrieval_ranks"))
        del calls[:]
        off = coem.evaluate_3modalities(model, data, 2, args, pair_ranks=False)
        n_off = (calls.count("retrieval_pair_ranks"), calls.count("retrieval_ranks"))
    finally:
        ops.KTIMER = prev
    assert n_on == (1, 0) and n_off == (0, 6)
    assert without(on, "val_loss") == without(off, "val_loss") == without(got, "val_loss") and abs(on["val_loss"] - off["val_loss"]) <= 1e-6
    args.val_frequency = 3
    assert coem.evaluate_3modalities(model, data, 2, args) == {}
    # duplicate-IR targets: the same-feature matrix as class probabilities (the identity on these features)
    args.val_frequency, args.correct_label = 1, 1
    soft = coem.evaluate_3modalities(model, data, 1, args)
    want = E.val_loss(ref_batches, correct_label=True)
    print(f"val_loss with correct_label {soft['val_loss']!r} / {want!r}")
    assert abs(soft["val_loss"] - want) <= 1e-6 * max(1.0, abs(want))


def test_oct_ir_equals_evaluate_on_the_same_data_as_tuples(tmp_path):
    from octcubem_amd import coem
    model = T.tiny_clip(21)
    loader = dict_loader()
    tuples = [(x["oct"], x["ir"]) for x, _ in loader]
    base = coem.evaluate(model, {"val": types.SimpleNamespace(dataloader=tuples)}, 2, eval_args(tmp_path / "a", "default", save_logs=False))
    os.makedirs(str(tmp_path / "b"))
    args = eval_args(tmp_path / "b", "oct_ir")
    for pair_ranks in (None, True, False):
        got = coem.evaluate_multimodal(model, {"val": types.SimpleNamespace(dataloader=loader)}, 2, args, pair_ranks=pair_ranks)
        assert len(got) == 13 and without(got, "val_loss") == without(base, "val_loss") and abs(got["val_loss"] - base["val_loss"]) <= 1e-6
    z = np.load(os.path.join(str(tmp_path / "b"), "retrieval_results_2.npz"))
    assert set(z.files) == {"image_features", "text_features", "logit_scale"} and z["logit_scale"].shape == (3,)
    assert z["image_features"].shape == (N, 64)
    # through the dispatcher, 'default' IS evaluate
    same = coem.evaluate_multimodal(model, {"val": types.SimpleNamespace(dataloader=tuples)}, 2, eval_args(tmp_path / "a", "default", save_logs=False))
    assert without(same, "val_loss") == without(base, "val_loss") and abs(same["val_loss"] - base["val_loss"]) <= 1e-6
    with pytest.raises(NotImplementedError, match="oct_faf_ir"):
        coem.evaluate(model, {"val": types.SimpleNamespace(dataloader=tuples)}, 2, eval_args(tmp_path / "a", "oct_faf_ir", save_logs=False))
