"""CPU: the SLIViT baseline's reference (tests/slivit_ref.py) against HF's ConvNextModel and against the committed golden
(tests/golden/slivit_small.npz, tools/gen_golden_slivit.py); the package's key layout, ``pretrained_weights`` mapping, positional table
and reshapes; and what the per-element bound of the depthwise convolution passes and catches."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import slivit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "slivit_small.npz")
TINY = dict(depths=(1, 1, 2, 1), hidden_sizes=(32, 64, 96, 128))


def _subsample(t, n=256):
    f = t.reshape(-1)
    return f[::max(1, f.numel() // n)][:n]


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def ref_run():
    torch.manual_seed(0)
    P = R.init_params(R.SMALL, seed=0)
    img, target = R.make_inputs(R.SMALL, seed=1)
    return P, img, R.forward_backward(P, img, target, R.SMALL, None)


def test_reference_extractor_equals_the_hf_model():
    tf = pytest.importorskip("transformers")
    cfg = R.SMALL
    P = R.init_params(cfg, seed=0)
    img, _ = R.make_inputs(cfg, seed=1)
    hf = tf.ConvNextModel(tf.ConvNextConfig(depths=list(cfg["depths"]), hidden_sizes=list(cfg["hidden_sizes"]))).eval()
    sd = {("embeddings." if k[len(R.FE)] == "0" else "encoder.") + k[len(R.FE) + 2:]: v for k, v in P.items() if k.startswith(R.FE)}
    res = hf.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and sorted(res.missing_keys) == ["layernorm.bias", "layernorm.weight"]
    with torch.no_grad():
        want = hf.encoder(hf.embeddings(img)).last_hidden_state
        got = R.extractor_forward(P, img, cfg, None, prefix=R.FE)
    assert got.shape == want.shape == (2, 128, 2, 6)
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    hf_keys = [("0." if k.startswith("embeddings.") else "1.") + k.split(".", 1)[1] for k in hf.state_dict() if not k.startswith("layernorm.")]
    assert hf_keys == list(R.extractor_shapes(cfg).keys())
    from octcubem_amd import model_slivit_baseline as M
    assert list(M.ConvNextFeatureExtractor(**TINY).state_dict().keys()) == hf_keys
    # the default configuration is ConvNextConfig()'s
    c = tf.ConvNextConfig()
    fe = M.ConvNextFeatureExtractor()
    assert (list(fe.depths), list(fe.hidden_sizes), c.patch_size, c.layer_scale_init_value) == (list(c.depths), list(c.hidden_sizes), 4, 1e-6)


def test_reference_reproduces_the_golden(ref_run):
    P, img, (feat, logits, loss, G) = ref_run
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert list(g["keys"]) == list(P.keys()) == list(R.model_shapes(R.SMALL).keys())
    assert [R.FE + k for k in g["extractor_keys"]] == [k for k in P if k.startswith(R.FE)]
    # the golden's ConvNeXt half is HF's model, this run is the restatement: fp32 both, another order of additions
    assert _rel(feat, g["feat"]) <= 1e-5 and _rel(logits, g["logits"]) <= 1e-5
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    norms = np.array([float(G[k].double().norm()) for k in P])
    assert np.all(np.abs(norms - g["grad_norm"]) <= 1e-4 * g["grad_norm"]), np.max(np.abs(norms - g["grad_norm"]) / g["grad_norm"])
    for k in g["sample_keys"]:
        assert _rel(_subsample(G[str(k)]), g["grad_sample/" + str(k)]) <= 1e-4, k
    for dt in ("bfloat16", "float16"):
        assert g[f"rounding_err/{dt}/grad"].shape == (len(P),)
        assert 0 < float(g[f"rounding_err/{dt}/logits"]) < 0.05 and 0 < float(g[f"rounding_err/{dt}/feat"]) < 0.05
    assert float(g["rounding_err/float16/logits"]) < float(g["rounding_err/bfloat16/logits"])
    # every ConvNeXt branch is visible: no gradient of the extractor vanishes beside its parameter
    assert float(g["grad_norm"].min()) > 1e-4


def test_rounding_model_rounds_where_it_says(ref_run):
    """the switch changes the result by about one 16-bit rounding per operand, and not at all when off"""
    P, img, (feat, logits, _, _) = ref_run
    with torch.no_grad():
        f16, l16 = R.forward(P, img, R.SMALL, torch.float16)
        fbf, lbf = R.forward(P, img, R.SMALL, torch.bfloat16)
        f32, l32 = R.forward(P, img, R.SMALL, None)
    assert torch.equal(f32, feat) and torch.equal(l32, logits)
    assert 1e-5 < _rel(f16, feat) < _rel(fbf, feat) < 3e-2


def test_state_dict_layout_of_the_shipped_model_and_its_positional_table():
    from octcubem_amd import model_slivit_baseline as M
    args = types.SimpleNamespace(slivit_fe_path="", nb_classes=1, slivit_num_of_patches=20)
    m = M.get_slivit_model(args)
    full = dict(depths=(3, 3, 9, 3), hidden_sizes=(96, 192, 384, 768), num_patches=20, vit_dim=256, heads=20, dim_head=64, vit_depth=5,
                mlp_dim=512, patch_height=768, patch_width=64, num_classes=1)
    want = R.model_shapes(full)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got.keys()) == list(want.keys()) and got == dict(want)
    pe = m.pos_embedding.detach()
    assert pe.shape == (1, 21, 256) and m.pos_embedding.requires_grad
    assert torch.equal(pe, torch.arange(21).repeat(256, 1).t().unsqueeze(0).float())
    assert torch.equal(pe[0, :, 0], torch.arange(21).float()) and bool((pe[0] == pe[0, :, :1]).all())
    # HF's initialisation: layer scale 1e-6, LayerNorm ones / zeros, zero biases, N(0, 0.02^2) weights
    sd = m.feature_extractor.state_dict()
    assert bool((sd["1.stages.2.layers.4.layer_scale_parameter"] == 1e-6).all())
    assert bool((sd["0.layernorm.weight"] == 1).all()) and bool((sd["1.stages.1.downsampling_layer.1.bias"] == 0).all())
    assert abs(float(sd["1.stages.3.layers.0.pwconv1.weight"].std()) - 0.02) < 1e-3
    with pytest.raises(AssertionError):
        M.ConvNextFeatureExtractor(drop_path_rate=0.1, **TINY)
    with pytest.raises(AssertionError):
        M.SLIViT(feature_extractor=M.ConvNextFeatureExtractor(**TINY), vit_dim=64, vit_depth=1, heads=2, mlp_dim=128, num_of_patches=3, dropout=0.1)
    # a checkpoint in the reference's layout loads strictly
    P = R.init_params(R.SMALL, seed=3)
    small = M.SLIViT(feature_extractor=M.ConvNextFeatureExtractor(**TINY), vit_dim=64, vit_depth=2, heads=2, mlp_dim=128, num_of_patches=3,
                     patch_height=128, patch_width=4, num_classes=3)
    res = small.load_state_dict(P, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(small.feature_extractor[1].stages[2].layers[1].dwconv.weight.detach(), P[R.FE + "1.stages.2.layers.1.dwconv.weight"])


def test_pretrained_weights_mapping(tmp_path):
    from octcubem_amd import model_slivit_baseline as M
    P = R.init_params(R.SMALL, seed=5)
    ck = {}
    for k, v in P.items():
        if k.startswith(R.FE + "0."):
            ck["model.convnext.embeddings." + k[len(R.FE) + 2:]] = v
        elif k.startswith(R.FE + "1."):
            ck["model.convnext.encoder." + k[len(R.FE) + 2:]] = v
    ck["model.convnext.layernorm.weight"] = torch.ones(128)
    ck["model.convnext.layernorm.bias"] = torch.zeros(128)
    ck["model.classifier.weight"] = torch.zeros(4, 128)
    ck["model.classifier.bias"] = torch.zeros(4)
    path = str(tmp_path / "convnext_chf.pth")
    torch.save(ck, path)
    fe = M.get_feature_extractor(4, path, **TINY)
    sd = fe.state_dict()
    assert list(sd.keys()) == list(R.extractor_shapes(R.SMALL).keys())
    for k, v in sd.items():
        assert torch.equal(v, P[R.FE + k]), k
    mapped = M.map_pretrained_keys(ck)
    assert "0.patch_embeddings.weight" in mapped and not any("classifier" in k or k.startswith("layernorm") for k in mapped)
    with pytest.raises(KeyError):
        M.map_pretrained_keys({"model.vit.something": torch.zeros(1)})
    assert float(M.get_feature_extractor(4, "", **TINY).state_dict()["1.stages.0.layers.0.layer_scale_parameter"][0]) == pytest.approx(1e-6)


def test_flat_reshape_and_the_loop_reshape():
    """the head reads the NCHW feature map's memory flat, as the reference's ``x.reshape((B, P, 768, 64))`` and its Rearrange with
    h = w = 1 do; the loop lays the slices side by side as engine_finetune.py:417-419 writes it"""
    cfg = R.SMALL
    B, P, ph, pw = 2, cfg["num_patches"], cfg["patch_height"], cfg["patch_width"]
    feat = torch.arange(B * 128 * 2 * 6, dtype=torch.float32).view(B, 128, 2, 6)
    ref = feat.reshape((B, P, ph, pw)).reshape(B, P, 1, ph, 1, pw).permute(0, 1, 2, 4, 3, 5).reshape(B, P, ph * pw)   # 'b c (h p1) (w p2) -> b (c h w) (p1 p2)'
    assert torch.equal(feat.reshape(B, P, ph * pw), ref)
    assert torch.equal(ref[1, 2], torch.arange(ph * pw, dtype=torch.float32) + (1 * P + 2) * ph * pw)
    from octcubem_amd import engine_finetune as E
    x = torch.randn(2, 3, 5, 8, 4)
    on = types.SimpleNamespace(patient_dataset_type="convnext_slivit")
    y = x.permute(0, 2, 3, 4, 1)
    want = y.reshape(-1, y.shape[1], y.shape[2], y.shape[3] * y.shape[4])
    got = E._slivit_reshape(x, on)
    assert got.shape == (2, 5, 8, 12) and torch.equal(got, want)
    for other in (types.SimpleNamespace(patient_dataset_type="3D"), types.SimpleNamespace(), None):
        assert E._slivit_reshape(x, other) is x


# ---- what the per-element bound of the depthwise convolution passes and catches (the style of tests/test_cpu_gemm_elem.py)
def _dwconv_f32(x, wt, bias, order, drop=None, flip=False):
    """fp32 evaluation, one tap at a time in ``order``; drop = (channel, tap) left out; flip = the filter applied back to front"""
    B, H, W, C = x.shape
    xp = F.pad(x.permute(0, 3, 1, 2), (3, 3, 3, 3))
    acc = torch.zeros((B, C, H, W), dtype=torch.float32)
    for t in order:
        i, j = divmod(t, 7)
        w = (wt[:, 6 - i, 6 - j] if flip else wt[:, i, j]).clone()
        if drop is not None and drop[1] == t:
            w[drop[0]] = 0.0
        acc = acc + w.view(1, C, 1, 1) * xp[:, :, i:i + H, j:j + W]
    return (acc + bias.view(1, C, 1, 1)).permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 3, 7, 32), (1, 17, 5, 96), (3, 9, 20, 136)])
def test_dwconv_bound_passes_another_order_and_catches_a_lost_tap(shape):
    g = torch.Generator().manual_seed(sum(shape))
    B, H, W, C = shape
    x, wt, bias = torch.randn(shape, generator=g), torch.randn((C, 7, 7), generator=g) / 7.0, torch.randn((C,), generator=g)
    z64, mag = R.dwconv_ref64(x, wt, bias)
    bound = R.dwconv_bound(mag)
    assert R.gamma_n(50) == pytest.approx(50 * 2.0 ** -24, rel=1e-5)
    for order in (range(49), reversed(range(49)), [(t * 20) % 49 for t in range(49)]):
        err = (_dwconv_f32(x, wt, bias, list(order)).double() - z64).abs()
        assert bool((err <= bound).all()), float((err / bound).max())
    centre = 24                                               # the tap that meets every pixel, also in a 1 x 1 map
    err = (_dwconv_f32(x, wt, bias, range(49), drop=(C - 1, centre)).double() - z64).abs()
    assert bool((err[..., C - 1] > bound[..., C - 1]).any()) and bool((err[..., :C - 1] <= bound[..., :C - 1]).all())
    if H * W > 1:                                             # a 1 x 1 map meets the centre tap only: flipping changes nothing there
        err = (_dwconv_f32(x, wt, bias, range(49), flip=True).double() - z64).abs()
        assert float((err > bound).double().mean()) > 0.5


def test_restated_launch_plans_follow_the_kernel_constants_and_the_trip_shapes_lie_past_the_caps():
    """Whoever changes a constant of csrc/convnext.hip is told here to move the shapes at which tests/test_gpu_slivit_kernels.py makes
    a workgroup walk a second tile or a second round of rows."""
    import re
    src = open(os.path.join(ROOT, "octcubem_amd", "csrc", "convnext.hip")).read()
    m = re.search(r"constexpr int DW_TH = (\d+), DW_TW = (\d+);", src)
    assert (int(m.group(1)), int(m.group(2))) == (R.DW_TH, R.DW_TW)
    assert int(re.search(r"constexpr int DW_CB = (\d+),", src).group(1)) == R.DW_CB
    assert int(re.search(r"constexpr int DWW_ROWS = (\d+);", src).group(1)) == 50
    assert int(re.search(r"int cap = (\d+) / s\.cblocks;", src).group(1)) == R.WGRAD_CAP
    assert int(re.search(r"int cap = (\d+) / s->ncb;", src).group(1)) == R.LS_CAP
    assert re.search(r"s->CVB = CV < 256 \? CV : 256;\s*s->RP = 256 / s->CVB;", src)
    for shape, want in zip(R.DW_TRIP_SHAPES, R.DW_TRIP_PLANS):
        ntiles, cblocks, G = R.dw_wgrad_plan(*shape)
        assert (ntiles, cblocks, G) == want and G < ntiles < 2 * G           # some workgroups take two tiles, the others one
    assert R.dw_wgrad_plan(2, 33, 100, 512)[0] - R.dw_wgrad_plan(2, 33, 100, 512)[2] == 6
    assert R.dw_wgrad_plan(3, 33, 40, 136) == (45, 5, 45)                    # the largest earlier case: one tile per workgroup
    assert R.dw_wgrad_plan(13, 56, 56, 96)[0] > R.dw_wgrad_plan(13, 56, 56, 96)[2] == 341 >= R.dw_wgrad_plan(12, 56, 56, 96)[0]
    M, C = R.LS_TRIP_SHAPE
    CVB, RP, ncb, G = R.ls_bwd_plan(M, C)
    assert (CVB, RP, ncb, G) == R.LS_TRIP_PLAN and 2 * G * RP < M < 3 * G * RP and M % RP != 0
    assert R.ls_bwd_plan(1031, 1032) == (256, 1, 2, 512) and R.ls_bwd_plan(1031, 136) == (34, 7, 1, 148)


def test_dyadic_layer_scale_problem_is_exact_and_every_trip_shows_in_it():
    """The exact gamma-gradient case of tests/test_gpu_slivit_kernels.py: its sums are fp32 numbers in any order of addition, the
    restated walk visits every row once, and a restarted accumulator, one workgroup's dropped second trip or a fold that stops one
    row part short each change the gradient -- which the GPU test compares with torch.equal."""
    M, C = R.LS_TRIP_SHAPE
    dout, branch, gamma, gg0 = R.ls_dyadic_problem(M, C, seed=5)
    p = dout.double() * branch.double()
    want = gg0.double() + p.sum(0)
    assert torch.equal(want.float().double(), want) and float(p.abs().sum(0).max() + gg0.abs().max()) * 16 < 2 ** 24
    assert torch.equal((p * 16).round(), p * 16) and float(p.abs().max()) <= 0.25
    # fp32 sums in two very different orders: a running sum down the rows, and blocks of 4099 rows summed then added
    run = torch.zeros(C)
    for blk in p.float().split(4099):
        run = run + blk.sum(0)
    assert torch.equal(run.double(), p.sum(0)) and torch.equal(p.float().flip(0).cumsum(0)[-1].double(), p.sum(0))
    assert torch.equal(R.ls_bwd_walk_sum(dout, branch), p.sum(0))
    for fault in ("restart", "drop_trip", "fold"):
        got = gg0.double() + R.ls_bwd_walk_sum(dout, branch, fault)
        assert not torch.equal(got, want) and int((got != want).sum()) >= C - 1, fault
