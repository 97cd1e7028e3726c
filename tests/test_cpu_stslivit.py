"""CPU side of OCTCube with the SLIViT slice head: the committed golden (tests/golden/stslivit_small.npz, written by
tools/gen_golden_stslivit.py from the reference's own model class) against the restatement tests/stslivit_ref.py, without the reference
present; the shipped model's state-dict layout, constructor and refusals."""
import os

import numpy as np
import pytest
import torch

from tests import slivit_ref as R
from tests import stslivit_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stslivit_small.npz")


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def ref_run():
    torch.set_num_threads(1)
    P = S.init_params()
    x, target = S.make_inputs()
    return P, x, target, S.forward_backward(P, x, target)


def test_golden_file_is_complete_and_small():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 256 * 1024
    keys = [str(k) for k in g["keys"]]
    assert sorted(keys) == sorted(S.model_shapes().keys())
    assert not any(k.startswith("head.") for k in keys) and "norm.weight" in keys and "norm.bias" in keys
    assert sum(k.startswith(S.HP) for k in keys) == len(R.head_shapes(S.head_cfg()))
    T, C, L = 3, 64, 9
    assert g["embedding"].shape == (S.SMALL["batch"], T, C, L) and g["logits"].shape == (S.SMALL["batch"], 1) and g["embedding"].dtype == np.float32
    assert g["grad_norm"].shape == (len(keys),)
    for k, n in zip(keys, g["grad_norm"]):
        assert (n == 0) == (k in S.NO_GRAD), k                      # only ``norm.*`` has no gradient
    for dt in ("bfloat16", "float16"):
        for q in ("embedding", "logits", "loss"):
            assert 0 < float(g[f"rounding_err/{dt}/{q}"]) < 9.5e-3, (dt, q)             # the fixture is well conditioned: below the cap
        assert g[f"rounding_err/{dt}/grad"].shape == (len(keys),)
        for k in (str(k) for k in g["sample_keys"]):
            assert g["grad_sample/" + k].dtype == np.float32 and 0 < float(g[f"rounding_err/{dt}/sample/{k}"]) < 3e-2, (dt, k)
    assert float(np.abs(g["logits"]).min()) > 0.5                                      # no logit near 0: relative errors mean something


def test_restatement_reproduces_the_golden(ref_run):
    P, x, target, (emb, logits, loss, G) = ref_run
    g = np.load(GOLDEN)
    keys = [str(k) for k in g["keys"]]
    assert _rel(emb, g["embedding"]) <= 1e-5 and _rel(logits, g["logits"]) <= 1e-5
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * float(g["loss"])
    total = float(np.sqrt((g["grad_norm"].astype(np.float64) ** 2).sum()))
    for i, k in enumerate(keys):
        want = float(g["grad_norm"][i])
        if k in S.NO_GRAD:
            assert G[k] is None and want == 0.0
        elif want < 1e-6 * total:                                   # attn.k.bias: mathematically zero, fp32 noise on both sides
            assert float(G[k].double().norm()) <= 1e-4 * total, k
        else:
            assert abs(float(G[k].double().norm()) - want) <= 1e-4 * want, k
    for k in (str(k) for k in g["sample_keys"]):
        assert _rel(S.subsample(G[k]), g["grad_sample/" + k]) <= 1e-4, k


def test_embedding_is_the_transposed_view_and_rows_are_the_slabs(ref_run):
    """the golden's embedding [N, T, C, L], flattened per slice, is the patch matrix the slab LayerNorm kernel is specified on"""
    from tests import slabnorm_ref as SR
    P, x, *_ = ref_run
    stream = S.trunk_forward(P, x)
    g = np.load(GOLDEN)
    rows = SR.patch_rows(stream, 3, 9, 1)
    N = S.SMALL["batch"]
    assert _rel(rows.reshape(N, 3, 64, 9), g["embedding"]) <= 1e-5
    assert torch.equal(rows.reshape(N, 3, 64, 9), stream[:, 1:].reshape(N, 3, 9, 64).transpose(2, 3))


def test_rounding_model_rounds_where_it_says(ref_run):
    P, x, target, (emb, logits, loss, G) = ref_run
    g = np.load(GOLDEN)
    e1, l1, s1, G1 = S.forward_backward(P, x, target, dt=torch.bfloat16)
    assert abs(_rel(l1, logits) - float(g["rounding_err/bfloat16/logits"])) <= 0.05 * float(g["rounding_err/bfloat16/logits"]) + 1e-6
    assert abs(_rel(e1, emb) - float(g["rounding_err/bfloat16/embedding"])) <= 0.05 * float(g["rounding_err/bfloat16/embedding"]) + 1e-6


def build(**kw):
    from functools import partial
    from octcubem_amd import models_vit_st_flash_attn_slivit as M
    c = S.SMALL
    args = dict(num_frames=c["num_frames"], t_patch_size=c["t_patch_size"], img_size=c["img_size"], patch_size=c["patch_size"],
                in_chans=c["in_chans"], num_classes=c["num_classes"], embed_dim=c["embed_dim"], depth=c["depth"], num_heads=c["num_heads"],
                mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), sep_pos_embed=True, cls_embed=True, global_pool=True,
                slivit_depth_num=c["slivit_depth_num"])
    args.update(kw)
    return M.VisionTransformer(**args)


def test_state_dict_layout_and_constructor_of_the_shipped_model():
    from octcubem_amd import models_slivit_head, models_vit_st_flash_attn_slivit as M
    m = build()
    g = np.load(GOLDEN)
    sd = m.state_dict()
    assert sorted(sd.keys()) == sorted(str(k) for k in g["keys"])
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in S.model_shapes().items()}
    res = m.load_state_dict(S.init_params(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    h = m.SLIViT_head
    assert isinstance(h, models_slivit_head.SLIViT) and not hasattr(m, "head")
    assert (h.num_patches, h.patch_height, h.patch_width) == (3, 64, 9)
    at = h.transformer.layers[0][0]
    assert (at.heads, at.dim_head, h.mlp_head.in_features, h.transformer.layers[0][1].net[1].out_features) == (20, 64, 256, 512)
    assert len(h.transformer.layers) == 2 and len(build(slivit_depth_num=5).SLIViT_head.transformer.layers) == 5
    assert torch.equal(h.pos_embedding.detach(), torch.arange(4.0).view(1, 4, 1).expand(1, 4, 256))       # rnd_pos_emb=False: row i is i
    rnd = models_slivit_head.SLIViT(num_of_patches=3, vit_depth=2, patch_height=64, patch_width=9, rnd_pos_emb=True)
    assert rnd.pos_embedding.shape == (1, 4, 256) and float(rnd.pos_embedding.detach().std()) > 0.5
    assert sorted(rnd.state_dict().keys()) == sorted(R.head_shapes(S.head_cfg()).keys())
    import inspect
    sig = inspect.signature(M.VisionTransformer.__init__).parameters
    assert sig["slivit_depth_num"].default == 5 and sig["global_pool"].default is False and sig["use_flash_attn"].default is False
    for f in ("vit_base_patch16", "vit_large_patch16", "flash_attn_vit_large_patch16", "vit_huge_patch14"):
        assert callable(getattr(M, f))
    flash = build(use_flash_attn=True)
    assert "blocks.0.mixer.Wqkv.weight" in flash.state_dict() and flash.use_flash_attn


def test_refusals():
    from octcubem_amd import models_slivit_head
    with pytest.raises(ValueError, match="Class token can not be implemented for Slivit head"):
        build(global_pool=False)(torch.zeros(1, 1, 9, 48, 48))
    with pytest.raises(AssertionError):
        models_slivit_head.SLIViT(num_of_patches=3, patch_height=64, patch_width=9, dropout=0.1)
    with pytest.raises(AssertionError):
        models_slivit_head.SLIViT(num_of_patches=3, patch_height=64, patch_width=9, emb_dropout=0.1)
    with pytest.raises(ValueError):
        models_slivit_head.SLIViT(num_of_patches=3, patch_height=60, patch_width=9)


def test_lock_treats_the_slivit_head_as_the_head_group():
    m = build()
    m.lock(unlocked_groups=1)
    on = {k for k, p in m.named_parameters() if p.requires_grad}
    assert on and all(k.startswith(S.HP) for k in on) and len(on) == len(R.head_shapes(S.head_cfg()))
    m.lock(unlocked_groups=2)
    on = {k for k, p in m.named_parameters() if p.requires_grad}
    assert any(k.startswith("blocks.1.") for k in on) and "norm.weight" in on and not any(k.startswith("blocks.0.") for k in on)
