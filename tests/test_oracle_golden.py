"""CPU: the oracle restatement (oracle/mae3d_ref.py) against golden vectors produced by the
real reference (oracle/gen_golden.py, run in the build container).  Tolerance: 1e-5 relative
(fp32 CPU vs fp32 CPU, same torch build; the only differences are op ordering)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import mae3d_ref as O

REL = 1e-5


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _small(golden_dir):
    z = _load(golden_dir, "mae3d_small.npz")
    cfg = O.MAEConfig(**json.loads(str(z["cfg"])))
    P = O.init_params(cfg, seed=int(z["param_seed"]), bias_std=float(z["param_bias_std"]))
    chk = sum(float(v.double().sum()) for v in P.values())
    assert abs(chk - float(z["param_checksum"])) < 1e-9, "torch CPU RNG stream differs from the build container"
    return z, cfg, P


def golden_grad(z, k, g):
    """Golden grads are stored whole (<=8192 elements) or strided by 7, plus the full L2 norm."""
    ref = torch.from_numpy(z[f"grad/{k}"])
    mine = g if g.numel() <= 8192 else g.flatten()[::7]
    return mine.reshape(ref.shape), ref, float(z[f"gnorm/{k}"])


def relerr(a, b):
    a = torch.as_tensor(a).double(); b = torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_param_keys_and_count(golden_dir):
    z, cfg, P = _small(golden_dir)
    assert set(P) == set(O.param_shapes(cfg))
    for k, s in O.param_shapes(cfg).items():
        assert tuple(P[k].shape) == tuple(s), k
    pins = _load(golden_dir, "vitl_pins.npz")
    n = sum(int(np.prod(s)) for s in O.param_shapes(O.VIT_L).values())
    assert n == int(pins["n_params"]) == 331_632_384          # SURVEY §6 [probe]


def test_small_forward_backward_matches_reference(golden_dir):
    z, cfg, P = _small(golden_dir)
    imgs, noise = torch.from_numpy(z["imgs"]), torch.from_numpy(z["noise"])
    loss, pred, mask, ids_restore, grads = O.forward_backward(P, imgs, cfg, float(z["mask_ratio"]), noise)
    assert torch.equal(ids_restore, torch.from_numpy(z["ids_restore"]))        # bit-exact
    assert torch.equal(mask, torch.from_numpy(z["mask"]))
    assert abs(float(loss) - float(z["loss"])) <= REL * abs(float(z["loss"]))
    assert relerr(pred, z["pred"]) <= REL
    # The key bias gets an exactly zero gradient: it shifts every score of a query row by the same q.b, which the softmax
    # cancels.  Both sides hold fp32 summation noise there (~2e-10 of the global norm), whose pattern follows the host's thread
    # count, so those tensors are held to an absolute bound against the global gradient norm instead of a relative error.
    gall = sum(float(z[f"gnorm/{k}"]) ** 2 for k in grads) ** 0.5
    zero_bound = 1e-8 * gall
    for k, g in grads.items():
        mine, ref, gn = golden_grad(z, k, g)
        if gn == 0.0:
            assert float(g.abs().max()) == 0.0, k
            continue
        if k.endswith(".attn.k.bias"):
            assert gn <= zero_bound and float(g.double().norm()) <= zero_bound, (k, gn, float(g.double().norm()), zero_bound)
            continue
        assert relerr(mine, ref) <= 5e-5, k
        assert abs(float(g.double().norm()) - gn) <= 5e-5 * gn, k
    # parameters that must receive no gradient on the 256-style path
    for k in ("high_res_patch_embed.proj.weight", "high_res_patch_embed.proj.bias"):
        assert float(grads[k].abs().max()) == 0.0 and float(z[f"gnorm/{k}"]) == 0.0


def test_small_frame_losses(golden_dir):
    z, cfg, P = _small(golden_dir)
    imgs, noise = torch.from_numpy(z["imgs"]), torch.from_numpy(z["noise"])
    (loss, fl), pred, mask, _ = O.forward(P, imgs, cfg, 0.75, noise, frame_loss=True)
    assert relerr(fl, z["frame_losses"]) <= REL


def test_variants_normpix_ratio90_and_highres(golden_dir):
    z, cfg, P = _small(golden_dir)
    v = _load(golden_dir, "mae3d_small_variants.npz")
    imgs, noise = torch.from_numpy(z["imgs"]), torch.from_numpy(z["noise"])
    cfg_np = O.MAEConfig(**{**cfg.__dict__, "norm_pix_loss": True})
    loss, pred, mask, _ = O.forward(P, imgs, cfg_np, 0.9, noise)
    assert torch.equal(mask, torch.from_numpy(v["mask_r90"]))
    assert abs(float(loss) - float(v["loss_normpix_r90"])) <= REL * abs(float(v["loss_normpix_r90"]))
    assert relerr(pred, v["pred_r90"]) <= REL
    # high-res (2-D / 512-style) branch: T == t_patch frames, un-interpolated spatial table, no temporal
    loss, pred, mask, _ = O.forward(P, torch.from_numpy(v["imgs_hr"]), cfg, 0.75, torch.from_numpy(v["noise_hr"]))
    assert torch.equal(mask, torch.from_numpy(v["mask_hr"]))
    assert abs(float(loss) - float(v["loss_hr"])) <= REL * abs(float(v["loss_hr"]))
    assert relerr(pred, v["pred_hr"]) <= REL


def test_masking_bit_exact_tie_free_rows(golden_dir):
    m = _load(golden_dir, "masking.npz")
    noise = torch.from_numpy(m["noise_free"])
    for ratio, sfx in ((0.75, ""), (0.9, "_r90")):
        ids_shuffle, ids_restore, ids_keep, mask = O.masking_indices(noise, ratio)
        assert torch.equal(ids_keep, torch.from_numpy(m["ids_keep_free" + sfx]))
        assert torch.equal(mask, torch.from_numpy(m["mask_free" + sfx]))
        if not sfx:
            assert torch.equal(ids_restore, torch.from_numpy(m["ids_restore_free"]))


def test_masking_rows_with_ties_properties(golden_dir):
    """On rows with exact fp32 ties the reference's unstable argsort is not a function of the input
    alone; what is well defined and must hold: the sorted noise, the kept SET unless a
    tie straddles len_keep, ids_restore∘ids_shuffle = id, and mask.sum()."""
    m = _load(golden_dir, "masking.npz")
    noise = torch.from_numpy(m["noise_tie"])
    ids_shuffle, ids_restore, ids_keep, mask = O.masking_indices(noise, 0.75)
    L = noise.shape[1]
    ar = torch.arange(L).expand_as(ids_shuffle)
    assert torch.equal(torch.gather(ids_restore, 1, ids_shuffle), ar)
    ref_keep = torch.from_numpy(m["ids_keep_tie"])
    assert torch.equal(torch.gather(noise, 1, ids_keep), torch.gather(noise, 1, ref_keep))   # same sorted values
    assert float(mask.sum()) == float(m["mask_tie"].sum())
    srt = torch.sort(noise, dim=1).values
    straddle = srt[:, 1279] == srt[:, 1280]
    same = (torch.from_numpy(m["mask_tie"]) == mask).all(dim=1)
    assert bool((same | straddle).all())


def test_train_utils(golden_dir):
    z, cfg, P = _small(golden_dir)
    t = _load(golden_dir, "train_utils.npz")
    imgs, noise = torch.from_numpy(z["imgs"]), torch.from_numpy(z["noise"])
    _, _, _, _, G = O.forward_backward(P, imgs, cfg, 0.75, noise)
    assert abs(float(O.grad_norm(G.values())) - float(t["grad_norm"])) <= 1e-5 * float(t["grad_norm"])
    no_decay, decay = O.weight_decay_groups([(k, tuple(v.shape)) for k, v in P.items()], 0.05)
    # group membership (order inside a group follows module registration order and has no effect)
    assert set(no_decay) == set(json.loads(str(t["no_decay"]))) and set(decay) == set(json.loads(str(t["decay"])))
    assert len(no_decay) + len(decay) == len(P)
    for e, (lr, g0, g1) in zip(t["lr_epochs"], t["lr_values"]):
        mine = O.cosine_lr(float(e), 1.6e-3, 1e-6, 5, 50)
        assert abs(mine - lr) <= 1e-12 and abs(mine - g0) <= 1e-12 and abs(0.5 * mine - g1) <= 1e-12
    # two AdamW steps (lr 1.6e-3, betas .9/.95, wd .05 on the decay group) vs torch.optim.AdamW
    nd = set(no_decay)
    for k in [f[len("adamw2/"):] for f in t.files if f.startswith("adamw2/")]:
        p = P[k].clone(); m_ = torch.zeros_like(p); v_ = torch.zeros_like(p)
        g = G[k]
        wd = 0.0 if k in nd else 0.05
        p, m_, v_ = O.adamw_step(p, g, m_, v_, 1, 1.6e-3, 0.9, 0.95, 1e-8, wd)
        p, m_, v_ = O.adamw_step(p, 0.5 * g, m_, v_, 2, 1.6e-3, 0.9, 0.95, 1e-8, wd)
        assert relerr(p, t[f"adamw2/{k}"]) <= 1e-6, k   # grads differ from the reference's by <=5e-5 rel


@pytest.mark.skipif(os.environ.get("OCTMAE_SLOW", "0") != "1", reason="full ViT-L oracle forward (~20 s, 8 GB); set OCTMAE_SLOW=1")
def test_vitl_pins(golden_dir):
    pins = _load(golden_dir, "vitl_pins.npz")
    P = O.init_params(O.VIT_L, seed=0)
    imgs = torch.rand(1, 1, 60, 256, 256, generator=torch.Generator().manual_seed(0))
    torch.manual_seed(int(pins["noise_seed"]))
    noise = torch.rand(1, 5120)
    with torch.no_grad():
        loss, pred, mask, ids_restore = O.forward(P, imgs, O.VIT_L, 0.75, noise)
    assert torch.equal(ids_restore.int(), torch.from_numpy(pins["ids_restore"]))
    assert float(mask.sum()) == float(pins["mask_sum"]) == 3840.0
    assert abs(float(loss) - float(pins["loss"])) <= 1e-5 * float(pins["loss"])
    samp = pred.flatten()[torch.from_numpy(pins["pred_idx"])]
    assert relerr(samp, pins["pred_samples"]) <= 1e-4
