"""GPU tests of the full-coverage reconstruction: octmae_cover_accumulate / octmae_cover_finish through ops.cover_accumulate /
ops.cover_finish against the fp32 oracle of tests/cover_ref.py, bit for bit unless stated; ``MaskedAutoencoderViT.reconstruct_full`` on
the small fixture model against the manual loop; ``engine_pretrain.cover_one_epoch`` on a two-batch loader.

``pred`` is always the [:, 1:, :] view of a [B, 1 + L, PD] buffer whose cls rows hold 10.0, a value drawn as grey level 255.
The token score is the one output with an order of its own: it is held to the float64 mean of the oracle's fp32 terms within
(PD - 1) 2^-24 sum|terms| / PD plus one rounding of the division, which any summation order keeps (cover_ref.score_and_bound)."""
import csv
import os
import types

import numpy as np
import pytest
import torch

from tests import cover_ref as CR
from tests import recon_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL, SENTINEL_CNT = 12345.0, -77


def small_case(name):
    """(imgs, preds, masks, frame_idx, u, p): (a) four passes from the schedule; (b) eight frames, six of them predicted; (c) the real
    patch size on one token layer; (d) hand-made masks: one token never masked, one masked in every pass, one in pass 0 alone (its
    mean is the first prediction, which lies on the grey-level edges there)."""
    from octcubem_amd.models_mae import cover_noise
    if name == "c":
        B, T, H, p, u, Tp, fi = 1, 3, 32, 16, 3, 3, None
    elif name == "b":
        B, T, H, p, u, Tp, fi = 2, 8, 16, 4, 3, 6, torch.linspace(0, 7, 6).long().to(torch.int32)
    else:
        B, T, H, p, u, Tp, fi = 2, 6, 16, 4, 3, 6, None
    L = (Tp // u) * (H // p) ** 2
    len_keep = int(L * 0.25)
    noise = cover_noise(B, L, 0.75, generator=torch.Generator().manual_seed(ord(name)))
    K = noise.shape[0]
    imgs, preds, _ = CR.make_case(50 + ord(name), B, T, H, p, u, Tp, K)
    masks = [m.clone() for m in CR.schedule_masks(noise, len_keep)]
    assert K == 4 and preds[0].shape == (B, L, u * p * p) and (L, u * p * p) == ((4, 768) if name == "c" else (32, 48))
    if name == "d":
        for k in range(K):
            masks[k][0, 3], masks[k][1, 7], masks[k][0, 9] = 0.0, 1.0, float(k == 0)
    return imgs, preds, masks, fi, u, p


def strided(pred):
    full = torch.full((pred.shape[0], pred.shape[1] + 1, pred.shape[2]), 10.0)
    full[:, 1:] = pred
    view = full.to(DEV)[:, 1:, :]
    assert not view.is_contiguous() or pred.shape[0] == 1
    return view


def gpu_chain(preds, masks):
    from octcubem_amd import ops
    acc = cnt = None
    for pred, mask in zip(preds, masks):
        acc, cnt = ops.cover_accumulate(strided(pred), mask.to(DEV), acc, cnt)
    return acc, cnt


def gpu_finish(acc, cnt, imgs, fi, u, p, **kw):
    from octcubem_amd import ops
    return ops.cover_finish(acc, cnt, imgs.to(DEV), None if fi is None else fi.to(DEV), u, p, **kw)


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def check_score(score, terms, what=""):
    want, bound = CR.score_and_bound(terms)
    excess = ((score.cpu().double() - want).abs() / bound).max()
    print(f"{what} token score: worst |diff| / bound {float(excess):.3f}")
    assert bool(((score.cpu().double() - want).abs() <= bound).all())


def check_small(name):
    from octcubem_amd import ops
    imgs, preds, masks, fi, u, p = small_case(name)
    acc = cnt = None
    want_acc = want_cnt = None
    for k, (pred, mask) in enumerate(zip(preds, masks)):
        prev_acc, prev_cnt = want_acc, want_cnt
        want_acc, want_cnt = CR.accumulate(prev_acc, prev_cnt, pred, mask, k == 0)
        acc, cnt = ops.cover_accumulate(strided(pred), mask.to(DEV), acc, cnt)
        assert acc.dtype == torch.float32 and cnt.dtype == torch.int32 and acc.is_contiguous()
        assert torch.equal(bits(acc), bits(want_acc)) and torch.equal(cnt.cpu(), want_cnt), f"case {name} pass {k}"
        # the rows a pass must not touch, behind a sentinel (a first pass over filled buffers rewrites every row)
        m = mask != 0
        if k == 0:
            s_acc = torch.full_like(want_acc, SENTINEL).to(DEV)
            s_cnt = torch.full_like(want_cnt, SENTINEL_CNT).to(DEV)
            ops.cover_accumulate(strided(pred), mask.to(DEV), s_acc, s_cnt, first=True)
            assert torch.equal(bits(s_acc), bits(want_acc)) and torch.equal(s_cnt.cpu(), want_cnt)
        else:
            s_acc = torch.where(m.unsqueeze(-1), prev_acc, torch.tensor(SENTINEL)).to(DEV)
            s_cnt = torch.where(m, prev_cnt, torch.tensor(SENTINEL_CNT, dtype=torch.int32)).to(DEV)
            ops.cover_accumulate(strided(pred), mask.to(DEV), s_acc, s_cnt)
            assert torch.equal(bits(s_acc), bits(torch.where(m.unsqueeze(-1), want_acc, torch.tensor(SENTINEL))))
            assert torch.equal(s_cnt.cpu(), torch.where(m, want_cnt, torch.tensor(SENTINEL_CNT, dtype=torch.int32)))
    recon, err, score = gpu_finish(acc, cnt, imgs, fi, u, p)
    want_recon, want_err, v, terms = CR.finish(want_acc, want_cnt, imgs, fi, u, p)
    assert recon.dtype == torch.uint8 and recon.shape == want_recon.shape and err.shape == want_err.shape
    assert torch.equal(recon.cpu().int(), want_recon), f"case {name}: {int((recon.cpu().int() != want_recon).sum())} levels differ"
    assert torch.equal(bits(err), bits(want_err)), f"case {name}: {int((bits(err) != bits(want_err)).sum())} errors differ"
    compose = ops.mae_compose(v.to(DEV), imgs.to(DEV), torch.ones(v.shape[:2], device=DEV), None if fi is None else fi.to(DEV), u, p)
    assert torch.equal(recon, compose[:, 2])
    check_score(score, terms, f"case {name}")
    if name == "d":
        assert want_cnt[0, 3] == 0 and want_cnt[1, 7] == 4 and want_cnt[0, 9] == 1
        assert float(score[0, 3]) == 0.0 and torch.equal(v[0, 3], CR._target(imgs, fi, 6, u, p)[0, 3])
        assert torch.equal(v[0, 9], preds[0][0, 9])
    else:
        assert int(want_cnt.min()) == 3 == int(want_cnt.max())
    return True


@pytest.mark.parametrize("name", ("a", "b", "c", "d"))
def test_small_cases_equal_the_oracle_after_every_pass(name):
    check_small(name)


def check_denorm():
    """recon by the criteria of tests/test_gpu_recon.py::check_denorm for panel 2 (within one level of the float64 evaluation, equal
    wherever the float64 value is farther than 1e-3 from an integer, at least 95 % of the voxels in that class); err within the bound
    cover_ref.denorm64 derives from the arithmetic."""
    imgs, preds, masks, fi, u, p = small_case("d")
    preds = [(pr - 1.1) / 1.04 for pr in preds]                      # per-patch standardised units: about zero mean, unit spread
    acc, cnt = gpu_chain(preds, masks)
    want_acc, want_cnt = CR.accumulate_all(preds, masks)
    assert torch.equal(bits(acc), bits(want_acc))
    recon, err, score = gpu_finish(acc, cnt, imgs, fi, u, p, denorm=True)
    _, _, v, _ = CR.finish(want_acc, want_cnt, imgs, fi, u, p)       # v: the fp32 means, the input where cnt == 0
    seen = R.unpatchify((want_cnt > 0).float().unsqueeze(-1).repeat(1, 1, v.shape[-1]), 6, 16, 16, p, u)[:, 0] != 0
    want, raw, err64, err_bound = CR.denorm64(v, imgs, fi, u, p)
    exact = R.exact_class(raw)
    got = recon.cpu().int()
    plain = CR.finish(want_acc, want_cnt, imgs, fi, u, p)[0]
    excess = ((err.cpu().double() - err64).abs() / err_bound)[seen].max()
    print(f"denorm: exact class {float(exact[seen].double().mean()):.4f}, max level diff {int((got - want)[seen].abs().max())}, "
          f"err worst |diff| / bound {float(excess):.3f}")
    assert float(exact[seen].double().mean()) >= 0.95
    assert int((got - want)[seen].abs().max()) <= 1 and torch.equal(got[exact & seen], want[exact & seen])
    assert bool(((err.cpu().double() - err64).abs() <= err_bound)[seen].all())
    assert torch.equal(got[~seen], plain[~seen]) and float(err.cpu()[~seen].abs().max()) == 0.0      # a token never masked draws the input
    assert not torch.equal(got, plain)
    s64 = R.patchify(err.cpu().double().unsqueeze(1), p, u)          # the kernel's own fp32 terms
    want_s, bound = CR.score_and_bound(R.patchify(err.cpu().unsqueeze(1), p, u))
    assert bool(((score.cpu().double() - s64.mean(-1)).abs() <= bound).all()) and want_s.shape == score.shape


def test_denorm_against_float64():
    check_denorm()


def test_optional_outputs_keep_the_other_bits_and_two_runs_agree():
    imgs, preds, masks, fi, u, p = small_case("b")
    acc, cnt = gpu_chain(preds, masks)
    acc2, cnt2 = gpu_chain(preds, masks)
    assert torch.equal(bits(acc), bits(acc2)) and torch.equal(cnt, cnt2)
    for denorm in (False, True):
        recon, err, score = gpu_finish(acc, cnt, imgs, fi, u, p, denorm=denorm)
        again = gpu_finish(acc2, cnt2, imgs, fi, u, p, denorm=denorm)
        assert torch.equal(recon, again[0]) and torch.equal(bits(err), bits(again[1])) and torch.equal(bits(score), bits(again[2]))
        r1, e1, s1 = gpu_finish(acc, cnt, imgs, fi, u, p, denorm=denorm, error_volume=False)
        assert e1 is None and torch.equal(r1, recon) and torch.equal(bits(s1), bits(score))
        r2, e2, s2 = gpu_finish(acc, cnt, imgs, fi, u, p, denorm=denorm, token_score=False)
        assert s2 is None and torch.equal(r2, recon) and torch.equal(bits(e2), bits(err))
        r3, e3, s3 = gpu_finish(acc, cnt, imgs, fi, u, p, denorm=denorm, error_volume=False, token_score=False)
        assert e3 is None and s3 is None and torch.equal(r3, recon)


def test_planted_nan_reaches_exactly_the_outputs_that_use_it():
    imgs, preds, masks, fi, u, p = small_case("a")
    clean = gpu_finish(*gpu_chain(preds, masks), imgs, fi, u, p)
    PD = preds[0].shape[-1]
    b, l = 1, 11
    k_masked = next(k for k in range(4) if masks[k][b, l] != 0 and k > 0)
    k_kept = next(k for k in range(4) if masks[k][b, l] == 0)
    token = torch.zeros(preds[0].shape[:2], dtype=torch.bool)
    token[b, l] = True
    voxels = R.unpatchify(token.float().unsqueeze(-1).repeat(1, 1, PD), 6, 16, 16, p, u)[:, 0] != 0
    assert int(voxels.sum()) == PD

    def run(k, elems):
        bad = [pr.clone() for pr in preds]
        bad[k][b, l, elems] = float("nan")
        acc, cnt = gpu_chain(bad, masks)
        return gpu_finish(acc, cnt, imgs, fi, u, p)

    # the token's whole row in a pass that masks it: its PD voxels, and nothing else
    recon, err, score = run(k_masked, slice(None))
    assert bool(torch.isnan(err.cpu()[voxels]).all()) and int(recon.cpu()[voxels].max()) == 0 and bool(torch.isnan(score[b, l]))
    assert torch.equal(recon.cpu()[~voxels], clean[0].cpu()[~voxels]) and torch.equal(bits(err)[~voxels], bits(clean[1])[~voxels])
    assert torch.equal(bits(score)[~token], bits(clean[2])[~token])
    # one element of it: that one voxel, and the token's score
    recon, err, score = run(k_masked, 17)
    hit = torch.isnan(err.cpu())
    assert int(hit.sum()) == 1 and bool(voxels[hit].all()) and int(recon.cpu()[hit]) == 0 and bool(torch.isnan(score[b, l]))
    assert torch.equal(recon.cpu()[~hit], clean[0].cpu()[~hit]) and torch.equal(bits(err)[~hit], bits(clean[1])[~hit])
    assert torch.equal(bits(score)[~token], bits(clean[2])[~token])
    # in the pass that keeps the token: no output bit changes
    recon, err, score = run(k_kept, slice(None))
    assert torch.equal(recon, clean[0]) and torch.equal(bits(err), bits(clean[1])) and torch.equal(bits(score), bits(clean[2]))


def check_past_the_grid_cap():
    """Both kernels: one wave per token on at most 4096 workgroups of 4 (16 384 tokens).  p = 4, u = 1 on two frames of 516 x 516 is
    33 282 tokens, as the cap case of tests/test_gpu_recon.py: a third trip for 514 of them.  Two passes: the first-pass kernel and the
    adding one; the second mask leaves tokens with counts 0, 1 and 2."""
    B, T, H, u, p = 1, 2, 516, 1, 4
    L = (T // u) * (H // p) ** 2
    assert L > 2 * 4096 * 4 and (L - 2 * 4096 * 4) % 4 != 0
    g = torch.Generator().manual_seed(17)
    imgs = torch.randn(B, 1, T, H, H, generator=g)
    preds = [torch.randn(B, L, u * p * p, generator=g) for _ in range(2)]
    masks = [(torch.rand(B, L, generator=g) > 0.3).float() for _ in range(2)]
    acc, cnt = gpu_chain(preds, masks)
    want_acc, want_cnt = CR.accumulate_all(preds, masks)
    assert sorted(want_cnt.unique().tolist()) == [0, 1, 2]
    assert torch.equal(bits(acc), bits(want_acc)) and torch.equal(cnt.cpu(), want_cnt)
    recon, err, score = gpu_finish(acc, cnt, imgs, None, u, p)
    want_recon, want_err, _, terms = CR.finish(want_acc, want_cnt, imgs, None, u, p)
    assert torch.equal(recon.cpu().int(), want_recon) and torch.equal(bits(err), bits(want_err))
    check_score(score, terms, "past the cap")


def test_tokens_past_the_grid_cap():
    check_past_the_grid_cap()


# ---------------------------------------------------------------------------------------------- model and engine
def _small_model(golden_dir):
    from tests.test_gpu_model import build, small
    z, cfg, P = small(golden_dir)
    return build(cfg, P), cfg, z


def _manual(m, imgs, ratio, seed):
    """cover_noise, K forwards with it, the oracle's accumulate and finish on what they returned."""
    from octcubem_amd.models_mae import cover_noise
    N, L = imgs.shape[0], 64
    noise = cover_noise(N, L, ratio, generator=torch.Generator().manual_seed(seed))
    masks, losses, acc, cnt = [], [], None, None
    with torch.no_grad():
        for k in range(noise.shape[0]):
            loss, pred, mask = m(imgs.to(DEV), ratio, noise=noise[k].to(DEV))
            masks.append(mask.cpu())
            losses.append(float(loss))
            acc, cnt = CR.accumulate(acc, cnt, pred.cpu().contiguous(), mask.cpu(), k == 0)
    want_masks = CR.schedule_masks(noise, int(L * (1 - ratio)))
    assert torch.equal(torch.stack(masks), want_masks)                               # the model's masks are the schedule's
    fi = m._frame_idx(imgs.shape[2], "cpu")
    return noise.shape[0], losses, acc, cnt, CR.finish(acc, cnt, imgs, fi, m.t_pred_patch_size, m.patch_embed.patch_size[0])


@pytest.mark.parametrize("ratio", (0.75, 0.7))
def test_model_reconstruct_full_equals_the_manual_loop(ratio, golden_dir):
    m, cfg, z = _small_model(golden_dir)
    imgs = torch.from_numpy(z["imgs"])
    m.train()
    grads = [p.grad for p in m.parameters()]
    out = m.reconstruct_full(imgs.to(DEV), ratio, generator=torch.Generator().manual_seed(3), denormalize=False)
    assert m.training and all(p.grad is g for p, g in zip(m.parameters(), grads))
    m.eval()
    K, losses, acc, cnt, (recon, err, v, terms) = _manual(m, imgs, ratio, 3)
    len_keep = int(64 * (1 - ratio))
    twice = K * len_keep - 64
    assert out["passes"] == K == 4 and torch.equal(out["count"].cpu(), cnt)
    assert sorted(cnt.unique().tolist()) == ([K - 2, K - 1] if twice else [K - 1]) and int((cnt == K - 2).sum()) == 2 * twice * bool(twice)
    assert out["losses"] == losses
    assert out["recon"].dtype == torch.uint8 and torch.equal(out["recon"].cpu().int(), recon)
    assert torch.equal(bits(out["error"]), bits(err))
    check_score(out["token_score"], terms, f"model at {ratio}")
    assert out["frame_score"].dtype == torch.float64 and out["frame_score"].shape == (2, m.pred_t_dim)
    assert torch.allclose(out["frame_score"].cpu(), err.double().mean(dim=(2, 3)), rtol=1e-12, atol=0)
    assert out["volume_score"].dtype == torch.float64
    assert torch.allclose(out["volume_score"].cpu(), out["token_score"].cpu().double().mean(dim=1), rtol=1e-12, atol=0)
    # the same inside autocast, without the error volume, and with the default denormalize (the model's norm_pix_loss: False here)
    with torch.cuda.amp.autocast():
        ac = m.reconstruct_full(imgs.to(DEV), ratio, generator=torch.Generator().manual_seed(3), error_volume=False)
    assert not m.training and ac["error"] is None and ac["frame_score"] is None
    assert torch.equal(ac["recon"], out["recon"]) and torch.equal(bits(ac["token_score"]), bits(out["token_score"]))
    assert ac["losses"] == losses and torch.equal(ac["count"], out["count"])
    den = m.reconstruct_full(imgs.to(DEV), ratio, generator=torch.Generator().manual_seed(3), denormalize=True)
    assert torch.equal(den["count"], out["count"]) and not torch.equal(den["recon"], out["recon"])


def test_cover_one_epoch_on_a_two_batch_loader(golden_dir, tmp_path):
    from octcubem_amd import engine_pretrain
    m, cfg, z = _small_model(golden_dir)
    g = torch.Generator().manual_seed(9)
    shape = tuple(z["imgs"].shape)
    loader = [(torch.rand(shape, generator=g), [f"b{k}/vol{i}" for i in range(shape[0])]) for k in range(2)]
    args = types.SimpleNamespace(output_dir=str(tmp_path), mask_ratio=0.75)
    m.train()
    res = engine_pretrain.cover_one_epoch(m, loader, torch.device(DEV), 2, args=args, generator=torch.Generator().manual_seed(21),
                                          save_volumes=3)
    assert m.training and all(p.grad is None for p in m.parameters())
    gen = torch.Generator().manual_seed(21)
    outs = [m.reconstruct_full(samples.to(DEV), 0.75, generator=gen) for samples, _ in loader]
    vol = torch.cat([o["volume_score"] for o in outs]).cpu().numpy()
    frm = torch.cat([o["frame_score"] for o in outs]).cpu().numpy()
    assert np.array_equal(res["volume_score"], vol) and np.array_equal(res["frame_score"], frm)
    assert res["names"] == ["b0/vol0", "b0/vol1", "b1/vol0", "b1/vol1"] and np.array_equal(res["max_frame"], frm.argmax(axis=1))
    with open(tmp_path / "cover_scores_2.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 4 and [r["name"] for r in rows] == res["names"] and [int(r["index"]) for r in rows] == [0, 1, 2, 3]
    for i, r in enumerate(rows):
        assert float(r["volume_score"]) == vol[i] and float(r["max_frame_score"]) == frm[i].max() and int(r["max_frame"]) == frm[i].argmax()
    dump = np.load(tmp_path / "cover_volumes_2.npz")
    assert dump["recon"].shape[0] == 3 and np.array_equal(dump["recon"][2], outs[1]["recon"][0].cpu().numpy())
    assert np.array_equal(dump["error"][:2], outs[0]["error"].cpu().numpy())
