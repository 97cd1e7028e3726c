"""GPU tests of the reconstruction volumes: octmae_mae_compose called directly (ops.mae_compose) against the torch restatement of the
reference's chain (tests/recon_ref.py; cases (a) and (b) are tests/golden/recon_small.npz, which the reference's own functions wrote),
``MaskedAutoencoderViT.reconstruct`` on a model, ``engine_pretrain.eval_one_epoch`` with its dump, and the direct cases once more on the
half-operand build in a child process (tests/f16_worker.py, started before this process touches the GPU).

Without ``denorm`` every voxel of all four panels must be EQUAL: the kernel rounds where the reference's tensor ops round.  With it the
reference is the fp64 restatement: every voxel within one grey level, and equal wherever the fp64 value before truncation is farther
than 1e-3 from an integer -- the fp32 chain (mean and variance of at most 768 values, one sqrt, one fma, g) is off by a few ulp of 255,
about 1e-4, and 1e-3 is ten times that; at least 95 % of the voxels are in that class (tests/test_cpu_recon.py shows it for these inputs)."""
import os
import types

import numpy as np
import pytest
import torch

from tests import children
from tests import recon_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")
DIRECT = ("a", "b", "c", "d", "e")


def compose(pred, imgs, mask, fi, u, p, denorm=False):
    from octcubem_amd import ops
    out = ops.mae_compose(pred.to(DEV), imgs.to(DEV), mask.to(DEV), None if fi is None else fi.to(DEV, torch.int32), u, p, denorm)
    assert out.dtype == torch.uint8 and out.is_contiguous()
    return out.cpu().int()


def check_direct(name, golden_dir):
    imgs, pred, mask, fi, u, p = R.case(name, golden_dir)
    got = compose(pred, imgs, mask, fi, u, p)
    want = R.panels(pred, imgs, mask, fi, u, p)
    assert got.shape == want.shape
    assert torch.equal(got, want), f"case {name}: {int((got != want).sum())} voxels differ"
    if name in ("a", "b"):
        assert torch.equal(got, R.load_fixture(golden_dir)["panels_" + name].int())


def check_denorm(name, golden_dir):
    imgs, pred, mask, fi, u, p = R.denorm_case(name, golden_dir)
    got = compose(pred, imgs, mask, fi, u, p, denorm=True)
    want, raw = R.panels_denorm(pred, imgs, mask, fi, u, p)
    exact = R.exact_class(raw)
    Tp, (H, W) = want.shape[2], imgs.shape[-2:]
    removed = R.unpatchify(mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1]), Tp, H, W, p, u)[:, 0] != 0    # panel 3 shows the prediction there
    print(f"denorm {name}: max |diff| {int((got - want).abs().max())}, exact class {float(exact.double().mean()):.4f}, "
          f"unequal in it {int((got[:, 2] != want[:, 2])[exact].sum())}")
    assert float(exact.double().mean()) >= 0.95
    assert int((got - want).abs().max()) <= 1
    assert torch.equal(got[:, :2], want[:, :2])
    assert torch.equal(got[:, 2][exact], want[:, 2][exact])
    assert torch.equal(got[:, 3][exact | ~removed], want[:, 3][exact | ~removed])


@pytest.mark.parametrize("name", DIRECT)
def test_compose_equals_the_reference_chain(name, golden_dir):
    check_direct(name, golden_dir)


def test_compose_reads_the_strided_decoder_output_in_place(golden_dir):
    """(f) pred as the [:, 1:, :] view of a [B, 1 + L, PD] buffer whose cls rows hold a value that would be drawn as 255, while nothing
    else in the inputs reaches grey level 100."""
    imgs, pred, mask, fi, u, p = R.case("a", golden_dir)
    imgs, pred = imgs.clamp(max=0.5), pred.clamp(max=0.5)
    full = torch.full((pred.shape[0], pred.shape[1] + 1, pred.shape[2]), 10.0)
    full[:, 1:] = pred
    full = full.to(DEV)
    from octcubem_amd import ops
    view = full[:, 1:, :]
    assert not view.is_contiguous()
    got = ops.mae_compose(view, imgs.to(DEV), mask.to(DEV), None, u, p).cpu().int()
    assert torch.equal(got, R.panels(pred, imgs, mask, fi, u, p))
    assert int(got.max()) < 100 and int(R.untransform_image(torch.tensor(10.0))) == 255


def test_compose_clips_at_both_ends(golden_dir):
    """(g)"""
    imgs, pred, mask, fi, u, p = R.case("a", golden_dir)
    imgs, pred = imgs * 3, pred * 3
    got = compose(pred, imgs, mask, fi, u, p)
    assert torch.equal(got, R.panels(pred, imgs, mask, fi, u, p))
    for k in (0, 2):
        assert int((got[:, k] == 0).sum()) > 0 and int((got[:, k] == 255).sum()) > 0
    assert int(got.min()) == 0 and int(got.max()) == 255


@pytest.mark.parametrize("value", (1.0, 0.0))
def test_compose_all_removed_and_all_visible(value, golden_dir):
    """(h)"""
    imgs, pred, mask, fi, u, p = R.case("a", golden_dir)
    mask = torch.full_like(mask, value)
    got = compose(pred, imgs, mask, fi, u, p)
    assert torch.equal(got, R.panels(pred, imgs, mask, fi, u, p))
    if value:
        assert int(got[:, 1].max()) == 0 and torch.equal(got[:, 3], got[:, 2])
    else:
        assert torch.equal(got[:, 1], got[:, 0]) and torch.equal(got[:, 3], got[:, 0])


def test_compose_draws_non_finite_values_as_zero(golden_dir):
    """The one departure from the reference (whose .int() of a NaN is undefined): a non-finite prediction is 0 in panels 2 and 3, a
    non-finite frame value 0 in panels 0, 1 and 3; every other voxel is untouched."""
    imgs, pred, mask, fi, u, p = R.case("a", golden_dir)
    mask = mask.clone()
    mask[0, 3], mask[1, 6], mask[1, 0] = 1.0, 0.0, 0.0      # a bad prediction on a removed and on a visible token, a bad frame value on a visible one
    want = R.panels(pred, imgs, mask, fi, u, p)
    imgs, pred = imgs.clone(), pred.clone()
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")])
    imgs[1, 0, 2, 5, 8:11] = bad
    pred[0, 3, 100:103] = bad
    pred[1, 6, 40:43] = bad
    got = compose(pred, imgs, mask, fi, u, p)
    clean_x, clean_p = torch.isfinite(imgs[:, 0]), torch.isfinite(R.unpatchify(pred, 6, 32, 32, p, u)[:, 0])
    m = R.unpatchify(mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1]), 6, 32, 32, p, u)[:, 0] != 0
    assert int((~clean_x).sum()) == 3 and int((~clean_p).sum()) == 6
    assert int(got[:, 0][~clean_x].max()) == 0 and int(got[:, 1][~clean_x].max()) == 0 and int(got[:, 2][~clean_p].max()) == 0
    assert int(got[:, 3][(m & ~clean_p) | (~m & ~clean_x)].max()) == 0
    assert torch.equal(got[:, 0][clean_x], want[:, 0][clean_x]) and torch.equal(got[:, 2][clean_p], want[:, 2][clean_p])
    ok3 = (m & clean_p) | (~m & clean_x)
    assert torch.equal(got[:, 3][ok3], want[:, 3][ok3])


def check_past_the_grid_cap(denorm):
    """compose_kernel: one wave per token on at most 4096 workgroups of 4 (16 384 tokens).  p = 4, u = 1 (16 values per token) on two
    frames of 516 x 516 is 33 282 tokens: a third trip for 514 of them (128 workgroups and two waves).  The same comparisons as the small
    cases: every voxel equal without denorm, the fp64 criteria of check_denorm with it."""
    B, T, H, W, u, p = 1, 2, 516, 516, 1, 4
    L = (T // u) * (H // p) * (W // p)
    assert L > 2 * 4096 * 4 and (L - 2 * 4096 * 4) % 4 != 0
    g = torch.Generator().manual_seed(13)
    imgs = torch.randn(B, 1, T, H, W, generator=g)
    pred = torch.randn(B, L, u * p * p, generator=g)
    mask = (torch.rand(B, L, generator=g) > 0.3).float()
    got = compose(pred, imgs, mask, None, u, p, denorm=denorm)
    if not denorm:
        want = R.panels(pred, imgs, mask, None, u, p)
        assert torch.equal(got, want), f"{int((got != want).sum())} voxels differ"
        return
    want, raw = R.panels_denorm(pred, imgs, mask, None, u, p)
    exact = R.exact_class(raw)
    removed = R.unpatchify(mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1]), T, H, W, p, u)[:, 0] != 0
    assert float(exact.double().mean()) >= 0.95
    assert int((got - want).abs().max()) <= 1
    assert torch.equal(got[:, :2], want[:, :2])
    assert torch.equal(got[:, 2][exact], want[:, 2][exact])
    assert torch.equal(got[:, 3][exact | ~removed], want[:, 3][exact | ~removed])


@pytest.mark.parametrize("denorm", (False, True))
def test_compose_tokens_past_the_grid_cap(denorm):
    check_past_the_grid_cap(denorm)


@pytest.mark.parametrize("name", ("a", "d"))
def test_compose_denorm_against_fp64(name, golden_dir):
    check_denorm(name, golden_dir)


# ---------------------------------------------------------------------------------------------- model and engine
def _small_model(golden_dir):
    from tests.test_gpu_model import build, small
    z, cfg, P = small(golden_dir)
    return build(cfg, P), cfg, z


def test_model_reconstruct_equals_the_chain_and_ignores_autocast(golden_dir):
    m, cfg, z = _small_model(golden_dir)
    imgs = torch.from_numpy(z["imgs"])
    noise = torch.from_numpy(z["noise"]).to(DEV)
    with torch.no_grad():
        loss, pred, mask = m(imgs.to(DEV), 0.75, noise=noise)
    assert not pred.is_contiguous()                                   # the view of the decoder's [N, 1 + L, PD] output
    out = m.reconstruct(imgs.to(DEV), pred, mask)
    T = imgs.shape[2]
    fi = m._frame_idx(T, "cpu")
    want = R.panels(pred.cpu().contiguous(), imgs, mask.cpu(), fi, m.t_pred_patch_size, m.patch_embed.patch_size[0])
    assert out.dtype == torch.uint8 and out.shape == (imgs.shape[0], 4, m.pred_t_dim, imgs.shape[3], imgs.shape[4])
    assert torch.equal(out.cpu().int(), want)
    assert int((out[:, 1] != out[:, 0]).sum()) > 0 and int((out[:, 3] != out[:, 0]).sum()) > 0
    with torch.autocast("cuda", dtype=torch.float16):
        out_ac = m.reconstruct(imgs.to(DEV), pred, mask)
        den_ac = m.reconstruct(imgs.to(DEV), pred, mask, denormalize=True)
    assert torch.equal(out_ac, out) and torch.equal(den_ac, m.reconstruct(imgs.to(DEV), pred, mask, denormalize=True))
    assert torch.equal(den_ac[:, :2], out[:, :2]) and not torch.equal(den_ac[:, 2], out[:, 2])


def _read_dump(d, n_frames):
    try:
        from PIL import Image
    except ImportError:
        return torch.from_numpy(np.load(os.path.join(d, "frames.npy")))
    v = np.stack([np.array(Image.open(os.path.join(d, f"frame_{z}.png"))) for z in range(n_frames)])
    Tp, H, W4 = v.shape
    return torch.from_numpy(v.reshape(Tp, H, 4, W4 // 4).transpose(2, 0, 1, 3).copy())


def test_eval_one_epoch_on_a_two_batch_loader(golden_dir, tmp_path):
    from octcubem_amd import engine_pretrain
    m, cfg, z = _small_model(golden_dir)
    g = torch.Generator().manual_seed(9)
    shape = tuple(z["imgs"].shape)
    loader = [(torch.rand(shape, generator=g), [f"b{k}/vol{i}" for i in range(shape[0])]) for k in range(2)]
    args = types.SimpleNamespace(output_dir=str(tmp_path), mask_ratio=0.75, accum_iter=1)
    torch.manual_seed(1234)
    stats = engine_pretrain.eval_one_epoch(m, loader, torch.device(DEV), 0, args=args)
    assert not m.training and all(p.grad is None for p in m.parameters())
    # the same two forwards under the same seed
    torch.manual_seed(1234)
    losses, first = [], None
    with torch.no_grad():
        for samples, _ in loader:
            loss, pred, mask = m(samples.to(DEV), mask_ratio=0.75)
            losses.append(loss.item())
            if first is None:
                first = m.reconstruct(samples.to(DEV), pred, mask).cpu()
    assert np.isfinite(stats["loss"]) and stats["loss"] == pytest.approx(sum(losses) / 2, rel=1e-12) and stats["mask_ratio"] == 0.75
    root = tmp_path / "val_images_0"
    assert sorted(os.listdir(root)) == ["b0"]                                            # step 0 only
    for i in range(shape[0]):
        assert torch.equal(_read_dump(str(root / "b0" / f"vol{i}"), first.shape[2]), first[i])


# ---------------------------------------------------------------------------------------------- the half build
def half_build_cases():
    """What tests/f16_worker.py runs on the half-operand build."""
    golden, passed = os.path.join(ROOT, "tests", "golden"), []
    for name in DIRECT:
        check_direct(name, golden)
        passed.append(name)
    for name in ("a", "d"):
        check_denorm(name, golden)
        passed.append("denorm " + name)
    for denorm in (False, True):
        check_past_the_grid_cap(denorm)
        passed.append("past the cap denorm" if denorm else "past the cap")
    return {"passed": passed}


def start_children():
    """tests/conftest.py calls this once the collection holds a test of this module, before this process has touched the GPU;
    tests/children.py releases the worker when the GPU has room for it."""
    if os.path.exists(LIB_F16):
        children.spawn_f16_worker("recon_f16", "tests.test_gpu_recon:half_build_cases")


def test_half_build_runs_the_same_compose_kernel():
    """The entry point has no 16-bit operand: liboctmae_f16.so must give the same panels on every direct case and both denorm cases."""
    assert os.path.exists(LIB_F16), "make -C octcubem_amd/csrc both"
    start_children()
    res = children.f16_worker_result("recon_f16")
    assert res["lib"] == "liboctmae_f16.so" and res["lp_is_f16"] is True
    assert res["passed"] == [*DIRECT, "denorm a", "denorm d", "past the cap", "past the cap denorm"], res
