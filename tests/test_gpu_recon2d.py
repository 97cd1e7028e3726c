"""GPU tests of the 2-D half of the validation pass (csrc/recon2d.hip): octmae_mae_compose_nc and octmae_white_border called directly on
buffers that sit between guard bytes, against the restatements of tests/recon2d_ref.py and the fixture the reference's own functions
wrote (tests/golden/recon2d_small.npz); then ``reconstruct`` on the 2-D MAE and on the joint model's B-scan branch,
``engine_pretrain.eval_one_epoch`` with its 2-D loader, and the direct cases once more on the half-operand build in a child process
(tests/f16_worker.py, started before this process touches the GPU).

Without ``denorm`` every byte of all four panels must be EQUAL: the kernel rounds where the reference's tensor ops round.  With it the
reference is the fp64 restatement, under the rule of tests/test_gpu_recon.py: every value within one level, and equal wherever the fp64
value before truncation is farther than 1e-3 from an integer (the fp32 chain -- mean and variance of at most 768 values, one sqrt, one
fma, the level -- is off by a few ulp of 255, about 1e-4); at least 95 % of the values are in that class
(tests/test_cpu_recon2d.py shows it for these inputs).  The blanked images and the regions must be EQUAL to the fixture."""
import json
import os
import types
from functools import partial

import numpy as np
import pytest
import torch

from tests import children
from tests import recon2d_ref as R
from tests import recon_ref as R0

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")
GUARD = 256                      # bytes of 0xA5 on either side of every buffer a kernel writes
DIRECT = ("rgb", "rgb_small", "triplet", "imagenet", "grey_oct", "clip")
DENORM = ("rgb", "rgb_small", "imagenet", "grey_oct")
BLANK = ("w128", "w64", "w100", "w512", "b2", "const", "nan", "thresh", "cap")


# ---------------------------------------------------------------------------------------------- direct calls between guard bytes
def guarded(nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes]


def assert_guards(*bufs):
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all()), "a guard byte was overwritten"


def _three(v):
    return [float(v)] * 3 if isinstance(v, (int, float)) else [float(x) for x in v]


def compose(pred, imgs, mask, u, p, scale=1.0, shift=0.0, denorm=False):
    """octmae_mae_compose_nc on a guarded output: int32 [B, 4, Tp, H, W, C].  ``pred`` on the GPU is used as it is (a strided view)."""
    from octcubem_amd import _lib
    B, C, T, H, W = imgs.shape
    L, PD = pred.shape[1:]
    Tp = R.pred_frames(pred, imgs, u, p)
    pd = pred if pred.is_cuda else pred.to(DEV).contiguous()
    assert pd.stride(2) == 1 and pd.stride(1) == PD
    im, mk = imgs.to(DEV).contiguous(), mask.to(DEV).contiguous()
    n = B * 4 * Tp * H * W * C
    buf, out = guarded(n)
    _lib.call("octmae_mae_compose_nc", pd.data_ptr(), pd.stride(0), im.data_ptr(), mk.data_ptr(), out.data_ptr(), B, C, T, H, W, u, p, L,
              *_three(scale), *_three(shift), int(denorm), torch.cuda.current_stream().cuda_stream)
    assert_guards(buf)
    return out.view(B, 4, Tp, H, W, C).cpu().int()


def blank(images):
    """octmae_white_border on guarded buffers: images f32 [B, T, H, W] -> (blanked f32, region bool)"""
    from octcubem_amd import _lib, ops
    B, T, H, W = images.shape
    n = images.numel()
    bi, im = guarded(4 * n)
    im = im.view(torch.float32).view(B, T, H, W)
    im.copy_(images)
    br, reg = guarded(n)
    nws = _lib.load().octmae_white_border_ws_floats(B, T, H, W)
    assert nws > 0
    bw, ws = guarded(4 * nws)
    _lib.call("octmae_white_border", im.data_ptr(), reg.data_ptr(), ws.data_ptr(), B, T, H, W, *ops.white_border_limits(W),
              torch.cuda.current_stream().cuda_stream)
    assert_guards(bi, br, bw)
    reg = reg.view(B, T, H, W).cpu()
    assert int(reg.max()) <= 1
    return im.cpu(), reg.bool()


def check_direct(name, golden_dir):
    imgs, pred, mask, u, p, scale, shift = R.case(name, golden_dir)
    got = compose(pred, imgs, mask, u, p, scale, shift)
    want = R.panels_nc(pred, imgs, mask, u, p, scale, shift)
    assert got.shape == want.shape
    assert torch.equal(got, want), f"case {name}: {int((got != want).sum())} bytes differ"
    if name == "rgb":
        assert torch.equal(got[:, :, 0], torch.from_numpy(R.load_fixture(golden_dir)["panels_rgb"]).int())
    if name == "triplet":
        assert torch.equal(got[..., 0], torch.from_numpy(R.load_fixture(golden_dir)["panels_triplet"]).int())
    if name == "clip":
        for k in (0, 2):
            assert int((got[:, k] == 0).sum()) > 100 and int((got[:, k] == 255).sum()) > 100
    if name == "grey_oct":       # the levels of recon.hip's grey(): the two kernels agree
        from octcubem_amd import ops
        old = ops.mae_compose(pred.to(DEV), imgs.to(DEV), mask.to(DEV), None, u, p)
        assert torch.equal(old.cpu().int(), got[..., 0])


def check_denorm(name):
    imgs, pred, mask, u, p, scale, shift = R.denorm_case(name)
    got = compose(pred, imgs, mask, u, p, scale, shift, denorm=True)
    want, raw = R.panels_nc_denorm(pred, imgs, mask, u, p, scale, shift)
    exact = R.exact_class(raw)
    Tp, (H, W), C = want.shape[2], imgs.shape[-2:], imgs.shape[1]
    removed = R.unpatchify(mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1]), Tp, H, W, p, u, C) != 0
    print(f"denorm {name}: max |diff| {int((got - want).abs().max())}, exact class {float(exact.double().mean()):.4f}, "
          f"unequal in it {int((got[:, 2] != want[:, 2])[exact].sum())}")
    assert float(exact.double().mean()) >= 0.95
    assert int((got - want).abs().max()) <= 1
    assert torch.equal(got[:, :2], want[:, :2])
    assert torch.equal(got[:, 2][exact], want[:, 2][exact])
    assert torch.equal(got[:, 3][exact | ~removed], want[:, 3][exact | ~removed])


def check_past_the_grid_cap():
    """compose_nc_kernel: one wave per token on at most 4096 workgroups of 4.  65 images of 16 x 16 patches are 16 640 tokens: the first
    256 waves make a second trip."""
    imgs, pred, mask, u, p, scale, shift = R.case("cap")
    assert pred.shape[0] * pred.shape[1] == 16640 > 4096 * 4
    got = compose(pred, imgs, mask, u, p, scale, shift)
    want = R.panels_nc(pred, imgs, mask, u, p, scale, shift)
    assert torch.equal(got, want), f"{int((got != want).sum())} bytes differ"


def blank_case(name):
    """-> (input [B, T, H, W], the fixture's image and region in that shape)"""
    if name == "cap":
        # wb_rows_kernel: one wave per row on at most 4096 workgroups of 4; 16 388 rows, of which the last four make a second trip (row
        # 16 386 is a marked one).  wb_extremes_kernel: 32 776 float4 groups on 64 x 256 threads, a third, ragged trip.  Too long for
        # the fixture: against the restatement, which the fixture's cases pin to the reference.
        img = R._background(1, 16388, 8)
        img[0, 0::3, 0:3] = 1.0          # followed from column 0, ends at 3 > 0.4: columns 3 .. 7 too
        img[0, 1::3, 1:4] = 1.0          # first white at 1 > 0.08: not followed
        img = torch.from_numpy(img)
        out, region = R.white_border(img)
        assert bool(region[0, 16386].all()) and not bool(region[0, 16387].any()) and 16388 > 4096 * 4
        return img.unsqueeze(0), out.unsqueeze(0).numpy(), region.unsqueeze(0).numpy()
    z = R.load_fixture(os.path.join(ROOT, "tests", "golden"))
    names = ("w128", "b2_second") if name == "b2" else (name,)
    ins = torch.stack([R.wb_case(n).reshape(-1, *R.wb_case(n).shape[-2:]) for n in names])
    outs = np.stack([z[f"wb_{n}_out"].reshape(ins.shape[1:]) for n in names])
    regions = np.stack([z[f"wb_{n}_region"].reshape(ins.shape[1:]) for n in names])
    return ins, outs, regions


def check_blank(name):
    ins, outs, regions = blank_case(name)
    got, region = blank(ins)
    assert np.array_equal(region.numpy(), regions), f"{name}: {int((region.numpy() != regions).sum())} marks differ"
    assert np.array_equal(got.numpy().view(np.uint32), outs.view(np.uint32)), name          # bit for bit, the NaN and -0 included
    if name in ("w64", "const"):
        assert not regions.any() and np.array_equal(got.numpy(), ins.numpy())
    if name == "nan":
        assert not regions.any() and np.array_equal(got[:, 0].numpy(), ins[:, 0].numpy(), equal_nan=True)
    if name == "b2":             # each image under its own extremes: the second alone gives the same
        alone, region_alone = blank(ins[1:])
        assert torch.equal(alone, got[1:]) and torch.equal(region_alone, region[1:]) and regions[1].sum() > 0


# ---------------------------------------------------------------------------------------------- the panels
@pytest.mark.parametrize("name", DIRECT)
def test_compose_nc_equals_the_reference_chain(name, golden_dir):
    check_direct(name, golden_dir)


def test_compose_nc_reads_the_strided_decoder_output_in_place():
    """pred as the [:, 1:, :] view of a [B, 1 + L, PD] buffer whose cls rows hold a value that would be drawn as 255, while nothing else
    in the inputs reaches level 100; directly and through ops.mae_compose_nc."""
    from octcubem_amd import ops
    imgs, pred, mask, u, p, scale, shift = R.case("rgb_small")
    imgs, pred = imgs.clamp(max=0.35), pred.clamp(max=0.35)
    full = torch.full((pred.shape[0], pred.shape[1] + 1, pred.shape[2]), 10.0)
    full[:, 1:] = pred
    view = full.to(DEV)[:, 1:, :]
    assert not view.is_contiguous()
    want = R.panels_nc(pred, imgs, mask, u, p)
    got = compose(view, imgs, mask, u, p)
    assert torch.equal(got, want)
    assert int(got.max()) < 100 and int(R.level(torch.tensor(10.0))) == 255
    out = ops.mae_compose_nc(view, imgs.to(DEV), mask.to(DEV), u, p)
    assert out.dtype == torch.uint8 and out.is_contiguous() and torch.equal(out.cpu().int(), want)


def test_compose_nc_draws_non_finite_values_as_zero():
    """A non-finite prediction is 0 in panels 2 and 3 (where it is shown), a non-finite image value 0 in panels 0, 1 and 3; every other
    byte equals the clean run."""
    imgs, pred, mask, u, p, scale, shift = R.case("imagenet")
    mask = mask.clone()
    mask[0, 3], mask[1, 2], mask[1, 0] = 1.0, 0.0, 0.0   # a bad prediction on a removed and on a visible token, a bad image value on a visible one
    imgs, pred = imgs.clone(), pred.clone()
    imgs[1, 1, 0, 5, 8:11], pred[0, 3, 100:103], pred[1, 2, 40:43] = 0.5, 0.5, 0.5        # mid-scale in the clean run: never level 0
    clean = compose(pred, imgs, mask, u, p, scale, shift)
    assert torch.equal(clean, R.panels_nc(pred, imgs, mask, u, p, scale, shift))
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")])
    imgs[1, 1, 0, 5, 8:11] = bad                         # token 0 of image 1, channel 1
    pred[0, 3, 100:103] = bad
    pred[1, 2, 40:43] = bad
    got = compose(pred, imgs, mask, u, p, scale, shift)
    ok_x = torch.isfinite(imgs[:, :, 0].permute(0, 2, 3, 1)).unsqueeze(1)                     # [B, 1, H, W, C]
    ok_p = torch.isfinite(R.unpatchify(pred, 1, 32, 32, p, u, 3))
    m = R.unpatchify(mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1]), 1, 32, 32, p, u, 3) != 0
    assert int((~ok_x).sum()) == 3 and int((~ok_p).sum()) == 6
    shows_bad = torch.stack([~ok_x, ~ok_x & ~m, ~ok_p, (m & ~ok_p) | (~m & ~ok_x)], dim=1)    # per panel: a bad value is drawn here
    masked_bad = (~ok_x & m)                                                                  # panel 1 draws 0 there anyway
    assert int(shows_bad[:, 0].sum()) == 3 and int(shows_bad[:, 2].sum()) == 6 and int(shows_bad[:, 3].sum()) == 6
    assert int(got[shows_bad].max()) == 0 and int(clean[shows_bad].min()) > 0
    assert int(masked_bad.sum()) == 0
    assert torch.equal(got[~shows_bad], clean[~shows_bad])


def test_compose_nc_tokens_past_the_grid_cap():
    check_past_the_grid_cap()


@pytest.mark.parametrize("name", DENORM)
def test_compose_nc_denorm_against_fp64(name):
    check_denorm(name)


# ---------------------------------------------------------------------------------------------- the blanking
@pytest.mark.parametrize("name", BLANK)
def test_white_border_equals_the_reference(name):
    check_blank(name)


def test_white_border_public_forms(golden_dir):
    """ops.white_border (in place), misc.find_and_convert_large_white_region on [T, H, W] and [H, W] from either device (the input
    untouched) and misc.blank_white_borders on [B, 1, T, H, W]."""
    from octcubem_amd import misc, ops
    z = R.load_fixture(golden_dir)
    x = R.wb_case("w128")
    for src in (x, x.to(DEV)):
        keep = src.clone()
        img, region = misc.find_and_convert_large_white_region(src)
        assert img.device == src.device and region.device == src.device and region.dtype == torch.bool
        assert torch.equal(src, keep)
        assert np.array_equal(img.cpu().numpy(), z["wb_w128_out"]) and np.array_equal(region.cpu().numpy(), z["wb_w128_region"])
    flat = R.wb_case("w100")
    img, region = misc.find_and_convert_large_white_region(flat.to(DEV))
    assert img.shape == flat.shape == region.shape
    assert np.array_equal(img.cpu().numpy(), z["wb_w100_out"]) and np.array_equal(region.cpu().numpy(), z["wb_w100_region"])
    batch = torch.stack([x, R.wb_case("b2_second")]).unsqueeze(1).to(DEV)                     # [2, 1, 3, 16, 128]
    keep = batch.clone()
    out, pre_mask = misc.blank_white_borders(batch)
    assert torch.equal(batch, keep) and out.shape == batch.shape == pre_mask.shape and pre_mask.dtype == torch.bool
    assert np.array_equal(out[1, 0].cpu().numpy(), z["wb_b2_second_out"]) and np.array_equal(pre_mask[0, 0].cpu().numpy(), z["wb_w128_region"])
    same, region = ops.white_border(batch[:, 0])
    assert same.data_ptr() == batch.data_ptr() and torch.equal(batch, out) and torch.equal(region.unsqueeze(1), pre_mask)


# ---------------------------------------------------------------------------------------------- models and the engine
def _mae2d(golden_dir):
    from octcubem_amd import models_mae_2d
    from oracle import vit_ref as V
    z = np.load(os.path.join(golden_dir, "mae2d_small.npz"))
    cfg = V.MAE2DConfig(**json.loads(str(z["cfg"])))
    m = models_mae_2d.MaskedAutoencoderViT(img_size=cfg.img_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, embed_dim=cfg.embed_dim,
                                           depth=cfg.depth, num_heads=cfg.num_heads, decoder_embed_dim=cfg.decoder_embed_dim,
                                           decoder_depth=cfg.decoder_depth, decoder_num_heads=cfg.decoder_num_heads, mlp_ratio=4,
                                           norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    m.load_state_dict(V.mae2d_init(cfg, seed=int(z["param_seed"])), strict=True)
    return m.to(DEV), cfg, torch.from_numpy(z["imgs"]), torch.from_numpy(z["noise"])


def test_mae2d_reconstruct_equals_the_chain(golden_dir):
    m, cfg, imgs, noise = _mae2d(golden_dir)
    p = cfg.patch_size
    with torch.no_grad():
        loss, pred, mask = m(imgs.to(DEV), 0.75, noise=noise.to(DEV))
    assert not pred.is_contiguous()                                   # the view of the decoder's [N, 1 + L, PD] output
    N, C, H, W = imgs.shape
    pc, mc = pred.cpu().contiguous(), mask.cpu()
    out = m.reconstruct(imgs.to(DEV), pred, mask)
    assert out.dtype == torch.uint8 and out.shape == (N, 4, H, W, C)
    want = R.panels_nc(pc, imgs.unsqueeze(2), mc, 1, p)[:, :, 0]
    assert torch.equal(out.cpu().int(), want)
    assert int((out[:, 1] != out[:, 0]).sum()) > 0 and int((out[:, 3] != out[:, 0]).sum()) > 0
    # the reconstruction panel is the reference-order unpatchify of the prediction
    assert torch.equal(out[:, 2].cpu().int(), R.level(m.unpatchify(pc).permute(0, 2, 3, 1)))
    inv = m.reconstruct(imgs.to(DEV), pred, mask, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD)
    assert torch.equal(inv.cpu().int(), R.panels_nc(pc, imgs.unsqueeze(2), mc, 1, p, R.IMAGENET_STD, R.IMAGENET_MEAN)[:, :, 0])
    with torch.autocast("cuda", dtype=torch.float16):
        assert torch.equal(m.reconstruct(imgs.to(DEV), pred, mask), out)
        den = m.reconstruct(imgs.to(DEV), pred, mask, denormalize=True)
    assert torch.equal(den[:, :2], out[:, :2]) and not torch.equal(den[:, 2], out[:, 2])
    with pytest.raises(ValueError):
        m.reconstruct(imgs.to(DEV), pred, mask, mean=R.IMAGENET_MEAN)


def _joint_model():
    from octcubem_amd import models_mae
    from oracle import mae3d_ref as O
    cfg = O.MAEConfig(input_size=64, in_chans=1, embed_dim=128, depth=2, num_heads=2, decoder_embed_dim=64, decoder_depth=2,
                      decoder_num_heads=2, num_frames=12, t_patch_size=3, pred_t_dim=12, high_res_input_size=128)
    m = models_mae.MaskedAutoencoderViT(
        input_size=64, patch_size=16, in_chans=1, embed_dim=128, depth=2, num_heads=2, decoder_embed_dim=64, decoder_depth=2,
        decoder_num_heads=2, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_frames=12, t_patch_size=3, sep_pos_embed=True,
        cls_embed=True, pred_t_dim=12, high_res_input_size=128)
    m.load_state_dict(O.init_params(cfg, seed=7, bias_std=0.02), strict=True)
    return m.to(DEV)


def test_joint_model_bscan_branch_draws_raw_levels():
    m = _joint_model()
    g = torch.Generator().manual_seed(3)
    trip = torch.rand(2, 1, 3, 128, 128, generator=g) * 1.4 - 0.2
    with torch.no_grad():
        loss, pred, mask = m(trip.to(DEV), mask_ratio=0.75)
    assert m._is_high_res(trip) and pred.shape == (2, 64, 768)
    out = m.reconstruct(trip.to(DEV), pred, mask, normalization=False)
    assert out.dtype == torch.uint8 and out.shape == (2, 4, 3, 128, 128)
    pc, mc = pred.cpu().contiguous(), mask.cpu()
    assert torch.equal(out.cpu().int(), R.panels_nc(pc, trip, mc, 3, 16)[..., 0])
    # the default path is the OCT levels of the 3-D dump, untouched
    assert torch.equal(m.reconstruct(trip.to(DEV), pred, mask).cpu().int(), R0.panels(pc, trip, mc, None, 3, 16))
    assert not torch.equal(m.reconstruct(trip.to(DEV), pred, mask), out)


def test_eval_one_epoch_writes_the_3d_and_the_2d_files(tmp_path):
    from octcubem_amd import engine_pretrain
    m = _joint_model()
    g = torch.Generator().manual_seed(9)
    loader = [(torch.rand(2, 1, 12, 64, 64, generator=g), ([f"b{k}/vol{i}" for i in range(2)], None)) for k in range(2)]
    trip = torch.rand(2, 1, 3, 128, 128, generator=g) * 0.6
    trip[:, 0, 0, 40:60, :10] = 1.0                                   # a white band at the left edge of frame 0
    loader_2d = [(trip.clone(), ("labels", ["scans/s0.png", "scans/s1"]))]
    args = types.SimpleNamespace(output_dir=str(tmp_path), mask_ratio=0.75, accum_iter=1)
    stats = engine_pretrain.eval_one_epoch(m, loader, torch.device(DEV), 0, args=args, joint=True, mask_ratio_2d=0.8,
                                           data_loader_2d=loader_2d)
    assert np.isfinite(stats["loss"]) and set(stats) == {"loss", "mask_ratio"}
    assert not m.training and all(p.grad is None for p in m.parameters())
    root = tmp_path / "val_images_0"
    assert sorted(os.listdir(root)) == ["b0", "visible_2d"] and sorted(os.listdir(root / "b0")) == ["vol0", "vol1"]      # step 0 only
    assert torch.equal(loader_2d[0][0], trip)
    try:
        from PIL import Image
    except ImportError:
        assert sorted(os.listdir(root / "visible_2d" / "scans")) == ["s0.png.npy", "s1.npy"]
        return
    assert sorted(os.listdir(root / "visible_2d" / "scans")) == ["s0.png", "s1.png"]
    img = np.array(Image.open(root / "visible_2d" / "scans" / "s1.png"))
    assert img.shape == (128, 4 * 128, 3)
    original = img[:, :128]                                           # panel 0: the blanked triplet, its frames as the colour channels
    blanked, region = R.white_border(trip[1, 0])
    assert bool(region[0, 40:60, :15].all()) and int(region[0].sum()) == 20 * 15          # the band and its five-column extension
    assert np.array_equal(original, R.level(blanked.permute(1, 2, 0)).numpy().astype(np.uint8))
    assert int(original[40:60, :15].max()) == 0 and (original[..., 0] == original[..., 1]).all()


# ---------------------------------------------------------------------------------------------- the half build
def half_build_cases():
    """What tests/f16_worker.py runs on the half-operand build."""
    golden, passed = os.path.join(ROOT, "tests", "golden"), []
    for name in DIRECT:
        check_direct(name, golden)
        passed.append(name)
    for name in DENORM:
        check_denorm(name)
        passed.append("denorm " + name)
    check_past_the_grid_cap()
    passed.append("past the cap")
    for name in BLANK:
        check_blank(name)
        passed.append("blank " + name)
    return {"passed": passed}


def start_children():
    """tests/conftest.py calls this once the collection holds a test of this module, before this process has touched the GPU;
    tests/children.py releases the worker when the GPU has room for it."""
    if os.path.exists(LIB_F16):
        children.spawn_f16_worker("recon2d_f16", "tests.test_gpu_recon2d:half_build_cases")


def test_half_build_runs_the_same_kernels():
    """Neither entry point has a 16-bit operand: liboctmae_f16.so must pass every direct compose and blanking case."""
    assert os.path.exists(LIB_F16), "make -C octcubem_amd/csrc both"
    start_children()
    res = children.f16_worker_result("recon2d_f16")
    assert res["lib"] == "liboctmae_f16.so" and res["lp_is_f16"] is True
    assert res["passed"] == [*DIRECT, *("denorm " + n for n in DENORM), "past the cap", *("blank " + n for n in BLANK)], res
