"""CPU side of the 2-D half of the validation pass: the restatements of tests/recon2d_ref.py against what the reference's own functions
gave (tests/golden/recon2d_small.npz, tools/gen_golden_recon2d.py), the exported symbols and the argument errors of
octmae_mae_compose_nc / octmae_white_border (reported before any launch), and the host logic of misc.get_visible_images_2d,
engine_pretrain.eval_one_epoch with a 2-D loader and engine_pretrain.eval_one_epoch_2d with stand-in models whose ``reconstruct`` is the
restatement."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import recon2d_ref as R
from tests import recon_ref as R0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- restatements and the fixture
def test_panel_restatement_equals_the_reference_fixture(golden_dir):
    z = R.load_fixture(golden_dir)
    for name in ("rgb", "triplet"):
        imgs, pred, mask, u, p, scale, shift = R.case(name, golden_dir)
        made = R.case(name)                                            # the generator's inputs are the stored ones
        assert all(torch.equal(a, b) for a, b in zip((imgs, pred, mask), made[:3]))
        got = R.panels_nc(pred, imgs, mask, u, p, scale, shift)
        want = torch.from_numpy(z["panels_" + name]).int()
        assert int(want.min()) == 0 and int(want.max()) == 255
        if name == "rgb":
            assert got.shape == (2, 4, 1, 32, 32, 3) and torch.equal(got[:, :, 0], want)
        else:
            assert got.shape == (2, 4, 3, 32, 32, 1) and torch.equal(got[..., 0], want)
    assert os.path.getsize(os.path.join(golden_dir, "recon2d_small.npz")) < 200 * 1024


def test_one_channel_with_the_oct_constants_is_the_3d_restatement():
    imgs, pred, mask, u, p, scale, shift = R.case("grey_oct")
    assert scale == R0.IMG_STD and shift == R0.IMG_MEAN
    assert torch.equal(R.panels_nc(pred, imgs, mask, u, p, scale, shift)[..., 0], R0.panels(pred, imgs, mask, None, u, p))


def test_imagenet_case_holds_values_where_one_fused_rounding_changes_the_level():
    """v * std + mean as ONE fused multiply-add (fp64: the product of two fp32 values is exact, then one rounding) gives another level
    on some of the case's values: a kernel that equals the restatement there does not contract."""
    imgs, pred, mask, u, p, scale, shift = R.case("imagenet")
    v = R.unpatchify(pred, 1, 32, 32, p, u, 3)
    s, m = torch.tensor(scale, dtype=torch.float32).double(), torch.tensor(shift, dtype=torch.float32).double()
    fused = torch.clip((v.double() * s + m).float() * 255, 0, 255).int()
    assert int((fused != R.level(v, scale, shift)).sum()) >= 8


def test_blanking_restatement_equals_the_reference_fixture(golden_dir):
    z = R.load_fixture(golden_dir)
    for name in R.WB_CASES:
        image = R.wb_case(name)
        assert np.array_equal(image.numpy(), z[f"wb_{name}_in"], equal_nan=True), name
        got, region = R.white_border(image)
        assert got.shape == image.shape and region.shape == image.shape
        assert np.array_equal(got.numpy(), z[f"wb_{name}_out"], equal_nan=True), name
        assert np.array_equal(region.numpy(), z[f"wb_{name}_region"]), name
    # what the cases are there to show
    assert z["wb_w64_region"].sum() == 0 and z["wb_const_region"].sum() == 0 and z["wb_nan_region"].sum() == 0
    w128 = z["wb_w128_region"][0]
    assert w128[3].all() and not w128[4, 5] and w128[4].sum() == 127               # the negative-stop slice, and the empty one
    assert w128[1, 120:].all() and not w128[1, :120].any() and w128[5, 1:25].all() and not w128[5, 25:].any()
    assert not w128[6].any() and not w128[7].any() and not w128[9].any()
    assert (z["wb_w128_out"][1:] == z["wb_w128_out"][:1]).all() and not (z["wb_w128_in"][1:] == z["wb_w128_in"][:1]).all()
    assert z["wb_thresh_region"].sum() == 2 and z["wb_thresh_region"][0, 0, 0] and z["wb_thresh_region"][0, 1, 1]
    assert np.isnan(z["wb_nan_out"]).sum() == 3                                       # frame 0, NaN and all, copied into every frame


def test_threshold_case_tells_the_roundings_apart():
    mx, mn = R.threshold_extremes()
    k32, gap = np.float32(15 / 255), np.float32(np.float32(mx) - np.float32(mn))
    sep = np.float32(np.float32(mx) - np.float32(k32 * gap))
    assert sep == np.float32(R.threshold(torch.tensor([mx, mn])))
    assert sep != np.float32(np.float64(mx) - np.float64(k32) * np.float64(gap))     # a fused multiply-add
    assert sep != np.float32(np.float64(mx) - (15 / 255) * np.float64(gap))          # the factor kept in double


def test_column_limits_are_the_references_double_comparisons():
    from octcubem_amd import ops
    assert ops.white_border_limits(512) == (6, 26, 507, 487)
    assert ops.white_border_limits(128) == (2, 7, 127, 122) and ops.white_border_limits(64) == (1, 4, 64, 61)
    assert ops.white_border_limits(100) == (2, 6, 99, 95)
    for W in (4, 64, 100, 128, 256, 500, 512, 1000):
        lim = ops.white_border_limits(W)
        assert lim == R.white_border_limits(W)
        for i in range(W + 1):
            assert (not (i > 0.01 * W)) == (i < lim[0]) and (i > 0.05 * W) == (i >= lim[1])
            assert (not (i < W - 0.01 * W)) == (i >= lim[2]) and (i < W - 0.05 * W) == (i < lim[3])


def test_denorm_cases_leave_most_values_in_the_exact_class():
    """tests/test_gpu_recon2d.py compares the denorm kernel exactly wherever the fp64 value is farther than 1e-3 from an integer (the
    rule and the margin of tests/test_gpu_recon.py) and asks that this covers >= 95 % of the values: shown here for its inputs."""
    for name in ("rgb", "rgb_small", "imagenet", "grey_oct"):
        imgs, pred, mask, u, p, scale, shift = R.denorm_case(name)
        pan, raw = R.panels_nc_denorm(pred, imgs, mask, u, p, scale, shift)
        assert float(R.exact_class(raw).double().mean()) >= 0.95, name
        assert torch.equal(pan[:, :2], R.panels_nc(pred, imgs, mask, u, p, scale, shift)[:, :2])
        assert float(((raw > 0) & (raw < 255)).double().mean()) > 0.3                     # and much of it is not clipped away


# ---------------------------------------------------------------------------------------------- the library
def test_both_libraries_export_the_symbols_at_abi_30():
    from octcubem_amd import _lib
    names = ("octmae_mae_compose_nc", "octmae_white_border", "octmae_white_border_ws_floats")
    assert _lib.expected_abi_version() >= 30 and all(n in _lib.SIGNATURES for n in names)
    lib = _lib.load()
    f16 = ctypes.CDLL(os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so"))
    assert all(hasattr(lib, n) and hasattr(f16, n) for n in names)
    assert f16.octmae_abi_version() == _lib.expected_abi_version() == lib.octmae_abi_version()
    mk = open(os.path.join(ROOT, "octcubem_amd", "csrc", "Makefile")).read()
    import re
    assert "recon2d.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert re.search(r"^\$\(O\)recon2d\.o:.*\n.*\n\t.*-ffp-contract=off", mk, re.M)


def _aligned():
    buf = ctypes.create_string_buffer(256)
    return buf, (ctypes.addressof(buf) + 15) & ~15      # never dereferenced: every call below is refused before a launch


def test_compose_nc_reports_argument_errors_without_a_gpu():
    from octcubem_amd import _lib, ops
    lib = _lib.load()
    buf, q = _aligned()
    f = ctypes.c_float

    def call(pred=q, bs=4 * 768, imgs=q, mask=q, out=q, B=2, C=3, T=1, H=32, W=32, u=1, p=16, L=4, scale=(1, 1, 1), shift=(0, 0, 0),
             denorm=0):
        return lib.octmae_mae_compose_nc(pred, bs, imgs, mask, out, B, C, T, H, W, u, p, L, *(f(x) for x in scale),
                                         *(f(x) for x in shift), denorm, None)

    for null in ("pred", "imgs", "mask", "out"):
        assert call(**{null: None}) == -1, null
    for bad in (dict(B=0), dict(T=0), dict(H=-32), dict(W=0), dict(u=0), dict(p=0), dict(L=0), dict(C=0)):
        assert call(**bad) == -1, bad
    assert call(C=2, bs=4 * 512) == -1 and call(C=4, bs=4 * 1024) == -1                       # one or three channels
    assert call(p=6, H=36, W=36, L=36, bs=36 * 108) == -1 and call(p=2, L=256, bs=256 * 12) == -1        # p % 4
    assert call(H=40) == -1 and call(W=40) == -1                                              # the patch does not tile the image
    assert call(p=4, H=8, W=10, L=4, bs=4 * 48) == -1                                         # W % 4
    assert call(L=3, bs=3 * 768) == -1 and call(L=5, bs=5 * 768) == -1                        # L is not a multiple of the 2 x 2 grid
    assert call(bs=4 * 768 - 4) == -1 and call(bs=0) == -1 and call(bs=4 * 768 + 2) == -1     # overlapping / misaligned samples
    assert call(pred=q + 4) == -1 and call(imgs=q + 8) == -1 and call(out=q + 1) == -1        # alignment
    assert call(L=8, bs=8 * 768) == -1                                                        # two predicted frames of a one-frame image
    assert call(C=1, T=3, u=3, L=8, bs=8 * 768) == -1                                         # six predicted frames of three
    assert call(scale=(1, float("nan"), 1)) == -1 and call(shift=(float("inf"), 0, 0)) == -1
    assert call(T=3, u=3, L=4, bs=4 * 2304) == -2                                             # a temporal patch of RGB frames
    assert call(denorm=2) == -2 and call(denorm=-1) == -2
    with pytest.raises(_lib.OctmaeError, match="bad argument"):
        _lib.call("octmae_mae_compose_nc", None, 0, None, None, None, 1, 1, 1, 4, 4, 1, 4, 1, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0, None)
    # ops.mae_compose_nc refuses the same before it looks for a device; and CPU tensors are an error, not a fall-back
    z = torch.zeros
    for args, kw in (((z(1, 1, 4 * 48), z(1, 3, 4, 4, 4), z(1, 1), 4, 4), {}),                # u > 1 with C > 1
                     ((z(1, 1, 32), z(1, 2, 1, 4, 4), z(1, 1), 1, 4), {}),                     # two channels
                     ((z(1, 1, 12), z(1, 3, 1, 2, 2), z(1, 1), 1, 2), {}),                     # p % 4
                     ((z(1, 2, 48), z(1, 3, 1, 4, 4), z(1, 2), 1, 4), {}),                     # two frames of one
                     ((z(1, 1, 47), z(1, 3, 1, 4, 4), z(1, 1), 1, 4), {}),                     # PD
                     ((z(1, 1, 48), z(1, 3, 1, 4, 4), z(1, 1), 1, 4), dict(scale=(1.0, float("inf"), 1.0))),
                     ((z(1, 1, 48), z(1, 3, 1, 4, 4), z(1, 1), 1, 4), dict(shift=(0.0, 0.0))),
                     ((z(1, 1, 48), z(1, 3, 1, 4, 4), z(1, 1), 1, 4), {})):                    # CPU tensors
        with pytest.raises(RuntimeError):
            ops.mae_compose_nc(*args, **kw)


def test_white_border_reports_argument_errors_without_a_gpu():
    from octcubem_amd import _lib, misc, ops
    lib = _lib.load()
    buf, q = _aligned()

    def call(imgs=q, region=q, ws=q, B=2, T=3, H=8, W=128, lim=(2, 7, 127, 122)):
        return lib.octmae_white_border(imgs, region, ws, B, T, H, W, *lim, None)

    for null in ("imgs", "region", "ws"):
        assert call(**{null: None}) == -1, null
    for bad in (dict(B=0), dict(T=0), dict(H=0), dict(W=-128), dict(W=126), dict(W=2)):
        assert call(**bad) == -1, bad
    assert call(imgs=q + 4) == -1 and call(region=q + 2) == -1 and call(ws=q + 1) == -1
    for k in range(4):
        for v in (-1, 130):
            lim = [2, 7, 127, 122]
            lim[k] = v
            assert call(lim=lim) == -1, lim
    ws = lib.octmae_white_border_ws_floats
    assert ws(2, 3, 8, 128) == 3 * 2 * 3 and ws(64, 3, 512, 512) == 3 * 64 * 64 and ws(1, 1, 1, 4) == 3
    assert ws(0, 3, 8, 128) == -1 and ws(2, 3, 8, 126) == -1 and ws(1 << 24, 3, 512, 512) == -2
    for bad in (torch.zeros(3, 8, 128), torch.zeros(1, 3, 8, 126), torch.zeros(1, 3, 8, 128, dtype=torch.float64), torch.zeros(1, 3, 8, 128)):
        with pytest.raises(RuntimeError):
            ops.white_border(bad)
    with pytest.raises(NotImplementedError):
        misc.find_and_convert_large_white_region(torch.zeros(8, 128), "pil")
    with pytest.raises(ValueError):
        misc.find_and_convert_large_white_region(torch.zeros(1, 3, 8, 128))
    with pytest.raises(ValueError):
        misc.blank_white_borders(torch.zeros(2, 3, 1, 8, 128))


# ---------------------------------------------------------------------------------------------- host logic with stand-in models
class _Joint:
    """What eval_one_epoch needs of the joint model: ``model(samples, mask_ratio)`` on [N, 1, T, H, W] (u = 1, p = 4) and ``reconstruct``
    with the ``normalization`` keyword."""

    def __init__(self):
        self.calls, self.seen, self.high_res_input_size = 0, [], (1, 2, 2)

    def parameters(self):
        return iter(())

    def eval(self):
        return self

    def __call__(self, samples, mask_ratio=0.75):
        assert not torch.is_grad_enabled()
        self.calls += 1
        self.seen.append((samples.clone(), mask_ratio))
        g = torch.Generator().manual_seed(self.calls)
        N, _, T, H, W = samples.shape
        L = T * (H // 4) * (W // 4)
        return torch.tensor(1.0 / self.calls), torch.rand(N, L, 16, generator=g) * 1.4 - 0.2, (torch.rand(N, L, generator=g) < mask_ratio).float()

    def reconstruct(self, imgs, pred, mask, denormalize=False, normalization=True):
        if normalization:
            return R0.panels(pred, imgs, mask, None, 1, 4).to(torch.uint8)
        return R.panels_nc(pred, imgs, mask, 1, 4)[..., 0].to(torch.uint8)


class _Flat:
    """The 2-D MAE's side of the same: [N, 3, H, W] images, p = 4, ``reconstruct(..., mean, std)``."""

    def __init__(self, losses=None):
        self.calls, self.means, self.losses = 0, [], losses

    def parameters(self):
        return iter(())

    def eval(self):
        return self

    def __call__(self, samples, mask_ratio=0.75):
        assert not torch.is_grad_enabled()
        self.calls += 1
        g = torch.Generator().manual_seed(100 + self.calls)
        N, C, H, W = samples.shape
        L = (H // 4) * (W // 4)
        loss = torch.tensor(1.0 / self.calls if self.losses is None else self.losses[min(self.calls, len(self.losses)) - 1])
        return loss, torch.rand(N, L, 16 * C, generator=g) * 1.4 - 0.2, (torch.rand(N, L, generator=g) < mask_ratio).float()

    def reconstruct(self, imgs, pred, mask, denormalize=False, mean=None, std=None):
        self.means.append(mean)
        scale, shift = (1.0, 0.0) if mean is None else (std, mean)
        return R.panels_nc(pred, imgs.unsqueeze(2), mask, 1, 4, scale, shift)[:, :, 0].to(torch.uint8)


def _read(path_without_npy):
    try:
        from PIL import Image
    except ImportError:
        return np.load(path_without_npy + ".npy")
    return np.array(Image.open(path_without_npy))


def _have_pillow():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


def _file(name):
    """the file get_visible_images_2d leaves for an image name (relative to visible_2d/), and the path to hand to _read"""
    if not _have_pillow():
        return name + ".npy", name
    shown = name if name.lower().endswith((".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".gif", ".webp")) else name + ".png"
    return shown, shown


def test_get_visible_images_2d_paths_and_file_shapes(tmp_path):
    from octcubem_amd import misc
    g = torch.Generator().manual_seed(0)
    # the 2-D MAE: RGB panels side by side, [H, 4 W, 3]; a sub-directory, a name with and one without an extension; a wrapper
    flat = _Flat()
    samples = torch.rand(3, 3, 8, 12, generator=g) * 1.4 - 0.2
    with torch.no_grad():
        _, pred, mask = flat(samples)
    names = ["pat1/scan_a.png", "scan_b", "pat2/deep/scan_c.PNG"]
    vars_ = {"reconstruct_imgs": pred, "samples": samples, "mask": mask, "img_names": names, "patch_embed": None}
    want = flat.reconstruct(samples, pred, mask)
    got = misc.get_visible_images_2d(vars_, types.SimpleNamespace(module=flat), str(tmp_path))
    assert got.dtype == torch.uint8 and got.shape == (3, 4, 8, 12, 3) and torch.equal(got, want)
    for i, name in enumerate(names):
        shown, readable = _file(name)
        assert os.path.isfile(tmp_path / "visible_2d" / shown), shown
        img = _read(str(tmp_path / "visible_2d" / readable))
        assert img.shape == (8, 48, 3) and img.dtype == np.uint8
        assert np.array_equal(img.reshape(8, 4, 12, 3).transpose(1, 0, 2, 3), want[i].numpy())
    assert sorted(os.listdir(tmp_path / "visible_2d")) == sorted(["pat1", "pat2", _file("scan_b")[0]])
    # mean / std travel as optional keys
    got = misc.get_visible_images_2d(dict(vars_, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD), flat, str(tmp_path / "inv"))
    assert flat.means[-1] == R.IMAGENET_MEAN and torch.equal(got, flat.reconstruct(samples, pred, mask, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD))
    assert not torch.equal(got, want)
    # one channel: [H, 4 W] grey
    grey = samples[:, :1].contiguous()
    with torch.no_grad():
        _, pred1, mask1 = flat(grey)
    got1 = misc.get_visible_images_2d({"reconstruct_imgs": pred1, "samples": grey, "mask": mask1, "img_names": ["g0", "g1", "g2"]}, flat,
                                      str(tmp_path / "grey"))
    img = _read(str(tmp_path / "grey" / "visible_2d" / _file("g1")[1]))
    assert got1.shape == (3, 4, 8, 12, 1) and img.shape == (8, 48)
    assert np.array_equal(img.reshape(8, 4, 12).transpose(1, 0, 2), got1[1, ..., 0].numpy())
    # the joint model's triplets: raw levels (normalization=False), the three frames as the three colour channels
    joint = _Joint()
    trip = torch.rand(2, 1, 3, 8, 8, generator=g) * 1.4 - 0.2
    with torch.no_grad():
        _, pred3, mask3 = joint(trip)
    got3 = misc.get_visible_images_2d({"reconstruct_imgs": pred3, "samples": trip, "mask": mask3, "img_names": ["t0.png", "t1.png"]},
                                      joint, str(tmp_path / "joint"))
    assert got3.shape == (2, 4, 3, 8, 8) and torch.equal(got3, joint.reconstruct(trip, pred3, mask3, normalization=False))
    assert not torch.equal(got3, joint.reconstruct(trip, pred3, mask3))
    img = _read(str(tmp_path / "joint" / "visible_2d" / _file("t1.png")[1]))
    assert img.shape == (8, 32, 3)
    assert np.array_equal(img.reshape(8, 4, 8, 3).transpose(1, 3, 0, 2), got3[1].numpy())
    with pytest.raises(ValueError):
        misc.get_visible_images_2d(dict(vars_, img_names=["only_one"]), flat, str(tmp_path / "bad"))


class _Loader2d:
    def __init__(self, batches):
        self.batches, self.iters = batches, 0

    def __iter__(self):
        self.iters += 1
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)


def test_eval_one_epoch_with_a_two_batch_2d_loader(tmp_path, monkeypatch):
    from octcubem_amd import engine_pretrain, misc
    blanked = []

    def blank(samples):           # the restatement in place of the kernel: this test is about the order of operations
        out = [R.white_border(s[0]) for s in samples]
        res = torch.stack([o[0] for o in out]).unsqueeze(1), torch.stack([o[1] for o in out]).unsqueeze(1)
        blanked.append(res[0].clone())
        return res

    monkeypatch.setattr(misc, "blank_white_borders", blank)
    g = torch.Generator().manual_seed(1)
    loader = [(torch.rand(1, 1, 2, 4, 4, generator=g), ([f"v{i}"], None)) for i in range(41)]
    band = torch.rand(2, 1, 3, 8, 64, generator=g) * 0.5
    band[:, :, 0, 2:5, :3] = 1.0                      # a white band at the left edge of frame 0: blanking changes the batch
    loader_2d = _Loader2d([(band.clone(), ("labels", [f"b0/s{i}.png" for i in range(2)])),
                           (band.flip(0).contiguous(), ("labels", [f"b1/s{i}.png" for i in range(2)]))])
    args = types.SimpleNamespace(output_dir=str(tmp_path / "with"), mask_ratio=0.75, accum_iter=1, repeat_aug=1)
    model = _Joint()
    stats = engine_pretrain.eval_one_epoch(model, loader, torch.device("cpu"), 2, args=args, joint=True, mask_ratio_2d=0.85,
                                           data_loader_2d=loader_2d, visible_frame_freq=1)
    # dump steps 0, 20 and 40: three 2-D batches off a two-batch loader, which is restarted once
    assert model.calls == 41 + 3 and len(blanked) == 3 and loader_2d.iters == 2
    two_d = [(s, r) for s, r in model.seen if s.shape[2] == 3]
    assert [r for _, r in two_d] == [0.85] * 3
    for (seen, _), want, src in zip(two_d, blanked, (band, band.flip(0), band)):
        assert torch.equal(seen, want) and not torch.equal(seen, src)                   # the model saw the blanked batch
        assert int((seen[:, :, :, 2:5, :3] != 0).sum()) == 0 and torch.equal(seen[:, :, 1], seen[:, :, 0])
    assert torch.equal(loader_2d.batches[0][0], band)                                      # the loader's tensors are left alone
    # the 2-D forward sits right after the 3-D forward of its dump step
    order = [s.shape[2] for s, _ in model.seen]
    assert [i for i, t in enumerate(order) if t == 3] == [1, 22, 43]
    root = tmp_path / "with" / "val_images_2"
    names_2d = sorted(os.path.join("visible_2d", _file(f"b{k}/s{i}.png")[0]) for k in (0, 1) for i in (0, 1))
    assert sorted(f for f in _tree(root) if f.startswith("visible_2d")) == names_2d
    assert sorted(os.listdir(root)) == ["v0", "v20", "v40", "visible_2d"]
    assert _read(str(root / "visible_2d" / _file("b1/s0.png")[1])).shape == (8, 4 * 64, 3)
    # the meters are those of the 3-D loader alone
    assert set(stats) == {"loss", "mask_ratio"} and stats["mask_ratio"] == 0.75
    losses = [1.0 / k for k in range(1, 45) if k not in (2, 23, 44)]
    assert stats["loss"] == pytest.approx(sum(losses) / 41, rel=1e-6)
    # without the loader, or without ``joint``: exactly the files of the 3-D pass, and no 2-D forward
    for sub, kw in (("none", dict(joint=True, data_loader_2d=None)), ("notjoint", dict(joint=False, data_loader_2d=loader_2d)),
                    ("plain", dict())):
        m2 = _Joint()
        a2 = types.SimpleNamespace(output_dir=str(tmp_path / sub), mask_ratio=0.75, accum_iter=1, repeat_aug=1)
        plain_loader = loader if kw.get("joint") else [(s, n[0]) for s, n in loader]
        engine_pretrain.eval_one_epoch(m2, plain_loader, torch.device("cpu"), 2, args=a2, mask_ratio_2d=0.85, visible_frame_freq=1, **kw)
        assert m2.calls == 41 and _tree(tmp_path / sub / "val_images_2") == [f for f in _tree(root) if not f.startswith("visible_2d")]
    assert len(blanked) == 3 and loader_2d.iters == 2


class _Writer:
    def __init__(self):
        self.log_dir, self.scalars = "unused", []

    def add_scalar(self, key, value, step):
        self.scalars.append((key, value, step))


def test_eval_one_epoch_2d_dump_steps_meters_and_nonfinite_guard(tmp_path):
    from octcubem_amd import engine_pretrain
    g = torch.Generator().manual_seed(2)
    loader = [(torch.rand(2, 3, 8, 8, generator=g), [f"s{i}/a.png", f"s{i}/b"]) for i in range(41)]
    args = types.SimpleNamespace(output_dir=str(tmp_path), mask_ratio=0.5, accum_iter=2)
    model, w = _Flat(), _Writer()
    stats = engine_pretrain.eval_one_epoch_2d(model, loader, torch.device("cpu"), 5, log_writer=w, args=args, visible_frame_freq=1,
                                              fp32=True, joint=False)
    assert model.calls == 41 and model.means == [None, None]
    # (step + 1) % 20 == 0: steps 19 and 39, the whole batch under its names
    root = tmp_path / "val_images_5" / "visible_2d"
    assert sorted(os.listdir(root)) == ["s19", "s39"]
    assert sorted(os.listdir(root / "s39")) == sorted([_file("a.png")[0], _file("b")[0]])
    assert _read(str(root / "s19" / _file("b")[1])).shape == (8, 32, 3)
    assert stats["mask_ratio"] == 0.5 and stats["loss"] == pytest.approx(sum(1.0 / k for k in range(1, 42)) / 41, rel=1e-6)
    assert [k for k, _, _ in w.scalars] == ["val_loss"] * 20 and w.scalars[0][2] == int((1 / 41 + 5) * 1000)
    # the default of 20 dumps nothing in a 41-step epoch (step 399 would be the first)
    m2 = _Flat()
    engine_pretrain.eval_one_epoch_2d(m2, loader, torch.device("cpu"), 6, args=args)
    assert m2.calls == 41 and os.listdir(tmp_path / "val_images_6") == []
    # the inverse ImageNet transform: any value but None switches the levels
    m3 = _Flat()
    engine_pretrain.eval_one_epoch_2d(m3, loader[:20], torch.device("cpu"), 7, args=args, visible_frame_freq=1,
                                      inverse_imagenet_transform=True)
    assert m3.means == [R.IMAGENET_MEAN]
    a, b = (_read(str(tmp_path / f"val_images_{e}" / "visible_2d" / "s19" / _file("b")[1])) for e in (5, 7))
    assert a.shape == b.shape and not np.array_equal(a, b)
    # a non-finite loss ends the pass with None before that step is dumped
    m4 = _Flat(losses=[1.0] * 19 + [float("inf")])
    assert engine_pretrain.eval_one_epoch_2d(m4, loader, torch.device("cpu"), 8, args=args, visible_frame_freq=1) is None
    assert m4.calls == 20 and os.listdir(tmp_path / "val_images_8") == []
    assert torch.is_grad_enabled()
