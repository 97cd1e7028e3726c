"""CPU side of the reconstruction volumes: the torch restatement of the reference's get_visible_images chain (tests/recon_ref.py)
against what the reference's own functions gave (tests/golden/recon_small.npz, tools/gen_golden_recon.py), the exported symbol and the
argument errors of octmae_mae_compose (reported before any launch), and the host logic of misc.get_visible_images /
engine_pretrain.eval_one_epoch with a stand-in model whose ``reconstruct`` is the restatement."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import recon_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_the_reference_fixture(golden_dir):
    z = R.load_fixture(golden_dir)
    for name in ("a", "b"):
        imgs, pred, mask, fi, u, p = R.case(name, golden_dir)
        got = R.panels(pred, imgs, mask, fi, u, p)
        assert got.shape == (2, 4, 6, 32, 32) and got.dtype == torch.int32
        assert torch.equal(got, z["panels_" + name].int()), name
    assert z["frame_idx_b"].tolist() == [0, 1, 3, 4, 6, 8] == torch.linspace(0, 8, 6).long().tolist()
    assert os.path.getsize(os.path.join(golden_dir, "recon_small.npz")) < 200 * 1024


def test_fixture_holds_voxels_where_one_fused_rounding_changes_the_grey_level(golden_dir):
    """The chain rounds v * s, + m and * 255 separately.  v * s + m as ONE fused multiply-add (exact product, one rounding: computed here
    in fp64, where the product of two fp32 values is exact) gives another grey level on some of the fixture's values: the fixture can
    tell the two apart, so a kernel that matches it does not contract."""
    z = R.load_fixture(golden_dir)
    v = torch.cat([z["pred"].flatten(), z["imgs9"].flatten()])
    s = torch.tensor(R.IMG_STD, dtype=torch.float32).double()
    m = torch.tensor(R.IMG_MEAN, dtype=torch.float32).double()
    fused = torch.clip((v.double() * s + m).float() * 255, 0, 255).int()
    assert int((fused != R.untransform_image(v)).sum()) >= 8
    both = z["panels_a"]
    assert int(both.min()) == 0 and int(both.max()) == 255


def test_denorm_cases_leave_most_voxels_in_the_exact_class(golden_dir):
    """tests/test_gpu_recon.py compares the denorm kernel exactly wherever the fp64 value is farther than 1e-3 from an integer and asks
    that this covers >= 95 % of the voxels: shown here for the restatement alone, on the inputs that test uses."""
    for name in ("a", "d"):
        imgs, pred, mask, fi, u, p = R.denorm_case(name, golden_dir)
        pan, raw = R.panels_denorm(pred, imgs, mask, fi, u, p)
        assert float(R.exact_class(raw).double().mean()) >= 0.95
        assert torch.equal(pan[:, :2], R.panels(pred, imgs, mask, fi, u, p)[:, :2])       # the frame panels do not depend on denorm
        inside = ((raw > 0) & (raw < 255)).double().mean()
        assert float(inside) > 0.5                                                        # and most of it is not clipped away


def test_both_libraries_export_the_symbol_at_abi_16():
    from octcubem_amd import _lib
    assert _lib.expected_abi_version() >= 16 and "octmae_mae_compose" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "octmae_mae_compose")
    f16 = ctypes.CDLL(os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so"))
    assert hasattr(f16, "octmae_mae_compose") and f16.octmae_abi_version() == _lib.expected_abi_version()


def test_compose_reports_argument_errors_without_a_gpu():
    from octcubem_amd import _lib, ops
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    q = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned; never dereferenced: every call below is refused before a launch

    def call(pred=q, bs=8 * 768, imgs=q, fi=None, mask=q, out=q, B=2, T=6, H=32, W=32, u=3, p=16, L=8, denorm=0):
        return lib.octmae_mae_compose(pred, bs, imgs, fi, mask, out, B, T, H, W, u, p, L, denorm, None)

    for null in ("pred", "imgs", "mask", "out"):
        assert call(**{null: None}) == -1, null
    for bad in (dict(B=0), dict(T=0), dict(H=-32), dict(W=0), dict(u=0), dict(p=0), dict(L=0)):
        assert call(**bad) == -1, bad
    assert call(p=6, H=36, W=36, L=72, bs=72 * 108) == -1            # p % 4
    assert call(p=2, H=32, W=32, u=4, L=512, bs=512 * 16) == -1      # p % 4, with PD % 4 == 0
    assert call(H=40) == -1 and call(W=40) == -1                     # the patch does not tile the frame
    assert call(L=7, bs=7 * 768) == -1 and call(L=9, bs=9 * 768) == -1        # L is not a multiple of the 2 x 2 grid
    assert call(bs=8 * 768 - 4) == -1 and call(bs=0) == -1           # samples would overlap
    assert call(bs=8 * 768 + 2) == -1                                # float4 loads need a stride that is a multiple of 4
    assert call(pred=q + 4) == -1 and call(imgs=q + 8) == -1 and call(out=q + 1) == -1       # alignment
    assert call(L=12, bs=12 * 768) == -1                             # 9 predicted frames of a 6-frame volume without frame_idx
    assert call(denorm=2) == -2 and call(denorm=-1) == -2
    with pytest.raises(_lib.OctmaeError, match="bad argument"):
        _lib.call("octmae_mae_compose", None, 0, None, None, None, None, 1, 1, 4, 4, 1, 4, 1, 0, None)
    # the kernel has no CPU form: CPU tensors are an error, not a fall-back
    with pytest.raises(RuntimeError):
        ops.mae_compose(torch.zeros(1, 1, 16), torch.zeros(1, 1, 1, 4, 4), torch.zeros(1, 1), None, 1, 4)


class _StandIn:
    """What eval_one_epoch and get_visible_images need of a model: ``model(samples, mask_ratio)`` and ``reconstruct``.  u = 1, p = 4."""

    def __init__(self, losses=None):
        self.calls, self.eval_called = 0, False
        self.losses = losses          # None: call k returns 1 / k; a list: call k returns losses[k - 1], the last one from then on

    def parameters(self):
        return iter(())

    def eval(self):
        self.eval_called = True
        return self

    def __call__(self, samples, mask_ratio=0.75):
        assert not torch.is_grad_enabled()
        self.calls += 1
        g = torch.Generator().manual_seed(self.calls)
        N, _, T, H, W = samples.shape
        L = T * (H // 4) * (W // 4)
        pred = torch.rand(N, L, 16, generator=g) * 3 - 0.5
        mask = (torch.rand(N, L, generator=g) < mask_ratio).float()
        if self.losses is None:
            loss = torch.tensor(1.0 / self.calls)
        else:
            loss = torch.tensor(self.losses[min(self.calls, len(self.losses)) - 1])
        return loss, pred, mask

    def reconstruct(self, imgs, pred, mask, denormalize=False):
        return R.panels(pred, imgs, mask, None, 1, 4).to(torch.uint8)


def _read_dump(d, n_frames, suffix="", offset=0):
    try:
        from PIL import Image
    except ImportError:
        return torch.from_numpy(np.load(os.path.join(d, f"frames{suffix}.npy")))
    rows = [np.array(Image.open(os.path.join(d, f"frame_{z + offset}{suffix}.png"))) for z in range(n_frames)]
    v = np.stack(rows)                                              # [Tp, H, 4 W]
    Tp, H, W4 = v.shape
    return torch.from_numpy(v.reshape(Tp, H, 4, W4 // 4).transpose(2, 0, 1, 3).copy())


def test_get_visible_images_file_names_and_module_unwrapping(tmp_path):
    from octcubem_amd import misc
    inner = _StandIn()
    samples = torch.rand(2, 1, 3, 8, 12, generator=torch.Generator().manual_seed(0)) * 3 - 0.5
    _, pred, mask = _no_grad_call(inner, samples)
    vars_ = {"reconstruct_imgs": pred, "samples": samples, "mask": mask, "img_names": ["pat1/vol_a", "vol_b"]}
    want = inner.reconstruct(samples, pred, mask)
    got = misc.get_visible_images(vars_, types.SimpleNamespace(module=inner), str(tmp_path), offset=5, suffix="_x")
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    for i, name in enumerate(vars_["img_names"]):
        d = os.path.join(str(tmp_path), name)
        files = sorted(os.listdir(d))
        assert files in ([f"frame_{z}_x.png" for z in (5, 6, 7)], ["frames_x.npy"])
        assert torch.equal(_read_dump(d, 3, "_x", 5), want[i])
    # the same through the bare model, default offset / suffix
    misc.get_visible_images(vars_, inner, str(tmp_path / "bare"))
    assert sorted(os.listdir(tmp_path / "bare" / "vol_b")) in (["frame_0.png", "frame_1.png", "frame_2.png"], ["frames.npy"])
    with pytest.raises(ValueError):
        misc.get_visible_images(dict(vars_, img_names=["only_one"]), inner, str(tmp_path / "bad"))


def _no_grad_call(model, samples):
    with torch.no_grad():
        return model(samples)


class _Writer:
    def __init__(self):
        self.log_dir, self.scalars = "unused", []

    def add_scalar(self, key, value, step):
        self.scalars.append((key, value, step))


def test_eval_one_epoch_dump_steps_meters_and_nonfinite_guard(tmp_path):
    from octcubem_amd import engine_pretrain
    model = _StandIn()
    g = torch.Generator().manual_seed(1)
    loader = [(torch.rand(1, 1, 2, 4, 4, generator=g), [f"v{i}"]) for i in range(41)]
    args = types.SimpleNamespace(output_dir=str(tmp_path), mask_ratio=0.75, accum_iter=2, repeat_aug=1)
    w = _Writer()
    stats = engine_pretrain.eval_one_epoch(model, loader, torch.device("cpu"), 3, log_writer=w, args=args, visible_frame_freq=1)
    assert model.eval_called and model.calls == 41
    # print_freq (20) x visible_frame_freq (1): steps 0, 20 and 40 are dumped, nothing else
    assert sorted(os.listdir(tmp_path / "val_images_3")) == ["v0", "v20", "v40"]
    assert stats["mask_ratio"] == 0.75
    assert stats["loss"] == pytest.approx(sum(1.0 / k for k in range(1, 42)) / 41, rel=1e-6)
    assert [k for k, _, _ in w.scalars] == ["val_loss"] * 20 and w.scalars[0][2] == int((1 / 41 + 3) * 1000)
    # the reference's default of 20 dumps step 0 only in a 41-step epoch; a 6-D batch is folded into the batch axis
    model2 = _StandIn()
    loader2 = [(torch.rand(1, 2, 1, 2, 4, 4, generator=g), ["r0", "r1"])] + loader[:2]
    stats2 = engine_pretrain.eval_one_epoch(model2, loader2, torch.device("cpu"), 0, args=types.SimpleNamespace(
        output_dir=str(tmp_path / "second"), mask_ratio=0.5, accum_iter=1))
    assert sorted(os.listdir(tmp_path / "second" / "val_images_0")) == ["r0", "r1"] and stats2["mask_ratio"] == 0.5
    # a non-finite loss ends the pass with None (engine_finetune's convention), before that step is dumped
    model3 = _StandIn(losses=[float("nan")])
    assert engine_pretrain.eval_one_epoch(model3, loader, torch.device("cpu"), 9, args=args) is None
    assert os.listdir(tmp_path / "val_images_9") == []
    assert torch.is_grad_enabled()
