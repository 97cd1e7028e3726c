"""GPU: the fused volume transforms (csrc/transform3d.hip, ops.volume_box / ops.volume_resample, octcubem_amd.transforms) against the
torch CPU restatement of the reference's MONAI chain (tests/transform3d_ref.py).

Bounds (derived, not tuned):
  box        bit-exact (integers).
  resample   |out - ref| <= 2e-6 * max|x|: 7 linear interpolations of at most 3 fp32 roundings each = 21 * 2^-24 = 1.25e-6 of the range,
             rounded up (an unfused CPU restatement of the same formula sits at 1.2e-7 .. 4.2e-7 against F.interpolate).
  normalised the same bound times 4 (divisor 0.25), everywhere except on the mismatch set -- voxels where exactly one of ref_pre == 0 and
             out == 0 holds -- which may hold only voxels with ref_pre < 1e-6 * max|x|, and at most 0.1 % of the voxels.  (A voxel whose
             normalised value is exactly 0 on BOTH sides -- ref_pre == 0.25 exactly -- agrees; it is checked under the bound, not counted
             as a mismatch.)
Inputs are non-negative: uniform random values with x < 0.05 set to 0 and zero slabs cut at chosen faces."""
import argparse
from functools import lru_cache, partial

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import inference_utils as I, models_vit_st, ops
    from octcubem_amd.transforms import create_3d_transforms
from tests import transform3d_ref as R
from tests.conftest import parity

BOUND = 2e-6        # tests/transform3d_ref.py says what a value near it at a 61 -> 60 axis means (the host's ATen CPU capability)
DTYPES = {"u8": torch.uint8, "f32": torch.float32}
# (input [D, H, W], output (T, OH, OW)): down-sampling on every axis; up-sampling on every axis with D < T; the identity (every weight
# exactly 0 without the crop); a volume of several workgroups with rows that are no multiple of 16 bytes
CASES = {"down": ((7, 37, 45), (6, 32, 32)), "up": ((5, 19, 23), (6, 32, 48)), "same": ((3, 16, 16), (3, 16, 16)),
         "mid": ((61, 120, 130), (60, 64, 64))}
WORKLOAD = ((61, 496, 512), (60, 256, 256))
FLIPS = [(False, False), (True, False), (False, True), (True, True)]


def _volume(shape, dtype, seed):
    """[1, D, H, W], non-negative, thresholded, with empty slabs at the low d, low h and high w faces."""
    x = torch.rand(1, *shape, generator=torch.Generator().manual_seed(seed))
    x[x < 0.05] = 0
    x[:, :1] = 0
    x[:, :, :3] = 0
    x[:, :, :, -4:] = 0
    return (x * 255).to(torch.uint8) if dtype == torch.uint8 else x


@lru_cache(maxsize=None)
def volume(case, dt):
    shape = WORKLOAD[0] if case == "workload" else CASES[case][0]
    return _volume(shape, DTYPES[dt], seed=100 + len(case) + 7 * sum(shape))


@lru_cache(maxsize=None)
def ref_pre(case, dt, crop):
    """The restatement before flips and normalisation; computed once per input and shared (never modified)."""
    size = WORKLOAD[1] if case == "workload" else CASES[case][1]
    return R.resize(volume(case, dt), size, crop=crop)


def _maxabs(x):
    return float(x.float().abs().max())


# ---- the box ---------------------------------------------------------------------------------------------------------------------
def _box_inputs(dt):
    shape = (7, 37, 45)
    g = torch.Generator().manual_seed(5)
    base = torch.rand(1, *shape, generator=g)
    base[base < 0.05] = 0
    faces = base.clone()
    faces[0, 0, 0, 0] = 1.0
    faces[0, -1, -1, -1] = 1.0
    inside = base.clone()
    inside[:, :2] = 0; inside[:, -1:] = 0; inside[:, :, :5] = 0; inside[:, :, -3:] = 0; inside[:, :, :, :17] = 0; inside[:, :, :, -2:] = 0
    single = torch.zeros(1, *shape)
    single[0, 3, 17, 29] = 1.0
    last = torch.zeros(1, *shape)
    last[0, 6, 36, 44] = 1.0
    out = {"faces": faces, "inside": inside, "single": single, "last_voxel": last, "empty": torch.zeros(1, *shape)}
    if dt == "u8":
        return {k: (v * 255).to(torch.uint8) for k, v in out.items()}
    neg = -torch.rand(1, *shape, generator=g) - 0.1          # negative everywhere, positive only in an inner block
    neg[:, 2:5, 7:30, 11:40] = inside[:, 2:5, 7:30, 11:40]
    out["negative_background"] = neg
    out["all_negative"] = -torch.rand(1, *shape, generator=g) - 0.1
    return out


@pytest.mark.parametrize("dt", ["u8", "f32"])
def test_box_is_bit_exact(dt):
    for name, x in _box_inputs(dt).items():
        want = list(R.box(x))
        if name in ("empty", "all_negative"):
            assert want == [0, 7, 0, 37, 0, 45]
        got = ops.volume_box(x[0].cuda()).cpu().tolist()
        assert got == want, (dt, name, got, want)
        # a view into a larger allocation: the volume starts at an address that is no multiple of 16 bytes
        pad = torch.zeros(x.numel() + 3, dtype=x.dtype, device="cuda")
        pad[3:] = x.flatten().cuda()
        got = ops.volume_box(pad[3:].view(x.shape[1:])).cpu().tolist()
        assert got == want, (dt, name, "unaligned", got, want)


@pytest.mark.parametrize("dt", ["u8", "f32"])
@pytest.mark.parametrize("shape", [(1025, 513, 4), (17, 513, 1024)], ids=["narrow", "wide"])
def test_box_rows_past_the_grid_cap(shape, dt):
    """box_reduce_kernel: at most 2048 workgroups, each 4 waves x (64 >> lg) rows per pass, lg = log2 of the 16-byte chunks of a row
    (capped at 6).  Narrow rows (one chunk: 256 rows per workgroup, 524 288 per pass) of a 1025 x 513 stack and wide rows (64 chunks or
    more: 4 rows per workgroup, 8192 per pass) of a 17 x 513 one leave rows for a second pass that ends inside a workgroup.  The only
    voxels above zero are one early one and one in a row of the second pass: a pass that is dropped moves the box."""
    D, H, W = shape
    rows_per_pass = 2048 * 4 * (64 if W * (1 if dt == "u8" else 4) <= 16 else 1)
    assert W * (1 if dt == "u8" else 4) <= 16 or W * (1 if dt == "u8" else 4) >= 1024
    assert rows_per_pass < D * H < 2 * rows_per_pass and (D * H - rows_per_pass) % 4 != 0
    x = torch.zeros(1, D, H, W, dtype=DTYPES[dt])
    if dt == "f32":
        x -= 1.0                                                # a negative background is not foreground
    x[0, 1, 7, 1] = 1
    x[0, D - 1, H - 2, W - 2] = 3
    assert ((D - 1) * H + H - 2) >= rows_per_pass
    want = list(R.box(x))
    assert want == [1, D, 7, H - 1, 1, W - 1]
    assert ops.volume_box(x[0].cuda()).cpu().tolist() == want


# ---- the resample ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flips", FLIPS, ids=lambda f: f"flip{int(f[0])}{int(f[1])}")
@pytest.mark.parametrize("crop", [False, True], ids=["whole", "box"])
@pytest.mark.parametrize("dt", ["u8", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_resample_matches_the_restatement(case, dt, crop, flips):
    x = volume(case, dt)
    size = CASES[case][1]
    vol = x[0].cuda()
    box = ops.volume_box(vol) if crop else None
    if crop:
        assert box.cpu().tolist() == list(R.box(x))
    out = ops.volume_resample(vol, size, box=box, flip_d=flips[0], flip_w=flips[1])
    assert out.shape == tuple(size) and out.dtype == torch.float32
    ref = R.flip(ref_pre(case, dt, crop), flips)[0]
    err = float((out.cpu() - ref).abs().max()) / _maxabs(x)
    print(f"resample {case}/{dt}/{'box' if crop else 'whole'}/{flips}: max|out - ref| / max|x| = {err:.3e}")
    parity(f"transform3d/resample/{case}/{dt}/{'box' if crop else 'whole'}/flip{int(flips[0])}{int(flips[1])}", err, BOUND)
    if case == "same" and not crop:
        assert torch.equal(R.flip(out[None].cpu(), flips)[0], x[0].float())     # flipped back: the input, bit for bit


def test_resample_at_the_workload_size():
    x = volume("workload", "u8")
    vol = x[0].cuda()
    box = ops.volume_box(vol)
    assert box.cpu().tolist() == list(R.box(x)) == [1, 61, 3, 496, 0, 508]
    out = ops.volume_resample(vol, WORKLOAD[1], box=box, flip_d=True, flip_w=True)
    ref = R.flip(ref_pre("workload", "u8", True), (True, True))[0]
    err = float((out.cpu() - ref).abs().max()) / _maxabs(x)
    print(f"resample workload/u8/box/(1,1): max|out - ref| / max|x| = {err:.3e}")
    parity("transform3d/resample/workload/u8/box/flip11", err, BOUND)


@pytest.mark.parametrize("crop", [False, True], ids=["whole", "box"])
@pytest.mark.parametrize("dt", ["u8", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_normalised_output(case, dt, crop):
    x = volume(case, dt)
    size = CASES[case][1]
    flips = (crop, not crop)
    vol = x[0].cuda()
    out = ops.volume_resample(vol, size, box=ops.volume_box(vol) if crop else None, flip_d=flips[0], flip_w=flips[1],
                              normalize=(0.25, 0.25)).cpu()
    pre = R.flip(ref_pre(case, dt, crop), flips)[0]
    ref = R.normalize(pre, 0.25, 0.25)
    mx = _maxabs(x)
    both_zero = (ref == 0) & (out == 0)
    mismatch = ((pre == 0) ^ (out == 0)) & ~both_zero
    n_mis = int(mismatch.sum())
    print(f"normalised {case}/{dt}/{'box' if crop else 'whole'}: mismatch set {n_mis} of {out.numel()} voxels; "
          f"exact zeros in the restatement {int((pre == 0).sum())}")
    assert n_mis <= 1e-3 * out.numel()
    if n_mis:
        assert float(pre[mismatch].max()) < 1e-6 * mx
    err = float((out - ref).abs()[~mismatch].max()) / mx
    print(f"normalised {case}/{dt}/{'box' if crop else 'whole'}: max|out - ref| / max|x| = {err:.3e}")
    parity(f"transform3d/normalised/{case}/{dt}/{'box' if crop else 'whole'}", err, 4 * BOUND)


def test_resample_writes_into_a_slice_of_a_batch_tensor():
    x = volume("down", "f32")
    batch = torch.full((3, 1, 6, 32, 32), -7.0, device="cuda")
    ops.volume_resample(x[0].cuda(), (6, 32, 32), out=batch[1, 0])
    assert torch.equal(batch[1, 0], ops.volume_resample(x[0].cuda(), (6, 32, 32)))
    assert bool((batch[0] == -7).all()) and bool((batch[2] == -7).all())
    # an output row length that is no multiple of 4, at an address that is no multiple of 16 bytes
    flat = torch.full((1 + 6 * 9 * 7 + 1,), -7.0, device="cuda")
    out = ops.volume_resample(x[0].cuda(), (6, 9, 7), out=flat[1:-1].view(6, 9, 7))
    ref = R.resize(x, (6, 9, 7))[0]
    parity("transform3d/resample/odd_output_row", float((out.cpu() - ref).abs().max()) / _maxabs(x), BOUND)
    assert float(flat[0]) == -7 and float(flat[-1]) == -7
    with pytest.raises(RuntimeError):
        ops.volume_resample(x[0].cuda(), (6, 32, 32), out=batch[:, 0, 0])            # not contiguous, wrong shape
    with pytest.raises(RuntimeError):
        ops.volume_resample(x[0].cuda().double(), (6, 32, 32))


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def _transforms(**kw):
    return create_3d_transforms((32, 32), num_frames=6, **kw)


def test_create_3d_transforms_sizes():
    train, val = create_3d_transforms(256, num_frames=60)
    assert train.size == (60, 256, 256) and val.size == (60, 256, 256)
    x = volume("down", "u8")
    y = val({"pixel_values": x, "label": 3})
    assert y["label"] == 3 and y["pixel_values"].shape == (1, 60, 256, 256)
    ref = R.resize(x, (60, 256, 256))
    parity("transform3d/val/256", float((y["pixel_values"].cpu() - ref).abs().max()) / _maxabs(x), BOUND)


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalised"])
def test_train_transform_replayed_through_the_restatement(normalize):
    x = volume("down", "f32")
    train, val = _transforms(normalize=normalize, generator=torch.Generator().manual_seed(21))
    seen = set()
    for _ in range(6):
        y = train({"pixel_values": x})["pixel_values"]
        assert y.shape == (1, 6, 32, 32) and y.dtype == torch.float32 and y.is_cuda and not y.requires_grad
        seen.add(train.last_flips)
        ref = R.pipeline(x, (6, 32, 32), crop=True, flips=train.last_flips, norm=(0.25, 0.25) if normalize else None)
        err = float((y.cpu() - ref).abs().max()) / _maxabs(x)
        parity(f"transform3d/train/{'normalised' if normalize else 'plain'}/flip{int(train.last_flips[0])}{int(train.last_flips[1])}", err,
               (4 if normalize else 1) * BOUND)
    assert len(seen) > 1                                          # seed 21 draws more than one combination in six calls
    y = val({"pixel_values": x})["pixel_values"]
    assert val.last_flips == (False, False)
    ref = R.pipeline(x, (6, 32, 32), norm=(0.25, 0.25) if normalize else None)
    parity(f"transform3d/val/{'normalised' if normalize else 'plain'}", float((y.cpu() - ref).abs().max()) / _maxabs(x),
           (4 if normalize else 1) * BOUND)


def test_flip_decisions_seeded_and_forced():
    x = volume("down", "u8")
    a, _ = _transforms(generator=torch.Generator().manual_seed(9))
    b, _ = _transforms(generator=torch.Generator().manual_seed(9))
    for _ in range(4):
        ya, yb = a({"pixel_values": x})["pixel_values"], b({"pixel_values": x})["pixel_values"]
        assert a.last_flips == b.last_flips and torch.equal(ya, yb)
    never, _ = _transforms(RandFlipd_prob=0.0)
    always, _ = _transforms(RandFlipd_prob=1.0)
    y0, y1 = never({"pixel_values": x})["pixel_values"], always({"pixel_values": x})["pixel_values"]
    assert never.last_flips == (False, False) and always.last_flips == (True, True)
    assert torch.equal(y1, y0.flip(1).flip(3))                    # the flips are an index reversal of the same values


def test_batch_equals_the_single_calls():
    vols = [volume("down", "u8"), volume("up", "f32"), volume("mid", "u8"), volume("same", "f32").double()]
    a, _ = _transforms(normalize=True, generator=torch.Generator().manual_seed(4))
    b, _ = _transforms(normalize=True, generator=torch.Generator().manual_seed(4))
    out = a.batch(vols)
    assert out.shape == (4, 1, 6, 32, 32) and out.dtype == torch.float32 and out.is_cuda
    for i, v in enumerate(vols):
        y = b({"pixel_values": v})["pixel_values"]
        assert a.last_flips[i] == b.last_flips
        assert torch.equal(out[i], y), i


def test_cpu_and_gpu_input_autocast_and_channel_check():
    x = volume("down", "u8")
    train, val = _transforms(RandFlipd_prob=1.0, normalize=True)
    for t in (train, val):
        y_cpu = t({"pixel_values": x})["pixel_values"]
        y_gpu = t({"pixel_values": x.cuda()})["pixel_values"]
        with torch.cuda.amp.autocast():
            y_ac = t({"pixel_values": x.cuda()})["pixel_values"]
        assert y_cpu.is_cuda and y_cpu.dtype == torch.float32 and y_ac.dtype == torch.float32
        assert torch.equal(y_cpu, y_gpu) and torch.equal(y_ac, y_gpu)
        assert not y_gpu.requires_grad
        # other dtypes go through .float(): the same values, the same result
        assert torch.equal(t({"pixel_values": x.to(torch.int16)})["pixel_values"], t({"pixel_values": x.float()})["pixel_values"])
        with pytest.raises(ValueError):
            t({"pixel_values": torch.cat([x, x]).cuda()})


def test_process_dicom_array_into_a_model(monkeypatch):
    arr = volume("down", "u8")[0].numpy()
    assert arr.dtype == np.uint8 and arr.shape == (7, 37, 45)
    _, val = _transforms()
    t, shape = I.process_dicom_array(arr, val)
    assert tuple(shape) == (1, 6, 32, 32) and t.shape == (1, 6, 32, 32) and t.is_cuda and t.dtype == torch.float32
    ref = R.resize(torch.from_numpy(arr)[None], (6, 32, 32))
    parity("transform3d/process_dicom_array", float((t.cpu() - ref).abs().max()) / 255.0, BOUND)
    monkeypatch.setattr(models_vit_st, "vit_tiny_test", lambda **kw: models_vit_st.VisionTransformer(
        patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw), raising=False)
    args = argparse.Namespace(model_type="3D_st_flash_attn", model="vit_tiny_test", num_frames=6, t_patch_size=3, input_size=32,
                              nb_classes=8, drop_path=0.0, global_pool=True, sep_pos_embed=True, cls_embed=True, ckpt=None)
    model = I.create_models(args).eval()
    with torch.no_grad():
        logits = model(torch.stack([t, t]))
    assert logits.shape == (2, 8) and bool(torch.isfinite(logits).all())
