"""GPU: mixup / cutmix in place by one launch (csrc/mixup.hip through ops.mix_batch and octcubem_amd.mixup.Mixup) against the plain-torch
restatement of timm's three modes with its clone and per-sample loop (tests/mix_ref.py, CPU, float32).

Samples are compared BIT FOR BIT (torch.equal): both sides do one rounded multiply per operand and one add, or a copy, so there is no
tolerance to choose; a fused multiply-add in the kernel would show in the last bit.  Targets, a few float32 ops on values in [0, 1]
done by torch on either device, are compared to 1e-6 absolute: several ulps of 1 (2^-23 = 1.2e-7)."""
import json
import os
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from octcubem_amd import Mixup, ops
from tests import mix_ref as R

DEV = "cuda"
TARGET_ATOL = 1e-6          # several ulps of 1 in float32


def batch(shape, seed):
    """Distinct values everywhere (a misplaced element shows) with full mantissas (a fused multiply-add shows)."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    return (torch.randn(n, generator=g) * 3 + torch.arange(n, dtype=torch.float32) * 1e-3).reshape(shape)


def launch(x, kind, lam32, oml32, box):
    d = x.to(DEV)
    out = ops.mix_batch(d, kind, lam32, oml32, box, x.shape[-2], x.shape[-1])
    assert out is d
    return d.cpu()


def elem_tables(lam, use_cutmix, boxes):
    """The launch tables of per-sample decisions as the elem mode forms them: lam float32, 1 - lam a float32 subtraction."""
    lam = np.asarray(lam, dtype=np.float32)
    cut = np.asarray(use_cutmix, dtype=bool)
    kind = np.where(lam == 1.0, 0, np.where(cut, 2, 1)).astype(np.int32)
    return kind, np.where(kind == 1, lam, np.float32(1)), np.where(kind == 1, np.float32(1) - lam, np.float32(0)), np.asarray(boxes, dtype=np.int32)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 5, 7), (2, 1, 1, 3), (4, 3, 8, 8), (2, 1, 3, 8, 20), (4, 1, 5, 7)])
def test_mixup_is_bit_equal_to_mul_mul_add(shape):
    """S = 35 and S = 3 < 4: partners are an odd number of samples apart, so with S % 4 != 0 they are out of phase against a 16-byte
    line and the pair takes the scalar path, with one pair and with two; S = 192 and 480: 16-byte accesses only (head, body and tail
    in one sample: test_a_view_that_starts_off_a_16_byte_line).  lam: 0, 0.3, one that float32 does not hold, the float32 below 1."""
    x = batch(shape, 1)
    B = shape[0]
    for lam in (0.0, 0.3, 0.7123456789012345, 1.0 - 2.0 ** -24):
        want = R.mix_batch(x.clone(), lam, False)
        got = launch(x, [1] * B, [np.float32(lam)] * B, [np.float32(1.0 - lam)] * B, np.zeros((B, 4)))
        assert torch.equal(got, want), (shape, lam, int((got != want).sum()))
    # the fixture of this test can tell a fused multiply-add from mul + add (computed in double: exact product, one rounding)
    if x[0].numel() >= 192:
        fused = (x.double() * float(np.float32(0.3)) + (x.flip(0) * np.float32(1.0 - 0.3)).double()).float()
        assert int((fused != R.mix_batch(x.clone(), 0.3, False)).sum()) > 0


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 2, 5, 7), (6, 1, 8, 12), (6, 1, 2, 6, 10)])
def test_elem_mode_uses_the_partners_original_values(shape):
    """Pairs (0, 5): 0 untouched, 5 mixes; (1, 4): 1 mixes, 4 cuts; (2, 3): both mix with different lam.  Every output must come from
    the partner's ORIGINAL values although both members of a pair are rewritten by one launch without a copy."""
    H, W = shape[-2:]
    x = batch(shape, 2)
    lam = np.array([1.0, 0.25, 0.8, 0.4567891, 0.5, 0.6], dtype=np.float32)
    cut = [False, False, False, False, True, False]
    boxes = [(0, 0, 0, 0)] * 4 + [(1, H - 1, 1, W - 2)] + [(0, 0, 0, 0)]
    want = R.mix_elem(x.clone(), lam, cut, boxes)
    got = launch(x, *elem_tables(lam, cut, boxes))
    assert torch.equal(got, want)
    assert torch.equal(got[0], x[0]) and not torch.equal(got[5], x[5])
    # sample 4 outside its box is the input, inside it sample 1 as it was
    inside = torch.zeros(shape[1:], dtype=torch.bool)
    inside[..., 1:H - 1, 1:W - 2] = True
    assert torch.equal(got[4][~inside], x[4][~inside]) and torch.equal(got[4][inside], x[1][inside])


def test_samples_longer_than_the_grid_cap():
    """A pair gets ceil(4096 / pairs) workgroups of 256 threads at the most and a thread strides on over its sample's 16-byte lines (the
    full pass) or over the lines of its box rows (the box pass).  Two pairs -> 524 288 threads each; samples of 1450 x 1452 = 2 105 400
    floats are 526 350 lines (2062 on a second trip), the whole-plane box 1450 rows x 364 lines = 527 800 and the box that leaves a rim
    1448 x 363 = 525 624.  Pair (0, 3) mixes both ways, pair (1, 2) cuts both ways with those two boxes."""
    shape = (4, 1, 1450, 1452)
    H, W = shape[-2:]
    threads = 256 * (4096 // 2)
    assert (H * W + 3) // 4 > threads and H * ((W + 3) // 4 + 1) > threads and (H - 2) * ((W - 4 + 3) // 4 + 1) > threads
    x = batch(shape, 9)
    lam = np.array([0.3, 0.5, 0.5, 0.7123456789012345], dtype=np.float32)
    cut = [False, True, True, False]
    boxes = [(0, 0, 0, 0), (0, H, 0, W), (2, H, 1, W - 3), (0, 0, 0, 0)]
    want = R.mix_elem(x.clone(), lam, cut, boxes)
    got = launch(x, *elem_tables(lam, cut, boxes))
    assert torch.equal(got, want), int((got != want).sum())
    assert torch.equal(got[1], x[2]) and not torch.equal(got[2], x[1]) and not torch.equal(got[0], x[0])


def test_elem_mode_two_different_overlapping_boxes_in_one_pair():
    """Both members of a pair cut, each with its own box: where the boxes overlap the two samples swap, elsewhere each takes the other's
    original.  Pair (1, 2): one side cuts, the other is untouched."""
    for shape in [(4, 2, 9, 10), (4, 1, 2, 8, 12)]:
        H, W = shape[-2:]
        x = batch(shape, 3)
        lam = np.array([0.5, 0.5, 1.0, 0.5], dtype=np.float32)
        boxes = [(0, 6, 1, 8), (2, H, 0, W), (0, 0, 0, 0), (3, H, 4, W)]
        want = R.mix_elem(x.clone(), lam, [True] * 4, boxes)
        got = launch(x, *elem_tables(lam, [True] * 4, boxes))
        assert torch.equal(got, want) and torch.equal(got[2], x[2])


# 3 ---------------------------------------------------------------------------------------------------------------------
def cut_boxes(H, W):
    return {"empty_rows": (3, 3, 2, 7), "empty_cols": (2, 6, 5, 5), "whole": (0, H, 0, W), "pixel": (4, 5, 3, 4),
            "odd_xl_odd_width": (1, H - 1, 3, 8), "top": (0, 3, 2, 6), "bottom": (H - 2, H, 1, 5), "left": (2, 5, 0, 3),
            "right": (2, 5, W - 3, W), "corner": (H - 1, H, W - 1, W)}


@pytest.mark.parametrize("shape", [(4, 3, 9, 10), (2, 1, 3, 8, 12)])
def test_cutmix_boxes(shape):
    """W = 10 is no multiple of 4 (the phase of a row segment changes from row to row); the 5-D batch cuts every frame alike."""
    H, W = shape[-2:]
    B = shape[0]
    x = batch(shape, 4)
    for name, box in cut_boxes(H, W).items():
        yl, yh, xl, xh = box
        want = R.mix_batch(x.clone(), 0.5, True, box)
        got = launch(x, [2] * B, [1.0] * B, [0.0] * B, [box] * B)
        assert torch.equal(got, want), name
        inside = torch.zeros(shape, dtype=torch.bool)
        inside[..., yl:yh, xl:xh] = True
        assert int(inside.sum()) == B * (x[0].numel() // (H * W)) * (yh - yl) * (xh - xl)
        assert torch.equal(got[~inside], x[~inside]), name                   # everything outside the box, bit for bit
        assert torch.equal(got[inside], x.flip(0)[inside]), name
    with pytest.raises(ValueError, match="box"):
        ops.mix_batch(x.to(DEV), [2] * B, [1.0] * B, [0.0] * B, [(0, H + 1, 0, W)] * B, H, W)
    with pytest.raises(ValueError):
        ops.mix_batch(x.to(DEV), [2] * B, [1.0] * B, [0.0] * B, [(0, H, 0, W)] * B, H + 1, W)      # H * W does not divide S
    with pytest.raises(ValueError):
        ops.mix_batch(x.to(DEV)[:, :, ::2], [2] * B, [1.0] * B, [0.0] * B, [(0, 1, 0, 1)] * B, H, W)   # not contiguous


def test_a_view_that_starts_off_a_16_byte_line():
    """A contiguous batch whose first element is 4 bytes past a 16-byte line: head, body and tail of every sample and row segment."""
    shape = (4, 2, 6, 12)
    x = batch(shape, 5)
    n = x.numel()
    for kind, lam, box in ((1, 0.3, (0, 0, 0, 0)), (2, 1.0, (1, 5, 2, 11))):
        buf = torch.zeros(n + 8, device=DEV)
        buf[1:n + 1] = x.flatten().to(DEV)
        view = buf[1:n + 1].view(shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        ops.mix_batch(view, [kind] * 4, [np.float32(lam)] * 4, [np.float32(1.0 - lam)] * 4, [box] * 4, 6, 12)
        want = R.mix_batch(x.clone(), lam if kind == 1 else 0.5, kind == 2, box)
        assert torch.equal(view.cpu(), want)
        assert float(buf[0]) == 0.0 and not buf[n + 1:].any()                # nothing written beside the batch


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_pair_mode_swaps_boxes_and_mixes_both_members():
    for shape in [(4, 3, 9, 10), (4, 1, 2, 8, 8)]:
        H, W = shape[-2:]
        x = batch(shape, 6)
        lam, cut, boxes = np.array([0.5, 0.35], dtype=np.float32), [True, False], [(2, 7, 1, 6), (0, 0, 0, 0)]
        want = R.mix_pair(x.clone(), lam, cut, boxes)
        kind, lam32, oml32, box = elem_tables(np.concatenate((lam, lam[::-1])), cut + cut[::-1], boxes + boxes[::-1])
        got = launch(x, kind, lam32, oml32, box)
        assert torch.equal(got, want)
        assert torch.equal(got[0][..., 2:7, 1:6], x[3][..., 2:7, 1:6]) and torch.equal(got[3][..., 2:7, 1:6], x[0][..., 2:7, 1:6])


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_non_finite_values_come_out_as_torch_produces_them():
    shape = (4, 1, 6, 8)
    x = batch(shape, 7)
    nan, inf = float("nan"), float("inf")
    own, partner = x[0].view(-1), x[3].view(-1)          # element e of sample 0 meets element e of sample 3
    own[[3, 7, 11, 13, 14, 20]] = torch.tensor([nan, inf, -inf, inf, inf, nan])
    partner[[3, 13, 14, 15, 20]] = torch.tensor([inf, -inf, inf, nan, nan])          # NaN | inf, inf - inf, inf + inf, x | NaN, NaN | NaN
    x[1].view(-1)[[0, 47]] = torch.tensor([-inf, nan])
    x[2].view(-1)[[1, 47]] = torch.tensor([inf, -inf])
    cases = [([1] * 4, 0.3, (0, 0, 0, 0)), ([1] * 4, 0.0, (0, 0, 0, 0)), ([2] * 4, 1.0, (0, 6, 0, 8)), ([2] * 4, 1.0, (1, 4, 2, 7))]
    for kind, lam, box in cases:
        want = R.mix_batch(x.clone(), lam if kind[0] == 1 else 0.5, kind[0] == 2, box)
        got = launch(x, kind, [np.float32(lam)] * 4, [np.float32(1.0 - lam)] * 4, [box] * 4)
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(torch.nan_to_num(got, nan=0.0, posinf=1e30, neginf=-1e30), torch.nan_to_num(want, nan=0.0, posinf=1e30, neginf=-1e30))
    # lam = 0 turns the partner's infinities into themselves and the own ones into NaN (inf * 0): more NaN than the input had
    assert int(torch.isnan(R.mix_batch(x.clone(), 0.0, False)).sum()) > int(torch.isnan(x).sum())


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["batch", "elem", "pair"])
def test_mixup_call_end_to_end(mode):
    kinds = set()
    for shape in [(6, 3, 9, 10), (6, 1, 3, 8, 12)]:
        m = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, label_smoothing=0.1, num_classes=5, rng=np.random.RandomState(12))
        for call in range(6):
            x = batch(shape, 20 + call)
            t = torch.randint(0, 5, (6,), generator=torch.Generator().manual_seed(call))
            d = x.to(DEV)
            out, y = m(d, t.to(DEV))
            assert out is d and out.data_ptr() == d.data_ptr()                        # in place, the same storage
            p = m.last_params
            kinds |= set(p["kind"].tolist())
            want_x, want_y = R.apply_params(x, t, p, 5, 0.1)
            assert torch.equal(out.cpu(), want_x), (mode, shape, call)
            assert y.shape == (6, 5) and y.dtype == torch.float32 and y.device == d.device
            assert float((y.cpu() - want_y).abs().max()) <= TARGET_ATOL
    assert {1, 2} <= kinds                                                            # the seeded stream mixed and cut
    # a non-contiguous input: equal values, a new tensor, the caller's memory untouched
    wide = batch((6, 3, 9, 20), 40).to(DEV)
    view = wide[..., ::2]
    before = wide.clone()
    m = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, num_classes=5, rng=np.random.RandomState(3))
    t = torch.arange(6) % 5
    out, y = m(view, t.to(DEV))
    want_x, want_y = R.apply_params(view.cpu().contiguous(), t, m.last_params, 5, 0.1)
    assert out.is_contiguous() and torch.equal(out.cpu(), want_x) and torch.equal(wide, before)
    assert float((y.cpu() - want_y).abs().max()) <= TARGET_ATOL
    # a closed gate: no launch, the input comes back as it is
    m = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, prob=0.0, label_smoothing=0.0, num_classes=5, rng=np.random.RandomState(3))
    d = before.clone()
    out, y = m(d, t.to(DEV))
    assert out is d and torch.equal(d, before) and torch.equal(y.cpu(), torch.nn.functional.one_hot(t, 5).float())


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_one_engine_step_with_mixup_fn(golden_dir):
    """engine_finetune.train_one_epoch with mixup_fn=Mixup(...) and SoftTargetCrossEntropy on the first batch of the smallest fine-tune
    fixture: the loss is finite and equals the loss of the same step on samples and targets mixed beforehand by the restatement, within
    the 3e-2 relative that tests/test_gpu_finetune.py allows its per-iteration loss."""
    from oracle import vit_ref as V
    from octcubem_amd import engine_finetune, losses, lr_decay, misc, models_vit_st
    from octcubem_amd import optim as foptim
    z = np.load(os.path.join(golden_dir, "finetune_small.npz"))
    cfg = V.ViTSTConfig(**json.loads(str(z["cfg"])))
    P0 = V.init_from_shapes(V.vit_st_param_shapes(cfg), seed=int(z["param_seed"]))
    xs = torch.rand(6, 2, 1, 12, 64, 64, generator=torch.Generator().manual_seed(int(z["data_seed"])))
    x, t = xs[0], torch.from_numpy(z["target"])[0]
    assert x.shape[0] % 2 == 0 and t.shape == (x.shape[0],)

    class A:
        accum_iter = 1; lr = 2e-4; min_lr = 1e-6; warmup_epochs = 1; epochs = 4; task_mode = "binary_cls"

    def step(loader, mixup_fn):
        m = models_vit_st.VisionTransformer(num_frames=cfg.num_frames, t_patch_size=cfg.t_patch_size, img_size=cfg.img_size,
                                            patch_size=cfg.patch_size, in_chans=cfg.in_chans, num_classes=cfg.num_classes,
                                            embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4,
                                            norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), sep_pos_embed=True, cls_embed=True,
                                            global_pool=True, drop_path_rate=0.0, dropout=0.0)
        m.load_state_dict(P0, strict=True)
        m = m.to(DEV)
        opt = foptim.FusedAdamW(lr_decay.param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75), lr=A.lr)
        crit, seen = losses.SoftTargetCrossEntropy(), []

        def rec(o, tt):
            l = crit(o, tt)
            seen.append(float(l.detach()))
            return l
        stats = engine_finetune.train_one_epoch(m, rec, loader, opt, torch.device(DEV), 0, misc.NativeScalerWithGradNormCount(), 1.0,
                                                mixup_fn, None, A)
        assert stats is not None and len(seen) == 1
        return seen[0]

    fn = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", label_smoothing=0.1, num_classes=cfg.num_classes, rng=np.random.RandomState(8))
    loss = step([(x.clone(), t)], fn)
    p = fn.last_params
    assert p["kind"].any() and np.isfinite(loss)
    want_x, want_y = R.apply_params(x, t, p, cfg.num_classes, 0.1)
    assert not torch.equal(want_x, x)
    ref = step([(want_x, want_y)], None)
    print(f"engine step: loss with mixup_fn {loss:.7f}, with samples mixed beforehand {ref:.7f}")
    assert abs(loss - ref) <= 3e-2 * abs(ref)


# 8 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_autocast_changes_nothing(mode):
    x = batch((4, 3, 9, 10), 9)
    t = torch.tensor([0, 2, 1, 4])
    outs = []
    for inside in (False, True):
        m = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, num_classes=5, rng=np.random.RandomState(31))
        for _ in range(3):                                            # three calls: the stream mixes and cuts
            d = x.to(DEV)
            if inside:
                with torch.cuda.amp.autocast():
                    out, y = m(d, t.to(DEV))
            else:
                out, y = m(d, t.to(DEV))
            assert out.dtype == torch.float32 and y.dtype == torch.float32
            outs.append((out.cpu(), y.cpu()))
    for (a, ya), (b, yb) in zip(outs[:3], outs[3:]):
        assert torch.equal(a, b) and torch.equal(ya, yb)
