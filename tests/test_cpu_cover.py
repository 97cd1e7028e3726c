"""CPU side of the full-coverage reconstruction: the mask schedule (models_mae.cover_noise) and its refusals, the fp32 oracle of
tests/cover_ref.py against the float64 one, three planted faults the oracle must catch, the bindings of the two entry points in both
builds of the library and their argument errors (reported before any launch)."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests import cover_ref as CR
from tests import recon_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = ((5120, 0.75), (32, 0.5), (1024, 0.85), (257, 0.75))


@pytest.mark.parametrize("L,ratio", SCHEDULES)
def test_schedule_counts(L, ratio):
    from octcubem_amd.models_mae import cover_noise
    N = 3
    len_keep = int(L * (1 - ratio))
    K = math.ceil(L / len_keep)
    noise = cover_noise(N, L, ratio, generator=torch.Generator().manual_seed(5))
    assert noise.dtype == torch.float32 and tuple(noise.shape) == (K, N, L)
    again = cover_noise(N, L, ratio, generator=torch.Generator().manual_seed(5))
    assert torch.equal(noise, again) and not torch.equal(noise, cover_noise(N, L, ratio, generator=torch.Generator().manual_seed(6)))
    as_int = noise.to(torch.int64)
    assert torch.equal(as_int.to(torch.float32), noise) and torch.equal(as_int.double(), noise.double())     # the fp32 noise is its integer
    for k in range(K):                                                    # every pass: a permutation of 0 .. L - 1 per sample
        assert torch.equal(as_int[k].sort(dim=1).values, torch.arange(L).expand(N, L))
    rank = as_int[0]
    assert not torch.equal(rank[0], rank[1])                              # one draw per sample
    for k in range(K):
        assert torch.equal(as_int[k], torch.remainder(rank - k * len_keep, L))
    mask = CR.schedule_masks(noise, len_keep)
    kept = (mask == 0)
    assert torch.equal(kept.sum(dim=2), torch.full((K, N), len_keep))     # every pass keeps exactly len_keep tokens
    for k in range(K):                                                    # ... those whose rank lies in [k len_keep, (k + 1) len_keep) mod L
        assert torch.equal(kept[k], torch.remainder(rank - k * len_keep, L) < len_keep)
    times_kept = kept.sum(dim=0)
    twice = K * len_keep - L
    assert torch.equal(times_kept, torch.where(rank < twice, 2, 1))       # 2 on exactly the `twice` lowest ranks, 1 elsewhere
    assert int((times_kept == 2).sum()) == N * twice
    assert int((mask != 0).sum(dim=0).min()) >= 1                         # every token is masked at least once
    assert int((mask != 0).sum(dim=0).min()) == (K - 2 if twice else K - 1)


def test_schedule_refusals():
    from octcubem_amd.models_mae import cover_noise
    with pytest.raises(ValueError, match=r"K = 2.*19.*32"):
        cover_noise(1, 32, 0.4)
    with pytest.raises(ValueError, match=r"len_keep = 0.*L = 32"):
        cover_noise(1, 32, 0.99)
    with pytest.raises(ValueError, match=r"len_keep = 32.*L = 32"):
        cover_noise(1, 32, 0.0)
    with pytest.raises(ValueError, match=r"2\^24"):
        cover_noise(1, 1 << 24, 0.75)
    assert cover_noise(1, 32, 0.5).shape[0] == 2                          # K == 2 without a remainder is a schedule


def _case(seed=41, K=4):
    B, T, H, p, u = 2, 6, 16, 4, 3
    imgs, preds, fi = CR.make_case(seed, B, T, H, p, u, T, K)
    from octcubem_amd.models_mae import cover_noise
    L = preds[0].shape[1]
    noise = cover_noise(B, L, 0.75, generator=torch.Generator().manual_seed(seed))
    masks = list(CR.schedule_masks(noise, int(L * 0.25)))
    return imgs, preds, masks, fi, u, p


def test_fp32_oracle_agrees_with_the_float64_one():
    imgs, preds, masks, fi, u, p = _case()
    acc, cnt = CR.accumulate_all(preds, masks)
    acc64, cnt64 = CR.accumulate_all(preds, masks, torch.float64)
    assert torch.equal(cnt, cnt64) and int(cnt.min()) == 3 and int(cnt.max()) == 3
    recon, err, v, terms = CR.finish(acc, cnt, imgs, fi, u, p)
    recon64, raw, tol, err64, err_bound = CR.finish64(acc64, cnt, imgs, fi, u, p, CR.abs_sum(preds, masks))
    near = CR.boundary(raw, tol)
    print(f"voxels on a level boundary: {int(near.sum())} of {near.numel()}; unequal levels {int((recon != recon64).sum())}; "
          f"max err excess {float(((err.double() - err64).abs() / err_bound.clamp(min=1e-300)).max()):.3f}")
    assert int(near.sum()) <= 0.01 * near.numel()
    assert torch.equal(recon[~near], recon64[~near]) and int((recon - recon64).abs().max()) <= 1
    assert bool(((err.double() - err64).abs() <= err_bound).all())
    assert int(recon.min()) < 64 and int(recon.max()) > 192               # the levels are spread, not clipped away
    score, bound = CR.score_and_bound(terms)
    assert bool((bound < 1e-4 * score.abs() + 1e-30).all())              # the order-free bound is tight enough to mean something


def test_oracle_catches_planted_faults():
    imgs, preds, masks, fi, u, p = _case()
    masks = [m.clone() for m in masks]
    k = next(k for k in range(len(masks)) if masks[k][0, 5] != 0)
    masks[k][0, 5] = 0.0                                                  # one token of sample 0 is masked only twice: cnt != K - 1 there
    acc, cnt = CR.accumulate_all(preds, masks)
    recon, err, v, _ = CR.finish(acc, cnt, imgs, fi, u, p)
    K = len(preds)
    # (1) an unmasked token added into the sum
    bad = preds[0].clone() * masks[0].unsqueeze(-1)
    for pr in preds[1:]:
        bad = bad + pr
    assert not torch.equal(bad, acc)
    r1, e1, _, _ = CR.finish(bad, cnt, imgs, fi, u, p)
    assert not torch.equal(r1, recon) and not torch.equal(e1, err)
    # (2) a division by K - 1 (the schedule's count) instead of cnt
    r2, e2, _, _ = CR.finish(acc, torch.full_like(cnt, K - 1), imgs, fi, u, p)
    differs = (r2 != recon).flatten(1).any(dim=1)
    assert differs.tolist() == [True, False] and not torch.equal(e2, err)
    # (3) (py, px) swapped in the un-shuffle
    B, L, PD = v.shape
    swapped = v.reshape(B, L, u, p, p).transpose(3, 4).reshape(B, L, PD)
    r3 = R.untransform_image(R.unpatchify(swapped, 6, 16, 16, p, u)[:, 0])
    assert not torch.equal(r3, recon) and torch.equal(r3.sum(), recon.sum())


def test_bindings_history_and_both_libraries():
    from octcubem_amd import _lib
    names = ("octmae_cover_accumulate", "octmae_cover_finish")
    for name in names:
        assert name in _lib.SIGNATURES and name not in _lib.RESTYPES
    assert len(_lib.SIGNATURES[names[0]]) == 10 and len(_lib.SIGNATURES[names[1]]) == 16
    assert _lib.SIGNATURES[names[0]][1] is ctypes.c_longlong                                     # the 64-bit batch stride
    with open(os.path.join(ROOT, "include", "octmae.h")) as f:
        hdr = f.read()
    history = hdr[:hdr.index("#define OCTMAE_ABI_VERSION")]
    assert all(name in history for name in names) and "csrc/cover.hip" in history
    with open(os.path.join(ROOT, "octcubem_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert "cover.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert re.search(r"^\$\(O\)cover\.o:.*\n.*\n.*-ffp-contract=off", mk, re.M)
    for lib in (_lib.load(), ctypes.CDLL(os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so"))):
        assert all(hasattr(lib, name) for name in names)
        assert lib.octmae_abi_version() == _lib.expected_abi_version() == _lib.CONSTANTS["OCTMAE_ABI_VERSION"]


def test_entry_points_report_argument_errors_without_a_gpu():
    from octcubem_amd import _lib, ops
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    q = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned; never dereferenced: every call below is refused before a launch
    q2 = q + 64

    def acc(pred=q, bs=8 * 768, mask=q, s=q2, c=q, B=2, L=8, PD=768, first=1):
        return lib.octmae_cover_accumulate(pred, bs, mask, s, c, B, L, PD, first, None)

    for null in ("pred", "mask", "s", "c"):
        assert acc(**{null: None}) == -1, null
    for bad in (dict(B=0), dict(L=0, bs=0), dict(PD=0), dict(PD=-4), dict(PD=766, bs=8 * 766)):
        assert acc(**bad) == -1, bad
    assert acc(bs=8 * 768 - 4) == -1 and acc(bs=8 * 768 + 2) == -1 and acc(bs=0) == -1
    assert acc(pred=q + 4) == -1 and acc(s=q2 + 8) == -1 and acc(c=q + 2) == -1 and acc(s=q) == -1
    assert acc(B=1 << 20, L=1 << 11, bs=(1 << 11) * 768) == -2           # 2^31 tokens

    def fin(s=q, c=q, imgs=q, fi=None, recon=q, err=q, score=q, B=2, T=6, H=32, W=32, u=3, p=16, L=8, denorm=0):
        return lib.octmae_cover_finish(s, c, imgs, fi, recon, err, score, B, T, H, W, u, p, L, denorm, None)

    for null in ("s", "c", "imgs", "recon"):
        assert fin(**{null: None}) == -1, null
    for bad in (dict(B=0), dict(T=0), dict(H=-32), dict(W=0), dict(u=0), dict(p=0), dict(L=0)):
        assert fin(**bad) == -1, bad
    assert fin(p=6, H=36, W=36, L=72) == -1 and fin(p=2, u=4, L=512) == -1
    assert fin(H=40) == -1 and fin(W=40) == -1 and fin(L=7) == -1 and fin(L=9) == -1
    assert fin(s=q + 4) == -1 and fin(imgs=q + 8) == -1 and fin(err=q + 4) == -1 and fin(recon=q + 1) == -1 and fin(score=q + 2) == -1
    assert fin(L=12) == -1                                                # 9 predicted frames of a 6-frame volume without frame_idx
    assert fin(denorm=2) == -2 and fin(denorm=-1) == -2
    with pytest.raises(_lib.OctmaeError, match="bad argument"):
        _lib.call("octmae_cover_finish", None, None, None, None, None, None, None, 1, 1, 4, 4, 1, 4, 1, 0, None)
    # no CPU form, and the Python wrappers refuse first, naming the argument
    with pytest.raises(RuntimeError, match="pred"):
        ops.cover_accumulate(torch.zeros(1, 1, 16), torch.zeros(1, 1))
    with pytest.raises(RuntimeError, match="sum"):
        ops.cover_finish(torch.zeros(1, 1, 16), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, 1, 1, 4, 4), None, 1, 4)
