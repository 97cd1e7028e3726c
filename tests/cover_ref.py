"""Torch restatement, on the CPU, of the full-coverage reconstruction (csrc/cover.hip, models_mae.cover_noise / reconstruct_full).

``schedule_masks``   the masks of a noise schedule, from a stable ``torch.argsort`` as the reference's random_masking takes them
``accumulate``       one pass into the sums: the entry point's contract op by op (fp32, or float64 when the sums are float64)
``finish``           the finishing pass op by op in fp32: division, subtraction, product, each a tensor op of its own
``finish64``         the same formulas in float64, with the per-voxel error bounds of the fp32 chain
``g()`` (untransform_image), the un-shuffle and the denorm restatement are tests/recon_ref.py's.  The formulas are exact, so there is no
golden file: the GPU tests compare bit for bit against ``accumulate`` / ``finish``.

Bounds (EPS = 2^-24, the relative error of one fp32 rounding to nearest):
  v     c masked passes: c - 1 additions, each off by at most EPS * S with S = sum_k |pred_k| (every partial sum is below S), and one
        division, off by EPS * |v| <= EPS * S / c.  |v32 - v64| <= EPS * S  (times 1.01 for the second-order terms).
  err   d = v - x adds EPS |d|;  e = d * d adds EPS d^2:  |e32 - e64| <= 2 |d| dd + dd^2 + EPS d^2,  dd = dv + EPS |d|.
  level raw = ((v s) + m) 255: dv s 255 from v, then three roundings of at most EPS (|raw| + 255 m) each.
  score any order of summing PD fp32 terms is within (PD - 1) EPS sum|terms| of the exact sum; the division adds one rounding."""
import torch

from tests import recon_ref as R

EPS = 2.0 ** -24


def schedule_masks(noise, len_keep):
    """noise [K, N, L] -> mask [K, N, L] float32, 1 = removed: ids_shuffle = argsort(noise), ids_restore = argsort(ids_shuffle), the
    first len_keep of the shuffled order are kept (models_mae_joint_res_flash_attn.py:350-366)."""
    K, N, L = noise.shape
    ids_shuffle = torch.argsort(noise.reshape(K * N, L), dim=1, stable=True)
    ids_restore = torch.argsort(ids_shuffle, dim=1, stable=True)
    mask = torch.ones(K * N, L)
    mask[:, :len_keep] = 0
    return torch.gather(mask, 1, ids_restore).reshape(K, N, L)


def accumulate(acc, cnt, pred, mask, first):
    """One pass.  first: a removed token's row is its prediction (a copy), every other row +0.0.  Later: where(mask, sum + pred, sum).
    The arithmetic is that of ``acc``'s dtype on later passes (float64 sums for the float64 chain); ``first`` takes pred's values."""
    m = (mask != 0)
    if first:
        dtype = torch.float32 if acc is None else acc.dtype
        return torch.where(m.unsqueeze(-1), pred.to(dtype), torch.zeros((), dtype=dtype)), m.to(torch.int32)
    return torch.where(m.unsqueeze(-1), acc + pred.to(acc.dtype), acc), cnt + m.to(torch.int32)


def accumulate_all(preds, masks, dtype=torch.float32):
    acc, cnt = accumulate(torch.zeros((), dtype=dtype), None, preds[0], masks[0], True)
    for pred, mask in zip(preds[1:], masks[1:]):
        acc, cnt = accumulate(acc, cnt, pred, mask, False)
    return acc, cnt


def _target(imgs, frame_idx, Tp, u, p):
    return R.patchify(R.select_frames(imgs, frame_idx, Tp), p, u)              # [N, L, PD], the source frames' voxels per token


def finish(acc, cnt, imgs, frame_idx, u, p):
    """fp32, op by op -> recon int32 [N, Tp, H, W], err f32 [N, Tp, H, W], v f32 [N, L, PD] (the input where cnt == 0), and the fp32
    terms [N, L, PD] whose mean is the token score."""
    H, W = imgs.shape[-2:]
    Tp = R.pred_frames(acc, imgs, u, p)
    x = _target(imgs, frame_idx, Tp, u, p)
    seen = (cnt > 0).unsqueeze(-1)
    v = acc / cnt.clamp(min=1).to(torch.float32).unsqueeze(-1)
    d = v - x
    e = d * d
    v = torch.where(seen, v, x)
    e = torch.where(seen, e, torch.zeros(()))
    recon = R.untransform_image(R.unpatchify(v, Tp, H, W, p, u)[:, 0])
    recon = torch.where(torch.isfinite(R.unpatchify(v, Tp, H, W, p, u)[:, 0]), recon, torch.zeros((), dtype=recon.dtype))
    return recon, R.unpatchify(e, Tp, H, W, p, u)[:, 0], v, e


def score_and_bound(terms):
    """float64 mean of the fp32 terms, and the bound any fp32 summation order plus the division's rounding keeps: [N, L] each."""
    PD = terms.shape[-1]
    t = terms.double()
    mean = t.sum(-1) / PD
    return mean, ((PD - 1) * EPS * t.abs().sum(-1) / PD + EPS * mean.abs()) * 1.01 + 1e-45


def finish64(acc64, cnt, imgs, frame_idx, u, p, abs_sum):
    """The same formulas in float64.  ``abs_sum`` [N, L, PD] = sum_k |pred_k| over the passes that removed the token.  Returns
    (recon int32, raw64 before clip / truncation, level_tol, err64, err_bound), volumes [N, Tp, H, W]."""
    H, W = imgs.shape[-2:]
    Tp = R.pred_frames(acc64, imgs, u, p)
    x = _target(imgs.double(), frame_idx, Tp, u, p)
    seen = (cnt > 0).unsqueeze(-1)
    v = acc64 / cnt.clamp(min=1).double().unsqueeze(-1)
    dv = torch.where(seen, 1.01 * EPS * abs_sum.double(), torch.zeros((), dtype=torch.float64))
    d = v - x
    e = torch.where(seen, d * d, torch.zeros((), dtype=torch.float64))
    dd = dv + EPS * d.abs()
    e_bound = torch.where(seen, (2 * d.abs() * dd + dd * dd + EPS * d * d) * 1.01, torch.zeros((), dtype=torch.float64))
    v = torch.where(seen, v, x)
    s = float(torch.tensor(R.IMG_STD, dtype=torch.float32))
    m = float(torch.tensor(R.IMG_MEAN, dtype=torch.float32))
    raw = (v * s + m) * 255
    tol = (dv * s * 255 + 3 * EPS * (raw.abs() + 255 * m)) * 1.01
    un = lambda t: R.unpatchify(t, Tp, H, W, p, u)[:, 0]
    raw, tol = un(raw), un(tol)
    return torch.clip(raw, 0, 255).int(), raw, tol, un(e), un(e_bound)


def boundary(raw, tol):
    """Voxels whose float64 level lies within the fp32 chain's error of an integer: there the truncation may go either way."""
    return (raw - raw.round()).abs() <= tol


def denorm64(v, imgs, frame_idx, u, p):
    """``denorm``: v [N, L, PD] (fp32 means, standardised units) mapped through the target patch's mean and unbiased variance in
    float64 -> (panel 2 int32, raw64, err64, err_bound), volumes [N, Tp, H, W].  The fp32 kernel's value differs from the float64 one
    by at most  |v| dsd + dmu + EPS |v sd + mu|  with  dmu <= PD EPS max|x|  (PD - 1 additions and a division, any order) and
    dsd <= (PD + 6) EPS sd  (per term a subtraction and a fused square-add, PD - 1 additions, a division, the + 1e-6, the square
    root; the error of mu enters the variance only in second order because sum (x - mu) = 0, covered by the 1.01)."""
    H, W = imgs.shape[-2:]
    Tp = R.pred_frames(v, imgs, u, p)
    PD = v.shape[-1]
    pan, raw = R.panels_denorm(v, imgs, torch.ones(v.shape[:2]), frame_idx, u, p)
    x = _target(imgs.double(), frame_idx, Tp, u, p)
    mu, sd = x.mean(-1, keepdim=True), (x.var(-1, keepdim=True) + 1.0e-6) ** 0.5
    vd = v.double() * sd + mu
    dv = (v.double().abs() * (PD + 6) * EPS * sd + PD * EPS * x.abs().amax(-1, keepdim=True) + EPS * vd.abs()) * 1.01
    d = vd - x
    dd = dv + EPS * d.abs()
    un = lambda t: R.unpatchify(t, Tp, H, W, p, u)[:, 0]
    return pan[:, 2], raw, un(d * d), un((2 * d.abs() * dd + dd * dd + EPS * d * d) * 1.01)


# ---------------------------------------------------------------------------------------------- inputs
def make_case(seed, B, T, H, p, u, Tp, K, frame_idx=None):
    """imgs [B, 1, T, H, H] and K predictions [B, L, PD] spread past both clip ends (recon_ref.make_inputs).  The first values of imgs
    and of the FIRST prediction lie on the grey-level edges: a token masked in pass 0 alone is drawn from them.  The later passes carry
    none: the level is affine in v, so the mean of three edge values would sit on an integer level a third of the time, where the
    float64 chain cannot say which way the fp32 truncation must go."""
    imgs, pred0, _ = R.make_inputs(seed, B, T, H, H, p, u, Tp)
    preds = [pred0] + [R.make_inputs(seed + 100 * k, B, T, H, H, p, u, Tp, edges=False)[1] for k in range(1, K)]
    return imgs, preds, frame_idx


def abs_sum(preds, masks):
    out = torch.zeros_like(preds[0])
    for pred, mask in zip(preds, masks):
        out = out + torch.where((mask != 0).unsqueeze(-1), pred.abs(), torch.zeros(()))
    return out
