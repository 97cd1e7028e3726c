"""Float64 reference and per-element error bounds for the slab LayerNorm (csrc/slabnorm.hip, ops.slab_norm_fwd / _bwd).  A helper, not
a test module and not a conftest: tests/test_cpu_slabnorm.py proves on the CPU what the bounds see, tests/test_gpu_slabnorm_kernels.py
applies them to the kernels.

The reference is stated in the REFERENCE's own order of operations (OCTCube/models_vit_st_flash_attn_slivit.py:245-249 and
models_slivit_head.py:37-38): drop the prefix tokens, view [N, T, L, C], ``transpose(2, 3)``, einops' ``'b c (h p1) (w p2) -> b (c h w)
(p1 p2)'`` with p1 = C, p2 = L, ``layer_norm`` over the C L columns; the backward is autograd through exactly that, in float64.

Bounds, derived from the arithmetic and never from what a kernel was seen to give.  u = 2^-24 (fp32 round to nearest), gamma_n =
n u / (1 - n u): n fp32 additions in ANY order are off by at most gamma_n * sum |terms| (Higham, Accuracy and Stability, section 3.1).
U16: tests/gemm_elem.LP_U, the largest relative error of one rounding into the 16-bit operand type is 2 U16.

  mean     dm  = gamma_K mean|x| + u |mean|                        (a sum of K terms, one rounding of the stored value)
  variance dv  = dm^2 + gamma_{K+4} (var + dm^2)                   (deviations from a mean that is off by dm: + dm^2 exactly; each
                                                                    deviation and square rounded, K terms summed in any order)
  rstd     ds  = rstd (q / 2 / (1 - q)^1.5 + 2 u), q = dv / (var + eps)   (the derivative of v^-1/2, the remainder bounded for q < 1/2;
                                                                    one rounding of the result, one for the stored value)
  xhat     dxh = dm rstd + |x - mean| ds + 2 u (|x - mean| + dm)(rstd + ds)
  y        dy  = |gamma| dxh + u |y|                               (one fused multiply-add)
  A        dy + 2 U16 (|y| + dy) [+ 2^-25 in half: subnormal spacing]   (ONE rounding to 16 bits)
  backward, on the given dA (its 16-bit rounding is the input, not an error), g = dA gamma rounded once:
  mean(g)     d1 = gamma_{K+2} mean|g|
  mean(g xh)  d2 = gamma_{K+2} mean|g xh| + mean(|g| dxh)
  dS       (ds / rstd) |dS| + (rstd + ds)(d1 + |xh| d2 + dxh |m2| + 4 u (|g| + |m1| + |xh m2|))
  dgamma   gamma_{R+1} (|start| + sum_r |dA xh|) + sum_r |dA| dxh       (R = N T rows added onto the start value in any order)
  dbeta    gamma_{R+1} (|start| + sum_r |dA|)
The backward bounds take the statistics' errors as arguments: a test that hands the kernel the reference's statistics rounded to fp32
passes dm = u |mean|, ds = u rstd."""
import torch

from tests.gemm_elem import LP_U

F64 = torch.float64
U32 = 2.0 ** -24


def gamma_n(n):
    return n * U32 / (1.0 - n * U32)


def patch_rows(x, T, L, n_prefix):
    """[N, n_prefix + T L, C] -> [N, T, C L] in the reference's order, with einops where the reference uses it.  Works on any dtype;
    returns a copy."""
    from einops import rearrange
    N, _, C = x.shape
    e = x[:, n_prefix:, :].reshape(N, T, L, C).transpose(2, 3)
    return rearrange(e, "b c (h p1) (w p2) -> b (c h w) (p1 p2)", p1=C, p2=L)


def forward64(x, gamma, beta, eps, T, L, n_prefix):
    """{'rows': [R, K] the patch matrix, 'mean', 'rstd': [R], 'xh', 'y': [R, K]} in float64, R = N T, K = C L."""
    rows = patch_rows(x.detach().cpu().to(F64), T, L, n_prefix)
    rows = rows.reshape(-1, rows.shape[-1])
    K = rows.shape[1]
    y, mean, rstd = torch.native_layer_norm(rows, (K,), gamma.detach().cpu().to(F64), beta.detach().cpu().to(F64), eps)
    mean, rstd = mean.reshape(-1), rstd.reshape(-1)
    return {"rows": rows, "mean": mean, "rstd": rstd, "xh": (rows - mean[:, None]) * rstd[:, None], "y": y}


def backward64(dA, x, gamma, eps, T, L, n_prefix):
    """autograd in float64 through the reference's order for the gradient dA [R, K] at the LayerNorm's output: {'dx' of x's shape,
    'dgamma', 'dbeta' [K]}"""
    xd = x.detach().cpu().to(F64).requires_grad_(True)
    gd = gamma.detach().cpu().to(F64).requires_grad_(True)
    bd = torch.zeros_like(gd).requires_grad_(True)
    rows = patch_rows(xd, T, L, n_prefix)
    K = rows.shape[-1]
    y = torch.nn.functional.layer_norm(rows, (K,), gd, bd, eps)
    y.backward(dA.detach().cpu().to(F64).reshape(y.shape))
    return {"dx": xd.grad, "dgamma": gd.grad, "dbeta": bd.grad}


def stat_bounds(f, eps):
    """(dm, ds) [R]: the bounds of a computed mean and rstd, f = forward64(...)"""
    rows, mean, rstd = f["rows"], f["mean"], f["rstd"]
    K = rows.shape[1]
    dm = gamma_n(K) * rows.abs().mean(dim=1) + U32 * mean.abs()
    var = (rows - mean[:, None]).pow(2).mean(dim=1)
    dv = dm ** 2 + gamma_n(K + 4) * (var + dm ** 2)
    q = dv / (var + eps)
    ds = torch.where(q < 0.5, rstd * (0.5 * q / (1.0 - q).clamp_min(0.5) ** 1.5 + 2 * U32), torch.full_like(q, float("inf")))
    return dm, ds


def xhat_bound(f, dm, ds):
    dev = (f["rows"] - f["mean"][:, None]).abs()
    rstd = f["rstd"][:, None]
    dm, ds = dm[:, None], ds[:, None]
    return dm * rstd + dev * ds + 2 * U32 * (dev + dm) * (rstd + ds)


def fwd_bounds(f, gamma, eps, lp_dtype):
    """{'mean', 'rstd': [R], 'A': [R, K]} per-element bounds of the forward's outputs"""
    dm, ds = stat_bounds(f, eps)
    dy = gamma.detach().cpu().to(F64).abs()[None, :] * xhat_bound(f, dm, ds) + U32 * f["y"].abs()
    floor = 2.0 ** -25 if lp_dtype == torch.float16 else 0.0
    return {"mean": dm, "rstd": ds, "A": dy + 2 * LP_U[lp_dtype] * (f["y"].abs() + dy) + floor}


def bwd_bounds(f, dA, gamma, dm, ds, x_shape, T, L, n_prefix, start_gamma=None, start_beta=None):
    """{'dx': of x's shape (0 on the prefix rows: they must be exact zeros), 'dgamma', 'dbeta': [K]} for statistics that are off by at
    most dm / ds [R]"""
    d = dA.detach().cpu().to(F64).reshape(f["rows"].shape)
    gm = gamma.detach().cpu().to(F64)[None, :]
    R, K = d.shape
    xh, rstd = f["xh"], f["rstd"][:, None]
    dxh = xhat_bound(f, dm, ds)
    g = d * gm
    m1, m2 = g.mean(dim=1, keepdim=True), (g * xh).mean(dim=1, keepdim=True)
    d1 = gamma_n(K + 2) * g.abs().mean(dim=1, keepdim=True)
    d2 = gamma_n(K + 2) * (g * xh).abs().mean(dim=1, keepdim=True) + (g.abs() * dxh).mean(dim=1, keepdim=True)
    dS = rstd * (g - m1 - xh * m2)
    b = (ds[:, None] / rstd) * dS.abs() + (rstd + ds[:, None]) * (d1 + xh.abs() * d2 + dxh * m2.abs()
                                                                  + 4 * U32 * (g.abs() + m1.abs() + (xh * m2).abs()))
    N, tokens, C = x_shape
    bx = torch.zeros(x_shape, dtype=F64)
    bx[:, n_prefix:, :] = b.reshape(N, T, C, L).transpose(2, 3).reshape(N, T * L, C)          # the inverse of patch_rows
    sg = torch.zeros(K, dtype=F64) if start_gamma is None else start_gamma.detach().cpu().to(F64).abs()
    sb = torch.zeros(K, dtype=F64) if start_beta is None else start_beta.detach().cpu().to(F64).abs()
    tiny = 1e-300                       # worst() wants positive bounds; an all-zero column must be matched exactly
    return {"dx": bx, "dgamma": gamma_n(R + 1) * (sg + (d * xh).abs().sum(0)) + (d.abs() * dxh).sum(0) + tiny,
            "dbeta": gamma_n(R + 1) * (sb + d.abs().sum(0)) + tiny}


def worst(got, ref, bound):
    """max |got - ref| / bound over the elements with a positive bound; where the bound is 0 (the prefix rows of dx) got must EQUAL
    ref, otherwise the result is inf.  A NaN counts as inf."""
    got, ref, bound = (t.detach().cpu().to(F64) for t in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    e = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    e = torch.where(torch.isfinite(e) | (got == ref), e, torch.full_like(e, float("inf")))
    e = torch.where(got == ref, torch.zeros_like(e), e)
    return float(e.max())


def measure(x, gamma, beta, dA, T, L, n_prefix, lp_dtype, got, start_gamma=None, start_beta=None, eps=1e-5):
    """{quantity: worst error / bound} for got = {'mean', 'rstd', 'A', 'dx', 'dgamma', 'dbeta'} (any subset); the backward is judged
    with the statistics' own forward bounds: it ran on computed statistics"""
    f = forward64(x, gamma, beta, eps, T, L, n_prefix)
    fb = fwd_bounds(f, gamma, eps, lp_dtype)
    b = backward64(dA, x, gamma, eps, T, L, n_prefix)
    bb = bwd_bounds(f, dA, gamma, fb["mean"], fb["rstd"], x.shape, T, L, n_prefix, start_gamma, start_beta)
    ref = {"mean": f["mean"], "rstd": f["rstd"], "A": f["y"], "dx": b["dx"],
           "dgamma": b["dgamma"] + (0 if start_gamma is None else start_gamma.double()),
           "dbeta": b["dbeta"] + (0 if start_beta is None else start_beta.double())}
    bound = {**fb, **bb}
    return {k: worst(got[k], ref[k], bound[k]) for k in ref if k in got}


def draw(N, T, L, C, n_prefix, kind="plain", seed=0, lp_dtype=torch.bfloat16):
    """x [N, n_prefix + T L, C], gamma, beta [C L], dA [N T, C L] (already a 16-bit value, widened to fp32).  Slabs are not
    exchangeable: every slice has its own offset and spread, and the prefix tokens are large (statistics that include them are far off).
    kind: 'plain'; 'offset' = 1000 + noise of spread 0.5; 'const' = every slab a constant whose fp32 sums are exact (a small integer
    times a power of two), so that mean = the constant and xhat = 0 exactly whatever the summation order."""
    g = torch.Generator().manual_seed(seed)
    K = C * L
    r = torch.arange(N * T, dtype=torch.float32).view(N, T, 1, 1)
    z = torch.randn(N, T, L, C, generator=g)
    if kind == "plain":
        s = z * (0.5 + 0.37 * (r % 4)) + (0.3 * r - 0.5)
    elif kind == "offset":
        s = 1000.0 + 0.5 * z
    elif kind == "const":
        s = (0.25 * (1 + r % 5)).expand(N, T, L, C).clone()
    else:
        raise ValueError(kind)
    x = torch.empty(N, n_prefix + T * L, C)
    x[:, :n_prefix] = 50.0 + 10.0 * torch.randn(N, n_prefix, C, generator=g)
    x[:, n_prefix:] = s.reshape(N, T * L, C)
    gamma = 1.0 + 0.2 * torch.randn(K, generator=g)
    beta = 0.3 * torch.randn(K, generator=g)
    dA = (torch.randn(N * T, K, generator=g) * (0.5 + (torch.arange(N * T) % 3).float())[:, None]).to(lp_dtype).float()
    return x, gamma, beta, dA
