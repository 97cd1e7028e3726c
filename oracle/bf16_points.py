"""TEST INFRASTRUCTURE (see oracle/__init__): a CPU model of ONE pre-norm transformer Block -- forward and backward of
Pre-training/custom_util/video_vit.py:141-184 (Block), :86-138 (Attention), timm Mlp -- evaluated in float64 with a bfloat16
rounding inserted at exactly the points where the HIP path (octcubem_amd.ops.BlockFn -> csrc/*.hip) rounds:

  forward   y1 = bf(LN1 x) ; qkv = bf(y1 Wqkv^T + b) ; attention with q * scale*log2e rounded to bf16, P rounded to bf16 for the
            P V product only (the row sum uses the unrounded P), o = bf(O / l) ; x2 = x + o Wp^T + b (fp32) ;
            y2 = bf(LN2 x2) ; pre = bf(y2 W1^T + b1) ; act = bf(gelu(pre)) ; x3 = x2 + act W2^T + b2 (fp32)
  backward  every gradient entering a GEMM is bf16 (d3b, dpre, dy2, dx2b, do, dqkv, dy1); dpre = bf(bf(d3b W2) * gelu'(pre));
            attention: P and dS rounded to bf16 for their products, K * scale*log2e rounded to bf16 in the kernels that keep the
            key on the lane (fused backward, dK/dV kernel), Q * scale*log2e in the dQ kernel of the two-kernel form;
            LayerNorm backward, residual adds, bias / weight gradients in fp32.
  weights   the MFMA operands are the bf16 mirror of the fp32 master weights.

GELU is the fc1 epilogue's polynomial (exact_gelu=False; |Phi error| <= 1.72e-5 absolute, far below the bf16 resolution of the stored
activation; the test prices what it costs against the erf form).  GELU' is the erf form itself: since round 3 the fc2-dgrad
epilogue evaluates it to 3e-7 (csrc/common.hpp dgelu_exact_f; the degree-19 polynomial it replaced, |error| 4.4e-4, is kept
here as dgelu_poly only to show what it used to cost).  What remains between this model and the HIP result is accumulation order
(fp32 vs float64), the hardware exp2, and rare rounding flips of values that land within 1e-7 of a bf16 tie.  The GPU test
(tests/test_gpu_rounding_model.py) requires <= 1e-3 relative for every output, which separates "bf16 operand rounding" from
"kernel arithmetic error": the plain fp32 oracle differs from both by the 2^-9-per-operation rounding the north star's 1e-3
bound cannot absorb element-wise (loss-level quantities do meet 1e-3, see tests/test_gpu_fullsize_pins.py).
"""
from __future__ import annotations

import math
from typing import Dict

import torch

D = torch.float64
LOG2E = 1.4426950408889634


# Every rounding of this model goes through bf() / f32() below, and the GELU choice through _EXACT: with exact_arithmetic() active
# both are the identity and the erf form is used, so the SAME code evaluates the reference's mathematics in plain float64 --
# that is how tests/test_oracle_rounding_model.py pins the model (its hand-written backward formulas included) to the fp64
# autograd of oracle/mae3d_ref.py, which is itself pinned to the reference's golden vectors.
_EXACT = False
# The 16-bit type the rounding points round to: bfloat16 (the shipped library) or float16 (`with operand_type(torch.float16)`: the
# model of the half verification build, liboctmae_f16.so -- same rounding points, 3 more mantissa bits).
LP_DTYPE = torch.bfloat16


class operand_type:
    """Context manager: the 16-bit type of every rounding point (torch.bfloat16 | torch.float16)."""

    def __init__(self, dtype):
        assert dtype in (torch.bfloat16, torch.float16)
        self.dtype = dtype

    def __enter__(self):
        global LP_DTYPE
        self.prev, LP_DTYPE = LP_DTYPE, self.dtype
        return self

    def __exit__(self, *a):
        global LP_DTYPE
        LP_DTYPE = self.prev


LP_BITS = None      # not None: round to this many significant bits with an UNBOUNDED exponent instead of to LP_DTYPE


class operand_bits:
    """Context manager: every rounding point keeps `bits` significant bits (8 = bfloat16's, 11 = half's) and any exponent -- the
    arithmetic of the half build under loss scaling (nothing underflows), and the tool that shows how each quantity's error scales
    with the operand epsilon (tests/test_oracle_rounding_model.py)."""

    def __init__(self, bits: int):
        self.bits = int(bits)

    def __enter__(self):
        global LP_BITS
        self.prev, LP_BITS = LP_BITS, self.bits
        return self

    def __exit__(self, *a):
        global LP_BITS
        LP_BITS = self.prev


class exact_arithmetic:
    """Context manager: switch every rounding point off (bf / f32 become the identity, GELU is the erf form)."""

    def __enter__(self):
        global _EXACT
        self.prev, _EXACT = _EXACT, True
        return self

    def __exit__(self, *a):
        global _EXACT
        _EXACT = self.prev


def bf(x: torch.Tensor) -> torch.Tensor:
    """Round to bfloat16 (nearest even) and return as float64."""
    if _EXACT:
        return x.to(D)
    if LP_BITS is not None:
        m, e = torch.frexp(x.to(torch.float32).to(D))
        return torch.ldexp(torch.round(m * 2.0 ** LP_BITS) / 2.0 ** LP_BITS, e)
    return x.to(torch.float32).to(LP_DTYPE).to(D)


def f32(x: torch.Tensor) -> torch.Tensor:
    """Round to float32 and return as float64 (values the kernels form or store in fp32: scale*log2e, LSE, delta)."""
    return x.to(D) if _EXACT else x.to(torch.float32).to(D)


def ln_fwd(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mu) * rstd
    return xhat * g + b, xhat, rstd


def ln_bwd(dy, xhat, rstd, g):
    gy = dy * g
    dx = rstd * (gy - gy.mean(-1, keepdim=True) - xhat * (gy * xhat).mean(-1, keepdim=True))
    return dx, (dy * xhat).reshape(-1, dy.shape[-1]).sum(0), dy.reshape(-1, dy.shape[-1]).sum(0)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_poly(x):
    """The GEMM epilogue's GELU (csrc/common.hpp gelu_f): x * (0.5 + u P(u^2)), u = clamp(x, +-4.2), |Phi error| <= 1.72e-5."""
    u = x.clamp(-4.2, 4.2)
    t = u * u
    p = torch.full_like(x, -2.306640613e-12)
    for c in (2.495095069e-10, -1.216585654e-08, 3.568801260e-07, -7.116507187e-06, 1.035454878e-04, -1.148414365e-03,
              9.898752642e-03, -6.641823237e-02, 3.989180135e-01):
        p = p * t + c
    return x * (u * p + 0.5)


def dgelu_poly(x):
    """The fc2-dgrad epilogue's GELU' UNTIL round 3 (csrc/common.hpp dgelu_poly_f): 0.5 + u Q(u^2), u = clamp(x, +-5),
    |error| <= 4.4e-4.  Not used by the model below any more (poly_dgelu=True brings it back for comparisons)."""
    u = x.clamp(-5.0, 5.0)
    t = u * u
    q = torch.full_like(x, -8.945184002e-12)
    for c in (1.221804868e-09, -7.286091231e-08, 2.499930865e-06, -5.482182127e-05, 8.080908045e-04, -8.191250186e-03,
              5.702680522e-02, -2.631234724e-01, 7.970332990e-01):
        q = q * t + c
    return u * q + 0.5


def scale_log2e(scale: float) -> torch.Tensor:
    """scale*log2e as the kernels form it: an fp32 product (of two fp32 values: exact in float64, then rounded once)."""
    return f32(f32(torch.tensor(scale, dtype=D)) * f32(torch.tensor(LOG2E, dtype=D)))


def attention_forward(q, k, v, sc2):
    """The attention part of block_forward: q, k, v [B, H, N, hd] float64 holding 16-bit values, sc2 = scale_log2e(scale).
    Returns (o rounded to 16 bits, lse rounded to fp32 [B, H, N], qs = the pre-scaled rounded query the pair's dQ kernel reuses)."""
    qs = bf(f32(q * sc2))                                                   # fp32 product, then bf16, as scale_frag does
    S2 = qs @ k.transpose(-1, -2)                                           # exp2-domain scores
    Pm = torch.exp2(S2)                                                     # optimistic forward: no running max
    l = Pm.sum(-1, keepdim=True)
    o = bf((bf(Pm) @ v) / l)                                                # [B, H, N, hd]
    lse = torch.log2(l.squeeze(-1)) * math.log(2.0)                         # natural log, as the kernel stores it
    lse = f32(lse)
    return o, lse, qs


def attention_backward(q, k, v, qs, o, lse, do, scale, sc2, both_dq: bool = True):
    """The attention part of block_backward: do [B, H, N, hd] 16-bit values in float64.  Returns (dQ of the fused form, dQ of the
    two-kernel pair -- None unless both_dq --, dK, dV), all BEFORE their rounding to 16 bits."""
    delta = f32((do * o).sum(-1, keepdim=True))
    nl = f32(-(lse * f32(torch.tensor(LOG2E, dtype=D)))).unsqueeze(-1)      # -lse*log2e (fp32 product)
    ks = bf(f32(k * sc2))
    Pk = torch.exp2(q @ ks.transpose(-1, -2) + nl)                          # key-on-the-lane kernels: K pre-scaled
    dPk = do @ v.transpose(-1, -2) - delta
    dSk = Pk * dPk
    dV = bf(Pk).transpose(-1, -2) @ do
    dK = scale * (bf(dSk).transpose(-1, -2) @ q)
    dQf = scale * (bf(dSk) @ k)
    dQp = None
    if both_dq:                                                             # the dQ kernel of the pair pre-scales Q
        Pq = torch.exp2(qs @ k.transpose(-1, -2) + nl)
        dQp = scale * (bf(Pq * dPk) @ k)
    return dQf, dQp, dK, dV


def attention_forward_backward(q, k, v, do, scale: float, o=None, lse=None):
    """The attention kernels alone, as the model above evaluates them: q, k, v, do [B, H, N, hd] holding 16-bit values.
    Returns a dict of float64 tensors: o, dq_fused, dq_pair, dk, dv (rounded to 16 bits, as the kernels store them) and lse (fp32).
    o [B, H, N, hd], lse [B, H, N] (both or neither): the forward results the backward is fed INSTEAD of the model's own -- a backward
    kernel under test reads the o and lse its caller hands it (delta = rowsum(dO * o) moves a whole row of dS), so its model must too.
    Evaluated one (b, h) slice at a time: the [N, N] intermediates of one slice are all that is ever alive."""
    q, k, v, do = (t.to(D) for t in (q, k, v, do))
    sc2 = scale_log2e(scale)
    assert (o is None) == (lse is None)
    B, H = q.shape[:2]
    out = {n: [] for n in ("o", "lse", "dq_fused", "dq_pair", "dk", "dv")}
    for i in range(B * H):
        qi, ki, vi, di = (t.reshape(B * H, 1, *t.shape[2:])[i:i + 1] for t in (q, k, v, do))
        o_m, lse_m, qs = attention_forward(qi, ki, vi, sc2)
        o_b, lse_b = (o_m, lse_m) if o is None else (o.to(D).reshape(B * H, 1, *o.shape[2:])[i:i + 1], lse.to(D).reshape(B * H, 1, -1)[i:i + 1])
        dQf, dQp, dK, dV = attention_backward(qi, ki, vi, qs, o_b, lse_b, di, scale, sc2)
        for n, t in zip(out, (o_m, lse_m, bf(dQf), bf(dQp), bf(dK), bf(dV))):
            out[n].append(t)
    return {n: torch.cat(ts, 0).reshape(B, H, *ts[0].shape[2:]) for n, ts in out.items()}


def block_forward(P: Dict[str, torch.Tensor], x: torch.Tensor, num_heads: int, eps: float = 1e-6, exact_gelu: bool = False):
    """Forward of one Block with the HIP path's roundings.  P: the Block's parameters by their reference names
    (norm1.weight, attn.q.weight, ..., mlp.fc2.bias); x [B, N, C].  Returns (x3 float64, saved) -- `saved` is what
    block_backward needs."""
    B, N, C = x.shape
    H = num_heads
    hd = C // H
    scale = hd ** -0.5
    sc2 = scale_log2e(scale)
    p = {k: v.to(D) for k, v in P.items()}
    x = x.to(D)
    wqkv = bf(torch.cat([p["attn.q.weight"], p["attn.k.weight"], p["attn.v.weight"]], 0))
    bqkv = torch.cat([p["attn.q.bias"], p["attn.k.bias"], p["attn.v.bias"]], 0)
    wp, w1, w2 = bf(p["attn.proj.weight"]), bf(p["mlp.fc1.weight"]), bf(p["mlp.fc2.weight"])
    y1f, xh1, rs1 = ln_fwd(x, p["norm1.weight"], p["norm1.bias"], eps)
    y1 = bf(y1f)
    qkv = bf(y1 @ wqkv.T + bqkv)                                            # [B, N, 3C]
    q, k, v = (t.reshape(B, N, H, hd).transpose(1, 2) for t in qkv.split(C, dim=-1))     # [B, H, N, hd]
    o, lse, qs = attention_forward(q, k, v, sc2)
    o2 = o.transpose(1, 2).reshape(B, N, C)
    x2 = x + o2 @ wp.T + p["attn.proj.bias"]
    y2f, xh2, rs2 = ln_fwd(x2, p["norm2.weight"], p["norm2.bias"], eps)
    y2 = bf(y2f)
    pre = bf(y2 @ w1.T + p["mlp.fc1.bias"])
    act = bf(gelu(pre) if (exact_gelu or _EXACT) else gelu_poly(pre))
    x3 = x2 + act @ w2.T + p["mlp.fc2.bias"]
    saved = dict(p=p, B=B, N=N, C=C, H=H, hd=hd, scale=scale, sc2=sc2, wqkv=wqkv, wp=wp, w1=w1, w2=w2, xh1=xh1, rs1=rs1, y1=y1,
                 q=q, k=k, v=v, qs=qs, o=o, o2=o2, lse=lse, xh2=xh2, rs2=rs2, y2=y2, pre=pre, act=act)
    return x3, saved


def block_backward(saved, dx3: torch.Tensor, fused_bwd: bool = True, poly_dgelu: bool = False):
    """Backward of one Block with the HIP path's roundings: dx3 [B, N, C] (the fp32 gradient of the block output).
    Returns (dx float64, grads by reference parameter name)."""
    s = saved
    p, B, N, C, H, hd, scale, sc2 = s["p"], s["B"], s["N"], s["C"], s["H"], s["hd"], s["scale"], s["sc2"]
    wqkv, wp, w1, w2 = s["wqkv"], s["wp"], s["w1"], s["w2"]
    q, k, v, qs, o, o2, lse, pre, act, y1, y2 = s["q"], s["k"], s["v"], s["qs"], s["o"], s["o2"], s["lse"], s["pre"], s["act"], s["y1"], s["y2"]
    dx3 = dx3.to(D)
    G = {}
    d3b = bf(dx3)
    G["mlp.fc2.weight"] = (d3b.reshape(-1, C).T @ act.reshape(-1, act.shape[-1]))
    G["mlp.fc2.bias"] = dx3.reshape(-1, C).sum(0)
    # fc2 dgrad x GELU': the kernels with the LDS-transposing epilogue -- the 256-tile kernels and, since round 6, the small-launch kernel
    # that takes every problem the 256-tile kernels do not (csrc/gemm.hip gemm128_ok: hidden % 8 == 0 and whole k-tiles, C % 64 == 0)
    # -- round the product to bf16 on its way through the LDS transpose and multiply the ROUNDED value by gelu'(pre) (two roundings);
    # the 128-tile register-staged kernel, what is left for the other shapes, multiplies its fp32 accumulator and rounds once
    dg = dgelu_poly(pre) if (poly_dgelu and not _EXACT) else dgelu(pre)
    hidden = w1.shape[0]
    big = hidden % 8 == 0 and C % 64 == 0
    dpre = bf(bf(d3b @ w2) * dg) if big else bf((d3b @ w2) * dg)
    G["mlp.fc1.bias"] = dpre.reshape(-1, dpre.shape[-1]).sum(0)
    G["mlp.fc1.weight"] = dpre.reshape(-1, dpre.shape[-1]).T @ y2.reshape(-1, C)
    dy2 = bf(dpre @ w1)
    dln2, G["norm2.weight"], G["norm2.bias"] = ln_bwd(dy2, s["xh2"], s["rs2"], p["norm2.weight"])
    dx2 = dx3 + dln2
    dx2b = bf(dx2)
    G["attn.proj.bias"] = dx2.reshape(-1, C).sum(0)
    G["attn.proj.weight"] = dx2b.reshape(-1, C).T @ o2.reshape(-1, C)
    do = bf(dx2b @ wp).reshape(B, N, H, hd).transpose(1, 2)                 # [B, H, N, hd]
    dQf, dQp, dK, dV = attention_backward(q, k, v, qs, o, lse, do, scale, sc2, both_dq=not fused_bwd)
    dQ = dQf if fused_bwd else dQp
    dqkv = bf(torch.cat([t.transpose(1, 2).reshape(B, N, C) for t in (dQ, dK, dV)], -1))
    gb = dqkv.reshape(-1, 3 * C).sum(0)
    gw = dqkv.reshape(-1, 3 * C).T @ y1.reshape(-1, C)
    for i, nme in enumerate("qkv"):
        G[f"attn.{nme}.weight"] = gw[i * C:(i + 1) * C]
        G[f"attn.{nme}.bias"] = gb[i * C:(i + 1) * C]
    dy1 = bf(dqkv @ wqkv)
    dln1, G["norm1.weight"], G["norm1.bias"] = ln_bwd(dy1, s["xh1"], s["rs1"], p["norm1.weight"])
    dx = dx2 + dln1
    return dx, G


def block_forward_backward(P: Dict[str, torch.Tensor], x: torch.Tensor, dx3: torch.Tensor, num_heads: int, eps: float = 1e-6,
                           fused_bwd: bool = True, exact_gelu: bool = False, poly_dgelu: bool = False):
    """P: the Block's parameters by their reference names (norm1.weight, attn.q.weight, ..., mlp.fc2.bias), fp32.
    x, dx3: [B, N, C] fp32.  Returns (x3, dx, grads) in float64."""
    x3, saved = block_forward(P, x, num_heads, eps, exact_gelu)
    dx, G = block_backward(saved, dx3, fused_bwd, poly_dgelu)
    return x3, dx, G
