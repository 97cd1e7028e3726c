"""Per-element error bounds for the GEMM tests (a helper, not a conftest; tests/test_cpu_gemm_elem.py proves on the CPU that plain
fp32 arithmetic in any summation order stays inside them and that one-element, one-k-tile and one-slab faults do not).

A relative L2 norm over a whole [M, N] output dilutes a fault confined to one element by sqrt(M N): in a 1281 x 384 16-bit output one
element replaced by garbage of typical size moves it by 1.4e-3, inside the 3e-3 the whole-matrix checks of tests/test_gpu_kernels.py
allow.  Here every element has a bound of its own, derived from the arithmetic -- never from what a kernel was seen to give:

  acc_bound       fp32 accumulation of `terms` exact products (+ what the epilogue adds), in ANY order
  lp_round_bound  one round-to-nearest into the 16-bit operand type
  half_spacing    half the spacing of the 16-bit type at a value: worst(got, exp, half_spacing(exp)) > 1 <=> got is not exp (bit_exact)

and worst() returns the largest |got - ref| / bound with the index of that element.  U is the convention of
tests/test_gpu_lp_edges.py: 2^-9 for bfloat16, 2^-12 for half (the largest relative rounding error is 2 U)."""
import math

import numpy as np
import torch

F64 = torch.float64
EPS32 = 2.0 ** -23
LP_U = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}
LP_MANT = {torch.bfloat16: 7, torch.float16: 10}
N_FINITE = {torch.bfloat16: 65280, torch.float16: 63488}


def _d(t):
    return t.detach().to("cpu", F64) if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=F64)


def worst(got, ref, bound, with_index=True):
    """max over elements of |got - ref| / bound, and the index (a tuple) of the worst element.  bound: a tensor of the output's shape,
    > 0 everywhere.  NaN in got counts as infinite error (so does an inf where the reference is finite); got == ref counts as zero,
    inf == inf included."""
    got, ref, bound = _d(got), _d(ref), _d(bound)
    assert got.shape == ref.shape == bound.shape and got.numel() > 0, (got.shape, ref.shape, bound.shape)
    assert bool((bound > 0).all()), "every element needs a positive bound"
    e = (got - ref).abs() / bound
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, math.inf))
    e = torch.where(got == ref, torch.zeros_like(e), e)
    flat = int(e.argmax())
    val = float(e.flatten()[flat])
    return (val, tuple(int(i) for i in np.unravel_index(flat, tuple(e.shape)))) if with_index else val


def acc_bound(absA, absB, terms, extra=None):
    """(terms + 4) 2^-23 (absA @ absB^T + extra): fp32 accumulation of `terms` products per element, absA [M, K], absB [N, K].
    extra: the magnitude of what the epilogue adds (|bias|, |residual|, |accumulator|), broadcast to [M, N].
    The factor is twice the textbook n 2^-24: the order of the additions inside and across MFMAs, k slices and atomics is not
    specified and the MFMA's internal additions are not promised to round to nearest.  The + 4 pays for the epilogue's additions."""
    s = _d(absA) @ _d(absB).t()
    if extra is not None:
        s = s + _d(extra)
    return (terms + 4) * EPS32 * s


def sum_bound(abs_terms, n, extra=None):
    """(n + 4) 2^-23 (sum of |terms| + extra) for an fp32 sum of n numbers along dim 0 (column sums, row-head sums)."""
    s = _d(abs_terms)
    if extra is not None:
        s = s + _d(extra)
    return (n + 4) * EPS32 * s


def lp_round_bound(ref, U, tiny):
    """2 U |ref| + tiny: one round-to-nearest of ref into the 16-bit type (half an ulp is at most 2 U |ref|); tiny = the type's smallest
    normal number, because results below it may be flushed."""
    return 2.0 * U * _d(ref).abs() + tiny


def half_spacing(t, dtype):
    """half the distance between neighbouring numbers of `dtype` at |t| (the subnormal spacing below the smallest normal number)"""
    a = _d(t).abs()
    mant = LP_MANT[dtype]
    lo = math.log2(torch.finfo(dtype).tiny)
    ex = torch.frexp(a.clamp_min(torch.finfo(dtype).tiny))[1].to(F64) - 1.0          # floor(log2 |t|), >= the smallest normal's
    ex = torch.where(torch.isfinite(a), ex, torch.full_like(ex, lo))
    return 0.5 * torch.exp2(ex.clamp_min(lo) - mant)


def bit_exact(got, exp):
    """(ratio, index) -- 0 when the two 16-bit tensors hold the same bits; otherwise >= 2 (the first differing element is at least a
    whole spacing away, or differs in the sign of a zero / the payload of a NaN)."""
    assert got.dtype == exp.dtype and got.dtype in LP_U and got.shape == exp.shape
    g, e = got.detach().cpu().contiguous(), exp.detach().cpu().contiguous()
    same = g.view(torch.int16) == e.view(torch.int16)
    if bool(same.all()):
        return 0.0, (0,) * g.dim()
    val, idx = worst(g, e, half_spacing(e, g.dtype))
    if val > 1.0:
        return val, idx
    flat = int((~same).flatten().to(torch.uint8).argmax())
    return 2.0, tuple(int(i) for i in np.unravel_index(flat, tuple(g.shape)))


def all_finite_lp(dtype):
    """every finite bit pattern of the 16-bit type (65 280 for bfloat16, 63 488 for half: +-0, all subnormals, the largest numbers), in
    the order of their bits, padded with zeros to [256, 256]"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = bits.view(dtype)
    fin = v[torch.isfinite(v.float())]
    assert fin.numel() == N_FINITE[dtype]
    out = torch.zeros(65536, dtype=dtype)
    out[: fin.numel()] = fin
    return out.view(256, 256)


# ---- the two activation formulas: float64 references and the fp32 restatement of csrc/common.hpp --------------------------------------
def gelu64(x):
    """x Phi(x) in float64 through erfc (no cancellation in the left tail)"""
    x = _d(x)
    return x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def dgelu64(x):
    """Phi(x) + x phi(x) in float64"""
    x = _d(x)
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _f(v):
    return np.float32(v)


def _fma(a, b, c):
    """fp32 fused multiply-add through float64: the product of two fp32 numbers is exact there"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


GELU_COEF = (-2.306640613e-12, 2.495095069e-10, -1.216585654e-08, 3.568801260e-07, -7.116507187e-06, 1.035454878e-04,
             -1.148414365e-03, 9.898752642e-03, -6.641823237e-02, 3.989180135e-01)


def gelu_f32(x, low_branch=True):
    """gelu_f of csrc/common.hpp in numpy fp32: u = clamp(x, +-4.2), Phi = 0.5 + u P(u^2) (Horner with fma), (x < -4.2 ? 0 : x) Phi.
    low_branch=False: the form without the x < -4.2 branch (a planted defect of the CPU test)."""
    x = np.asarray(x, dtype=np.float32)
    u = np.clip(x, _f(-4.2), _f(4.2))
    t = u * u
    p = np.full_like(x, _f(GELU_COEF[0]))
    for c in GELU_COEF[1:]:
        p = _fma(p, t, _f(c))
    phi = _fma(u, p, _f(0.5))
    xs = np.where(x < _f(-4.2), _f(0.0), x) if low_branch else x
    return (xs * phi).astype(np.float32)


def dgelu_f32(x):
    """dgelu_exact_f of csrc/common.hpp in numpy fp32, with 1 / x and exp2 exact (float64, rounded to fp32): the hardware's
    reciprocal and exp2 add up to one ulp each"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a = np.abs(x)
        t = (1.0 / _fma(a, _f(0.2316419), _f(1.0)).astype(np.float64)).astype(np.float32)
        m = ((a * a).astype(np.float32) * _f(-0.72134752044448170)).astype(np.float32)
        e = np.exp2(m.astype(np.float64)).astype(np.float32)
        w = np.full_like(x, _f(0.53070271))
        for c in (-0.72657601, 0.71070687, -0.14224837, 0.12741479):
            w = _fma(w, t, _f(c))
        w = (w * t).astype(np.float32)
        g = (e * _fma(a, _f(-0.39894228040143268), w)).astype(np.float32)
        return (_f(0.5) + np.copysign(_f(0.5) - g, x)).astype(np.float32)


def gelu_bounds(x, U, tiny):
    """(ref, bound) of the activation a GELU epilogue stores for the 16-bit pre-activation x: for x >= -4.2 one rounding of gelu(x) plus
    2e-5 |x| for the polynomial (its fp32 restatement is within 1.72e-5 |x| over every finite 16-bit x; the rest is the device's own
    contraction of the products); below, where the kernels store 0, |act| <= 6e-5 (|gelu(x)| < 6e-5 there: csrc/common.hpp)."""
    x = _d(x)
    g = gelu64(x)
    low = x < -4.2
    return torch.where(low, torch.zeros_like(g), g), torch.where(low, torch.full_like(g, 6e-5), lp_round_bound(g, U, tiny) + 2e-5 * x.abs())


def dgelu_bounds(x, U, tiny):
    """(ref, bound) of a stored gelu'(x): one rounding + 1e-6 (the formula's 3e-7 and an ulp each for the hardware reciprocal and exp2)"""
    g = dgelu64(x)
    return g, lp_round_bound(g, U, tiny) + 1e-6
