"""Float64 references and per-element bounds of the adapter kernels (csrc/lora.hip), from the same operand bits.

merge   v = W + s B A.  The kernel: delta by r fused multiply-adds in ascending k, v = fma(s, delta, W); every rounding is at most
        2^-24 of a partial result no larger than |W| + s |B| |A|, so |v - ref| <= (r + 2) 2^-23 (|W| + s |B| |A|)  (twice the textbook
        figure, as tests/gemm_elem.py::acc_bound).  The 16-bit output is ONE rounding of that v.
wgrad   T = X A_lp^T and U = dY B_lp are fp32 sums of I resp. O products (acc_bound) rounded once to the operand type (lp_round_bound):
        |T_kernel - T| <= dT.  gB = g0 + s dY^T T_kernel: the error of T enters as |dY|^T dT, the fp32 sum over the M rows in any order as
        acc_bound(|dY|^T, |T| + dT, M); the closing fma(s, sum, g0) is one more rounding of |s sum| + |g0|.  gA alike with U and X.
        Rows / columns >= r of a gradient view are not touched: bit-equal to what was there.

The fp32 emulation (emulate_wgrad) does the stated roundings in a shuffled order of additions on the CPU and takes planted faults; the
CPU test shows that it stays inside the bounds without a fault and leaves them with each."""
import torch

from tests import gemm_elem as GE

F64, F32 = torch.float64, torch.float32
EPS32 = 2.0 ** -23


def _d(t):
    return t.detach().to("cpu", F64)


def pad_operands(A, B, lp):
    """A f32 [r, I], B f32 [O, r] -> (A_lp [rp, I], B_lp [O, rp]) in the 16-bit type with zero padding: what the merge kernel writes"""
    r, I = A.shape
    O = B.shape[0]
    rp = (r + 15) // 16 * 16
    A_lp = torch.zeros((rp, I), dtype=lp)
    B_lp = torch.zeros((O, rp), dtype=lp)
    A_lp[:r] = A.detach().cpu().to(lp)
    B_lp[:, :r] = B.detach().cpu().to(lp)
    return A_lp, B_lp


def merge_ref(W, A, B, s):
    """(v float64 [O, I], bound) of the merge"""
    W, A, B = _d(W), _d(A), _d(B)
    r = A.shape[0]
    v = W + s * (B @ A)
    bound = (r + 2) * EPS32 * (W.abs() + abs(s) * (B.abs() @ A.abs())) + 1e-300
    return v, bound


def wgrad_ref(x, dy, A_lp, B_lp, s, r, gA0, gB0, U, tiny):
    """x [M, I], dy [M, O], A_lp [rp, I], B_lp [O, rp] (16-bit operand bits), gA0 [r, I] / gB0 [O, r] the gradients before the call (fp32).
    Returns ((gA_ref, gA_bound), (gB_ref, gB_bound)) over the first r rows / columns, float64."""
    x, dy, A_lp, B_lp = _d(x), _d(dy), _d(A_lp)[:r], _d(B_lp)[:, :r]
    M, I = x.shape
    O = dy.shape[1]
    T, Uu = x @ A_lp.t(), dy @ B_lp                                        # [M, r]
    dT = GE.acc_bound(x.abs(), A_lp.abs(), I) + GE.lp_round_bound(T, U, tiny)
    dU = GE.acc_bound(dy.abs(), B_lp.t().abs(), O) + GE.lp_round_bound(Uu, U, tiny)
    out = []
    for G, S, dS, g0 in ((x, Uu, dU, _d(gA0).t()), (dy, T, dT, _d(gB0))):           # P [cols of G, r] = G^T S
        P = G.t() @ S
        ref = g0 + s * P
        bound = abs(s) * (G.abs().t() @ dS + GE.acc_bound(G.abs().t(), (S.abs() + dS).t(), M)) + EPS32 * ((s * P).abs() + g0.abs()) + 1e-300
        out.append((ref, bound))
    (ra, ba), gb = out
    return (ra.t(), ba.t()), gb


def _shuffled_matmul(a, b, gen, parts=4):
    """fp32 a @ b.T with the reduction index permuted and cut into `parts` partial sums added in order: another order of fp32 additions"""
    K = a.shape[1]
    perm = torch.randperm(K, generator=gen)
    a, b = a[:, perm].contiguous(), b[:, perm].contiguous()
    acc = None
    for idx in torch.tensor_split(torch.arange(K), min(parts, K)):
        part = a[:, idx] @ b[:, idx].t()
        acc = part if acc is None else acc + part
    return acc


def emulate_wgrad(x, dy, A_lp, B_lp, s, gA0, gB0, lp, chunk, seed=0, fault=None):
    """The kernel's arithmetic in fp32 torch on the CPU, on the FULL padded width: returns gA [rp, I], gB [O, rp] given the fp32 gA0 [rp, I],
    gB0 [O, rp] before the call.  T and U: fp32 sums in a shuffled order, one rounding to `lp`; per row chunk an fp32 partial (shuffled
    inside), the partials added in ascending chunk order, one fma with s.  fault: None, or one of
      "row" (one token row left out of both products), "chunk" (one row chunk left out), "rank" (one rank column of T and U left out),
      "scale" (s forgotten), "swap" (T and U exchanged; needs I == O)."""
    gen = torch.Generator().manual_seed(seed)
    xf, dyf, Af, Bf = x.float(), dy.float(), A_lp.float(), B_lp.float()
    M = xf.shape[0]
    T = _shuffled_matmul(xf, Af, gen).to(lp).float()                     # [M, rp]
    Uu = _shuffled_matmul(dyf, Bf.t().contiguous(), gen).to(lp).float()
    if fault == "rank":
        T[:, 0] = 0
        Uu[:, 0] = 0
    if fault == "swap":
        T, Uu = Uu, T
    keep = torch.ones(M, dtype=torch.bool)
    if fault == "row":
        keep[M // 2] = False
    starts = list(range(0, M, chunk))
    if fault == "chunk":
        starts = starts[:-1] if len(starts) > 1 else []
    res = []
    for G, S, g0, transpose in ((xf, Uu, gA0, True), (dyf, T, gB0, False)):
        total = torch.zeros((G.shape[1], S.shape[1]), dtype=F32)
        for i, m0 in enumerate(starts):
            rows = torch.arange(m0, min(m0 + chunk, M))
            rows = rows[keep[rows]]
            part = _shuffled_matmul(G[rows].t().contiguous(), S[rows].t().contiguous(), gen) if rows.numel() else torch.zeros_like(total)
            total = part if i == 0 else total + part
        sc = 1.0 if fault == "scale" else s
        P = total.t() if transpose else total
        res.append((g0.double() + sc * P.double()).float())               # fma: one rounding of the exact s * P + g0
    return res[0], res[1]


def check(got, ref, bound, before, r, dim):
    """worst |got - ref| / bound over the first r rows (dim 0) / columns (dim 1) of a gradient view, and whether the rest kept the bits of
    `before`"""
    first = got.narrow(dim, 0, r)
    rest_same = torch.equal(got.narrow(dim, r, got.shape[dim] - r).cpu().view(torch.int32),
                            before.narrow(dim, r, got.shape[dim] - r).cpu().view(torch.int32))
    w, idx = GE.worst(first, ref, bound)
    return w, idx, rest_same
