"""float64 reference, derived error bounds and an f32 restatement of one step of attention rollout (octcubem_amd/csrc/rollout.hip,
ops.rollout_step) and of the chain ``saliency.attention_rollout`` runs.  A helper, not a conftest; tests/test_cpu_rollout.py shows on
the CPU that the restatement stays inside the bounds and that five planted faults do not; tests/test_gpu_rollout.py holds the kernel to
the same bounds.

Definition.  Per sample: q, k f32 [N, H * HD], s^h = q^h k^h^T, z = scale s, P^h = softmax_j z^h, F = fuse_h P^h (mean, max, min),
rho_i = 1 + sum_j F_ij (2 for the mean), c_i = r_i / rho_i, T = F + I:

    r_out[j] = sum_i c_i T_ij            (one block: r_out = r^T Ahat, Ahat = T / rho;  the chain: from the last block down)

The reference starts from the kernel's own score bits: ``chain_scores`` is the f32 chain acc = fmaf(q_ik, k_jk, acc) evaluated exactly
(the product of two f32 numbers is exact in float64; the float64 sum is turned into a round-to-odd value by an error-free TwoSum, so
the final rounding to f32 is the single rounding of a true fma).  Everything after s is float64.

Bounds.  u = 2^-24, gamma_k = k u / (1 - k u); T0 = the smallest normal f32 (2^-126): what one flushed or denormal result can lose in
absolute terms.  Analysis of the arithmetic stated in the head comment of csrc/rollout.hip, not measurements:

  logit   one rounding of scale * s:  |z~ - z| <= ez = u |z|.
  lse     as tests/cliploss_ref.py derives it for the same online (max, sum): a perturbation ez of the logits moves a log-sum-exp by at
          most log sum_j p_j exp(ez_j); every term exp(z_j - M) carries the rounding of its argument (2 u |z_j - M|, + 4 ez for the
          perturbed operands), EXP_ULPS ulp of expf (exp_rel = 2 u EXP_ULPS) and, once per stage that rescales it, one more exp, one
          product and one sum: STAGES (exp_rel + 2 u), STAGES = ceil(N / 64) + 2 (the column tiles, the half-wave merge, the wave merge);
          N positive additions in any order: gamma; an underflowed term: T0 each (the sum is >= 1).  Then logf (LOG_ULPS ulp of
          |lse - M|) and the addition M + log.  -> E_lse per (h, i).
  P       P~ = expf(fl(z~ - lse~)):  eP = P expm1(ez + E_lse + 2 u |z - lse| + exp_rel) + T0.
  F       mean: H - 1 additions of positive terms, the rounded 1 / H and the product: eF = (1 + gamma_{H+2}) mean_h eP + gamma_{H+2} F + T0.
          max / min: a selection is exact and 1-Lipschitz in the largest deviation: eF = max_h eP.
  rho     mean: 2 exactly, c = r / 2 exactly (a power of two; T0 for an underflow).  max / min: N positive additions in any order and the
          leading 1: e_rho = sum_j eF + gamma_{N+1} (rho + sum_j eF);  c~ = fl(r / rho~): ec = c ((1 + u) rho / (rho - e_rho) - 1) + T0.
  T       the diagonal's F + 1 is one rounding: eT = eF + [i = j] u (1 + F + eF).
  column  term_ij = fl(c~ T~): e_term = ec T + c eT + ec eT + u (c + ec)(T + eT) + T0;  N additions of non-negative terms in ANY order
          (registers, half-waves, waves, row tiles, slabs -- the fold changes the order, not the count):
          E_out_j = sum_i e_term_ij + gamma_{N+1} sum_i (c T + e_term)_ij + T0.
  chain   the step is linear in r and Ahat's rows sum to 1: an input error |e_in| <= E_in passes through as E_in^T Ahat (gain at most 1
          in the 1-norm, element by element here), and the step's own error is the bound above taken at r + E_in:
          E_next = E_out(r + E_in) + E_in^T Ahat.
"""
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
EXP_ULPS = 1.0          # HIP device library: expf, logf <= 1 ulp
LOG_ULPS = 1.0
TILE = 64               # SIM_ROWS == SIM_COLS (csrc/simtile.hpp)
TARGET_WGS = 1024       # SIM_TARGET_WGS
MAX_SPLIT = 64          # RO_MAX_SPLIT (csrc/rollout.hip)
MAX_HD = 128            # RO_MAX_HD
T0 = float(np.finfo(np.float32).tiny)
FUSIONS = ("mean", "max", "min")

# (B, N, H, HD) of the GPU tests.  The last one comes from the kernel's split rule (``split``): at N = 2049 -- the smallest such N -- a
# column block's 33 row tiles are dealt to 32 workgroups, so one of them makes a second trip (its sums carried across) and 32 slabs are
# folded.  From N = 65 on every shape has split > 1: the fold runs.  No grid cap sits in front of that rule (the grids are flat in x
# and the entry point refuses what does not fit), so there is no further shape for one.
SHAPES = ((1, 1, 1, 32), (1, 2, 1, 64), (2, 63, 2, 32), (1, 64, 3, 64), (1, 65, 2, 64), (2, 129, 2, 32), (1, 197, 3, 64),
          (1, 130, 1, 40), (1, 2049, 1, 8))
SPLITS = (1, 1, 1, 1, 2, 3, 4, 3, 32)
TRIP_SHAPE = SHAPES[-1]
STARTS = ("cls", "patches", "random", "zeros")


def gamma(k):
    return k * U / (1.0 - k * U)


def split(N):
    """ro_plan: the workgroups that share one column block's row tiles -- sim_split under RO_MAX_SPLIT, of N alone"""
    blocks = -(-N // TILE)
    return max(1, min(-(-TARGET_WGS // blocks), blocks, MAX_SPLIT))


def ws_bytes(B, N, H, fusion):
    """octmae_rollout_ws: lse [B][H][N], rho [B][N] for max / min, the slabs [split][B][N] where split > 1"""
    s = split(N)
    return 4 * (B * H * N + (0 if fusion == 0 else B * N) + (s * B * N if s > 1 else 0))


def walked_tiles(tiles, nsplit, y):
    return list(range(y, tiles, nsplit))


def _t(x):
    return x.detach().to("cpu", F64) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=F64)


# ------------------------------------------------------------------------------------------------ problems
def make_problem(B, N, H, HD, seed):
    """q, k f32 [B * N, H * HD] and scale = HD^-0.5 (as f32).  Per head the rows of q cycle through three kinds: hot (the row's
    largest |z| is 80: a near one-hot softmax row whose tail underflows in f32), cold (largest |z| 0.9: a nearly flat row) and plain
    (unit Gaussians, |z| of a few units)."""
    rng = np.random.default_rng([seed, B, N, H, HD])
    q = rng.standard_normal((B, N, H, HD))
    k = rng.standard_normal((B, N, H, HD))
    scale = np.float32(HD ** -0.5)
    z = float(scale) * np.einsum("bihd,bjhd->bhij", q, k)
    top = np.abs(z).max(axis=3).transpose(0, 2, 1)                  # [B, N, H]
    kind = (np.arange(N)[None, :, None] + np.arange(H)[None, None, :]) % 3
    mult = np.where(kind == 0, 80.0 / top, np.where(kind == 1, 0.9 / top, 1.0))
    q = q * mult[..., None]
    f = lambda x: np.ascontiguousarray(x.reshape(B * N, H * HD), dtype=np.float32)
    return f(q), f(k), scale


def make_start(kind, B, N, seed=0):
    """r_in f32 [B, N]: the class-token one-hot, uniform over the patch tokens (token 0 is the prefix), random positive, random with
    exact zeros"""
    rng = np.random.default_rng([seed, B, N, STARTS.index(kind)])
    r = np.zeros((B, N), dtype=np.float32)
    if kind == "cls":
        r[:, 0] = 1.0
    elif kind == "patches":
        r[:, min(1, N - 1):] = 1.0 / max(N - 1, 1)
    else:
        r = (rng.random((B, N)) + 0.05).astype(np.float32)
        if kind == "zeros":
            r[rng.random((B, N)) < 0.4] = 0.0
            r[:, N // 2] = 0.0
    return r


# ------------------------------------------------------------------------------------------------ the scores, bit for bit
def _fma32(a64, b64, acc32):
    """fmaf(a, b, acc) for f32 values, exactly: p = a b is exact in float64; s = fl64(acc + p) with its TwoSum residual e; where e != 0
    the pair is replaced by the neighbour of s with an odd last bit on e's side (round to odd: 53 bits >= 24 + 2), and the rounding
    to f32 is then the one rounding of the exact sum."""
    p = a64 * b64
    acc = acc32.astype(np.float64)
    s = acc + p
    bb = s - acc
    e = (acc - (s - bb)) + (p - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def chain_scores(q, k, B, N, H, HD, skip=None):
    """s f32 [B, H, N, N]: the tile's chain acc = 0; for kk = 0 .. HD-1: acc = fmaf(q[i][h HD + kk], k[j][h HD + kk], acc)."""
    q = np.asarray(q, dtype=np.float32).reshape(B, N, H, HD).astype(np.float64)
    k = np.asarray(k, dtype=np.float32).reshape(B, N, H, HD).astype(np.float64)
    acc = np.zeros((B, H, N, N), dtype=np.float32)
    for kk in range(HD):
        a = q[:, :, :, kk].transpose(0, 2, 1)[:, :, :, None]       # [B, H, N, 1]
        b = k[:, :, :, kk].transpose(0, 2, 1)[:, :, None, :]       # [B, H, 1, N]
        acc = _fma32(a, b, acc)
    return acc


# ------------------------------------------------------------------------------------------------ float64 reference with bounds
def fuse64(P, fusion):
    """[H, N, N] -> [N, N]"""
    return {"mean": lambda: P.mean(dim=0), "max": lambda: P.max(dim=0).values, "min": lambda: P.min(dim=0).values}[fusion]()


class StepRef:
    """One block of one sample in float64 from its score bits ``s`` f32 [H, N, N]: F, rho, T = F + I, Ahat, and the error terms of the
    module docstring that do not depend on r.  ``apply(r, e_in)`` -> (r_out, bound)."""

    def __init__(self, s, scale, fusion):
        s = _t(s)
        H, N, _ = s.shape
        self.N, self.fusion = N, fusion
        z = float(np.float32(scale)) * s
        ez = U * z.abs()
        stages = math.ceil(N / TILE) + 2
        exp_rel = EXP_ULPS * 2.0 * U
        lse = torch.logsumexp(z, dim=2, keepdim=True)
        P = torch.exp(z - lse)
        M = z.max(dim=2, keepdim=True).values
        per_term = stages * (exp_rel + 2.0 * U) + 2.0 * U * ((z - M).abs() + 4.0 * ez) + exp_rel
        R = (P * per_term).sum(dim=2, keepdim=True) + gamma(N + stages) + N * T0
        pert = torch.log((P * torch.exp(ez)).sum(dim=2, keepdim=True))
        e_lse = pert - torch.log1p(-R) + LOG_ULPS * 2.0 * U * (lse - M).abs() + 2.0 * U * lse.abs() + U * M.abs()
        eP = P * torch.expm1(ez + e_lse + 2.0 * U * (z - lse).abs() + exp_rel) + T0
        F = fuse64(P, fusion)
        if fusion == "mean":
            eF = (1.0 + gamma(H + 2)) * eP.mean(dim=0) + gamma(H + 2) * F + T0
            rho = torch.full((N,), 2.0, dtype=F64)
            e_rho = torch.zeros(N, dtype=F64)
        else:
            eF = eP.max(dim=0).values
            rho = 1.0 + F.sum(dim=1)
            e_rho = eF.sum(dim=1) + gamma(N + 1) * (rho + eF.sum(dim=1))
        eye = torch.eye(N, dtype=F64)
        self.rho, self.e_rho = rho, e_rho
        self.T = F + eye
        self.eT = eF + eye * (U * (1.0 + F + eF))
        self.F, self.P, self.lse, self.e_lse = F, P, lse.squeeze(2), e_lse.squeeze(2)

    def ahat(self):
        return self.T / self.rho[:, None]

    def apply(self, r, e_in=None):
        r = _t(r).reshape(self.N)
        e_in = torch.zeros_like(r) if e_in is None else _t(e_in).reshape(self.N)
        N, T, eT, rho, e_rho = self.N, self.T, self.eT, self.rho, self.e_rho
        c = r / rho
        out = c @ T
        cm = (r + e_in) / rho                                       # the magnitudes the step's own roundings act on
        ec = cm * ((1.0 + U) * rho / (rho - e_rho) - 1.0) + T0 if self.fusion != "mean" else torch.full_like(cm, T0)
        e_terms = ec @ T + cm @ eT + ec @ eT + U * ((cm + ec) @ (T + eT)) + N * T0
        bound = e_terms + gamma(N + 1) * (cm @ T + e_terms) + T0
        return out, bound + (e_in / rho) @ T


def step_reference(s, scale, r, fusion, e_in=None):
    """s f32 [B, H, N, N], r [B, N] -> (r_out f64 [B, N], bound f64 [B, N])"""
    outs = [StepRef(s[b], scale, fusion).apply(r[b], None if e_in is None else e_in[b]) for b in range(len(s))]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def chain_reference(scores, scales, w, fusion, first_layer=0):
    """The vector chain over blocks: ``scores`` a list (block 0 first) of f32 [B, H, N, N], ``w`` [B, N].  From the last block down to
    ``first_layer``; the bound propagated as the module docstring says.  -> (tokens f64 [B, N], bound f64 [B, N])"""
    r, e = _t(w), None
    for layer in range(len(scores) - 1, first_layer - 1, -1):
        r, e = step_reference(scores[layer], scales[layer], r, fusion, e)
    return r, e


def worst(got, ref_bound):
    """max over elements of |got - ref| / bound (inf for a NaN or a wrong inf)"""
    ref, bound = ref_bound
    got = _t(got).reshape(ref.shape)
    assert bool((bound > 0).all())
    e = (got - ref).abs() / bound
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, math.inf))
    e = torch.where(got == ref, torch.zeros_like(e), e)
    return float(e.max())


# ------------------------------------------------------------------------------------------------ f32 restatement of the kernel
FAULTS = ("identity", "tile", "head", "rho2", "scale2")
_STREAMS = [(wc, h, [wc * 32 + 4 * h + (g & 3) + 8 * (g >> 2) for g in range(16)]) for wc in (0, 1) for h in (0, 1)]   # SIM_COL


def _merge(m1, s1, m2, s2):
    """ro_merge in f32"""
    f = np.float32
    M = np.maximum(m1, m2)
    with np.errstate(invalid="ignore"):
        e1 = np.where(m1 == M, f(1), np.exp((m1 - M).astype(f))).astype(f)
        e2 = np.where(m2 == M, f(1), np.exp((m2 - M).astype(f))).astype(f)
    return M, ((s1 * e1).astype(f) + (s2 * e2).astype(f)).astype(f)


def _lane_lse(z):
    """ro_stats_kernel: z f32 [R, N] -> lse f32 [R]; a lane's online (max, sum) over its 16 columns of every tile, then the two
    half-waves, then the two waves"""
    f = np.float32
    R, N = z.shape
    parts = {}
    for wc, h, cols in _STREAMS:
        mx = np.full(R, -np.inf, dtype=f)
        sm = np.zeros(R, dtype=f)
        for j0 in range(0, N, TILE):
            cc = [j0 + c for c in cols if j0 + c < N]
            if not cc:
                continue
            blk = z[:, cc]
            nm = np.maximum(mx, blk.max(axis=1))
            with np.errstate(invalid="ignore"):
                fac = np.where(mx == nm, f(1), np.exp((mx - nm).astype(f))).astype(f)
            s = (sm * fac).astype(f)
            e = np.exp((blk - nm[:, None]).astype(f)).astype(f)
            for c in range(e.shape[1]):
                s = (s + e[:, c]).astype(f)
            mx, sm = nm, s
        parts[wc, h] = (mx, sm)
    m0, s0 = _merge(*parts[0, 0], *parts[0, 1])
    m1, s1 = _merge(*parts[1, 0], *parts[1, 1])
    m, s = _merge(m0, s0, m1, s1)
    with np.errstate(divide="ignore"):
        return (m + np.log(s).astype(f)).astype(f)


def _lane_sum(X, nsplit=1, drop_tile=None):
    """sum over axis 0 of X f32 [n, cols] in the kernels' order: workgroup y of ``nsplit`` walks the 64-row tiles y, y + nsplit, ...; a
    lane adds its 16 rows of every tile in ascending order; half-waves, then waves; the workgroups' slabs are folded in ascending y"""
    f = np.float32
    n = X.shape[0]
    tiles = -(-n // TILE)
    total = None
    for y in range(nsplit):
        part = {}
        for wc, h, rows in _STREAMS:
            acc = np.zeros(X.shape[1:], dtype=f)
            for t in walked_tiles(tiles, nsplit, y):
                if t == drop_tile:
                    continue
                for c in rows:
                    if t * TILE + c < n:
                        acc = (acc + X[t * TILE + c]).astype(f)
            part[wc, h] = acc
        slab = ((part[0, 0] + part[0, 1]).astype(f) + (part[1, 0] + part[1, 1]).astype(f)).astype(f)
        total = slab if total is None else (total + slab).astype(f)
    return total


def emulate_step(s, scale, r, fusion, fault=None):
    """The kernel's passes in numpy f32 for one sample: s f32 [H, N, N] (the chain's bits), r f32 [N] -> r_out f32 [N].  ``fault`` in
    FAULTS plants the named defect: the identity term dropped, one 64-row tile skipped in the column sums, one head left out of the
    fusion, rho left at 2 under max / min fusion, scale applied twice."""
    f = np.float32
    s = np.asarray(s, dtype=f)
    H, N, _ = s.shape
    scale = f(scale)
    r = np.asarray(r, dtype=f).reshape(N)
    z = (scale * s).astype(f)
    if fault == "scale2":
        z = (scale * z).astype(f)
    lse = np.stack([_lane_lse(z[h]) for h in range(H)])                                     # pass 1
    with np.errstate(under="ignore"):
        P = np.exp((z - lse[:, :, None]).astype(f)).astype(f)
    heads = [h for h in range(H) if not (fault == "head" and h == H - 1 and H > 1)]
    Fu = P[heads[0]]
    for h in heads[1:]:
        Fu = (Fu + P[h]).astype(f) if fusion == "mean" else (np.maximum(Fu, P[h]) if fusion == "max" else np.minimum(Fu, P[h]))
    if fusion == "mean":
        Fu = (Fu * (f(1) / f(H))).astype(f)
        c = (r * f(0.5)).astype(f)
    else:
        rho = (f(1) + _lane_sum(np.ascontiguousarray(Fu.T), split(N))).astype(f)             # pass 2: the sum over j, and its fold
        if fault == "rho2":
            rho = np.full(N, 2, dtype=f)
        c = (r / rho).astype(f)
    T = Fu.copy()
    if fault != "identity":
        T[np.arange(N), np.arange(N)] = (T[np.arange(N), np.arange(N)] + f(1)).astype(f)
    with np.errstate(under="ignore"):
        terms = (c[:, None] * T).astype(f)
    tiles = -(-N // TILE)
    return _lane_sum(terms, split(N), drop_tile=(tiles // 2) if fault == "tile" else None)   # pass 3 and the fold


def emulate(s, scale, r, fusion, fault=None):
    """[B, H, N, N], [B, N] -> f32 [B, N]"""
    return np.stack([emulate_step(s[b], scale, r[b], fusion, fault) for b in range(len(s))])


# ------------------------------------------------------------------------------------------------ the published algorithm, literally
def published_rollout(attentions, fusion, first_layer=0):
    """Abnar & Zuidema's rollout as it is usually written: ``attentions`` a list (block 0 first) of float64 [B, H, N, N] softmax
    matrices; per layer fuse the heads, add the identity, normalise the rows, multiply in layer order.  -> R float64 [B, N, N]."""
    B, _, N, _ = attentions[0].shape
    eye = torch.eye(N, dtype=F64)
    R = eye.expand(B, N, N).clone()
    for A in attentions[first_layer:]:
        if fusion == "mean":
            Fu = A.mean(dim=1)
        elif fusion == "max":
            Fu = A.max(dim=1).values
        else:
            Fu = A.min(dim=1).values
        a = Fu + eye
        a = a / a.sum(dim=-1, keepdim=True)
        R = a @ R
    return R
