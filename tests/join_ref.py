"""Float64 reference, per-element error bounds and an f32 restatement of the join kernel (octcubem_amd/csrc/join.hip): a helper, not a
conftest.  tests/test_cpu_join.py proves on the CPU that the bounds pass correct f32 arithmetic and catch planted faults,
tests/test_gpu_join.py holds the kernels to them.

    n_k = f_k / max(||f_k||, 1e-12)   (zeros where the modality is absent)        y = LayerNorm(concat_k n_k; gamma, beta, eps)

The bounds follow the arithmetic, with u = 2^-24 (one f32 rounding), first order plus the products of two errors, nothing fitted to a result:
  * the norm is a sum of D squares in ANY order: relative error (D + 1) u on the sum, half of it after the square root, plus the root,
    the reciprocal and the final product -> |n| (D / 2 + 4) u, the same for inv_norm;
  * the LayerNorm statistics are sums over the M D columns in any order, on inputs that carry the error above;
  * y is rounded ONCE to the 16-bit operand type (unit roundoff 2^-8 for bfloat16, 2^-11 for half, whose subnormal spacing adds 2^-25);
  * the backward recomputes n = f * inv_norm and reads mean / rstd with their forward errors; its two row means are sums over M D terms,
    the projection n . dn a sum over D; dgamma / dbeta are sums of B terms in any order, accumulated into a buffer (one more rounding).
Every bound has a floor at the smallest normal f32, as tests/cliploss_ref.py has: a reference value of exactly zero (an absent slot, the
output of an all-zero row) must come back as zero or a subnormal."""
import numpy as np

U = 2.0 ** -24
FLOOR = float(np.finfo(np.float32).tiny)
NORM_EPS = 1e-12
LN_EPS = 1e-5                        # nn.LayerNorm's default: ClassificationHead.input_norm
FWD_KEYS = ("n", "inv_norm", "mean", "rstd", "y")
BWD_KEYS = ("df", "dgamma", "dbeta")


def lp_roundoff(lp_is_f16):
    """(unit roundoff, absolute floor) of one rounding to the library's 16-bit operand type"""
    return (2.0 ** -11, 2.0 ** -25) if lp_is_f16 else (2.0 ** -8, FLOOR)


def make_problem(B, D, M, seed, special=True):
    """feats: M float32 [B, D] arrays with rows that are not exchangeable (own scale per row and modality); with ``special`` and enough rows:
    row 0 has one all-zero feature (modality 1), row 1 is all zeros in every modality, row 2 is scaled by 1e-20 and row 3 by 1e18.
    gamma, beta [M D], dy [B, M D], dn_extra [M, B, D], all float32."""
    g = np.random.default_rng(seed)
    feats = []
    for k in range(M):
        sc = 2.0 ** (4.0 * ((np.arange(B) * 0.381966 + 0.25 * k) % 1.0) - 2.0)
        feats.append((g.standard_normal((B, D)) * sc[:, None] + 0.3 * k).astype(np.float32))
    if special:
        if B > 0:
            feats[1][0] = 0.0
        if B > 1:
            for f in feats:
                f[1] = 0.0
        if B > 2:
            for f in feats:
                f[2] *= np.float32(1e-20)
        if B > 3:
            for f in feats:
                f[3] *= np.float32(1e18)
    gamma = (1.0 + 0.1 * g.standard_normal(M * D)).astype(np.float32)
    beta = (0.1 * g.standard_normal(M * D)).astype(np.float32)
    dy = (g.standard_normal((B, M * D)) * (2.0 ** (2.0 * ((np.arange(B) * 0.618034) % 1.0) - 1.0))[:, None]).astype(np.float32)
    extra = (0.5 * g.standard_normal((M, B, D))).astype(np.float32)
    return feats, gamma, beta, dy, extra


def _present(mask, k):
    return bool((mask >> k) & 1)


def reference(feats, mask, gamma, beta, dy=None, extra=None, eps=LN_EPS, lp_is_f16=False, dgamma0=None, dbeta0=None):
    """-> (ref, bound): two dicts of float64 arrays with the keys FWD_KEYS (+ BWD_KEYS when ``dy`` is given).  ``eps`` enters as the f32
    number the kernel receives.  df slices of absent modalities are NaN in ``ref`` (the kernel does not write them).  ``dgamma0`` /
    ``dbeta0``: what the gradient buffers held before the call (the kernel accumulates)."""
    M = len(feats)
    some = next(f for k, f in enumerate(feats) if _present(mask, k))
    B, D = some.shape
    W = M * D
    eps = float(np.float32(eps))
    gam, bet = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    rel_n = (D / 2 + 4) * U
    n = np.zeros((M, B, D)); inv = np.zeros((B, M)); tiny = np.zeros((B, M), bool)
    f64 = [None] * M
    for k in range(M):
        if not _present(mask, k):
            continue
        f64[k] = np.asarray(feats[k], np.float64)
        nrm = np.sqrt((f64[k] ** 2).sum(1))
        tiny[:, k] = nrm < NORM_EPS
        inv[:, k] = 1.0 / np.maximum(nrm, NORM_EPS)
        n[k] = f64[k] * inv[:, k, None]
    e_n = np.abs(n) * rel_n + FLOOR
    for k in range(M):
        if not _present(mask, k):
            e_n[k] = 0.0
    e_inv = inv * rel_n + FLOOR
    x = n.transpose(1, 0, 2).reshape(B, W)
    ex = e_n.transpose(1, 0, 2).reshape(B, W)

    def stats_chain(x, ex):
        """the errors of d = x - mu, rstd and xhat for column errors ex (forward: e_n; backward: the recomputed n)"""
        mu = x.mean(1)
        e_mu = ex.sum(1) / W + (W + 2) * U * np.abs(x).sum(1) / W + U * np.abs(mu)
        d = x - mu[:, None]
        e_d = ex + e_mu[:, None] + U * np.abs(d)
        q = (d ** 2).sum(1)
        var = q / W
        e_var = ((2 * np.abs(d) * e_d + e_d ** 2).sum(1) + (W + 1) * U * q) / W + 2 * U * var
        v = var + eps
        e_v = e_var + U * v
        rs = 1.0 / np.sqrt(v)
        lo = v - e_v
        e_rs = np.where(lo > 0, 1.0 / np.sqrt(np.where(lo > 0, lo, 1.0)) - rs, np.inf) + 4 * U * rs
        return mu, e_mu, d, e_d, rs, e_rs

    mu, e_mu, d, e_d, rs, e_rs = stats_chain(x, ex)
    xhat = d * rs[:, None]
    e_xh = e_d * rs[:, None] + np.abs(d) * e_rs[:, None] + e_d * e_rs[:, None] + U * np.abs(xhat)
    y = xhat * gam + bet
    e_y32 = e_xh * np.abs(gam) + 2 * U * (np.abs(xhat * gam) + np.abs(bet))
    u_lp, floor_lp = lp_roundoff(lp_is_f16)
    ref = {"n": n, "inv_norm": inv, "mean": mu, "rstd": rs, "y": y}
    bound = {"n": e_n + FLOOR, "inv_norm": e_inv, "mean": e_mu + FLOOR, "rstd": e_rs + FLOOR,
             "y": e_y32 + u_lp * (np.abs(y) + e_y32) + floor_lp}
    if dy is None:
        return ref, bound
    dy = np.asarray(dy, np.float64)
    # the backward recomputes n = f * inv_norm: inv_norm's error and one more rounding
    ex_b = np.where(ex > 0, np.abs(x) * (rel_n + U) + FLOOR, 0.0)
    e_d = ex_b + e_mu[:, None] + U * np.abs(d)                        # mean as the forward saved it
    e_xh = e_d * rs[:, None] + np.abs(d) * e_rs[:, None] + e_d * e_rs[:, None] + U * np.abs(xhat)
    gy = dy * gam
    e_g = U * np.abs(gy)
    m1 = gy.mean(1)
    e_m1 = (e_g.sum(1) + W * U * np.abs(gy).sum(1)) / W + 2 * U * np.abs(m1)
    gx = gy * xhat
    m2 = gx.mean(1)
    e_m2 = ((e_g * np.abs(xhat) + np.abs(gy) * e_xh + e_g * e_xh).sum(1) + (W + 1) * U * np.abs(gx).sum(1)) / W + 2 * U * np.abs(m2)
    t = gy - m1[:, None] - xhat * m2[:, None]
    e_t = (e_g + e_m1[:, None] + e_xh * np.abs(m2)[:, None] + np.abs(xhat) * e_m2[:, None] + e_xh * e_m2[:, None]
           + 3 * U * (np.abs(gy) + np.abs(m1)[:, None] + np.abs(xhat * m2[:, None])))
    dx = rs[:, None] * t
    e_dx = e_rs[:, None] * np.abs(t) + rs[:, None] * e_t + e_rs[:, None] * e_t + U * np.abs(dx)
    df = np.full((M, B, D), np.nan); e_df = np.full((M, B, D), np.nan)
    for k in range(M):
        if not _present(mask, k):
            continue
        sl = slice(k * D, (k + 1) * D)
        dn, e_dn = dx[:, sl], e_dx[:, sl]
        if extra is not None:
            dn = dn + np.asarray(extra[k], np.float64)
            e_dn = e_dn + U * np.abs(dn)
        nk, enk = x[:, sl], ex_b[:, sl]
        dot = (nk * dn).sum(1)
        e_dot = (enk * np.abs(dn) + np.abs(nk) * e_dn + enk * e_dn).sum(1) + (D + 1) * U * np.abs(nk * dn).sum(1)
        w = dn - nk * dot[:, None]
        e_w = (e_dn + enk * np.abs(dot)[:, None] + np.abs(nk) * e_dot[:, None] + enk * e_dot[:, None]
               + 2 * U * (np.abs(dn) + np.abs(nk * dot[:, None])))
        ik, eik = inv[:, k, None], e_inv[:, k, None]
        full = ik * w
        e_full = eik * np.abs(w) + ik * e_w + eik * e_w + U * np.abs(full)
        clamped = dn / NORM_EPS                                        # below the clamp: no projection term (autograd's F.normalize)
        e_clamped = e_dn / NORM_EPS + np.abs(clamped) * 2 * U          # 1e12 is no f32 number (4e-9 off) + the product
        tk = tiny[:, k, None]
        df[k] = np.where(tk, clamped, full)
        e_df[k] = np.where(tk, e_clamped, e_full) + FLOOR
    dgam = (dy * xhat).sum(0)
    e_dgam = (np.abs(dy) * e_xh).sum(0) + (B + 1) * U * np.abs(dy * xhat).sum(0)
    dbet = dy.sum(0)
    e_dbet = B * U * np.abs(dy).sum(0)
    if dgamma0 is not None:
        dgam = dgam + np.asarray(dgamma0, np.float64)
    if dbeta0 is not None:
        dbet = dbet + np.asarray(dbeta0, np.float64)
    ref.update(df=df, dgamma=dgam, dbeta=dbet)
    bound.update(df=e_df, dgamma=e_dgam + U * np.abs(dgam) + FLOOR, dbeta=e_dbet + U * np.abs(dbet) + FLOOR)
    return ref, bound


def worst(got, ref, bound, with_index=False):
    """max over the elements the reference defines (not NaN) of |got - ref| / bound; a NaN or Inf in ``got`` there is the worst one"""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    live = ~np.isnan(ref)
    e = np.where(live, np.abs(got - np.where(live, ref, 0.0)) / bound, 0.0) if live.any() else np.zeros(ref.shape)
    e = np.where(live & ~np.isfinite(got), np.inf, e)
    e = np.where(np.isnan(e), np.inf, e)
    i = int(np.argmax(e))
    return (float(e.flat[i]), i) if with_index else float(e.flat[i])


# --------------------------------------------------------------------------------------------------- the f32 restatement
F = np.float32


def _pow2_scale(amax):
    """s = 2^(127 - E) (E: the exponent field of amax), and 1 / s kept a normal number: the kernel's join_ld_inv_s"""
    E = (np.asarray(amax, F).view(np.uint32) >> 23) & 0xFF
    fs = np.where(E >= 254, 1, 254 - E.astype(np.int64)).astype(np.uint32)
    fi = np.clip(E, 1, 254).astype(np.uint32)
    return (fs << 23).view(F), (fi << 23).view(F)


def to_lp(x, lp_is_f16):
    """one round-to-nearest-even to the 16-bit operand type, returned as float32"""
    x = np.asarray(x, F)
    if lp_is_f16:
        return x.astype(np.float16).astype(F)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(F)


def emulate(feats, mask, gamma, beta, dy=None, extra=None, eps=LN_EPS, lp_is_f16=False, fault=None):
    """The kernel's arithmetic in float32 numpy, in its order of operations (sums by numpy's pairwise order: the bounds hold for any).
    ``fault``: 'slot' (the last present modality's slot dropped), 'stale_inv' (the normalisation backward without its projection term),
    'stats_D' (statistics over the first D columns instead of M D), 'dgamma_row' (dgamma misses the last row), 'mask' (a clear mask bit
    ignored: the absent modality's features are used)."""
    M = len(feats)
    if fault == "mask":
        assert mask != (1 << M) - 1 and all(f is not None for f in feats)
        mask = (1 << M) - 1
    if fault == "slot":
        mask &= ~(1 << max(k for k in range(M) if _present(mask, k)))
        assert mask
    some = next(f for k, f in enumerate(feats) if _present(mask, k))
    B, D = some.shape
    W = M * D
    eps = F(eps)
    gam, bet = np.asarray(gamma, F), np.asarray(beta, F)
    n = np.zeros((M, B, D), F); inv = np.zeros((B, M), F)
    for k in range(M):
        if not _present(mask, k):
            continue
        f = np.asarray(feats[k], F)
        s, inv_s = _pow2_scale(np.abs(f).max(1))
        t = f * s[:, None]
        r = np.sqrt((t * t).sum(1, dtype=F))
        with np.errstate(over="ignore", invalid="ignore"):
            tiny = ~(r * inv_s >= F(NORM_EPS))
        with np.errstate(divide="ignore", over="ignore"):
            b = np.where(tiny, F(1e12), F(1) / r).astype(F)
            a = np.where(tiny, F(1), s).astype(F)
            inv[:, k] = np.where(tiny, F(1e12), b * s)
        n[k] = (f * a[:, None]) * b[:, None]
    x = n.transpose(1, 0, 2).reshape(B, W)
    cols = D if fault == "stats_D" else W
    invW = F(1) / F(cols)
    mu = x[:, :cols].sum(1, dtype=F) * invW
    d = x - mu[:, None]
    var = (d[:, :cols] * d[:, :cols]).sum(1, dtype=F) * invW
    rs = (F(1) / np.sqrt(var + eps)).astype(F)
    y = to_lp((d * rs[:, None]) * gam + bet, lp_is_f16)
    out = {"n": n, "inv_norm": inv, "mean": mu, "rstd": rs, "y": y}
    if dy is None:
        return out
    dy = np.asarray(dy, F)
    xb = np.zeros((B, W), F)
    for k in range(M):
        if _present(mask, k):
            xb[:, k * D:(k + 1) * D] = np.asarray(feats[k], F) * inv[:, k, None]
    xhat = (xb - mu[:, None]) * rs[:, None]
    gy = dy * gam
    m1 = gy[:, :cols].sum(1, dtype=F) * invW
    m2 = (gy * xhat)[:, :cols].sum(1, dtype=F) * invW
    dx = rs[:, None] * (gy - m1[:, None] - xhat * m2[:, None])
    df = np.full((M, B, D), np.nan, F)
    for k in range(M):
        if not _present(mask, k):
            continue
        sl = slice(k * D, (k + 1) * D)
        dn = dx[:, sl] + (np.asarray(extra[k], F) if extra is not None else F(0))
        dot = (xb[:, sl] * dn).sum(1, dtype=F)
        dot = np.where(inv[:, k] >= F(1e12), F(0), dot)
        if fault == "stale_inv":
            dot = np.zeros_like(dot)
        df[k] = inv[:, k, None] * (dn - xb[:, sl] * dot[:, None])
    rows = slice(0, B - 1) if fault == "dgamma_row" else slice(0, B)
    out.update(df=df, dgamma=(dy * xhat)[rows].sum(0, dtype=F), dbeta=dy[rows].sum(0, dtype=F))
    return out
