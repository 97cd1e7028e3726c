"""float64 reference, derived error bounds and an f32 restatement of the fused contrastive loss (octcubem_amd/csrc/cliploss.hip,
ops.clip_pair_loss).  A helper, not a conftest; tests/test_cpu_cliploss.py shows on the CPU that the restatement stays inside the bounds
and that a dropped column tile, a dropped k-step, a shifted partner and a weight on the wrong direction do not.

Definition.  a f32 [n, d], b f32 [m, d], s = a b^T, z = scale s, t_i = i + offset, row weights wr [n], optional pair weights wc [n]:

    L = sum_i wr_i (lse_j z_ij - z_it)  +  sum_i wc_i (lse_i' z_i't - z_it)
    G_ij = wr_i (p_ij - [j = t_i]) + wc_{j - offset} (q_ij - [j = t_i]),  p = exp(z - lse_row_i),  q = exp(z - lse_col_j)
    da = g scale G b,   db = g scale G^T a,   dscale = g sum G o s

Bounds.  u = 2^-24 (unit roundoff of f32), gamma_k = k u / (1 - k u).  They are analysis of the arithmetic, not measurements:

  score   the f32 dot product of d terms in ANY order: |s~ - s| <= gamma_d A_ij, A_ij = sum_k |a_ik b_jk|.
  logit   one rounding for scale * s~:  |z~ - z| <= ez_ij = (1 + u) |scale| gamma_d A_ij + u |z_ij|.
  lse     log sum exp is monotone and (sum p e^-x)(sum p e^x) >= 1, so a perturbation |e_j| <= ez_j of the logits moves it by at most
          log sum_j p_j exp(ez_j).  The sum itself: every term exp(z_j - M) carries the rounding of the subtraction, u |z_j - M| -- which is
          also what an exp2 route loses when it rounds (z_j - M) log2 e, hence 2 u |z_j - M| (+ 4 ez for the perturbed operands) -- and
          EXP_ULPS ulp of the exp (documented: expf <= 1 ulp).  An online sum rescales a term once per stage, each stage one more exp
          (its argument roundings telescope to <= u (M - z_j), covered above by the factor 2), one multiplication and one addition:
          STAGES (exp_rel + 2 u) with STAGES = ceil(max(n, m) / 64) + 66 (column tiles + half-wave + wave pair + up to 64 partials).
          m additions of positive terms in any order: gamma_m relative.  Then log (LOG_ULPS ulp of |lse - M|) and the addition M + log.
  loss    per row: the weight times (lse error + ez of the partner + 2 u |lse - z_t|: the subtraction and the product); n f32 additions of
          the rows in any order, (n + 4) u sum |terms|; one rounding of L.
  G       p~ = exp(z~ - lse~): p expm1(ez + E_lse + 2 u |z - lse| + exp_rel); the subtraction of the hit, the product with the weight and
          the sum of the two directions: 3 u |p - hit| per direction + u |G|.
  da, db  the second product is an f32 dot of m (n) terms in any order: sum_j E_G |b| + gamma_{m+2} sum_j (|G| + E_G) |b|; g scale and
          its product with the sum: 2 u |da|.  A floor of the smallest normal f32 keeps an exactly-zero expectation testable.
  dscale  sum_ij (E_G |s| + (|G| + E_G) gamma_d A) + (n + m + 4) u sum |G s| (f32 additions in any order), times |g|, + u |dscale|.
"""
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
EXP_ULPS = 1.0          # HIP device library: expf, logf <= 1 ulp
LOG_ULPS = 1.0
TILE = 64
KSTEP = 32
FLOOR = float(np.finfo(np.float32).tiny)


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------ the forward's launch plan, restated
TARGET_WGS = 1024       # SIM_TARGET_WGS (csrc/simtile.hpp)
MAX_SPLIT = 64          # CL_MAX_SPLIT
# (n, m, d, offset) at which a workgroup of clip_lse_kernel walks more than one column tile, with the plan the constants above give:
# tests/test_cpu_cliploss.py compares the constants with csrc/cliploss.hip and the plans with this table, so whoever changes a constant
# is told to move the shapes; tests/test_gpu_cliploss.py runs them.
TRIP_SHAPES = ((8, 8325, 3, 8200), (3001, 3001, 5, 0), (130, 65500, 2, 65000))
TRIP_PLANS = (dict(row_blocks_a=1, tiles_a=131, split_a=64, row_blocks_b=131, tiles_b=1, split_b=1),          # a side: 2 or 3 trips
              dict(row_blocks_a=47, tiles_a=47, split_a=22, row_blocks_b=47, tiles_b=47, split_b=22),         # both sides: 2 or 3 trips
              dict(row_blocks_a=3, tiles_a=1024, split_a=64, row_blocks_b=1024, tiles_b=3, split_b=1))        # a: 16 trips; b: split 1, 3 tiles


def split(row_blocks, col_tiles, target_wgs=TARGET_WGS):
    """sim_split under CL_MAX_SPLIT: the workgroups that share one row block's column tiles"""
    return max(1, min(-(-target_wgs // row_blocks), col_tiles, MAX_SPLIT))


def plan(n, m, target_wgs=TARGET_WGS):
    """cl_plan: the a side owns rows of a and walks tiles of b, the b side the other way round"""
    p = dict(row_blocks_a=-(-n // TILE), row_blocks_b=-(-m // TILE), tiles_a=-(-m // TILE), tiles_b=-(-n // TILE))
    p["split_a"] = split(p["row_blocks_a"], p["tiles_a"], target_wgs)
    p["split_b"] = split(p["row_blocks_b"], p["tiles_b"], target_wgs)
    return p


def ws_floats(n, m):
    """cl_ws_floats: one (max, sum) per row and workgroup of each side"""
    p = plan(n, m)
    return 2 * (p["split_a"] * n + p["split_b"] * m)


def walked_tiles(col_tiles, nsplit, y):
    """the column tiles workgroup y of a row block visits, in its order"""
    return list(range(y, col_tiles, nsplit))


def _d(t):
    return t.detach().to("cpu", F64) if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t), dtype=F64)


def make_problem(n, m, d, seed, offset=0, zero_frac=0.0, equal_weights=False):
    """unit-norm a [n, d]; b [m, d] with b[i + offset] = normalize(g_i + 0.12 a_i), g unit-norm Gaussian directions (the other rows of b
    are such directions alone); weights wr, wc > 0 summing to 1/2 each (``equal_weights``: 1 / (2 n)), ``zero_frac`` of them zero."""
    rng = np.random.default_rng([seed, n, m, d])
    nz = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    a = nz(rng.standard_normal((n, d)))
    b = nz(rng.standard_normal((m, d)))
    b[offset:offset + n] = nz(b[offset:offset + n] + 0.12 * a)
    if equal_weights:
        wr = np.full(n, 0.5 / n)
        wc = np.full(n, 0.5 / n)
    else:
        wr = rng.random(n) + 0.25
        wc = rng.random(n) + 0.25
        wr[rng.random(n) < zero_frac] = 0.0
        wc[rng.random(n) < zero_frac] = 0.0
        wr *= 0.5 / max(wr.sum(), 1e-30)
        wc *= 0.5 / max(wc.sum(), 1e-30)
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    return f(a), f(b), f(wr), f(wc)


def _lse_bound(z, ez, dim, stages):
    """(lse, softmax, bound on a computed lse) of z along dim, as derived in the module docstring"""
    lse = torch.logsumexp(z, dim=dim, keepdim=True)
    p = torch.exp(z - lse)
    M = z.max(dim=dim, keepdim=True).values
    terms = z.shape[dim]
    exp_rel = EXP_ULPS * 2.0 * U
    rho = stages * (exp_rel + 2.0 * U) + 2.0 * U * ((z - M).abs() + 4.0 * ez) + exp_rel
    R = (p * rho).sum(dim=dim, keepdim=True) + gamma(terms + stages)
    pert = torch.log((p * torch.exp(ez)).sum(dim=dim, keepdim=True))
    bound = pert - torch.log1p(-R) + LOG_ULPS * 2.0 * U * (lse - M).abs() + 2.0 * U * lse.abs() + U * M.abs()
    return lse.squeeze(dim), p, bound.squeeze(dim)


def reference(a, b, scale, wr, wc=None, offset=0, g=1.0):
    """float64 values and per-element bounds: {"loss", "da", "db", "dscale", "lse_row", "lse_col"} -> (value, bound)."""
    a64, b64, wr64 = _d(a), _d(b), _d(wr)
    scale, g = float(scale), float(g)
    n, d = a64.shape
    m = b64.shape[0]
    assert 0 <= offset and n + offset <= m
    idx = torch.arange(n)
    t = idx + offset
    s = a64 @ b64.t()
    A = a64.abs() @ b64.abs().t()
    z = scale * s
    ez = (1.0 + U) * abs(scale) * gamma(d) * A + U * z.abs()
    stages = math.ceil(max(n, m) / TILE) + 66
    exp_rel = EXP_ULPS * 2.0 * U
    hit = torch.zeros(n, m, dtype=F64)
    hit[idx, t] = 1.0
    zt, ezt = z[idx, t], ez[idx, t]

    lse_r, p, e_lse_r = _lse_bound(z, ez, 1, stages)
    terms = wr64 * (lse_r - zt)
    e_terms = wr64.abs() * (e_lse_r + ezt + 2.0 * U * (lse_r - zt).abs())
    G = wr64[:, None] * (p - hit)
    eG = wr64.abs()[:, None] * (p * torch.expm1(ez + e_lse_r[:, None] + 2.0 * U * (z - lse_r[:, None]).abs() + exp_rel) + 3.0 * U * (p - hit).abs())
    out = {"lse_row": (lse_r, e_lse_r)}
    if wc is not None:
        wc64 = _d(wc)
        lse_c, q, e_lse_c = _lse_bound(z, ez, 0, stages)
        wcol = torch.zeros(m, dtype=F64)
        wcol[t] = wc64
        tc = wc64 * (lse_c[t] - zt)
        terms = terms + tc
        e_terms = e_terms + wc64.abs() * (e_lse_c[t] + ezt + 2.0 * U * (lse_c[t] - zt).abs()) + U * terms.abs()
        G = G + wcol[None, :] * (q - hit)
        eG = eG + wcol.abs()[None, :] * (q * torch.expm1(ez + e_lse_c[None, :] + 2.0 * U * (z - lse_c[None, :]).abs() + exp_rel)
                                         + 3.0 * U * (q - hit).abs())
        out["lse_col"] = (lse_c, e_lse_c)
    eG = eG + U * G.abs()
    L = terms.sum()
    out["loss"] = (L, e_terms.sum() + (n + 4) * U * terms.abs().sum() + U * L.abs() + FLOOR)
    c = g * scale
    da = c * (G @ b64)
    db = c * (G.t() @ a64)
    Gm = G.abs() + eG
    out["da"] = (da, abs(c) * (eG @ b64.abs() + gamma(m + 2) * (Gm @ b64.abs())) + 2.0 * U * da.abs() + FLOOR)
    out["db"] = (db, abs(c) * (eG.t() @ a64.abs() + gamma(n + 2) * (Gm.t() @ a64.abs())) + 2.0 * U * db.abs() + FLOOR)
    ds = g * (G * s).sum()
    out["dscale"] = (ds, abs(g) * ((eG * s.abs() + Gm * gamma(d) * A).sum() + (n + m + 4) * U * (G * s).abs().sum()) + U * ds.abs() + FLOOR)
    return out


def worst(got, ref_bound):
    """max over elements of |got - ref| / bound (inf for a NaN or a wrong inf)"""
    ref, bound = ref_bound
    got = _d(got).reshape(ref.shape)
    assert bool((bound > 0).all())
    e = (got - ref).abs() / bound
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, math.inf))
    e = torch.where(got == ref, torch.zeros_like(e), e)
    return float(e.max())


# ------------------------------------------------------------------------------------------------ f32 restatement of the kernel
def _fma_scores(a, b, skip=None):
    """s[i, j] = the f32 chain acc = fmaf(a[i, k], b[j, k], acc) over k (the product is exact in float64; the one float64 addition before
    the f32 rounding can differ from a true fma only by a double rounding, 2^-29 ulp).  skip = (column tile, k0): that tile's columns
    miss the k-step [k0, k0 + 32)."""
    n, d = a.shape
    m = b.shape[0]
    acc = np.zeros((n, m), dtype=np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for k in range(d):
        nxt = (acc.astype(np.float64) + a64[:, k:k + 1] * b64[None, :, k]).astype(np.float32)
        if skip is not None and skip[1] <= k < skip[1] + KSTEP:
            j0 = skip[0] * TILE
            nxt[:, j0:j0 + TILE] = acc[:, j0:j0 + TILE]
        acc = nxt
    return acc


def _online_lse(z, drop_tile=None):
    """f32 online (max, sum) over 64-column tiles of z [rows, cols] -> lse [rows]"""
    f = np.float32
    rows, cols = z.shape
    mx = np.full(rows, -np.inf, dtype=f)
    sm = np.zeros(rows, dtype=f)
    for ct, j0 in enumerate(range(0, cols, TILE)):
        if ct == drop_tile:
            continue
        blk = z[:, j0:j0 + TILE]
        nm = np.maximum(mx, blk.max(axis=1))
        with np.errstate(invalid="ignore"):
            fac = np.where(mx == nm, f(1), np.exp((mx - nm).astype(f))).astype(f)
        s = (sm * fac).astype(f)
        e = np.exp((blk - nm[:, None]).astype(f)).astype(f)
        for c in range(e.shape[1]):
            s = (s + e[:, c]).astype(f)
        mx, sm = nm, s
    return (mx + np.log(sm).astype(f)).astype(f)


def _merge(m1, s1, m2, s2):
    """cl_merge in f32: (m1, s1) + (m2, s2) of two partial log-sum-exps"""
    f = np.float32
    M = np.maximum(m1, m2)
    with np.errstate(invalid="ignore"):
        e1 = np.where(m1 == M, f(1), np.exp((m1 - M).astype(f))).astype(f)
        e2 = np.where(m2 == M, f(1), np.exp((m2 - M).astype(f))).astype(f)
    return M, ((s1 * e1).astype(f) + (s2 * e2).astype(f)).astype(f)


def split_lse(z, nsplit, fault=None):
    """The forward as launched: workgroup y of ``nsplit`` walks the 64-column tiles y, y + nsplit, ... of the f32 logits z [rows, cols]
    with the online (max, sum) of ``_online_lse`` and the partials are merged in order.  fault in {None, "no_rescale", "inverse",
    "restart"}: the carried sum is not rescaled when the maximum rises, is rescaled by exp(nm - mx), or is dropped at every trip."""
    f = np.float32
    rows, cols = z.shape
    tiles = -(-cols // TILE)
    M = S = None
    for y in range(nsplit):
        mx = np.full(rows, -np.inf, dtype=f)
        sm = np.zeros(rows, dtype=f)
        for ct in walked_tiles(tiles, nsplit, y):
            blk = z[:, ct * TILE:(ct + 1) * TILE]
            nm = np.maximum(mx, blk.max(axis=1))
            with np.errstate(invalid="ignore", over="ignore"):
                arg = (nm - mx) if fault == "inverse" else (mx - nm)
                fac = np.where(mx == nm, f(1), np.exp(arg.astype(f))).astype(f)
            if fault == "no_rescale":
                fac = np.ones(rows, dtype=f)
            if fault == "restart":
                fac = np.zeros(rows, dtype=f)
            with np.errstate(invalid="ignore", over="ignore"):
                s = (sm * fac).astype(f)
            e = np.exp((blk - nm[:, None]).astype(f)).astype(f)
            for c in range(e.shape[1]):
                s = (s + e[:, c]).astype(f)
            mx, sm = nm, s
        M, S = (mx, sm) if M is None else _merge(M, S, mx, sm)
    return (M + np.log(S).astype(f)).astype(f)


# ---- ordered scores on the first trip shape: b[j] = c_j u + noise with every a[i] close to u, so that the order of c fixes the order of
# the tile maxima a workgroup meets, and with it which branch of nm = max(mx, tmax), sm * exp(mx - nm) each of its trips takes
ORDERS = ("rising", "falling", "peak")
ORDER_SCALE = 3.0         # a trip (64 tiles on) moves the tile maximum by about 2: the carried sum stays a visible part of the new one
ORDER_MARGIN = 1e-3       # on float64 logits of size <= 4; the f32 logits differ from them by less than 1e-5 (``reference``'s ez)


def ordered_problem(order):
    n, m, d, off = TRIP_SHAPES[0]
    rng = np.random.default_rng([77, ORDERS.index(order)])
    u = np.array([2.0, -1.0, 2.0]) / 3.0
    pos = np.arange(m) / (m - 1.0)
    c = {"rising": 2.0 * pos - 1.0, "falling": 1.0 - 2.0 * pos, "peak": 1.0 - 4.0 * np.abs(pos - 0.5)}[order]
    a = u + 0.3 * rng.standard_normal((n, d)) / np.sqrt(d)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = c[:, None] * u + 0.02 * rng.standard_normal((m, d))
    _, _, wr, wc = make_problem(n, m, d, seed=78, offset=off)
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a, b, np.float32(ORDER_SCALE), wr, wc, off


def trip_maxima(a, b, scale):
    """[y] -> float64 array [trips of workgroup y, n]: the maximum of every row of the float64 logits over each tile that workgroup y of
    the a side walks, in its order"""
    z = float(scale) * a.astype(np.float64) @ b.astype(np.float64).T
    p = plan(a.shape[0], b.shape[0])
    tmax = np.stack([z[:, j0:j0 + TILE].max(axis=1) for j0 in range(0, b.shape[0], TILE)])      # [tiles, n]
    return [tmax[walked_tiles(p["tiles_a"], p["split_a"], y)] for y in range(p["split_a"])]


def assert_trip_order(order, walks):
    """the condition on the inputs: what the tile maxima of every row do from trip to trip of every workgroup"""
    assert sorted({len(w) for w in walks}) == [2, 3]
    for w in walks:
        step = np.diff(w, axis=0)
        if order == "rising":                      # every trip raises the maximum of every row: the carried sum is rescaled each time
            assert (step > ORDER_MARGIN).all()
        elif order == "falling":                   # no trip after the first raises it: the factor is 1, the new terms are the small ones
            assert (step < -ORDER_MARGIN).all()
        elif len(w) == 3:                          # up, then down
            assert (step[0] > ORDER_MARGIN).all() and (step[1] < -ORDER_MARGIN).all()
    if order == "peak":
        assert sum(len(w) == 3 for w in walks) == 3
    assert float(np.abs(np.concatenate(walks)).max()) <= 4.0


def emulate(a, b, scale, wr, wc=None, offset=0, g=1.0, fault=None):
    """The kernel's arithmetic in numpy f32: the fmaf chain, z = scale * s, an online max / sum over 64-column tiles, a backward that adds
    the tiles of the other side in order.  fault in {None, "tile", "kstep", "partner", "weight"} injects the named defect."""
    f = np.float32
    a, b, wr = (np.asarray(x, dtype=f) for x in (a, b, wr))
    wc = None if wc is None else np.asarray(wc, dtype=f)
    scale, g = f(scale), f(g)
    n, d = a.shape
    m = b.shape[0]
    if fault == "weight":
        assert wc is not None
        wr, wc = wc, wr
    tiles = (m + TILE - 1) // TILE
    s = _fma_scores(a, b, skip=(0, KSTEP if d > KSTEP else 0) if fault == "kstep" else None)
    z = (scale * s).astype(f)
    idx = np.arange(n)
    t = idx + offset
    if fault == "partner":
        t = (t + 1) % m
    hit = np.zeros((n, m), dtype=f)
    hit[idx, t] = 1
    zt = z[idx, t]
    lse_r = _online_lse(z, drop_tile=(1 if tiles > 1 else 0) if fault == "tile" else None)
    terms = (wr * (lse_r - zt).astype(f)).astype(f)
    G = (wr[:, None] * (np.exp((z - lse_r[:, None]).astype(f)).astype(f) - hit).astype(f)).astype(f)
    if wc is not None:
        lse_c = _online_lse(np.ascontiguousarray(z.T))
        terms = (terms + (wc * (lse_c[t] - zt).astype(f)).astype(f)).astype(f)
        wcol = np.zeros(m, dtype=f)
        wcol[t] = wc
        G = (G + (wcol[None, :] * (np.exp((z - lse_c[None, :]).astype(f)).astype(f) - hit).astype(f)).astype(f)).astype(f)
    L = f(0)
    for v in terms:
        L = f(L + v)
    c = f(g * scale)
    da = np.zeros((n, d), dtype=f)
    for j0 in range(0, m, TILE):
        da = (da + G[:, j0:j0 + TILE] @ b[j0:j0 + TILE]).astype(f)
    db = np.zeros((m, d), dtype=f)
    for i0 in range(0, n, TILE):
        db = (db + G[i0:i0 + TILE].T @ a[i0:i0 + TILE]).astype(f)
    ds = f(g * (G * s).astype(f).sum(axis=1, dtype=f).sum(dtype=f))
    return {"loss": L, "da": (c * da).astype(f), "db": (c * db).astype(f), "dscale": ds}


def torch_losses(a, b, scale, wr, wc=None, offset=0):
    """The same value from F.cross_entropy on explicit logits (torch, the inputs' dtype): what the ATen path of coem.py composes."""
    import torch.nn.functional as F
    z = scale * a @ b.t()
    n = a.shape[0]
    labels = torch.arange(n) + offset
    L = (F.cross_entropy(z, labels, reduction="none") * wr).sum()
    if wc is not None:
        L = L + (F.cross_entropy(z.t()[offset:offset + n], torch.arange(n), reduction="none") * wc).sum()
    return L
