"""Planted NaN / Inf: the helpers and the rules of tests/test_gpu_nonfinite.py (a helper module, not a conftest;
tests/test_cpu_nonfinite.py shows on the CPU that every rule is float64's and that check() sees what it is for).

Two claims of the kernels on the training path are checked with one exact instrument:
  1. a non-finite value is never dropped: one NaN planted in one element of one input reaches EXACTLY the output elements the
     operation's arithmetic carries it to (a rule below: index arithmetic on shapes, no reference is run), and every other output
     element keeps the bits of the clean run;
  2. whatever lies past the edge of an operand reads as zero: every input is a view into a NaN-filled buffer (embed), so that a load
     past the edge that is later multiplied by zero or masked by a product turns into a NaN (0 * NaN is NaN where 0 * finite is 0).

The ref_* functions restate each operation in float64 with plain torch ops on whatever device the operands live on; they are what the
CPU module holds the rules against and what the Inf plants (whose sets legitimately differ: inf - inf, 0 * inf) are compared with.
"""
import math

import torch

NAN = float("nan")
INF = float("inf")


# ------------------------------------------------------------------------------------------------------------------ helpers
def embed(x, pad_rows=3, pad_cols=8, fill=NAN, flat=False, device=None):
    """x on `device` as a view into a larger buffer filled with `fill`; the buffer is the view's ._base.
    2-D form: the buffer is [pad_rows + M + pad_rows, W + pad_cols], the view its rows pad_rows .. pad_rows + M and its columns 0 .. W:
    leading dimension W + pad_cols, `fill` to the right of every row, pad_rows rows of it above and below.  W and pad_cols are
    multiples of 8 elements, so every row starts 16-byte aligned.
    Flat form (flat=True, or x not 2-D; for packed tensors and for the entry points whose wrappers take no leading dimension):
    x contiguous between pad_rows * x.shape[-1] elements (rounded up to a multiple of 64) of `fill` before and after."""
    x = torch.as_tensor(x)
    device = x.device if device is None else device
    assert x.is_floating_point()
    if flat or x.dim() != 2:
        n = x.numel()
        pad = (max(1, pad_rows) * x.shape[-1] + 63) // 64 * 64
        buf = torch.full((pad + n + pad,), fill, dtype=x.dtype, device=device)
        view = buf[pad:pad + n].view(x.shape)
        view.copy_(x)
        return view
    M, W = x.shape
    assert pad_cols > 0 and pad_cols % 8 == 0 and W % 8 == 0, (W, pad_cols)
    buf = torch.full((M + 2 * pad_rows, W + pad_cols), fill, dtype=x.dtype, device=device)
    view = buf[pad_rows:pad_rows + M, :W]
    view.copy_(x)
    return view


def plant(x, index, value):
    """a copy of x (same device, same strides class: contiguous) with one element replaced"""
    y = x.clone()
    y[tuple(index) if isinstance(index, (tuple, list)) else index] = value
    return y


def _bits(t):
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _first(mask):
    return tuple(int(i) for i in torch.nonzero(mask)[0].tolist())


def _same_bits_outside(tag, got_clean, got_bad, m, loose=None):
    differs = (_bits(got_clean) != _bits(got_bad)) & ~m
    if loose is not None:
        differs &= ~loose.to(differs.device)
    if bool(differs.any()):
        i = _first(differs)
        raise AssertionError(f"{tag}: element {i} is outside the planted value's reach and differs from the clean run: "
                             f"{float(got_bad[i])!r} (bits {int(_bits(got_bad)[i])}) vs {float(got_clean[i])!r} (bits "
                             f"{int(_bits(got_clean)[i])}); {int(differs.sum())} such elements")


def check(tag, got_clean, got_bad, expect_mask, nonfinite=False, loose=None):
    """1. isnan(got_bad) (~isfinite with nonfinite=True) equals expect_mask element for element;
       2. where expect_mask is false, got_bad holds the bits of got_clean (integer views: -0 and NaN payloads count).
    The message names the first offending index.
    loose: a mask of elements that a documented choice of the kernel lets differ in bits (assertion 1 holds for them all the same)."""
    assert got_clean.shape == got_bad.shape == expect_mask.shape, (tag, got_clean.shape, got_bad.shape, expect_mask.shape)
    assert got_clean.dtype == got_bad.dtype and expect_mask.dtype == torch.bool
    m = expect_mask.to(got_bad.device)
    bad = ~torch.isfinite(got_bad) if nonfinite else torch.isnan(got_bad)
    wrong = bad != m
    if bool(wrong.any()):
        i = _first(wrong)
        what = "a NaN was dropped: the rule expects one" if bool(m[i]) else "a NaN leaked: the rule expects none"
        raise AssertionError(f"{tag}: {what} at element {i} (got {float(got_bad[i])!r}, clean {float(got_clean[i])!r}); "
                             f"{int((wrong & m).sum())} dropped, {int((wrong & ~m).sum())} leaked, {int(m.sum())} expected")
    _same_bits_outside(tag, got_clean, got_bad, m, loose)


def check_weak(tag, got_clean, got_bad, expect_mask, ref_nonfinite, loose=None):
    """The rule of the Inf plants: where the float64 reference has a non-finite element in this tensor (ref_nonfinite), the kernel's
    tensor has at least one; every element outside the NaN-plant rule's mask holds the bits of the clean run."""
    assert got_clean.shape == got_bad.shape == expect_mask.shape, (tag, got_clean.shape, got_bad.shape, expect_mask.shape)
    if ref_nonfinite:
        assert not bool(torch.isfinite(got_bad).all()), f"{tag}: float64 has a non-finite element in this tensor, the kernel has none"
    _same_bits_outside(tag, got_clean, got_bad, expect_mask.to(got_bad.device), loose)


def any_nonfinite(t):
    return not bool(torch.isfinite(t).all())


def draw(shape, seed, scale=1.0, clamp=3.0):
    """Position-dependent values (the model is tests/rowwise.py::draw_inputs): randn whose rows carry a scale that cycles through
    [0.5, 2] and a ramp along the first dimension, clamped to +-clamp so that no drawn value sits in a formula's far tail (below -4.2
    gelu_f is a documented zero: csrc/common.hpp) and none is exactly representable as zero by accident of the draw."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    n = torch.arange(shape[0], dtype=torch.float32).view(-1, *([1] * (len(shape) - 1)))
    x = x * torch.exp2(2.0 * ((n * 0.381966) % 1.0) - 1.0) + (n + 0.5) / shape[0] - 0.5
    x = x.clamp(-clamp, clamp) * scale
    return torch.where(x == 0, torch.full_like(x, 0.25 * scale), x)


# ------------------------------------------------------------------------------------------------------------------ rules
def _m(*shape):
    return torch.zeros(shape, dtype=torch.bool)


def rule_linear_fwd(M, N, what, idx, rows_per_scale=1):
    """y = x w^T + b (+ epilogue), every output [M, N] (pre and act of the gelu mode, out of the residual modes) the same set:
    x[i, k] -> row i; w[j, k], bias[j] -> column j; res[i, j] -> that element; rowscale[s] -> the rows of its group."""
    m = _m(M, N)
    if what == "x":
        m[idx[0]] = True
    elif what in ("w", "bias"):
        m[:, idx[0]] = True
    elif what == "res":
        m[idx[0], idx[1]] = True
    elif what == "rowscale":
        m[idx[0] * rows_per_scale:(idx[0] + 1) * rows_per_scale] = True
    else:
        raise ValueError(what)
    return m


def rule_linear_dgrad(M, K, what, idx):
    """dx = dy w (x gelu'(pre)), colsum = the column sums of dx: dy[i, n] -> row i of dx and the whole colsum; w[n, k] -> column k of
    dx and colsum[k]; pre[i, k] -> dx[i, k] and colsum[k]."""
    dx, cs = _m(M, K), _m(K)
    if what == "dy":
        dx[idx[0]] = True
        cs[:] = True
    elif what == "w":
        dx[:, idx[1]] = True
        cs[idx[1]] = True
    elif what == "pre":
        dx[idx[0], idx[1]] = True
        cs[idx[1]] = True
    else:
        raise ValueError(what)
    return {"dx": dx, "colsum": cs}


def rule_dgrad_delta(M, K, H, HD, what, idx):
    """dx = dy w, delta[i, h] = -sum over head h's HD columns of dx o: o[i, c] -> delta[i, c // HD] only; dy[i, n] -> row i of dx
    and of delta; w[n, k] -> column k of dx and column k // HD of delta."""
    dx, de = _m(M, K), _m(M, H)
    if what == "o":
        de[idx[0], idx[1] // HD] = True
    elif what == "dy":
        dx[idx[0]] = True
        de[idx[0]] = True
    elif what == "w":
        dx[:, idx[1]] = True
        de[:, idx[1] // HD] = True
    else:
        raise ValueError(what)
    return {"dx": dx, "delta": de}


def rule_wgrad(N, K, what, idx):
    """gw[N, K] += dy^T x, gb[N] += colsum(dy): dy[m, n] -> row n of gw and gb[n]; x[m, k] -> column k of gw, gb untouched."""
    gw, gb = _m(N, K), _m(N)
    if what == "dy":
        gw[idx[1]] = True
        gb[idx[1]] = True
    elif what == "x":
        gw[:, idx[1]] = True
    else:
        raise ValueError(what)
    return {"gw": gw, "gb": gb}


def rule_attn_fwd(B, H, N, HD, what, idx):
    """idx = (b, n, h, d) of the packed qkv [B, N, 3, H, HD].  q -> o[b, n, h, :] and lse[b, h, n]; k -> o[b, :, h, :] and
    lse[b, h, :]; v -> o[b, :, h, d] only.  o is [B, N, H, HD], lse [B, H, N]."""
    b, n, h, d = idx
    o, lse = _m(B, N, H, HD), _m(B, H, N)
    if what == "q":
        o[b, n, h] = True
        lse[b, h, n] = True
    elif what == "k":
        o[b, :, h] = True
        lse[b, h] = True
    elif what == "v":
        o[b, :, h, d] = True
    else:
        raise ValueError(what)
    return {"o": o, "lse": lse}


def attn_fwd_wave_rows(B, H, N, HD, idx):
    """The elements of o and lse that a planted q[b, n, h, d] may change in BITS without reaching them: the other query rows of the same
    wave of the online-max forward, rows 32 (n // 32) ... + 31 of (b, h).  That kernel defers the rescale of its accumulators until
    `!__all(ex <= RESCALE_SLACK)` (csrc/attn.hip, "Deferred rescale (wave-uniform, ...)"): the decision is taken for the 32 query
    rows of a wave together, a NaN row answers it with "rescale" at every tile, and its 31 neighbours then shift their own maxima at
    tiles where the clean run left them -- the same softmax, rounded at another reference point.  NaN set and finiteness hold."""
    b, n, h, _ = idx
    lo = n // ATTN_FWD_WAVE_ROWS * ATTN_FWD_WAVE_ROWS
    o, lse = _m(B, N, H, HD), _m(B, H, N)
    o[b, lo:lo + ATTN_FWD_WAVE_ROWS, h] = True
    lse[b, h, lo:lo + ATTN_FWD_WAVE_ROWS] = True
    return {"o": o, "lse": lse}


# the query rows one wave of attn_fwd_kernel owns, aligned: the kernel's own statement of it, which tests/test_cpu_nonfinite.py looks
# up in csrc/attn.hip so that a change of the kernel's row assignment fails there, not as a puzzle on the GPU
ATTN_FWD_WAVE_ROWS = 32
ATTN_FWD_WAVE_ROWS_SOURCE = "const int q0 = bc.x * 128 + wid * 32;"


def rule_attn_bwd(B, H, N, HD, what, idx):
    """The mask of dqkv [B, N, 3, H, HD] for given qkv, o, lse: dO[b, n, h, d] -> dV[b, :, h, d], dQ[b, n, h, :], dK[b, :, h, :];
    o[b, n, h, d] (or delta[b N + n, h] in the delta= form) -> dQ[b, n, h, :] and dK[b, :, h, :]; lse[b, h, n] -> those and
    dV[b, :, h, :].  idx is (b, n, h, d) for dO / o, (b, h, n) for lse, (b N + n, h) for delta."""
    m = _m(B, N, 3, H, HD)
    if what == "lse":
        b, h, n = idx
    elif what == "delta":
        (b, n), h = divmod(idx[0], N), idx[1]
    else:
        b, n, h, d = idx
    m[b, n, 0, h] = True
    m[b, :, 1, h] = True
    if what == "dO":
        m[b, :, 2, h, d] = True
    elif what == "lse":
        m[b, :, 2, h] = True
    elif what not in ("o", "delta"):
        raise ValueError(what)
    return m


def rule_ln_fwd(M, D, what, idx):
    """x[i, k] -> row i of y, mean[i], rstd[i]; gamma[k], beta[k] -> column k of y."""
    y, mean, rstd = _m(M, D), _m(M), _m(M)
    if what == "x":
        y[idx[0]] = True
        mean[idx[0]] = True
        rstd[idx[0]] = True
    elif what in ("gamma", "beta"):
        y[:, idx[0]] = True
    else:
        raise ValueError(what)
    return {"y": y, "mean": mean, "rstd": rstd}


def rule_ln_apply(M, D, what, idx):
    """y rebuilt from saved statistics: x[i, k] -> that element; mean[i], rstd[i] -> row i; gamma[k], beta[k] -> column k."""
    y = _m(M, D)
    if what == "x":
        y[idx[0], idx[1]] = True
    elif what in ("mean", "rstd"):
        y[idx[0]] = True
    elif what in ("gamma", "beta"):
        y[:, idx[0]] = True
    else:
        raise ValueError(what)
    return {"y": y}


def rule_ln_bwd(M, D, what, idx):
    """x[i, k] planted BEFORE the forward (mean[i] and rstd[i] are then NaN as well) -> row i of dx, all of dgamma, dbeta untouched;
    dy[i, k] -> row i of dx, dgamma[k], dbeta[k]; gamma[k] -> every row of dx, dgamma and dbeta untouched; dres[i, k] -> dx[i, k].
    dxsum is the column sum of dx: the columns dx has a NaN in."""
    dx, dg, db = _m(M, D), _m(D), _m(D)
    if what == "x":
        dx[idx[0]] = True
        dg[:] = True
    elif what == "dy":
        dx[idx[0]] = True
        dg[idx[1]] = True
        db[idx[1]] = True
    elif what == "gamma":
        dx[:] = True
    elif what == "dres":
        dx[idx[0], idx[1]] = True
    else:
        raise ValueError(what)
    return {"dx": dx, "dgamma": dg, "dbeta": db, "dxsum": dx.any(0)}


def _pool_used(T, cls):
    used = torch.zeros(T, dtype=torch.bool)
    if cls:
        used[0] = True
    else:
        used[1:] = True
    return used


def rule_slice_pool_fwd(B, S, T, D, cls, what, idx):
    """The composition of tests/slicehead_ref.py::slice_pool: pooled row r = token 0 (cls) or the mean of tokens 1 .. T-1 of slice r,
    LayerNorm, mean over the S slices of a volume.  x[r, t, k] with t a token the pooling uses -> pooled[r, k], mean[r], rstd[r] and
    out[r // S, :]; with a token it does not use -> nothing; gamma[k], beta[k] -> column k of out."""
    out, pooled, mean, rstd = _m(B, D), _m(B * S, D), _m(B * S), _m(B * S)
    if what == "x":
        r, t, k = idx
        if bool(_pool_used(T, cls)[t]):
            pooled[r, k] = True
            mean[r] = True
            rstd[r] = True
            out[r // S] = True
    elif what in ("gamma", "beta"):
        out[:, idx[0]] = True
    else:
        raise ValueError(what)
    return {"out": out, "pooled": pooled, "mean": mean, "rstd": rstd}


def rule_slice_pool_bwd(B, S, T, D, cls, what, idx):
    """The LayerNorm-backward rules per pooled group, spread over the tokens the pooling uses (the others get exact zeros):
    x[r, t, k] planted before the forward (a used token) -> dx[r, used, :] and all of dgamma, dbeta untouched; dout[b, k] ->
    dx[r, used, :] for the S slices r of volume b, dgamma[k], dbeta[k]; gamma[k] -> dx[:, used, :], dgamma and dbeta untouched."""
    dx, dg, db = _m(B * S, T, D), _m(D), _m(D)
    used = _pool_used(T, cls)
    if what == "x":
        r, t, k = idx
        if bool(used[t]):
            dx[r, used] = True
            dg[:] = True
    elif what == "dout":
        b, k = idx
        dx[b * S:(b + 1) * S, used] = True
        dg[k] = True
        db[k] = True
    elif what == "gamma":
        dx[:, used] = True
    else:
        raise ValueError(what)
    return {"dx": dx, "dgamma": dg, "dbeta": db, "dxsum": dx.any(0).any(0)}


# ---- token and loss kernels (csrc/tokens.hip): row-local gathers and scatters, one widening / add / cast per element, so a plant reaches
# single elements -- column k of exactly the destination rows the index tables (CPU integer tensors) map its source row to
def _rows(n_rows, width, rows, k):
    m = _m(n_rows, width)
    for r in rows:
        m[r, k] = True
    return m


def rule_enc_assemble(B, nkeep, D, ids_keep, what, idx):
    """x[b, 0] = cls + pos_cls, x[b, 1 + i] = tok[b nkeep + i] + pos[ids_keep[b, i]]; x is [B (nkeep + 1), D]"""
    R = nkeep + 1
    if what == "tok":
        b, i = divmod(idx[0], nkeep)
        rows = [b * R + 1 + i]
    elif what == "pos":
        rows = [b * R + 1 + i for b in range(B) for i in range(nkeep) if int(ids_keep[b, i]) == idx[0]]
    elif what in ("cls", "pos_cls"):
        rows = [b * R for b in range(B)]
    else:
        raise ValueError(what)
    return _rows(B * R, D, rows, idx[-1])


def rule_dec_assemble(B, nkeep, L, D, ids_restore, emb_has_cls, what, idx):
    """x[b, 1 + j] = (emb[b, r] if r = ids_restore[b, j] < nkeep else mask_token) + dpos[j]; x[b, 0] = dcls + dpos_cls, or
    emb[b, 0] + dpos_cls where emb carries a cls row of its own (emb_has_cls); x is [B (L + 1), D]"""
    R, erows = L + 1, nkeep + emb_has_cls
    if what == "emb":
        b, r = divmod(idx[0], erows)
        r -= emb_has_cls
        rows = [b * R] if r < 0 else [b * R + 1 + j for j in range(L) if int(ids_restore[b, j]) == r]
    elif what == "mask_token":
        rows = [b * R + 1 + j for b in range(B) for j in range(L) if int(ids_restore[b, j]) >= nkeep]
    elif what == "dpos":
        rows = [b * R + 1 + idx[0] for b in range(B)]
    elif what == "dpos_cls" or (what == "dcls" and not emb_has_cls):
        rows = [b * R for b in range(B)]
    else:
        raise ValueError(what)
    return _rows(B * R, D, rows, idx[-1])


def rule_patch_gather(B, C, T, H, W, tp, p, nkeep, ids, idx):
    """imgs[b, c, f, y, x] -> element ((c tp + u) p + py) p + px of the row of the token (f // tp, y // p, x // p), where ids[b]
    keeps that token; nothing where it does not.  out is [B nkeep, C tp p p]."""
    b, c, f, y, x = idx
    gh, gw = H // p, W // p
    l = ((f // tp) * gh + y // p) * gw + x // p
    e = ((c * tp + f % tp) * p + y % p) * p + x % p
    return _rows(B * nkeep, C * tp * p * p, [b * nkeep + i for i in range(nkeep) if int(ids[b, i]) == l], e)


def rule_gather_rows(B, n, D, ids, idx):
    """out[b n + i] = cast(src[b, 1 + ids[b, i]]) (ids None: the identity); the cls row src[b, 0] reaches nothing"""
    b, r, k = idx
    return _rows(B * n, D, [b * n + i for i in range(n) if (i if ids is None else int(ids[b, i])) == r - 1], k)


def rule_scatter_add_rows(B, nkeep, L, D, ids_restore, idx):
    """out[l] (+)= sum over the samples b with ids_restore[b, l] < nkeep of src[b, 1 + ids_restore[b, l]]; src[b, 0] reaches nothing"""
    b, r, k = idx
    return _rows(L, D, [l for l in range(L) if r >= 1 and int(ids_restore[b, l]) == r - 1], k)


def rule_dec_assemble_bwd(B, nkeep, L, D, ids_restore, idx):
    """ddpos[l] = sum_b dx[b, 1 + l]; part[l] = the same over the samples that MASK l (a select, not a product: a kept sample's
    NaN does not reach it); the cls row dx[b, 0] reaches nothing"""
    b, r, k = idx
    rows = [r - 1] if r >= 1 else []
    return {"ddpos": _rows(L, D, rows, k), "part": _rows(L, D, [l for l in rows if int(ids_restore[b, l]) >= nkeep], k)}


def rule_mse(B, C, T, H, W, u, p, norm_pix, what, idx):
    """loss_tok [B, L] and dpred [B (L + 1), PD] (row 0 of a sample = cls) for pred [B, L + 1, PD] and imgs [B, C, T, H, W], every
    frame predicted: pred[b, 1 + l, e] -> loss_tok[b, l] and dpred[b, 1 + l, e]; imgs[b, c, f, y, x] -> the token l it lies in:
    loss_tok[b, l] and its one element of that dpred row, or with norm_pix (the token's mean and variance) the whole row; the cls
    row pred[b, 0] -> nothing.
    The mask does not enter: the forward kernel knows none, and dpred = coef * mask * (pred - target) is NaN for mask = 0 as well --
    0 * NaN, as in the float64 gradient of forward_loss's (loss * mask).sum() / mask.sum() (tests/test_cpu_nonfinite.py shows it)."""
    gh, gw = H // p, W // p
    L, PD = (T // u) * gh * gw, u * p * p * C
    lt, dp = _m(B, L), _m(B * (L + 1), PD)
    if what == "pred":
        b, r, e = idx
        if r >= 1:
            lt[b, r - 1] = True
            dp[b * (L + 1) + r, e] = True
    elif what == "imgs":
        b, c, f, y, x = idx
        l = ((f // u) * gh + y // p) * gw + x // p
        lt[b, l] = True
        if norm_pix:
            dp[b * (L + 1) + 1 + l] = True
        else:
            dp[b * (L + 1) + 1 + l, ((f % u * p + y % p) * p + x % p) * C + c] = True
    else:
        raise ValueError(what)
    return {"loss_tok": lt, "dpred": dp}


def rule_optim(lengths, t, i):
    """A non-finite g[t][i]: sumsq[t] non-finite and the others untouched; in the update exactly element i of p, m, v and of the 16-bit
    mirror of tensor t."""
    sq = _m(len(lengths))
    sq[t] = True
    el = [_m(n) for n in lengths]
    el[t][i] = True
    return {"sumsq": sq, "elements": el}


# ------------------------------------------------------------------------------------------------------------------ float64
def _d(t):
    return None if t is None else t.double()


def gelu64(x):
    """x Phi(x); at x = -inf the limit -0, not the -inf * 0 of the formula: an overflowed pre-activation activates to zero, the
    choice csrc/common.hpp documents above gelu_f ("the product is taken with 0 there")"""
    return torch.where(x == -INF, torch.zeros_like(x), x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def ref_linear_fwd(x, w, bias, res=None, rowscale=None, rows_per_scale=1, gelu=False):
    y = _d(x) @ _d(w).t()
    if bias is not None:
        y = y + _d(bias)
    if gelu:
        return {"pre": y, "act": gelu64(y)}
    if rowscale is not None:
        y = _d(rowscale).repeat_interleave(rows_per_scale).unsqueeze(1) * y
    if res is not None:
        y = _d(res) + y
    return {"out": y}


def ref_linear_dgrad(dy, w, pre=None):
    dx = _d(dy) @ _d(w)
    if pre is not None:
        dx = dx * dgelu64(_d(pre))
    return {"dx": dx, "colsum": dx.sum(0)}


def ref_dgrad_delta(dy, w, o, H, HD):
    dx = _d(dy) @ _d(w)
    return {"dx": dx, "delta": -(dx * _d(o)).view(dx.shape[0], H, HD).sum(-1)}


def ref_wgrad(dy, x, gw0, gb0):
    return {"gw": _d(gw0) + _d(dy).t() @ _d(x), "gb": _d(gb0) + _d(dy).sum(0)}


def _qkv(qkv, B, N, H, HD):
    return _d(qkv).view(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)           # q, k, v [B, H, N, HD]


def ref_attn_fwd(qkv, B, N, H, HD):
    """o [B, N, H, HD] and lse [B, H, N]: softmax(q k^T / sqrt(HD)) v in float64"""
    q, k, v = _qkv(qkv, B, N, H, HD)
    s = (q @ k.transpose(-2, -1)) * HD ** -0.5
    return {"o": (s.softmax(-1) @ v).transpose(1, 2), "lse": torch.logsumexp(s, -1)}


def ref_attn_bwd(qkv, o, do, lse, B, N, H, HD, delta=None):
    """dqkv [B, N, 3, H, HD] from qkv, dO and the saved o and lse (or delta = -rowsum(dO o) in place of o), as the kernels are handed
    them: P = exp(s - lse), dV = P^T dO, dS = P (dO V^T + delta), dQ = dS K / sqrt(HD), dK = dS^T Q / sqrt(HD)."""
    q, k, v = _qkv(qkv, B, N, H, HD)
    dO = _d(do).view(B, N, H, HD).transpose(1, 2)
    sc = HD ** -0.5
    p = torch.exp((q @ k.transpose(-2, -1)) * sc - _d(lse).unsqueeze(-1))
    if delta is None:
        dl = -(dO * _d(o).view(B, N, H, HD).transpose(1, 2)).sum(-1)
    else:
        dl = _d(delta).view(B, N, H).transpose(1, 2)
    ds = p * (dO @ v.transpose(-2, -1) + dl.unsqueeze(-1))
    dq, dk, dv = (ds @ k) * sc, (ds.transpose(-2, -1) @ q) * sc, p.transpose(-2, -1) @ dO
    return torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4)


def ref_ln_fwd(x, gamma, beta, eps):
    x = _d(x)
    mean = x.mean(-1)
    rstd = (x.var(-1, unbiased=False) + eps).rsqrt()
    return {"y": (x - mean.unsqueeze(-1)) * rstd.unsqueeze(-1) * _d(gamma) + _d(beta), "mean": mean, "rstd": rstd}


def ref_ln_apply(x, mean, rstd, gamma, beta):
    return {"y": (_d(x) - _d(mean).unsqueeze(-1)) * _d(rstd).unsqueeze(-1) * _d(gamma) + _d(beta)}


def ref_ln_bwd(dy, x, mean, rstd, gamma, dres=None):
    """the backward from the saved statistics, as octmae_layernorm_bwd is handed them"""
    xh = (_d(x) - _d(mean).unsqueeze(-1)) * _d(rstd).unsqueeze(-1)
    g = _d(dy) * _d(gamma)
    dx = _d(rstd).unsqueeze(-1) * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + _d(dres)
    return {"dx": dx, "dgamma": (_d(dy) * xh).sum(0), "dbeta": _d(dy).sum(0), "dxsum": dx.sum(0)}


def ref_slice_pool(x, gamma, beta, dout, S, cls, eps):
    """forward and autograd backward of the pooling head on x [B S, T, D] (tests/slicehead_ref.py::slice_pool)"""
    xd, gd, bd = (_d(t).detach().clone().requires_grad_(True) for t in (x, gamma, beta))
    D = x.shape[-1]
    p = xd[:, 0] if cls else xd[:, 1:].mean(dim=1)
    mean = p.mean(-1)
    rstd = (p.var(-1, unbiased=False) + eps).rsqrt()
    yn = (p - mean.unsqueeze(-1)) * rstd.unsqueeze(-1) * gd + bd
    out = yn.view(-1, S, D).mean(dim=1)
    out.backward(_d(dout))
    return {"out": out.detach(), "pooled": p.detach(), "mean": mean.detach(), "rstd": rstd.detach(), "dx": xd.grad, "dgamma": gd.grad,
            "dbeta": bd.grad, "dxsum": xd.grad.sum(dim=(0, 1))}


def ref_adamw(p, g, m, v, gscale, lr, b1, b2, eps, wd, step):
    """one AdamW step in float64 on flat tensors (decoupled decay, bias correction as torch.optim.AdamW)"""
    p, g, m, v = _d(p), _d(g) * gscale, _d(m), _d(v)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p * (1 - lr * wd) - lr * (m / (1 - b1 ** step)) / ((v / (1 - b2 ** step)).sqrt() + eps)
    return {"p": p, "m": m, "v": v}


# ---- token and loss kernels; ids are integer tensors on the operands' device
def ref_enc_assemble(tok, pos, cls, pos_cls, ids_keep):
    B, nkeep = ids_keep.shape
    D = tok.shape[-1]
    x = torch.cat([(_d(cls) + _d(pos_cls)).expand(B, 1, D), _d(tok).view(B, nkeep, D) + _d(pos)[ids_keep]], 1)
    return x.reshape(-1, D)


def ref_dec_assemble(emb, mask_token, dpos, dcls, dpos_cls, ids_restore, nkeep, emb_has_cls):
    B, L = ids_restore.shape
    D = emb.shape[-1]
    e = _d(emb).view(B, nkeep + emb_has_cls, D)
    seq = torch.cat([e[:, emb_has_cls:], _d(mask_token).expand(B, L - nkeep, D)], 1)
    body = torch.gather(seq, 1, ids_restore.unsqueeze(-1).expand(-1, -1, D)) + _d(dpos)
    first = (e[:, 0] if emb_has_cls else _d(dcls).expand(B, D)) + _d(dpos_cls)
    return torch.cat([first.unsqueeze(1), body], 1).reshape(-1, D)


def ref_patch_gather(imgs, ids, tp, p):
    B, C, T, H, W = imgs.shape
    gt, gh, gw = T // tp, H // p, W // p
    kdim = C * tp * p * p
    full = _d(imgs).view(B, C, gt, tp, gh, p, gw, p).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, gt * gh * gw, kdim)
    return torch.gather(full, 1, ids.unsqueeze(-1).expand(-1, -1, kdim)).reshape(-1, kdim)


def ref_gather_rows(src, ids, n):
    B, _, D = src.shape
    idx = torch.arange(n, device=src.device).expand(B, n) if ids is None else ids
    return torch.gather(_d(src)[:, 1:], 1, idx.unsqueeze(-1).expand(-1, -1, D)).reshape(-1, D)


def ref_scatter_add_rows(src, ids_restore, nkeep, prior=None):
    """a sample takes part in row l by a select on ids_restore[b, l] < nkeep, as in tests/test_gpu_tokens.py"""
    B, L = ids_restore.shape
    out = torch.zeros(L, src.shape[-1], dtype=torch.float64, device=src.device) if prior is None else _d(prior)
    for b in range(B):
        rows = _d(src)[b, 1 + ids_restore[b].clamp(max=nkeep - 1)]
        out = torch.where((ids_restore[b] < nkeep).unsqueeze(1), out + rows, out)
    return out


def ref_dec_assemble_bwd(dx, ids_restore, nkeep):
    body = _d(dx)[:, 1:]
    return {"ddpos": body.sum(0), "part": torch.where((ids_restore >= nkeep).unsqueeze(-1), body, torch.zeros_like(body)).sum(0)}


def mse_diff(pred, imgs, cfg):
    """pred - target of oracle/mae3d_ref.py::forward_loss (every frame predicted), float64 [B, L, PD]"""
    from oracle import mae3d_ref as O
    target = O.patchify(_d(imgs), cfg)
    if cfg.norm_pix_loss:
        target = (target - target.mean(-1, keepdim=True)) / (target.var(-1, keepdim=True) + 1.0e-6) ** 0.5
    return _d(pred)[:, 1:] - target


def ref_mse(pred, imgs, mask, coef, cfg):
    """loss_tok [B, L] and dpred [B (L + 1), PD] = coef * mask * (pred - target) with a zero cls row, as octmae_mse_bwd states it"""
    d = mse_diff(pred, imgs, cfg)
    B, L, PD = d.shape
    body = float(coef) * _d(mask).view(B, L, 1) * d
    return {"loss_tok": (d ** 2).mean(-1), "dpred": torch.cat([torch.zeros_like(body[:, :1]), body], 1).reshape(-1, PD)}
