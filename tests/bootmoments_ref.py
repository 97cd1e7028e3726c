"""numpy / fractions.Fraction restatement of the two kernels of octcubem_amd/csrc/bootmoments.hip and of the float64 finish of
octcubem_amd.metrics.bootstrap_regression_measures -- independent of octcubem_amd -- with the error bounds the tests assert.

Stage 1 (``unit_moments``): F[u][c][0..7] = count, sum a, sum b, sum a^2, sum b^2, sum a b, sum e^2, sum |e| over the valid samples of
unit u in ascending sample index, a = x - cx[c], b = y - cy[c], e = y - x in float64.  ``unit_moments_exact`` gives the same sums,
and the sums of the magnitudes of their terms, in exact rational arithmetic on the float32 inputs and the float64 centre.
Stage 2 (``product``): D[r][j] = sum_u mult[r][u] F[u][j], restated lane by lane: 16 resamples and one 16-column tile per
v_mfma_f64_16x16x4_f64, A[l & 15][k = l >> 4], B[k = l >> 4][l & 15], C/D col = lane & 15, row = (lane >> 4) + 4 * reg, units in
ascending steps of 4 inside parts of ``split`` units, the parts added in ascending order; rows past R, units past the part and columns
at or past 8 C enter as literal zeros.  ``product_exact`` is the exact integer-times-float product.

The bounds, u = 2^-53.  They are derived here, not measured.

UNIT_BOUND(s) = (s + 6) u, relative to the sum of the magnitudes of the terms of an entry.  A term is formed from exact float32 ->
float64 conversions by at most three roundings (the difference a or b or e; the product; nothing else: |e| and the count are exact),
fused or not: relative error at most (1 + u)^3 - 1 < 3 u + 3 u^2.  The s terms of a unit are added one after the other: s - 1 additions
(the first lands on 0 exactly), each term passing through at most s - 1 of them: (1 + u)^(s - 1) - 1 < (s - 1) u + ... .  Together
below (s + 2) u + O(s^2 u^2); (s + 6) u leaves four units for the second-order terms, which need s^2 u < 4, i.e. s < 2^27.

PRODUCT_BOUND(U) = (U + 2) u, relative to sum_u mult |F|.  The standard inner-product bound: gamma_n = n u / (1 - n u) for n terms,
whatever the order of the additions and whether a product is rounded on its own or fused into the addition.  The int32 -> float64
conversion of a multiplicity is exact.  The parts add one more level of additions to the same sum, which the "any order" covers
(every term still passes through fewer than U additions: 256 k-steps of a part plus the parts before it).  U + 2 over U leaves the
1 / (1 - U u) factor, for U < 2^24.

END TO END (``finish_bound``).  The finish of the kernel's D against the finish of the exact D (exact stage 1, exact product, rounded
once).  Every D_k of the kernel is within eps = (s_max + 6 + U + 2) u of the exact one, relative to A_k = sum w |term|.  For the
positive sums A_k = D_k (k = 0, 3, 4, 6, 7); by Cauchy-Schwarz A_1 <= sqrt(W D3), A_2 <= sqrt(W D4), A_5 <= sqrt(D3 D4).  To first order
  dSxx <= eps (D3 + 2 |D1| A_1 / W) <= 3 eps D3,   dSyy <= 3 eps D4,   dSxy <= eps (A_5 + (|D1| A_2 + |D2| A_1) / W) <= 3 eps sqrt(D3 D4)
  d pearsonr <= dSxy / sqrt(Sxx Syy) + |r| / 2 (dSxx / Sxx + dSyy / Syy) <= 3 eps (sqrt(kx ky) + |r| (kx + ky) / 2)
  d R2 <= 2 |r| d pearsonr
  d r2 <= (D6 / Syy) (eps + 3 eps ky)
  d sum e <= eps (A_1 + A_2 + |cy - cx| W),   dV <= eps D6 + 2 |sum e| d(sum e) / W   for V = D6 - (sum e)^2 / W
  d explained_variance <= dV / Syy + |V| / Syy * 3 eps ky
  d mse <= 2 eps mse,   d mae <= 2 eps mae      (numerator and W)
with the amplifications kx = D3 / Sxx and ky = D4 / Syy computed PER RESAMPLE from the exact D, never assumed.  The asserted bound is
SLACK = 2 times the first-order bound plus 8 u: one factor covers (a) the finish's own roundings, made once on each side -- about four
roundings in front of each cancelling difference, so at most 8 u k, against eps k with eps >= 10 u -- and (b) the second-order terms,
which are eps k times the first-order ones; ``finish_bound`` refuses (returns inf) where eps k > 2^-7, so they stay below 1 % of it.
The 8 u cover the last division, square root and subtraction of results that are at most about 1 in magnitude (mse / mae: relative).

``fault=`` of ``product`` plants one mistake of such a kernel: "drop_last_kstep" (the last k-step of every part is skipped),
"transpose_cd" (the result registers are stored through the transposed C/D map) and "pad_multiplied" (columns at or past 8 C are
loaded from F's pad instead of entering as zeros)."""
import os
import re
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53
FAULTS = ("drop_last_kstep", "transpose_cd", "pad_multiplied")
KEYS = ("pearsonr", "r2", "explained_variance", "mse", "mae", "R2")
SLACK = 2.0


def UNIT_BOUND(s):
    return (s + 6) * U53


def PRODUCT_BOUND(U):
    return (U + 2) * U53


def kernel_constants():
    """BM_ROWS, BM_TILES, BM_SPLIT, BM_WAVES as csrc/bootmoments.hip defines them: the shapes of the tests follow the source."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "octcubem_amd", "csrc", "bootmoments.hip")).read()
    block = int(re.search(r"^constexpr int BM_BLOCK = (\d+);", src, re.M).group(1))
    rows, tiles, split = (int(re.search(rf"^constexpr int {name} = (\d+);", src, re.M).group(1)) for name in ("BM_ROWS", "BM_TILES", "BM_SPLIT"))
    return rows, tiles, split, block // 64


def limits():
    """(largest C, R, U) the launchers accept, from the source."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "octcubem_amd", "csrc", "bootmoments.hip")).read()
    c = int(re.search(r"^constexpr int BM_MAX_C = (\d+);", src, re.M).group(1))
    r, u = (1 << int(re.search(rf"^constexpr long long {name} = 1ll << (\d+);", src, re.M).group(1)) for name in ("BM_MAX_R", "BM_MAX_U"))
    return c, r, u


def cpad8(C):
    return (8 * C + 15) // 16 * 16


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _units(n, unit, U):
    """The sample indices of every unit, ascending."""
    if unit is None:
        return [[i] for i in range(n)]
    unit = _np(unit).astype(np.int64)
    members = [[] for _ in range(U)]
    for i, g in enumerate(unit):
        members[int(g)].append(i)
    return members


def column_means(pred, target, valid=None):
    """float64 [2, C]: the mean of the valid entries of each column (0 for a column without one)."""
    x, y = _np(pred).astype(np.float64), _np(target).astype(np.float64)
    v = np.ones(x.shape, dtype=bool) if valid is None else _np(valid) != 0
    cnt = np.maximum(v.sum(0), 1)
    return np.stack([np.where(v, x, 0.0).sum(0) / cnt, np.where(v, y, 0.0).sum(0) / cnt])


def unit_moments(pred, target, U, unit=None, valid=None, centre=None):
    """float64 [U, C, 8]: stage 1 in numpy, each (unit, column) summed sequentially in ascending sample index, products unfused."""
    x, y = _np(pred).astype(np.float64), _np(target).astype(np.float64)
    n, C = x.shape
    v = np.ones((n, C), dtype=bool) if valid is None else _np(valid) != 0
    c = _np(centre).astype(np.float64)
    F = np.zeros((U, C, 8))
    for u, members in enumerate(_units(n, unit, U)):
        for i in members:
            a, b, e = x[i] - c[0], y[i] - c[1], y[i] - x[i]
            terms = np.stack([np.ones(C), a, b, a * a, b * b, a * b, e * e, np.abs(e)], axis=1)
            F[u] += np.where(v[i][:, None], terms, 0.0)
    return F


def unit_moments_exact(pred, target, U, unit=None, valid=None, centre=None):
    """(sums, magnitudes): two [U][C][8] nested lists of Fractions, the exact sums and the sums of the magnitudes of their terms."""
    x, y = _np(pred), _np(target)
    assert x.dtype == np.float32 and y.dtype == np.float32
    n, C = x.shape
    v = np.ones((n, C), dtype=bool) if valid is None else _np(valid) != 0
    c = _np(centre).astype(np.float64)
    sums = [[[Fraction(0)] * 8 for _ in range(C)] for _ in range(U)]
    mags = [[[Fraction(0)] * 8 for _ in range(C)] for _ in range(U)]
    for u, members in enumerate(_units(n, unit, U)):
        for i in members:
            for j in range(C):
                if not v[i, j]:
                    continue
                fx, fy = Fraction(float(x[i, j])), Fraction(float(y[i, j]))
                a, b, e = fx - Fraction(float(c[0, j])), fy - Fraction(float(c[1, j])), fy - fx
                for k, t in enumerate((Fraction(1), a, b, a * a, b * b, a * b, e * e, abs(e))):
                    sums[u][j][k] += t
                    mags[u][j][k] += abs(t)
    return sums, mags


def unit_mismatches(F, pred, target, U, unit=None, valid=None, centre=None):
    """The entries of a stage-1 output ``F`` [U, C, 8] outside UNIT_BOUND of the exact sums: a list of (u, c, k, got, want)."""
    F = _np(F)
    n, C = _np(pred).shape
    sums, mags = unit_moments_exact(pred, target, U, unit, valid, centre)
    sizes = [len(m) for m in _units(n, unit, U)]
    bad = []
    for u in range(U):
        for j in range(C):
            for k in range(8):
                got = Fraction(float(F[u, j, k])) if np.isfinite(F[u, j, k]) else None
                if got is None or abs(got - sums[u][j][k]) > Fraction(UNIT_BOUND(sizes[u])) * mags[u][j][k]:
                    bad.append((u, j, k, float(F[u, j, k]), float(sums[u][j][k])))
    return bad


def product(mult, Fpad, cols, fault=None, split=None):
    """float64 [R, Cpad8]: stage 2 lane by lane.  ``Fpad`` [U, Cpad8] is the padded stage-1 output AS IT LIES IN MEMORY (the pad need
    not be zero: a correct kernel does not read it), ``cols`` = 8 C."""
    assert fault is None or fault in FAULTS
    rows, _, ksplit, _ = kernel_constants()
    split = split or ksplit
    mult, Fpad = _np(mult), _np(Fpad).astype(np.float64)
    R, U = mult.shape
    width = Fpad.shape[1]
    assert Fpad.shape[0] == U and width % 16 == 0 and width - 16 < cols <= width and rows == 16
    lane = np.arange(64)
    idx, grp = lane & 15, lane >> 4
    D = np.zeros((R, width))
    for r0 in range(0, R, 16):
        for t in range(width // 16):
            total = None
            for ubeg in range(0, U, split):
                uend = min(U, ubeg + split)
                acc = np.zeros((16, 16))
                steps = list(range(ubeg, uend, 4))
                if fault == "drop_last_kstep":
                    steps = steps[:-1]
                for u0 in steps:
                    u = u0 + grp
                    inside = u < uend
                    row_in = r0 + idx < R
                    a = np.where(row_in & inside, mult[np.minimum(r0 + idx, R - 1), np.minimum(u, U - 1)].astype(np.float64), 0.0)
                    col = t * 16 + idx
                    live = inside & ((col < cols) | (fault == "pad_multiplied"))
                    b = np.where(live, Fpad[np.minimum(u, U - 1), col], 0.0)
                    A = np.zeros((16, 4))
                    B = np.zeros((4, 16))
                    A[idx, grp] = a
                    B[grp, idx] = b
                    for k in range(4):                          # the instruction's own k order is not specified: any order is in the bound
                        acc = acc + A[:, k:k + 1] * B[k:k + 1, :]
                total = acc if total is None else total + acc
            for reg in range(4):
                for ln in range(64):
                    row, col = (ln >> 4) + 4 * reg, ln & 15
                    val = total[col, row] if fault == "transpose_cd" else total[row, col]
                    if r0 + row < R:
                        D[r0 + row, t * 16 + col] = val
    return D


def product_exact(mult, F):
    """(sums, magnitudes): [R][J] nested lists of Fractions, sum_u mult[r][u] F[u][j] and sum_u mult[r][u] |F[u][j]| for the float64
    ``F`` [U, J] (flattened over its trailing axes)."""
    mult, F = _np(mult), _np(F).astype(np.float64)
    F = F.reshape(F.shape[0], -1)
    frac = [[Fraction(float(v)) for v in row] for row in F]
    sums, mags = [], []
    for r in range(mult.shape[0]):
        nz = np.nonzero(mult[r])[0]
        s, m = [Fraction(0)] * F.shape[1], [Fraction(0)] * F.shape[1]
        for u in nz:
            w = int(mult[r, u])
            for j, f in enumerate(frac[u]):
                s[j] += w * f
                m[j] += w * abs(f)
        sums.append(s)
        mags.append(m)
    return sums, mags


def product_mismatches(D, mult, F):
    """The entries of ``D`` [R, J...] outside PRODUCT_BOUND of the exact product of ``mult`` and the float64 ``F``: (r, j, got, want)."""
    D = _np(D)
    D = D.reshape(D.shape[0], -1)
    sums, mags = product_exact(mult, F)
    bound = Fraction(PRODUCT_BOUND(_np(mult).shape[1]))
    bad = []
    for r in range(D.shape[0]):
        for j in range(D.shape[1]):
            if not np.isfinite(D[r, j]) or abs(Fraction(float(D[r, j])) - sums[r][j]) > bound * mags[r][j]:
                bad.append((r, j, float(D[r, j]), float(sums[r][j])))
    return bad


def exact_moments(pred, target, mult, unit=None, valid=None, centre=None):
    """float64 [R, C, 8]: exact stage 1, exact product, rounded once."""
    mult = _np(mult)
    R, U = mult.shape
    C = _np(pred).shape[1]
    sums, _ = unit_moments_exact(pred, target, U, unit, valid, centre)
    D = np.zeros((R, C, 8))
    for r in range(R):
        nz = np.nonzero(mult[r])[0]
        for j in range(C):
            for k in range(8):
                D[r, j, k] = float(sum((int(mult[r, u]) * sums[u][j][k] for u in nz), Fraction(0)))
    return D


def moments(pred, target, mult, unit=None, valid=None, centre=None, fault=None):
    """A function of the signature of ops.bootstrap_moments on host arrays (or CPU tensors): the two restatements chained."""
    x, y = _np(pred).astype(np.float32), _np(target).astype(np.float32)
    mult = _np(mult)
    R, U = mult.shape
    C = x.shape[1]
    centre = column_means(x, y, valid) if centre is None else _np(centre).astype(np.float64)
    F = unit_moments(x, y, U, unit, valid, centre)
    Fpad = np.zeros((U, cpad8(C)))
    Fpad[:, :8 * C] = F.reshape(U, 8 * C)
    D = product(mult, Fpad, 8 * C, fault=fault)
    return {"moments": D[:, :8 * C].reshape(R, C, 8), "centre": centre, "unit_moments": F}


def tau(n):
    return (n + 8) * 2.0 ** -50


def finish(D, centre, n):
    """The float64 finish: dict of the six keys, float64 [R, C], NaN where undefined (mse / mae: W == 0 only; the other four: W < 2,
    Sxx <= tau D3 or Syy <= tau D4)."""
    D, c = _np(D).astype(np.float64), _np(centre).astype(np.float64)
    out = {k: np.full(D.shape[:2], np.nan) for k in KEYS}
    for r in range(D.shape[0]):
        for j in range(D.shape[1]):
            W, D1, D2, D3, D4, D5, D6, D7 = (float(v) for v in D[r, j])
            if W == 0:
                continue
            out["mse"][r, j], out["mae"][r, j] = D6 / W, D7 / W
            sxx, syy, sxy = D3 - D1 * D1 / W, D4 - D2 * D2 / W, D5 - D1 * D2 / W
            if W < 2 or sxx <= tau(n) * D3 or syy <= tau(n) * D4:
                continue
            se = D2 - D1 + (c[1, j] - c[0, j]) * W
            rr = max(-1.0, min(1.0, sxy / float(np.sqrt(sxx * syy))))
            out["pearsonr"][r, j], out["R2"][r, j] = rr, rr * rr
            out["r2"][r, j], out["explained_variance"][r, j] = 1.0 - D6 / syy, 1.0 - (D6 - se * se / W) / syy
    return out


def finish_bound(D, centre, s_max, U):
    """The END TO END bound of the module docstring per key, float64 [R, C], from the exact ``D`` [R, C, 8]: inf where the first-order
    treatment does not apply (an undefined resample, or eps k > 2^-7)."""
    D, c = _np(D).astype(np.float64), _np(centre).astype(np.float64)
    eps = (s_max + 6 + U + 2) * U53
    W, D1, D2, D3, D4, D5, D6, D7 = (D[:, :, k] for k in range(8))
    with np.errstate(invalid="ignore", divide="ignore"):
        sxx, syy, sxy = D3 - D1 * D1 / W, D4 - D2 * D2 / W, D5 - D1 * D2 / W
        kx, ky = D3 / sxx, D4 / syy
        r = np.clip(sxy / np.sqrt(sxx * syy), -1, 1)
        A1, A2 = np.sqrt(W * D3), np.sqrt(W * D4)
        dr = 3 * eps * (np.sqrt(kx * ky) + np.abs(r) * (kx + ky) / 2)
        se = D2 - D1 + (c[1] - c[0])[None, :] * W
        dse = eps * (A1 + A2 + np.abs(c[1] - c[0])[None, :] * W)
        V = D6 - se * se / W
        dV = eps * D6 + 2 * np.abs(se) * dse / W
        first = {"pearsonr": dr, "R2": 2 * np.abs(r) * dr, "r2": (D6 / syy) * (eps + 3 * eps * ky),
                 "explained_variance": dV / syy + np.abs(V) / syy * 3 * eps * ky, "mse": 2 * eps * D6 / W, "mae": 2 * eps * D7 / W}
        ok = (W >= 2) & (sxx > 0) & (syy > 0) & (eps * kx <= 2.0 ** -7) & (eps * ky <= 2.0 ** -7)
        tail = {k: 8 * U53 * (np.maximum(D6 / W, 0) if k == "mse" else np.maximum(D7 / W, 0) if k == "mae" else 1.0) for k in KEYS}
    return {k: np.where(ok, SLACK * first[k] + tail[k], np.inf) for k in KEYS}


def materialised(pred, target, mult_row, unit=None, valid=None, c=0):
    """Column c of one resample as two float64 vectors, every sample repeated by its unit's multiplicity (np.repeat)."""
    x, y = _np(pred).astype(np.float64), _np(target).astype(np.float64)
    n = x.shape[0]
    unit = np.arange(n) if unit is None else _np(unit).astype(np.int64)
    reps = _np(mult_row).astype(np.int64)[unit]
    if valid is not None:
        reps = reps * (_np(valid)[:, c] != 0)
    return np.repeat(x[:, c], reps), np.repeat(y[:, c], reps)


class StubDataset:
    preset_label_mean = None
    preset_label_std = None

    def __init__(self, C):
        self.label_mean, self.label_std = [0.5 * j for j in range(C)], [1.0 + 0.25 * j for j in range(C)]


def coem_stub(n=48, C=3, batch=10, device="cpu", constant_column=None):
    """A loader and a stub model for coem_finetune.evaluate with multimodal_type 'oct3d_paired_ir_cls': ``(data, model, args)``.  The
    model reads the logits off the "oct" entry with a fixed linear map; the labels follow it loosely."""
    import types
    import torch
    g = torch.Generator().manual_seed(17)
    feats = torch.rand(n, C, generator=g)
    labels = feats @ (torch.eye(C) + 0.2) + 0.3 * torch.rand(n, C, generator=g)
    if constant_column is not None:
        labels[:, constant_column] = 1.0

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.eye(C) + 0.1)

        def forward(self, oct_volume, image):
            return oct_volume @ self.w, torch.ones((), device=oct_volume.device)

    class Loader(list):
        pass

    items = Loader(({"oct": feats[i:i + batch], "ir": feats[i:i + batch], "label": labels[i:i + batch]},
                    (None, None, (None, torch.arange(i, min(n, i + batch))))) for i in range(0, n, batch))
    items.num_samples, items.dataset = n, StubDataset(C)
    args = types.SimpleNamespace(device=device, rank=0, multimodal_type="oct3d_paired_ir_cls", single_modality=None, fold=-1, val_frequency=1,
                                 epochs=1, save_logs=False, cls_dataset_type="BCVA_and_GAA")
    return types.SimpleNamespace(dataloader=items), Stub().to(device), args
