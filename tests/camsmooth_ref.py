"""References for the eigen-smoothed CAM and the augmentation fold of csrc/saliency.hip (a helper, not a conftest; no GPU):

  planted(L, C, ratio, seed)        an input whose centred weighted activations have the singular values ratio^i
  eigen_ref64(A, w, n_prefix)       the float64 oracle: numpy's SVD per sample, the sign rule, sigma2 / sigma1
  residual64(A, w, n_prefix, v)     ||Mc^T Mc v - lambda v|| / lambda in float64 for a given direction
  eigen_model32(A, w, n_prefix, k)  the iteration of include/octmae.h (octmae_cam_eigen) restated operation by operation in float32
  eigen_bound(model_err)            what a float32 implementation with another summation order may be off the oracle
  accumulate_ref64 / accumulate_bound   the fold of octmae_cam_accumulate in float64 and its rounding bound

tests/test_cpu_camsmooth.py checks these against each other; tests/test_gpu_camsmooth.py holds the kernels to them."""
import numpy as np

F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24          # unit roundoff of fp32
FLOOR = 2.0 ** -20        # of the relative map error: sixteen roundings of the largest value


def planted(L, C, ratio, seed):
    """(A float32 [L, C], w float32 [C]) with  w o A = U diag(ratio^i) V^T + (a constant per column):
    U [L, k] orthonormal and orthogonal to the all-ones direction (k = min(L - 1, C): centring removes nothing from it), V [C, k]
    orthonormal, w of magnitudes in [0.5, 2] with random signs, and an N(0, 1) offset on every column of A, which centring must remove.
    The float32 rounding of A moves the singular values a little: eigen_ref64 measures what they are."""
    g = np.random.default_rng(seed)
    k = min(L - 1, C)
    w = g.uniform(0.5, 2.0, C) * g.choice([-1.0, 1.0], C)
    off = g.standard_normal(C)
    if k == 0:
        return (np.zeros((L, C)) + off).astype(F32), w.astype(F32)
    X = g.standard_normal((L, k))
    X -= X.mean(0, keepdims=True)
    U, _ = np.linalg.qr(X)
    U -= U.mean(0, keepdims=True)                      # QR keeps the column space; this only removes rounding
    V, _ = np.linalg.qr(g.standard_normal((C, k)))
    Mc = (U * ratio ** np.arange(k)) @ V.T
    return (Mc / w + off).astype(F32), w.astype(F32)


def planted_batch(B, L, C, ratio, seed, n_prefix=0, prefix_value=3e38):
    """float32 A [B, n_prefix + L, C], w [B, C]: B planted samples; the prefix rows hold +-prefix_value (they must never be read)"""
    A = np.empty((B, n_prefix + L, C), F32)
    w = np.empty((B, C), F32)
    for b in range(B):
        A[b, n_prefix:], w[b] = planted(L, C, ratio, 1000 * seed + b)
        A[b, :n_prefix] = prefix_value if b % 2 == 0 else -prefix_value
    return A, w


MIN_MARGIN = 0.05


def decided_batch(B, L, C, ratio, n_prefix=0):
    """planted_batch of the first seed (1, 2, ...) at which the sign rule is decided in every sample: where the projection is all but
    orthogonal to the centred plain CAM, float32 rounding picks the sign, and neither sign is wrong.  -> (A, w, per-sample oracles)"""
    for seed in range(1, 50):
        A, w = planted_batch(B, L, C, ratio, seed, n_prefix)
        refs = [eigen_ref64(A[b], w[b], n_prefix) for b in range(B)]
        if min(r[4] for r in refs) >= MIN_MARGIN:
            return A, w, refs
    raise AssertionError((B, L, C, ratio))


# gap 0.8, (L, C, seed of planted_batch(3, ...)): inputs on which two iterations are visibly too few.  The residual after two iterations
# depends on how well the uniform start happens to be aligned with v1, so the seeds are chosen -- tests/test_cpu_camsmooth.py checks on
# the float32 model that every sample sits 1.5 x above the GPU test's threshold after 2 iterations and 4 x below it after 32.
ITER_CASES = [(5, 4, 2), (257, 64, 4), (64, 1024, 5), (1280, 256, 5)]
RES_FEW, RES_MANY = 5e-2, 1e-4


def _centred64(A, w, n_prefix):
    M = w.astype(F64)[None, :] * A[n_prefix:].astype(F64)
    return M - M.mean(0, keepdims=True)


def eigen_ref64(A, w, n_prefix=0):
    """One sample in float64: (proj [L], v1 [C], sigma1, sigma2 / sigma1, sign margin).  proj = Mc v1 with the sign that makes
    sum_l proj[l] (Mc 1)[l] >= 0; the margin is that sum over (||proj|| ||Mc 1||), which must be well away from 0 for the sign of a
    float32 computation to be decided.  Mc == 0: zeros, ratio 0, margin 1."""
    Mc = _centred64(A, w, n_prefix)
    L, C = Mc.shape
    if not Mc.any():
        return np.zeros(L), np.full(C, C ** -0.5), 0.0, 0.0, 1.0
    _, s, Vt = np.linalg.svd(Mc, full_matrices=False)
    v = Vt[0]
    p = Mc @ v
    c1 = Mc.sum(1)
    d = float(p @ c1)
    if d < 0:
        p, v, d = -p, -v, -d
    margin = d / (np.linalg.norm(p) * np.linalg.norm(c1)) if c1.any() else 1.0
    return p, v, float(s[0]), float(s[1] / s[0]) if len(s) > 1 else 0.0, float(margin)


def residual64(A, w, n_prefix, v):
    Mc = _centred64(A, w, n_prefix)
    p = Mc @ v.astype(F64)
    lam = float(p @ p)
    if lam == 0.0:
        return 0.0
    return float(np.linalg.norm(Mc.T @ p - lam * v) / lam)


def _rowdots(X, q):
    """sum_c q[c] X[r, c] for every row r, float32 products and float32 sums, every row in the same order"""
    return (X * q[None, :]).sum(axis=1, dtype=F32)


def eigen_model32(A, w, n_prefix, iters, relu=False):
    """One sample, every operation in float32, in the order of octmae.h: (cam [L], residual, v [C]).  The sums are numpy's (pairwise),
    not the kernels' (lanes, waves, row splits): the two agree to rounding, not bit for bit."""
    A = np.ascontiguousarray(A[n_prefix:], F32)
    w = w.astype(F32)
    L, C = A.shape
    abar = (A.sum(axis=0, dtype=F32) / F32(L)).astype(F32)
    X = np.vstack([A, abar[None, :]])                  # abar as one more row: its dot with q is summed in the order of the rows'

    def rows(q):
        r = _rowdots(X, q)
        return (r[:-1] - r[-1]).astype(F32)

    def transposed(u):
        return (w * ((u[:, None] * A).sum(axis=0, dtype=F32) - abar * u.sum(dtype=F32))).astype(F32)

    v = np.full(C, F32(1.0) / np.sqrt(F32(C)), F32)
    bad = False
    with np.errstate(all="ignore"):
        c1 = rows(w)
        for _ in range(iters):
            t = transposed(rows(v * w))
            nrm = np.sqrt((t * t).sum(dtype=F32))
            if not np.isfinite(nrm):
                bad = True
            elif nrm > 0:
                v = (t / nrm).astype(F32)
        u = rows(v * w)
        t = transposed(u)
        lam = (u * u).sum(dtype=F32)
        d = t - lam * v
        res = F32(0.0) if lam == 0 else np.sqrt((d * d).sum(dtype=F32)) / lam
        if bad or not np.isfinite(lam) or not np.isfinite(res):
            res = F32(np.nan)
        p = -u if (u * c1).sum(dtype=F32) < 0 else u
    return (np.maximum(p, F32(0.0)) if relu else p).astype(F32), float(res), v


def map_error(p, p64):
    """max_l |p - p64| / max |p64|; 0 where both are all zero"""
    top = float(np.abs(p64).max())
    err = float(np.abs(p.astype(F64) - p64).max())
    return err / top if top > 0 else err


def eigen_bound(model_err):
    """The float32 model's own error against the oracle on this input measures what float32 arithmetic costs there; another order of the
    same sums may cost a few times that (8 x), and no float32 map is held to less than sixteen roundings of its largest value."""
    return max(8.0 * model_err, FLOOR)


def model_bound(A, w, n_prefix, sigma1, rho, iters):
    """What the float32 MODEL itself may be off the oracle, relative to max |proj| (first order, rounding errors adding as a random walk):
    every proj[l] is the difference of two C-term sums of products q[c] A[l, c] with |q| ~ C^-1/2, so its absolute rounding error is about
    u32 r, r the rms of |w o A|; max |proj| is at least sigma1 / sqrt(L); the direction v is computed from sums with the same relative
    errors and a perturbation E of Mc turns the first singular vector by about ||E|| / (sigma1 - sigma2) (Wedin), which adds the factor
    1 / (1 - rho).  16 = the operations in a row of the chain (mean, two dots, the transposed sum, its fold, the norm) with a margin of
    two.  Plus what `iters` iterations leave of the other directions, at most sqrt(C) rho^(2 iters) from the uniform start."""
    r = float(np.sqrt(np.mean((w.astype(F64)[None, :] * A[n_prefix:].astype(F64)) ** 2)))
    L = A.shape[0] - n_prefix
    return 16.0 * U32 * r * np.sqrt(L) / sigma1 * (1.0 + 1.0 / (1.0 - rho)) + 10.0 * np.sqrt(A.shape[1]) * rho ** (2 * iters)


# ---- the augmentation fold ------------------------------------------------------------------------------------------------------------
EPS32 = float(F32(1e-7))


def accumulate_ref64(acc, cam, width, flip, weight, first):
    """float64 [B, n]: acc (first ? = : +=) weight (cam' - min) / (1e-7f + (max - min)) per sample, cam' with every row of `width`
    mirrored when flip; weight as the float32 the kernel receives"""
    cam = cam.astype(F64)
    B, n = cam.shape
    mn, mx = cam.min(1, keepdims=True), cam.max(1, keepdims=True)
    v = (cam - mn) / (EPS32 + (mx - mn))
    if flip:
        v = v.reshape(B, n // width, width)[:, :, ::-1].reshape(B, n)
    v = float(F32(weight)) * v
    return v if first else acc.astype(F64) + v


def accumulate_bound(acc, cam, weight, first):
    """|kernel - float64|: the difference, the denominator (two roundings), the quotient and the product are one rounding each of a
    value of at most |weight| (5 roundings, relatively), the sum one more of the result: 6 u32 (|weight| + |acc| + |weight|), and the
    smallest normal on top so that an exact zero has a positive bound."""
    wt = abs(float(F32(weight)))
    a = 0.0 if first else np.abs(acc.astype(F64))
    return 6.0 * U32 * (2.0 * wt + a) + 1e-37
