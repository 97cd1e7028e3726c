"""Float64 reference, per-element error bounds and an fp32 emulation of the multi-tensor optimizer kernels (csrc/optim.hip):
mt_sumsq, mt_finish_norm and mt_adamw_kernel<LP, SQ>.  Plain numpy: tests/test_cpu_optim_model.py validates the bounds with it on the
CPU, tests/test_gpu_optim_kernels.py applies them to the kernels.

Which AdamW the kernel is.  octmae_mt_adamw_fused takes lr, beta1, beta2, eps and weight_decay as C ``float`` and derives bc1 = 1 -
beta1^t and bc2 = 1 - beta2^t from those floats: the kernel is a self-consistent AdamW at fl32(beta), not at the Python double.
fl32(0.999) = 0.99900001287..., so 1 - beta2 differs from 0.001 by 1.3e-5 relative: a reference at the exact 0.999 would show that
1.3e-5 in v as if it were a kernel error.  ref_step therefore rounds every hyper-parameter (and the gradient scale, a device float)
to float32 first and computes in float64 from there; the bias corrections stay un-rounded doubles of fl32(beta).

Error per step, not compounded: ref_step starts from the kernel's OWN fp32 state before the step, cast up.

Bounds.  e = 2^-24 (half an ulp, relative); every count below is the number of fp32 roundings on the path, times a margin of 2.
-ffp-contract=fast fuses a multiply into the add that consumes it, which only REMOVES a rounding, and hipcc's fp32 division and square
root are correctly rounded, one rounding each.  1 - beta is exact in fp32 (Sterbenz: 0.5 <= beta <= 1).
  m = fl(fl(b1 m0) + fl((1-b1) fl(g gs)))           3 roundings on the second term, 2 on the first, at most 4 on either
        |m - m_ref| <= 8 e (|b1 m0| + |(1-b1) g gs|)
  v = fl(fl(b2 v0) + fl(fl((1-b2) gg) gg)), gg = fl(g gs)   <= 5 on the second term (gg enters twice), 2 on the first; all terms >= 0
        |v - v_ref| <= 8 e (b2 v0 + (1-b2) (g gs)^2)
  p = fl(fl(p0 fl(1 - lr wd)) - fl(fl(lr / bc1) fl(m / denom)))   2 roundings relative to p: 4 e |p_ref|; the step u = (lr / bc1) m /
        denom carries bc1, bc2_sqrt (rounded to float by the host), lr / bc1, sqrt, two divisions, + eps and the product: 8 -> 16 e
        |p - p_ref| <= 4 e |p_ref| + 16 e |u_ref|
      NOT counted in the 16 e: the error m and v already carry.  v's is harmless (8 e of a sum of positive terms, halved by the square
      root).  m's is 8 e of |b1 m0| + |(1-b1) g gs|, which exceeds 8 e |m| by the cancellation factor K = (|b1 m0| + |(1-b1) g gs|) /
      |m|, so the bound as written can be missed by an element whose two m terms nearly cancel (K >> 1) AND whose |p| is so small that
      4 e |p_ref| does not cover K e |u|.  ref_step reports K so that a test can say which it was.
  sumsq[t]: every thread adds ceil(min(n, 65536) / 1024) quads (3 roundings + the squares) and a tail element, 6 wave levels, 2 block
      levels, one atomic add per chunk; all terms positive, so the relative error is at most the number of roundings on the longest
      path:  |sumsq - ref| <= (ceil(min(n, 65536) / 256) + 16 + chunks) e ref      (the scalar path adds min(n, 65536) / 256 terms)
  norm = sqrt(sum_t sumsq[t]): ceil(nt / 64) adds per lane, 6 levels, the root (which halves what came before):
        |norm - ref| <= (ceil(nt / 64) + 10) e ref, and the same for clip_coef = min(1, max_norm / (norm + 1e-6)).
"""
import math

import numpy as np

E = 2.0 ** -24
CHUNK = 65536

# one-hot sweep (exact checks): lengths at the vector loop's tail, the 1024-element stride of a workgroup and the chunk seams
SWEEP_LENGTHS = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, 65535, 65536, 65537, 65539, 131072, 131072 + 1029]
# random data and the alignment matrix
RANDOM_LENGTHS = [5, 1027, 65535, 65536, 65539, 131072 + 1029]


def f32(x):
    """the value a C ``float`` argument receives, held in a double"""
    return float(np.float32(x))


def sweep_cases():
    """[(n, index)]: ~40 tensors; over the table the index is 0, 3, 4, n-1, n-2, 4(n//4)-1, 4(n//4), 65535, 65536 and 65537 wherever
    the length allows.  Ordered so that neighbouring tensors differ in length (a write past one tensor's end lands in a guard band,
    a sum credited to the wrong tensor changes two exact values)."""
    kinds = ["0", "3", "4", "n-1", "n-2", "4q-1", "4q", "65535", "65536", "65537"]
    L = len(SWEEP_LENGTHS)
    cases, seen, start = [], set(), 0
    for kind in kinds:
        took = 0
        for j in range(L):
            n = SWEEP_LENGTHS[(start + 5 * j) % L]          # 5 is coprime to 16: every length is tried, neighbours differ
            q = 4 * (n // 4)
            idx = {"0": 0, "3": 3, "4": 4, "n-1": n - 1, "n-2": n - 2, "4q-1": q - 1, "4q": q,
                   "65535": 65535, "65536": 65536, "65537": 65537}[kind]
            if not 0 <= idx < n or (n, idx) in seen:
                continue
            seen.add((n, idx))
            cases.append((n, idx))
            took += 1
            if took == 4:
                start = (start + 5 * j + 5) % L
                break
    for n in SWEEP_LENGTHS:                                   # a length the rotation passed over: its last element
        if all(c[0] != n for c in cases):
            cases.append((n, n - 1))
    return cases


def ref_step(p, g, m, v, gs, step, lr, b1, b2, eps, wd):
    """One AdamW step in float64 from the fp32 state (p, m, v) and the raw gradient g; gs: the gradient scale (None: 1).
    Returns a dict: p, m, v, u (the step) and the per-element bounds bp, bm, bv, plus K (the cancellation factor of m)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    gs = 1.0 if gs is None else f32(gs)
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    gg = g * gs
    t1, t2 = b1 * m, (1.0 - b1) * gg
    m1 = t1 + t2
    s1, s2 = b2 * v, (1.0 - b2) * gg * gg
    v1 = s1 + s2
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = np.sqrt(v1) / math.sqrt(bc2) + eps
    u = (lr / bc1) * (m1 / denom)
    p1 = p * (1.0 - lr * wd) - u
    mag = np.abs(t1) + np.abs(t2)
    with np.errstate(divide="ignore", invalid="ignore"):
        K = np.where(m1 != 0, mag / np.abs(m1), 1.0)
    return {"p": p1, "m": m1, "v": v1, "u": u, "K": K,
            "bp": 4 * E * np.abs(p1) + 16 * E * np.abs(u), "bm": 8 * E * mag, "bv": 8 * E * (s1 + s2)}


def worst(got, ref, bound):
    """(max over elements of |got - ref| / bound, its flat index); a zero bound asks for equality; NaN counts as inf"""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    d = np.abs(got - np.asarray(ref, dtype=np.float64).reshape(-1))
    b = np.asarray(bound, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, d / b, np.where(d == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    if r.size == 0:
        return 0.0, -1
    i = int(np.argmax(r))
    return float(r[i]), i


def check_step(got_p, got_m, got_v, ref, where=""):
    """Assert the three per-element bounds; returns {"p": ratio, "m": ratio, "v": ratio} (measured / bound of the worst element)."""
    out = {}
    for name, got in (("m", got_m), ("v", got_v), ("p", got_p)):
        r, i = worst(got, ref[name], ref["b" + name])
        out[name] = r
        if r > 1.0:
            g_, r_, b_ = (float(np.asarray(a).reshape(-1)[i]) for a in (got, ref[name], ref["b" + name]))
            raise AssertionError(f"{where}{name}[{i}] = {g_!r}, reference {r_!r}: |diff| {abs(g_ - r_):.3e} is {r:.2f} x its bound "
                                 f"{b_:.3e} (cancellation factor of m there: {float(ref['K'].reshape(-1)[i]):.1f})")
    return out


def sumsq_ref(g):
    g = np.asarray(g, dtype=np.float64)
    return float(np.dot(g.reshape(-1), g.reshape(-1)))


def sumsq_factor(n):
    """bound on |sumsq - ref| / (e ref)"""
    chunks = -(-n // CHUNK)
    return -(-min(n, CHUNK) // 256) + 16 + chunks


def norm_factor(nt):
    """bound on |norm - ref| / (e ref) and on |coef - ref| / (e ref) for mt_finish_norm over nt entries"""
    return -(-nt // 64) + 10


def finish_ref(sumsq, max_norm):
    """(norm, coef) in float64 from the fp32 sumsq array the kernel reads; max_norm and the 1e-6 as the floats the kernel holds"""
    norm = math.sqrt(float(np.sum(np.asarray(sumsq, dtype=np.float64))))
    mx = f32(max_norm)
    coef = min(1.0, mx / (norm + f32(1e-6))) if mx > 0 else 1.0
    return norm, coef


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic in numpy fp32
MUTANTS = ("skip_tail", "skip_seam", "unscaled_update", "sumsq_of_scaled", "swap_m_v", "wd_after_step", "bc2_for_bc2_sqrt",
           "beta2_for_beta1", "eps_inside_sqrt")


def _tree(x):
    """butterfly sum of a power-of-two-length fp32 vector, as a wave reduction does it"""
    x = x.astype(np.float32)
    while x.size > 1:
        h = x.size // 2
        x = (x[:h] + x[h:]).astype(np.float32)
    return np.float32(x[0])


def emulate_sumsq_f32(g, skip=()):
    """sumsq of one tensor as mt_sumsq_kernel / mt_adamw_kernel<*, true> accumulate it (16-byte aligned: the vector path): per chunk
    256 threads stride over quads, then the n & 3 tail, wave and block reduction, one atomic add per chunk.  skip: indices left out."""
    g = np.asarray(g, dtype=np.float32).reshape(-1).copy()
    g[list(skip)] = 0.0                       # a skipped element adds nothing (x + 0 is exact)
    total = np.float32(0.0)
    for off in range(0, g.size, CHUNK):
        c = g[off:off + CHUNK]
        n4 = c.size // 4
        q = c[:4 * n4].reshape(n4, 4)
        q = q * q
        t = ((q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])).astype(np.float32)
        rows = -(-max(n4, 1) // 256)
        pad = np.zeros(rows * 256, dtype=np.float32)
        pad[:n4] = t
        s = np.zeros(256, dtype=np.float32)
        for r in pad.reshape(rows, 256):
            s = (s + r).astype(np.float32)
        tail = c[4 * n4:]
        s[:tail.size] = (s[:tail.size] + tail * tail).astype(np.float32)
        w = [_tree(s[64 * k:64 * k + 64]) for k in range(4)]
        total = np.float32(total + np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3])))
    return float(total)


def emulate_step_f32(p, g, m, v, gs, step, lr, b1, b2, eps, wd, mutant=None):
    """adam_one of csrc/optim.hip over one tensor in numpy float32, in the kernel's operation order and without contraction (every
    product rounded).  Returns (p, m, v, sumsq).  mutant: one of MUTANTS -- a planted defect, for tests/test_cpu_optim_model.py."""
    assert mutant is None or mutant in MUTANTS, mutant
    F = np.float32
    p0, g, m0, v0 = (np.asarray(a, dtype=F).reshape(-1) for a in (p, g, m, v))
    gsf = F(1.0) if gs is None else F(gs)
    lr, b1, b2, eps, wd = F(lr), F(b1), F(b2), F(eps), F(wd)
    bc1 = F(1.0 - float(b1) ** step)
    bc2 = 1.0 - float(b2) ** step
    bc2s = F(bc2) if mutant == "bc2_for_bc2_sqrt" else F(math.sqrt(bc2))
    gg = g if mutant == "unscaled_update" else (g * gsf).astype(F)
    if mutant == "swap_m_v":
        m0, v0 = v0, m0
    decay = F(F(1.0) - F(lr * wd))
    pd = p0 if mutant == "wd_after_step" else (p0 * decay).astype(F)
    bm = b2 if mutant == "beta2_for_beta1" else b1
    m1 = ((bm * m0).astype(F) + (F(F(1.0) - bm) * gg).astype(F)).astype(F)
    v1 = ((b2 * v0).astype(F) + ((F(F(1.0) - b2) * gg).astype(F) * gg).astype(F)).astype(F)
    with np.errstate(invalid="ignore"):       # swap_m_v takes the root of a first moment
        if mutant == "eps_inside_sqrt":
            denom = (np.sqrt((v1 + eps).astype(F)).astype(F) / bc2s).astype(F)
        else:
            denom = ((np.sqrt(v1).astype(F) / bc2s).astype(F) + eps).astype(F)
    p1 = (pd - (F(lr / bc1) * (m1 / denom).astype(F)).astype(F)).astype(F)
    if mutant == "wd_after_step":
        p1 = (p1 * decay).astype(F)
    if mutant == "swap_m_v":
        m1, v1 = v1, m1
    skip = ()
    if mutant == "skip_tail":
        skip = (g.size - 1,)
    elif mutant == "skip_seam" and g.size > CHUNK:
        skip = (CHUNK,)
    for i in skip:
        p1[i], m1[i], v1[i] = p0[i], np.asarray(m, dtype=F).reshape(-1)[i], np.asarray(v, dtype=F).reshape(-1)[i]
    sq = emulate_sumsq_f32(gg if mutant == "sumsq_of_scaled" else g, skip)
    return p1, m1, v1, sq


LR = 1e-3                 # the learning rate of the random-data tests
P_FLOOR = 16 * LR         # ... and the smallest |p| they draw


def draw(lengths, seed, gscale=None):
    """(p0 list, [g lists for 3 steps]) as float32 numpy arrays; g ~ N(0, 1), p = +-(P_FLOOR + |N(0, 1)|).
    Why p keeps away from zero: the p bound does not count the error m inherits (module docstring), 8 e K |u| at worst.  Over three
    steps from a zero state K |u| = (lr / bc1) (|b1 m0| + |(1-b1) g gs|) / denom <= 1.5 lr for the betas used here (step 1: lr (1-b1)
    bc2_sqrt / (bc1 sqrt(1-b2)) = lr; step 3: (lr / 0.271) (0.17 + 0.23) with sqrt(v) >= sqrt(1-b2) b2 (|g1| + |g2|) / sqrt 2), and
    the bound's margin on p is 2 e |p|: the bound as stated is a theorem for |p| >= 6 lr, and the draw keeps |p| >= 16 lr.  With
    p ~ N(0, 1) correct fp32 arithmetic misses it on about one element in 10^6 (|p| 4e-5, K 182: 2.3 x the bound).
    gscale == 2^-16 stands for a loss scale of 65536: the gradients are the same draw multiplied by 65536 (exactly), so that the scaled
    gradient the update sees is the unscaled draw."""
    rng = np.random.default_rng(seed)
    ps = []
    for n in lengths:
        x = rng.standard_normal(n)
        ps.append((np.where(x < 0, -1.0, 1.0) * (P_FLOOR + np.abs(x))).astype(np.float32))
    pre = np.float32(65536.0) if gscale is not None and gscale < 1e-3 else np.float32(1.0)
    gsteps = [[(rng.standard_normal(n).astype(np.float32) * pre) for n in lengths] for _ in range(3)]
    return ps, gsteps


# ---------------------------------------------------------------------------------------------- the one-hot sweep's exact checks
# lr wd = 2^-14: 1 - lr wd is exact in fp32 whether or not the compiler fuses it, so fl(p0 (1 - lr wd)) is one well-defined float
SWEEP = dict(lr=2.0 ** -10, b1=0.9, b2=0.95, eps=1e-8, wd=2.0 ** -4, gs=0.5, step=1)


def sweep_p0(n, t):
    return np.random.default_rng(1000 + t).standard_normal(n).astype(np.float32)


def sweep_grad(n, idx, t):
    g = np.zeros(n, dtype=np.float32)
    g[idx] = t + 1
    return g


def one_hot_violations(t, n, idx, p0, p, m, v, sumsq=None):
    """The exact checks of the one-hot sweep on tensor t (g = t + 1 at idx, zero elsewhere; m0 = v0 = 0; SWEEP's hyper-parameters)
    -> list of messages, empty when all hold."""
    bad = []
    if sumsq is not None and float(sumsq) != float((t + 1) ** 2):
        bad.append(f"tensor {t} (n {n}, one-hot at {idx}): sumsq {float(sumsq)!r} != {(t + 1) ** 2}")
    for name, a in (("m", m), ("v", v)):
        nz = np.flatnonzero(np.asarray(a).reshape(-1))
        if nz.tolist() != [idx]:
            bad.append(f"tensor {t} (n {n}, one-hot at {idx}): {name} is nonzero at {nz[:8].tolist()}")
    decay = 1.0 - SWEEP["lr"] * SWEEP["wd"]
    exp = (np.asarray(p0, dtype=np.float64) * decay).astype(np.float32)      # a 48-bit product: exact in double, rounded once
    diff = np.flatnonzero(exp.view(np.int32) != np.asarray(p, dtype=np.float32).reshape(-1).view(np.int32))
    if [i for i in diff.tolist() if i != idx]:
        bad.append(f"tensor {t} (n {n}, one-hot at {idx}): p differs from p0 (1 - lr wd) at {diff[:8].tolist()}")
    ref = ref_step(p0[idx], float(t + 1), 0.0, 0.0, SWEEP["gs"], SWEEP["step"], SWEEP["lr"], SWEEP["b1"], SWEEP["b2"], SWEEP["eps"],
                   SWEEP["wd"])
    for name, a in (("p", p), ("m", m), ("v", v)):
        r, _ = worst(np.asarray(a).reshape(-1)[idx], ref[name], ref["b" + name])
        if r > 1.0:
            bad.append(f"tensor {t} (n {n}): {name}[{idx}] is {r:.2f} x its bound from the reference")
    return bad
