"""Row-wise and column-wise error metrics, inputs and references for the LayerNorm and slice-pool tests (a helper, not a conftest;
tests/test_cpu_lnrows.py proves on the CPU what the metrics see, tests/test_gpu_layernorm_rows.py applies them to the kernels).

A relative L2 norm over a whole [M, D] tensor dilutes a fault confined to one row by sqrt(M): one row of 1281 that is 5 % off moves
it by 1.4e-3, inside the 3e-3 that tests/test_gpu_kernels.py::test_layernorm_fwd_bwd allows for y.  row_err() takes the worst ROW,
vec_err() the worst ENTRY of a per-row statistic or a per-column sum.

The inputs of draw() are rows that are NOT exchangeable (every row has its own mean and its own spread, so a result written to row
n +- 1 or n +- nwaves is wrong by the size of the row) and come in kinds that stress what a LayerNorm can get wrong: a mean far above
the spread, one huge channel, rows of zero variance."""
import torch

KINDS = ("plain", "offset", "outlier", "zero", "mixed")
PLAIN, OFFSET, OUTLIER, ZERO = range(4)          # the class of a row (row_classes)
EPS = 1e-6
OUTLIER_CHANNEL, OUTLIER_VALUE, OFFSET_MEAN = 7, 200.0, 1e3
STATS = ("mean", "rstd")                        # per row: vec_err; everything else that is not a column sum: [rows, D], row_err
COLS = ("dgamma", "dbeta", "dxsum")             # [D]: vec_err


def _worst(e, with_index):
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))      # a NaN entry is the worst one, not an ignored one
    worst = int(e.argmax())
    return (float(e[worst]), worst) if with_index else float(e[worst])


def _rms_floor(v, groups):
    """[n] the RMS of v, taken inside each group of entries when groups [n] is given."""
    if groups is None:
        return v.pow(2).mean().sqrt().expand_as(v)
    floor = torch.zeros_like(v)
    for c in groups.unique().tolist():
        m = groups == c
        floor[m] = v[m].pow(2).mean().sqrt()
    return floor


def row_err(got: torch.Tensor, ref: torch.Tensor, groups: torch.Tensor = None, with_index: bool = False):
    """max over rows of ||got_r - ref_r|| / max(||ref_r||, rms_r ||ref_r||) for [M, D].  The floor keeps reference rows of (almost)
    zero norm from dominating.  groups [M] (row_classes): the RMS is taken inside each group -- the dx rows of zero-variance inputs
    are 1e3 x the size of their neighbours and would otherwise be the floor for all of them.  with_index: also the worst row."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape and ref.dim() == 2, (got.shape, ref.shape)
    rn = ref.norm(dim=-1)
    return _worst((got - ref).norm(dim=-1) / torch.maximum(rn, _rms_floor(rn, groups)).clamp_min(1e-300), with_index)


def vec_err(got: torch.Tensor, ref: torch.Tensor, groups: torch.Tensor = None, with_index: bool = False):
    """max over entries of |got - ref| / max(|ref|, rms(ref)) for per-row statistics [M] and per-column sums [D].
    groups [M] (row_classes): the RMS floor is taken inside each group, so that the rows of mean 1e3 (or of rstd 1e3) of a mixed
    batch do not set the scale for the plain rows beside them; a group whose reference is all zero must be matched exactly."""
    got = got.detach().double().cpu().flatten()
    ref = ref.detach().double().cpu().flatten()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return _worst((got - ref).abs() / torch.maximum(ref.abs(), _rms_floor(ref, groups)).clamp_min(1e-300), with_index)


def rel_l2(got, ref):
    """The whole-tensor metric of tests/test_gpu_kernels.py."""
    got = got.detach().double().flatten().cpu()
    ref = ref.detach().double().flatten().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def row_classes(M: int, kind: str) -> torch.Tensor:
    """[M] the class of every row of draw(M, D, kind, .): `zero` zeroes every 5th row of a plain batch, `mixed` interleaves the four
    classes row by row."""
    n = torch.arange(M)
    if kind == "mixed":
        return n % 4
    if kind == "zero":
        return torch.where(n % 5 == 0, ZERO, PLAIN)
    return torch.full((M,), {"plain": PLAIN, "offset": OFFSET, "outlier": OUTLIER}[kind])


def draw(M: int, D: int, kind: str, seed: int, shift: float = 0.0):
    """x, gamma, beta, dy, dres (fp32, CPU) for an [M, D] LayerNorm.  Plain rows: randn * s_n + o_n + shift with the offset o_n
    ramping over [-1.5, 1.5] and the scale s_n cycling through [0.5, 2]; dy carries a row scale of its own.  offset rows: mean
    1e3 + o_n, spread 1.  outlier rows: a plain row whose channel 7 (mod D) is 200.  zero rows: all zeros."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, D, generator=g)
    n = torch.arange(M, dtype=torch.float32)
    off = (3.0 * (n + 0.5) / M - 1.5).unsqueeze(1)
    sc = (2.0 ** (2.0 * ((n * 0.381966) % 1.0) - 1.0)).unsqueeze(1)
    x = z * sc + off + shift
    cls = row_classes(M, kind)
    o = cls == OFFSET
    x[o] = OFFSET_MEAN + off[o] + z[o]
    u = cls == OUTLIER
    x[u, OUTLIER_CHANNEL % D] = OUTLIER_VALUE
    x[cls == ZERO] = 0.0
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(M, D, generator=g) * (2.0 ** (2.0 * (((n + 0.5) * 0.618034) % 1.0) - 1.0)).unsqueeze(1)
    dres = torch.randn(M, D, generator=g)
    return x, gamma, beta, dy, dres


def reference(x, gamma, beta, dy, dres=None, dtype=torch.float64):
    """layer_norm (eps 1e-6) and its autograd in `dtype` on the CPU, on the given operands: y, mean, rstd, dx (+ dres), dgamma, dbeta
    and dxsum = the column sums of dx.  float64: the reference; float32: torch's own kernels, the yardstick."""
    xd = x.detach().cpu().to(dtype).requires_grad_(True)
    gd = gamma.detach().cpu().to(dtype).requires_grad_(True)
    bd = beta.detach().cpu().to(dtype).requires_grad_(True)
    y, mean, rstd = torch.native_layer_norm(xd, (x.shape[1],), gd, bd, EPS)
    y.backward(dy.detach().cpu().to(dtype))
    dx = xd.grad if dres is None else xd.grad + dres.detach().cpu().to(dtype)
    return {"y": y.detach(), "mean": mean.detach().flatten(), "rstd": rstd.detach().flatten(), "dx": dx, "dgamma": gd.grad,
            "dbeta": bd.grad, "dxsum": dx.sum(0)}


def with_dres(ref, dres):
    """The reference of a backward that adds the residual-stream gradient, from the one without."""
    out = dict(ref)
    out["dx"] = ref["dx"] + dres.detach().cpu().to(ref["dx"].dtype)
    out["dxsum"] = out["dx"].sum(0)
    return out


def errors(got, ref, groups=None):
    """{quantity: {row class: error}} for the quantities of `got`: row_err for the [rows, D] ones, vec_err for the per-row statistics,
    each class of rows measured on its own (key None: all rows, when no groups are given); vec_err for the column sums (key None)."""
    out = {}
    for k, v in got.items():
        r = ref[k]
        if k in COLS:
            out[k] = {None: vec_err(v, r)}
            continue
        if k not in STATS:
            v, r = v.reshape(-1, v.shape[-1]), r.reshape(-1, r.shape[-1])
        fn = vec_err if k in STATS else row_err
        if groups is None:
            out[k] = {None: fn(v, r)}
        else:
            out[k] = {c: fn(v[groups == c], r[groups == c]) for c in groups.unique().tolist()}
    return out


def worst(err):
    """The largest error of one quantity of errors(), over the row classes."""
    return max(err.values())


def yardstick(x, gamma, beta, dy, dres=None, groups=None):
    """How far two correct implementations are apart: torch's fp32 CPU layer_norm, forward and autograd, against the float64 one on
    the same inputs, under the metrics the kernels are measured with.  1e-7 on plain rows; 3e-5 ... 1e-4 on rows of mean 1e3, where
    the accuracy of the fp32 mean sets everything."""
    return errors(reference(x, gamma, beta, dy, dres, torch.float32), reference(x, gamma, beta, dy, dres), groups)


# ------------------------------------------------------------------------------------------------------------------ slice pool
def pool_reference(x, gamma, beta, dout, S, cls, dtype=torch.float64):
    """The slice-pooling head in `dtype` on the CPU: x [B*S, T, D] -> pooled rows (token 0, or the mean of tokens 1..T-1), their
    LayerNorm statistics, out [B, D] = the mean over the S slices of the normalised rows; and the gradients for dout [B, D]."""
    xd = x.detach().cpu().to(dtype).requires_grad_(True)
    gd = gamma.detach().cpu().to(dtype).requires_grad_(True)
    bd = beta.detach().cpu().to(dtype).requires_grad_(True)
    D = x.shape[-1]
    p = xd[:, 0] if cls else xd[:, 1:].mean(dim=1)
    yn, mean, rstd = torch.native_layer_norm(p, (D,), gd, bd, EPS)
    out = yn.view(-1, S, D).mean(dim=1)
    out.backward(dout.detach().cpu().to(dtype))
    return {"pooled": p.detach(), "mean": mean.detach().flatten(), "rstd": rstd.detach().flatten(), "out": out.detach(),
            "dx": xd.grad, "dgamma": gd.grad, "dbeta": bd.grad, "dxsum": xd.grad.sum(dim=(0, 1))}


def pool_yardstick(x, gamma, beta, dout, S, cls):
    return errors(pool_reference(x, gamma, beta, dout, S, cls, torch.float32), pool_reference(x, gamma, beta, dout, S, cls))
