"""tests/lnrows.py on the CPU: the row / entry metrics see one-row faults that a whole-tensor L2 norm dilutes by sqrt(M), and the
yardstick (torch's own fp32 layer_norm against float64) stays inside the bounds tests/test_gpu_layernorm_rows.py applies to the
kernels, on every input kind.

The faults are injected into the float64 reference itself (the unfaulted error is 0) at M = 1281, D = 1280, and measured with both
metrics against the bounds of tests/test_gpu_kernels.py::test_layernorm_fwd_bwd (whole tensor) and of the row tests (per row / per
entry).  Measured here:

    fault                                      rel_l2 (old bound)    row / entry metric (new bound)
    one row of y 5 % off                       1.39e-3  (< 3e-3)     5.0e-2   (> 2.1 U = 4.1e-3)
    mean[n] <-> mean[n+1], rows of mean 1e3    ~1e-6    (< 1e-5)     ~4e-5    (> 1e-5)
    mean[n] <-> mean[n+1], plain rows          ~3e-3    (> 1e-5)     ~5e-2    (> 1e-5)
    dx[n, 1024:1280] = 0                       1.2e-2   (> 2e-5)     4e-1     (> 2e-5)
    one row of dx 5e-4 off                     1.4e-5   (< 2e-5)     5.0e-4   (> 2e-5)

The fp32 quantities are bounded so tightly as whole tensors (1e-5, 2e-5) that a GROSS one-row fault -- neighbouring means swapped on
plain rows, a fifth of a dx row dropped -- is over the old bound as well; what the old bound lets through there is a one-row fault of
relative size below bound * sqrt(M) = 7e-4, and for the statistics a swap between rows whose means differ by less than 1e-5 of their
size (the rows of mean 1e3).  Both are asserted below, each as what it is."""
import pytest
import torch

from tests import lnrows as LR

U = 2.0 ** -9                                   # bfloat16, as tests/test_gpu_lp_edges.py counts it: half an ulp is at most 2 U
L2 = {"y": 3e-3, "mean": 1e-5, "dx": 2e-5}      # test_layernorm_fwd_bwd, whole tensor
NEW = {"y": 2.1 * U, "mean": 1e-5, "dx": 2e-5}  # the row tests' bounds on plain rows (fp32 quantities: max(this, 4 x yardstick))
M, D = 1281, 1280
_CACHE = {}


def _ref(kind):
    if kind not in _CACHE:
        x, gamma, beta, dy, dres = LR.draw(M, D, kind, seed=11)
        dy = dy.to(torch.bfloat16)
        _CACHE[kind] = (LR.reference(x, gamma, beta, dy, dres), LR.yardstick(x, gamma, beta, dy, dres, LR.row_classes(M, kind)))
    return _CACHE[kind]


def test_one_row_of_y_off_by_5_percent():
    ref, _ = _ref("plain")
    n = 777
    bad = ref["y"].clone()
    bad[n] *= 1.05
    l2 = LR.rel_l2(bad, ref["y"])
    e, idx = LR.row_err(bad, ref["y"], with_index=True)
    assert l2 == pytest.approx(0.05 * float(ref["y"][n].norm() / ref["y"].norm()), rel=1e-9) and 1.0e-3 < l2 < L2["y"]
    assert idx == n and 0.045 < e <= 0.05 and e > NEW["y"]         # 0.05 of the row, measured against max(its norm, the RMS norm)


@pytest.mark.parametrize("kind", ["offset", "plain"])
def test_neighbouring_means_swapped(kind):
    ref, yard = _ref(kind)
    n = 640
    bad = ref["mean"].clone()
    bad[[n, n + 1]] = ref["mean"][[n + 1, n]]
    l2 = LR.rel_l2(bad, ref["mean"])
    e, idx = LR.vec_err(bad, ref["mean"], with_index=True)
    bound = max(NEW["mean"], 4 * LR.worst(yard["mean"]))
    assert idx in (n, n + 1) and e > bound, (e, bound)
    if kind == "offset":
        assert l2 < L2["mean"], l2               # means 1e3 +- 0.05: the whole-tensor bound cannot tell the two rows apart
    else:
        assert l2 > L2["mean"], l2               # plain rows differ by several % of their RMS: caught either way


def test_a_chunk_of_one_dx_row_dropped():
    """Columns 1024-1279 (the fifth chunk slot of the NC = 8 kernels at D = 1280) of one row."""
    ref, yard = _ref("plain")
    n = 1000
    bad = ref["dx"].clone()
    bad[n, 1024:] = 0
    e, idx = LR.row_err(bad, ref["dx"], with_index=True)
    bound = max(NEW["dx"], 4 * LR.worst(yard["dx"]))
    assert idx == n and e > 0.3 > bound
    assert LR.rel_l2(bad, ref["dx"]) > L2["dx"]  # a fifth of a row is 1.2e-2 of the tensor: far over the whole-tensor 2e-5 as well
    # the window the whole-tensor bound leaves open: a row that is off by less than 2e-5 * sqrt(M) = 7e-4 of itself
    bad = ref["dx"].clone()
    bad[n] *= 1 + 5e-4
    assert LR.rel_l2(bad, ref["dx"]) < L2["dx"]
    e, idx = LR.row_err(bad, ref["dx"], with_index=True)
    assert idx == n and e > bound and bound < 1e-4


# what the row tests allow the KERNELS on top of the yardstick Y: fp32 quantities max(floor, 4 Y); so Y itself must be a sane number
# (a reference that is off would hand the kernels a huge bound unnoticed).  Ceilings: 10 x the figures of the table in
# tests/test_gpu_layernorm_rows.py for plain / outlier / zero rows (fp32 roundoff, a few e-7), 5e-4 where rows of mean 1e3 take part
# (the fp32 mean of a row at 1e3 is off by ~1e-4 of the row's spread)
@pytest.mark.parametrize("kind", LR.KINDS)
@pytest.mark.parametrize("D_", [64, 768, 1024, 1280])
def test_yardstick_on_every_kind(kind, D_):
    Mk = 300
    x, gamma, beta, dy, dres = LR.draw(Mk, D_, kind, seed=D_)
    dy = dy.to(torch.bfloat16)
    groups = LR.row_classes(Mk, kind)
    ref = LR.reference(x, gamma, beta, dy, dres)
    Y = LR.yardstick(x, gamma, beta, dy, dres, groups)
    print(f"\nyardstick {kind} D={D_}: " + ", ".join(f"{k} {LR.worst(v):.2e}" for k, v in Y.items()))
    for k, per_class in Y.items():
        for c, v in per_class.items():
            far = c == LR.OFFSET or (c is None and kind in ("offset", "mixed"))      # column sums (c None) mix all rows
            assert v <= (5e-4 if far else 5e-6), (k, c, v)
        if k in ("y", "dx"):
            assert LR.worst(per_class) >= 2.0 ** -26, k      # and it is an fp32 computation, not the reference compared with itself
    # a float64 y rounded to the 16-bit type: at most half an ulp per element = 2 U of the row, and close to that on some row
    for lp, u in ((torch.bfloat16, 2.0 ** -9), (torch.float16, 2.0 ** -12)):
        e = LR.row_err(ref["y"].to(lp), ref["y"]) / u
        assert 0.5 < e <= 2.0, (lp, e)
    # zero rows: y is beta exactly, mean 0, rstd eps^-1/2, in float64 and in fp32 alike
    z = groups == LR.ZERO
    if bool(z.any()):
        f32 = LR.reference(x, gamma, beta, dy, dres, torch.float32)
        assert torch.equal(f32["y"][z], beta.expand(int(z.sum()), D_)) and torch.equal(ref["y"][z], beta.double().expand(int(z.sum()), D_))
        assert bool((f32["mean"][z] == 0).all()) and float((f32["rstd"][z] / 1e3 - 1).abs().max()) <= 1e-5


def test_metrics_floor_nan_and_groups():
    ref = torch.ones(4, 8, dtype=torch.float64)
    ref[2] = 1e-9
    got = ref.clone()
    got[2] += 1e-6                               # 1000 x the row's own size, 1e-6 of its neighbours'
    e, idx = LR.row_err(got, ref, with_index=True)
    assert idx == 2 and e == pytest.approx(1e-6 * 8 ** 0.5 / (0.75 * 8) ** 0.5, rel=1e-6)
    got = ref.clone()
    got[3, 0] = float("nan")
    assert LR.row_err(got, ref, with_index=True) == (float("inf"), 3)
    v = torch.tensor([1000.0, 1.0, 1000.0, 1.0], dtype=torch.float64)
    w = v.clone()
    w[1] += 1e-3
    assert LR.vec_err(w, v) == pytest.approx(1e-3 / (500000.5 ** 0.5), rel=1e-9)            # measured against the batch's RMS
    assert LR.vec_err(w, v, torch.tensor([1, 0, 1, 0]), with_index=True) == (pytest.approx(1e-3, rel=1e-9), 1)   # against its own kind
    zero = torch.zeros(3, dtype=torch.float64)
    assert LR.vec_err(zero, zero) == 0.0 and LR.vec_err(zero + 1e-30, zero) > 1.0          # an all-zero reference is matched exactly
    w[0] = float("nan")
    assert LR.vec_err(w, v) == float("inf")


def test_draw_rows_are_not_exchangeable():
    x, gamma, beta, dy, dres = LR.draw(2100, 512, "mixed", seed=3)
    cls = LR.row_classes(2100, "mixed")
    mean, std = x.double().mean(1), x.double().std(1)
    p = cls == LR.PLAIN
    assert float(mean[p].max() - mean[p].min()) > 2.5 and 3.0 < float(std[p].max() / std[p].min()) < 5.0
    assert float((mean[cls == LR.OFFSET] - 1e3).abs().max()) < 1.8 and float((std[cls == LR.OFFSET] - 1).abs().max()) < 0.15
    assert bool((x[cls == LR.OUTLIER, 7] == 200).all()) and int(torch.count_nonzero(x[cls == LR.ZERO])) == 0
    assert len(set(mean[p].tolist())) == int(p.sum()) and len(set(std[p].tolist())) == int(p.sum())
    assert torch.equal(LR.row_classes(11, "zero"), torch.tensor([3, 0, 0, 0, 0, 3, 0, 0, 0, 0, 3]))
    x4 = LR.draw(9, 4, "outlier", seed=1)[0]
    assert bool((x4[:, 3] == 200).all())         # D = 4: channel 7 mod D
