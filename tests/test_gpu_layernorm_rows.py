"""GPU: csrc/layernorm.hip and csrc/pool.hip row by row and column by column, at every edge of their dispatch, on whichever library
OCTMAE_LIB selects (bfloat16 here, IEEE half in the child of tests/test_gpu_f16_kernels.py).

Reference: float64 layer_norm and its autograd on the same fp32 x and the same 16-bit dy (tests/lnrows.py).  Metrics: the worst ROW of
y / dx / pooled / out, the worst ENTRY of mean / rstd and of the column sums dgamma / dbeta / dxsum -- each class of rows (plain,
mean 1e3, one channel at 200, all zero) measured on its own, so that a class of large rows is not the floor for the others.

Bounds (none of them measured on the kernels; Y = tests/lnrows.py::yardstick, torch's fp32 CPU layer_norm against float64 on the same
inputs, per quantity and row class):
  * 16-bit y rows: 2.1 U (half an ulp of an element is at most 2 U of its value, so a row is off by at most 2 U of its norm; fp32
    arithmetic adds 1e-7); on rows of mean 1e3, 2.1 U + 4 Y.  dxb is the cast of dx, bit for bit.
  * fp32 outputs: max(the whole-tensor bound of the existing tests, now per row / per entry, 4 Y): mean, rstd 1e-5; dx 2e-5; dgamma,
    dbeta, dxsum 1e-4; everything of the slice pool 1e-5.  4 = the room between two correct fp32 implementations that sum in
    different orders; Y is ~1e-7 on plain rows and 2e-5 ... 1e-4 on rows of mean 1e3, where the accuracy of the fp32 mean sets all.
  * rows of zero variance: y is the 16-bit cast of beta bit for bit, mean is 0, rstd within 1e-5 of eps^-1/2.

Measured on MI355X with the bfloat16 build, worst case per quantity and input kind (y in U, the rest absolute; the parity ledger of
a run holds every case, for both builds):
  LayerNorm                y            mean            rstd              dx          dgamma           dbeta           dxsum
  plain               0.95         1.5e-07         1.2e-07         1.0e-07         4.5e-07         1.1e-07         4.6e-07
  offset              0.95         1.2e-07         1.3e-07         7.0e-06         1.7e-04         1.1e-07         3.3e-06
  outlier             1.40         1.5e-07         2.1e-07         5.3e-08         2.6e-07         1.1e-07         4.3e-07
  zero                0.95         1.5e-07         1.2e-07         1.0e-07         3.7e-07         1.1e-07         4.1e-07
  mixed               1.91         2.3e-07         3.3e-07         6.8e-04         1.4e-04         2.1e-07         7.2e-06
  slice pool          pooled            mean            rstd             out              dx          dgamma           dbeta           dxsum
  plain            6.0e-08         1.8e-07         1.3e-07         6.2e-07         1.3e-07         3.5e-06         5.0e-07         2.6e-07
  offset           7.0e-08         1.4e-07         5.5e-05         8.8e-04         7.1e-05         3.5e-03         5.1e-07         1.2e-04
  outlier          2.7e-09         1.3e-07         1.0e-07         1.2e-07         1.8e-07         3.1e-07         3.3e-07         3.2e-07
  zero             7.0e-08         1.3e-07         1.0e-07         1.8e-06         2.2e-07         6.3e-06         4.6e-07         4.6e-07
  mixed            5.4e-08         1.0e-07         1.0e-06         5.0e-05         2.4e-06         1.3e-04         5.7e-07         2.0e-05
Every case is inside its bound; closest are the y rows of `mixed` batches (1.91 U of 2.1: the rows with one channel at 200, where
that single element's rounding is the row's).  The large entries are inputs on which fp32 itself is that far from float64, and the
bound follows through Y: rows of mean 1e3 (D = 4 worst: dx 6.8e-4 against 4.2e-3), and a slice pool whose pooled row is the mean of
196 tokens at 1e3 -- spread 0.07, fp32 mean good to 1e-4 (dgamma 3.5e-3 against 1.2e-2).
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import ops
    from octcubem_amd._lib import call, load
    LP = ops.BF16
else:
    LP = torch.bfloat16
from tests import lnrows as LR
from tests.conftest import parity

DEV = "cuda"
IS_F16 = LP == torch.float16
TAG = "f16" if IS_F16 else "bf16"
U = 2.0 ** -12 if IS_F16 else 2.0 ** -9           # unit roundoff of the operand type, as tests/test_gpu_lp_edges.py counts it
FLOOR = {"mean": 1e-5, "rstd": 1e-5, "dx": 2e-5, "dgamma": 1e-4, "dbeta": 1e-4, "dxsum": 1e-4}      # test_layernorm_fwd_bwd
POOL_FLOOR = 1e-5                                 # test_slice_pool_kernels_vs_fp32_composition
ZERO_RSTD = LR.EPS ** -0.5


def bits_equal(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
class Case:
    """One drawn [M, D] problem: the operands on the GPU, the float64 reference and the yardstick, without (`bare`) and with the
    residual-stream gradient.  Computed once per (M, D, kind) and shared by the tests that use the shape."""

    def __init__(self, M, D, kind):
        self.M, self.D, self.kind = M, D, kind
        x, gamma, beta, dy, dres = LR.draw(M, D, kind, seed=7 * M + D)
        dy = dy.to(LP)
        self.groups = LR.row_classes(M, kind)
        self.ref_bare = LR.reference(x, gamma, beta, dy)
        self.ref = LR.with_dres(self.ref_bare, dres)
        f32 = LR.reference(x, gamma, beta, dy, None, torch.float32)
        self.Y_bare = LR.errors(f32, self.ref_bare, self.groups)
        self.Y = LR.errors(LR.with_dres(f32, dres), self.ref, self.groups)
        self.beta16 = beta.to(LP)
        self.x, self.gamma, self.beta, self.dy, self.dres = (t.to(DEV) for t in (x, gamma, beta, dy, dres))


_CASES = {}


def case(M, D, kind="mixed"):
    key = (M, D, kind)
    if key not in _CASES:
        if len(_CASES) >= 3:                      # the big shapes hold ~0.3 GB of float64 each
            _CASES.pop(next(iter(_CASES)))
        _CASES[key] = Case(M, D, kind)
    return _CASES[key]


def forward(c):
    y, mean, rstd = ops.layernorm_fwd(c.x, c.gamma, c.beta, LR.EPS)
    return y, mean, rstd


def backward(c, mean, rstd, dres=True, want16=True, sums=("dgamma", "dbeta", "dxsum"), prior=None):
    """-> {dx, dxb, dgamma, dbeta, dxsum} (those that were asked for); the sums start from `prior` (or zeros)."""
    buf = {k: (torch.zeros(c.D, device=DEV) if prior is None else prior[k].clone()) for k in sums}
    dx, dxb = ops.layernorm_bwd(c.dy, c.x, mean, rstd, c.gamma, buf.get("dgamma"), buf.get("dbeta"), dres=c.dres if dres else None,
                                want_bf16=want16, dxsum=buf.get("dxsum"))
    torch.cuda.synchronize()
    assert (dxb is not None) == want16
    out = {"dx": dx, **buf}
    if want16:
        out["dxb"] = dxb
    return out


def y_bound(Y, cls):
    return 2.1 * U + (4 * Y["y"][cls] if cls == LR.OFFSET else 0.0)


def check(label, c, got, ref, Y):
    """Every quantity of `got` against `ref`, every row class against its own bound; one ledger entry per quantity: the class that
    came closest to its bound (y in U)."""
    got = {k: v.detach().cpu() for k, v in got.items()}
    if "dxb" in got:
        assert bits_equal(got["dxb"], got["dx"].to(LP)), f"{label}: dxb is not the cast of dx"
        del got["dxb"]
    if "y" in got:
        got["y"] = got["y"].double()
    for q, per_class in LR.errors(got, ref, c.groups).items():
        entries = []
        for cls, e in per_class.items():
            bound = y_bound(Y, cls) if q == "y" else max(FLOOR[q], 4 * Y[q][cls])
            entries.append((e / bound, e, bound))
        _, e, bound = max(entries)
        scale = U if q == "y" else 1.0
        parity(f"{TAG}/lnrows/{c.kind}/{q}/{label}", e / scale, bound / scale)


def fwd_bwd(label, c, bare=True):
    y, mean, rstd = forward(c)
    check(label, c, {"y": y, "mean": mean, "rstd": rstd}, c.ref, c.Y)
    check(label + "/full", c, backward(c, mean, rstd), c.ref, c.Y)
    if bare:
        got = backward(c, mean, rstd, dres=False, want16=False, sums=())
        check(label + "/bare", c, got, c.ref_bare, c.Y_bare)
    return y, mean, rstd


# forward: 512 workgroups x 4 waves -> a wave's second row from M = 2049, its third from 4097; backward: 256 x 4 -> 1025, 2049, ...
TRIPS = [(M, 64) for M in (1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 4100, 6145)] + \
        [(2049, 260), (4100, 260), (2049, 1280), (4100, 1280)]


@pytest.mark.parametrize("M,D", TRIPS)
def test_row_pipeline_trips(M, D):
    fwd_bwd(f"trips_M{M}_D{D}", case(M, D))


# every template bucket NC = 1, 2, 4, 8 at both of its edges, a partly filled last chunk in each, nc = 5, 6, 7 on NC = 8, one lane
WIDTHS = [4, 8, 252, 256, 260, 384, 508, 512, 516, 768, 1020, 1024, 1028, 1280, 1536, 1792, 2044, 2048]


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("M", [37, 1029])
def test_widths(M, D):
    fwd_bwd(f"widths_M{M}_D{D}", case(M, D), bare=False)


@pytest.mark.parametrize("M", [192, 196, 256, 260])
def test_finish_kernel_loop_edges(M):
    """48, 49, 64, 65 workgroups of partials: the 4-way unrolled loop of ln_bwd_finish_kernel and its remainder."""
    fwd_bwd(f"finish_M{M}_D128", case(M, 128), bare=False)


@pytest.mark.parametrize("M,D", [(333, 768), (2100, 512)])
@pytest.mark.parametrize("kind", [k for k in LR.KINDS if k != "mixed"])
def test_input_kinds(kind, M, D):
    fwd_bwd(f"kinds_M{M}_D{D}", case(M, D, kind), bare=False)


@pytest.mark.parametrize("kind,M,D", [("zero", 333, 768), ("mixed", 2100, 512), ("zero", 1, 4)])
def test_zero_variance_rows(kind, M, D):
    c = case(M, D, kind)
    y, mean, rstd = forward(c)
    z = c.groups == LR.ZERO
    assert bool(z.any())
    yz, n = y.cpu()[z], int(z.sum())
    assert bits_equal(yz, c.beta16.expand(n, D).contiguous())
    assert bool((mean.cpu()[z] == 0).all())
    parity(f"{TAG}/lnrows/{kind}/zero_rstd/M{M}_D{D}", float((rstd.cpu()[z].double() / ZERO_RSTD - 1).abs().max()), 1e-5)


def test_accumulation_and_optional_outputs():
    """The finish kernel ADDS to dgamma / dbeta / dxsum (gradient accumulation over micro-batches), each of them may be absent, and
    dx does not depend on which are asked for."""
    c = case(1029, 516)
    _, mean, rstd = forward(c)
    base = backward(c, mean, rstd)
    g = torch.Generator().manual_seed(5)
    prior = {k: (3 * torch.randn(c.D, generator=g)).to(DEV) for k in LR.COLS}
    acc = backward(c, mean, rstd, prior=prior)
    assert bits_equal(acc["dx"], base["dx"]) and bits_equal(acc["dxb"], base["dxb"])
    ref = dict(c.ref)
    for k in LR.COLS:
        ref[k] = c.ref[k] + prior[k].double().cpu()
    check("accum_M1029_D516", c, {k: acc[k] for k in LR.COLS}, ref, c.Y)
    for k in LR.COLS:                             # one of the three alone
        one = backward(c, mean, rstd, sums=(k,))
        assert bits_equal(one["dx"], base["dx"]) and bits_equal(one["dxb"], base["dxb"])
        assert bits_equal(one[k], base[k]), k
    none = backward(c, mean, rstd, sums=(), want16=False)
    assert bits_equal(none["dx"], base["dx"])


def test_backward_is_deterministic():
    c = case(4100, 1280)
    _, mean, rstd = forward(c)
    a, b = backward(c, mean, rstd), backward(c, mean, rstd)
    for k in ("dx", "dxb", "dgamma", "dbeta", "dxsum"):
        assert bits_equal(a[k], b[k]), k
    assert bits_equal(a["dxb"], a["dx"].to(LP))
    y2, mean2, rstd2 = forward(c)
    y1, _, _ = forward(c)
    assert bits_equal(y1, y2) and bits_equal(mean, mean2) and bits_equal(rstd, rstd2)


PAD = 64                                          # guard elements on either side: 128 / 256 bytes, so the views keep 16-byte alignment
SENTINEL = 7.0


class Guarded:
    """Named views into larger allocations filled with a sentinel."""

    def __init__(self):
        self.big = {}

    def new(self, name, n, dtype=torch.float32, init=None):
        big = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
        view = big[PAD:PAD + n]
        assert view.data_ptr() % 16 == 0
        if init is not None:
            view.copy_(init.flatten())
        self.big[name] = (big, n)
        setattr(self, name, view)
        return view

    def assert_intact(self):
        torch.cuda.synchronize()
        for name, (big, n) in self.big.items():
            assert bool((big[:PAD] == SENTINEL).all()), f"{name}: written before its first element"
            assert bool((big[PAD + n:] == SENTINEL).all()), f"{name}: written past its last element"


@pytest.mark.parametrize("M,D", [(5, 4), (1025, 260), (2049, 1280)])
def test_layernorm_stays_inside_outputs_and_workspace(M, D):
    """The C ABI with every output and the workspace (octmae_layernorm_bwd_ws_floats, exactly) between guard elements."""
    c = case(M, D)
    G = Guarded()
    G.new("y", M * D, LP); G.new("mean", M); G.new("rstd", M)
    call("octmae_layernorm_fwd", c.x.data_ptr(), c.gamma.data_ptr(), c.beta.data_ptr(), G.y.data_ptr(), G.mean.data_ptr(), G.rstd.data_ptr(),
         M, D, LR.EPS, ops._stream())
    G.assert_intact()
    y, mean, rstd = forward(c)
    assert bits_equal(G.y.view(M, D), y) and bits_equal(G.mean, mean) and bits_equal(G.rstd, rstd)
    G.new("ws", load().octmae_layernorm_bwd_ws_floats(M, D)); G.new("dx", M * D); G.new("dxb", M * D, LP)
    zeros = torch.zeros(D)
    G.new("dgamma", D, init=zeros); G.new("dbeta", D, init=zeros); G.new("dxsum", D, init=zeros)
    call("octmae_layernorm_bwd", c.dy.data_ptr(), c.x.data_ptr(), G.mean.data_ptr(), G.rstd.data_ptr(), c.gamma.data_ptr(), c.dres.data_ptr(),
         G.dx.data_ptr(), G.dxb.data_ptr(), G.dgamma.data_ptr(), G.dbeta.data_ptr(), G.dxsum.data_ptr(), G.ws.data_ptr(), M, D, ops._stream())
    G.assert_intact()
    got = {"dx": G.dx.view(M, D), "dxb": G.dxb.view(M, D), "dgamma": G.dgamma, "dbeta": G.dbeta, "dxsum": G.dxsum}
    base = backward(c, mean, rstd)
    for k, v in got.items():
        assert bits_equal(v, base[k]), k
    check(f"contained_M{M}_D{D}", c, got, c.ref, c.Y)


@pytest.mark.parametrize("M,D", [(8, 6), (8, 2052), (0, 64)])
def test_layernorm_rejects_bad_shapes(M, D):
    """Refused on the host, before any launch."""
    x = torch.zeros(M, D, device=DEV)
    gamma, beta = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    with pytest.raises(RuntimeError):
        ops.layernorm_fwd(x, gamma, beta, LR.EPS)
    with pytest.raises(RuntimeError):
        ops.layernorm_bwd(torch.zeros(M, D, dtype=LP, device=DEV), x, torch.zeros(max(M, 1), device=DEV), torch.ones(max(M, 1), device=DEV),
                          gamma, None, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ slice pool
POOL_D = [4, 260, 320, 768, 1280, 2048]
POOL_T = [2, 3, 17, 18, 34, 197]                  # L = T - 1 pooled tokens: 1; 2; one split of 16; 9 + 8; 11 + 11 + 11; 13 splits
POOL_BS = [(1, 1), (1, 3), (2, 12), (30, 20)]     # (30, 20): 600 slices, nsplit = 1 whatever T


def _pool_cases():
    """Every (D, T) pair once, the other axes cycled; 600 slices only where the volume stays small."""
    out = []
    for i, (D, T) in enumerate(itertools.product(POOL_D, POOL_T)):
        B, S = POOL_BS[(i + i // 6) % 4]
        if (B, S) == (30, 20) and T * D > 13000:
            B, S = POOL_BS[i % 3]
        out.append((B, S, T, D, bool((i + i // 6) % 2), LR.KINDS[i % 5]))
    out += [(30, 20, 2, 2048, False, "mixed"), (30, 20, 18, 320, True, "offset"), (1, 1, 2, 4, True, "plain"), (1, 3, 18, 1280, False, "zero")]
    return out


POOL_CASES = _pool_cases()
assert {c[:2] for c in POOL_CASES} >= set(POOL_BS) and {c[2] for c in POOL_CASES} >= set(POOL_T)
assert {c[3] for c in POOL_CASES} >= set(POOL_D) and {c[4] for c in POOL_CASES} == {False, True} and {c[5] for c in POOL_CASES} >= set(LR.KINDS)


def pool_run(x, gamma, beta, dout, S, cls, prior=None):
    """octmae_slice_pool_fwd + _bwd through the C ABI, every output and the workspace (octmae_slice_pool_ws_floats, exactly) between
    guard elements -> the results, after the guards have been checked."""
    BS, T, D = x.shape
    B = BS // S
    G = Guarded()
    G.new("out", B * D); G.new("pooled", BS * D); G.new("mean", BS); G.new("rstd", BS)
    G.new("ws", load().octmae_slice_pool_ws_floats(BS, T, D))
    G.new("dx", BS * T * D); G.new("dxb", BS * T * D, LP)
    for k in LR.COLS:
        G.new(k, D, init=torch.zeros(D) if prior is None else prior[k])
    call("octmae_slice_pool_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), G.out.data_ptr(), G.pooled.data_ptr(), G.mean.data_ptr(),
         G.rstd.data_ptr(), G.ws.data_ptr(), B, S, T, D, int(cls), LR.EPS, ops._stream())
    G.assert_intact()
    call("octmae_slice_pool_bwd", dout.data_ptr(), G.pooled.data_ptr(), G.mean.data_ptr(), G.rstd.data_ptr(), gamma.data_ptr(),
         G.dx.data_ptr(), G.dxb.data_ptr(), G.dgamma.data_ptr(), G.dbeta.data_ptr(), G.dxsum.data_ptr(), G.ws.data_ptr(), B, S, T, D,
         int(cls), ops._stream())
    G.assert_intact()
    return {"out": G.out.view(B, D), "pooled": G.pooled.view(BS, D), "mean": G.mean, "rstd": G.rstd, "dx": G.dx.view(BS, T, D),
            "dxb": G.dxb.view(BS, T, D), "dgamma": G.dgamma, "dbeta": G.dbeta, "dxsum": G.dxsum}


@pytest.mark.parametrize("B,S,T,D,cls,kind", POOL_CASES)
def test_slice_pool_rows(B, S, T, D, cls, kind):
    BS = B * S
    # + 0.5: the row offsets of draw() ramp symmetrically about 0 over the tokens, and a pooled row whose mean cancels by
    # construction would be measured against nothing
    x, gamma, beta, dy, _ = LR.draw(BS * T, D, kind, seed=BS + 3 * T + D + int(cls), shift=0.5)
    x, dout = x.view(BS, T, D), dy[:B].contiguous()
    ref = LR.pool_reference(x, gamma, beta, dout, S, cls)
    Y = LR.errors(LR.pool_reference(x, gamma, beta, dout, S, cls, torch.float32), ref)
    xg, gg, bg, dg = (t.to(DEV) for t in (x, gamma, beta, dout))
    got = pool_run(xg, gg, bg, dg, S, cls)
    assert bits_equal(got["dxb"], got["dx"].to(LP))
    # the tokens that are not pooled receive exact zeros
    assert int(torch.count_nonzero(got["dx"][:, 1:] if cls else got["dx"][:, 0])) == 0
    label = f"B{B}_S{S}_T{T}_D{D}_{'cls' if cls else 'mean'}"
    meas = {k: v.cpu() for k, v in got.items() if k != "dxb"}
    for q, e in LR.errors(meas, ref).items():
        parity(f"{TAG}/poolrows/{kind}/{q}/{label}", e[None], max(POOL_FLOOR, 4 * Y[q][None]))
    # a second call is bit-identical
    again = pool_run(xg, gg, bg, dg, S, cls)
    for k in got:
        assert bits_equal(got[k], again[k]), k
    # the sums are ADDED to what the buffers hold
    g = torch.Generator().manual_seed(D + T)
    prior = {k: (3 * torch.randn(D, generator=g)).to(DEV) for k in LR.COLS}
    acc = pool_run(xg, gg, bg, dg, S, cls, prior=prior)
    assert bits_equal(acc["dx"], got["dx"]) and bits_equal(acc["out"], got["out"])
    sums = {k: acc[k].cpu() for k in LR.COLS}
    for q, e in LR.errors(sums, {k: ref[k] + prior[k].double().cpu() for k in LR.COLS}).items():
        parity(f"{TAG}/poolrows/{kind}/{q}_accum/{label}", e[None], max(POOL_FLOOR, 4 * Y[q][None]))
