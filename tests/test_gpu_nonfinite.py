"""GPU: one planted NaN / Inf reaches exactly the outputs that use it, and NaN-filled surroundings reach none -- the kernels that carry
the gradient (GEMM entry points, attention, the LayerNorm family, the token and loss kernels, the optimizer), on whichever library
OCTMAE_LIB selects (bfloat16 here, IEEE half in the child of tests/test_gpu_f16_kernels.py).  `pytest -m gpu` on an MI355X.

Three kinds of test per family (tests/nonfinite.py holds the helpers and the rules, tests/test_cpu_nonfinite.py shows on the CPU that
every rule is the NaN set of the float64 evaluation):
  A. NaN plants: the NaN set of the outputs equals the rule element for element, every other element holds the bits of the clean run;
  B. +inf / -inf plants: where the float64 evaluation (NF.ref_*, on the same planted operands) has a non-finite element in a tensor the
     kernel's tensor has one too, and every element outside the NaN rule's set holds the bits of the clean run;
  C. NaN surroundings: every input is a view into a NaN-filled buffer (NF.embed) -- the result holds the bits of the clean run on
     plainly allocated inputs and no NaN.  A load past an operand's edge that a product with zero would hide shows here.
Every case draws position-dependent inputs (NF.draw), makes one clean run and one run per plant through the same path (the small-
launch counter of the GEMMs and the planner's answer are asserted to agree), and plants floating-point data only.

Results that fp32 atomics accumulate in an order that differs from run to run (a weight gradient split over several k slices, the
`atomic_colsum` form of the dgrad) have no bit-reproducible clean run: they are compared by NaN set only, and the same problem is run
once more with splitk = 1 / through the workspace form for the bit comparison."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import ops
    from octcubem_amd._lib import call, load
    LP = ops.BF16
else:
    LP = torch.bfloat16
from tests import nonfinite as NF
from tests.test_gpu_kernels import tile_variant  # noqa: F401  (the GEMM kernel-choice fixture)

DEV = "cuda"
NAN, INF = NF.NAN, NF.INF
VALUES = {"nan": NAN, "+inf": INF, "-inf": -INF}
EPS = 1e-6
TILE_PAD = 256          # rows of NaN above and below an embedded operand: a whole 256-row tile past the edge lands in them
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _judge(family, tag, value, clean, bad, rule, ref=None, bits=True, nonfinite=False, loose=None):
    """kind A for a NaN, kind B for an Inf (ref: a callable that returns the float64 tensors by name).  bits=False (or the names of
    some tensors): what fp32 atomics make irreproducible, NaN set only.  nonfinite: the rule speaks of non-finite values (the
    optimizer), NaN and Inf plants alike.  loose: per tensor, the elements a documented choice lets differ in bits (NF.check)."""
    r = None
    for name, mask in rule.items():
        exact = not (bits is False or (isinstance(bits, (set, tuple)) and name in bits))
        c = clean[name] if exact else torch.where(mask.to(DEV), clean[name], bad[name])      # no clean bits to compare with
        lo = None if loose is None else loose[name]
        if value != value or nonfinite:
            NF.check(f"{family}: {tag}/{name}", c, bad[name], mask, nonfinite=nonfinite, loose=lo)
        else:
            r = ref() if r is None else r
            NF.check_weak(f"{family}: {tag}/{name}", c, bad[name], mask, NF.any_nonfinite(r[name]), loose=lo)


def _same(family, tag, clean, got, bits=True):
    """kind C: the bits of the clean run and no NaN"""
    for name, t in got.items():
        exact = not (bits is False or (isinstance(bits, (set, tuple)) and name in bits))
        NF.check(f"{family}: {tag}/{name}", clean[name] if exact else t, t, torch.zeros(t.shape, dtype=torch.bool), nonfinite=True)


def _small_launches(fn):
    n0 = ops.set_option("gemm_small_launches", 0)
    out = fn()
    return out, ops.set_option("gemm_small_launches", 0) - n0


def _plan(kind, NA, NB, K, lda, ldb, splitk=0):
    out = (ctypes.c_int * 13)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rc = load().octmae_gemm_plan(kind, NA, NB, K, lda, ldb, ops._variant_bits(), splitk, 1, cus, out)
    return rc, list(out)


# ================================================================================================================== GEMM
GEMM_SHAPES = [(333, 264, 192),      # partial tiles in both directions
               (600, 512, 256),      # more than one 256-tile along M
               (130, 768, 512)]      # the small-launch kernel, with a forced split under the small*_split* variants
_GEMM = {}


def _gemm_case(M, N, K):
    """x [M, K], w [N, K], dy [M, N], pre [M, K] in the operand type; bias, res, the accumulators and the row scales fp32 (non-zero
    scales: a zero one is the drop-path's documented pass-through of the residual)"""
    if (M, N, K) not in _GEMM:
        s = 1000 * M + N + K
        rps = 3 if M % 3 == 0 else 2
        c = {"x": NF.draw((M, K), s + 1).to(LP), "w": NF.draw((N, K), s + 2, K ** -0.5).to(LP), "bias": NF.draw((N,), s + 3),
             "res": NF.draw((M, N), s + 4), "dy": NF.draw((M, N), s + 5).to(LP), "pre": NF.draw((M, K), s + 6).to(LP),
             "gw": NF.draw((N, K), s + 7), "gb": NF.draw((N,), s + 8), "cs": NF.draw((K,), s + 9),
             "rowscale": torch.tensor([1.25, 2.0, 0.5])[torch.arange(M // rps) % 3]}
        _GEMM[(M, N, K)] = ({k: v.to(DEV) for k, v in c.items()}, rps)
    return _GEMM[(M, N, K)]


def _fwd_modes(rps):
    """name -> (the launch on a dict of operands, the operands it reads, the float64 evaluation)"""
    def gelu(store):
        def run(t):
            pre, act = ops.linear_fwd(t["x"], t["w"], t["bias"], "gelu", store_dgelu=store)
            return {"pre": pre, "act": act}
        return run

    def ref_gelu(store):
        def ref(t):
            r = NF.ref_linear_fwd(t["x"], t["w"], t["bias"], gelu=True)
            return {"pre": NF.dgelu64(r["pre"]) if store else r["pre"], "act": r["act"]}
        return ref
    xwb = ("x", "w", "bias")
    return {
        "bf16": (lambda t: {"out": ops.linear_fwd(t["x"], t["w"], t["bias"], "bf16")}, xwb, lambda t: NF.ref_linear_fwd(t["x"], t["w"], t["bias"])),
        "f32": (lambda t: {"out": ops.linear_fwd(t["x"], t["w"], t["bias"], "f32")}, xwb, lambda t: NF.ref_linear_fwd(t["x"], t["w"], t["bias"])),
        "f32_nobias": (lambda t: {"out": ops.linear_fwd(t["x"], t["w"], None, "f32")}, ("x", "w"), lambda t: NF.ref_linear_fwd(t["x"], t["w"], None)),
        "gelu": (gelu(False), xwb, ref_gelu(False)),
        "gelu_stored_prime": (gelu(True), xwb, ref_gelu(True)),
        "resid": (lambda t: {"out": ops.linear_fwd(t["x"], t["w"], t["bias"], "resid", res=t["res"])}, xwb + ("res",),
                  lambda t: NF.ref_linear_fwd(t["x"], t["w"], t["bias"], res=t["res"])),
        "rowscale": (lambda t: {"out": ops.linear_fwd(t["x"], t["w"], t["bias"], "resid", res=t["res"], rowscale=t["rowscale"],
                                                      rows_per_scale=rps)}, xwb + ("res", "rowscale"),
                     lambda t: NF.ref_linear_fwd(t["x"], t["w"], t["bias"], res=t["res"], rowscale=t["rowscale"], rows_per_scale=rps)),
    }


def _fwd_plants(M, N, K, rps):
    """the first row, the last row of the last partial tile, the last k-tile"""
    return [("x", (0, 1)), ("x", (M - 1, 5)), ("x", (7, K - 1)), ("w", (0, 0)), ("w", (N - 1, 3)), ("w", (9, K - 1)),
            ("bias", (0,)), ("bias", (N - 1,)), ("res", (0, 0)), ("res", (M - 1, N - 1)), ("rowscale", (0,)), ("rowscale", (M // rps - 1,))]


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_linear_fwd_plants(M, N, K, value, tile_variant):
    """ops.linear_fwd in every mode (kinds A and B): x[i, k] -> row i of every output, w[j, k] and bias[j] -> column j, res[i, j] ->
    that element, rowscale[s] -> the rows of its group; in the gelu modes the second output follows the first."""
    c, rps = _gemm_case(M, N, K)
    v = VALUES[value]
    for mode, (run, reads, ref) in _fwd_modes(rps).items():
        clean, n_clean = _small_launches(lambda: run(c))
        for what, idx in _fwd_plants(M, N, K, rps):
            if what not in reads:
                continue
            t = dict(c)
            t[what] = NF.plant(c[what], idx, v)
            bad, n_bad = _small_launches(lambda: run(t))
            assert n_bad == n_clean, f"{mode}: the planted run took another kernel ({n_bad} small launches, the clean run {n_clean})"
            m = NF.rule_linear_fwd(M, N, what, idx, rps)
            _judge("gemm_fwd", f"[{tile_variant}] {mode} {what}{idx}={value}", v, clean, bad, {k: m for k in clean}, lambda: ref(t))


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_linear_fwd_nan_surroundings(M, N, K, tile_variant):
    """Kind C: x, w and res are column slices of wider NaN-filled buffers with 256 NaN rows above and below (leading dimensions K + 8 and
    N + 8), bias and the row scales sit between NaN elements.  Where tests/test_gpu_gemm_elements.py pads with zeros."""
    c, rps = _gemm_case(M, N, K)
    e = {k: NF.embed(v, TILE_PAD, 8) if v.dim() == 2 else NF.embed(v, 8, flat=True) for k, v in c.items()}
    assert _plan(0, N, M, K, K, K) == _plan(0, N, M, K, K + 8, K + 8), "the leading dimension changes the launch plan"
    for mode, (run, _, _) in _fwd_modes(rps).items():
        clean, n_clean = _small_launches(lambda: run(c))
        got, n_got = _small_launches(lambda: run(e))
        assert n_got == n_clean, (mode, n_got, n_clean)
        _same("gemm_fwd", f"[{tile_variant}] {mode} embedded", clean, got)


def _dgrad_forms():
    """plain; x gelu'(pre) with no column sums; the column sums through the per-slab workspace, and that entry point without them
    (fold_entry); through fp32 atomics (no bit-reproducible sums); and the stored-gelu' route"""
    def run(pre=False, colsum=None, **kw):
        def go(t):
            cs = (t["cs"].clone() if t["cs"]._base is None else NF.embed(t["cs"], 8, flat=True)) if colsum else None
            dx = ops.linear_dgrad(t["dy"], t["w"], pre=t["pre"] if pre else None, colsum=cs, **kw)
            return {"dx": dx, "colsum": cs} if colsum else {"dx": dx}
        return go

    def ref(pre, stored=False):
        def go(t):
            r = NF.ref_linear_dgrad(t["dy"], t["w"])
            if pre:
                dx = r["dx"] * (t["pre"].double() if stored else NF.dgelu64(t["pre"].double()))
                r = {"dx": dx, "colsum": dx.sum(0)}
            return r
        return go
    return {"plain": (run(), ("dy", "w"), ref(False), ()),
            "dgelu": (run(True), ("dy", "w", "pre"), ref(True), ()),
            "dgelu_colsum_ws": (run(True, True), ("dy", "w", "pre"), ref(True), ()),
            "dgelu_fold_entry": (run(True, fold_entry=True), ("dy", "w", "pre"), ref(True), ()),
            "dgelu_colsum_atomic": (run(True, True, atomic_colsum=True), ("dy", "w", "pre"), ref(True), ("colsum",)),
            "dgelu_stored_colsum_ws": (run(True, True, pre_is_dgelu=True), ("dy", "w", "pre"), ref(True, True), ())}


def _dgrad_plants(M, N, K):
    return [("dy", (0, 0)), ("dy", (M - 1, 5)), ("dy", (7, N - 1)), ("w", (0, 0)), ("w", (N - 1, K - 1)), ("w", (3, K // 2)),
            ("pre", (0, 0)), ("pre", (M - 1, K - 1))]


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_linear_dgrad_plants(M, N, K, value, tile_variant):
    """ops.linear_dgrad in its three branches (kinds A and B): dy[i, n] -> row i of dx and the whole column sum; w[n, k] -> column k of
    dx and colsum[k]; pre[i, k] -> dx[i, k] and colsum[k] only.  The column sums start from non-zero values."""
    c, _ = _gemm_case(M, N, K)
    v = VALUES[value]
    for form, (run, reads, ref, loose) in _dgrad_forms().items():
        clean, n_clean = _small_launches(lambda: run(c))
        for what, idx in _dgrad_plants(M, N, K):
            if what not in reads:
                continue
            t = dict(c)
            t[what] = NF.plant(c[what], idx, v)
            bad, n_bad = _small_launches(lambda: run(t))
            assert n_bad == n_clean, f"{form}: the planted run took another kernel ({n_bad} small launches, the clean run {n_clean})"
            rule = NF.rule_linear_dgrad(M, K, what, idx)
            _judge("gemm_dgrad", f"[{tile_variant}] {form} {what}{idx}={value}", v, clean, bad, {k: rule[k] for k in clean},
                   lambda: ref(t), bits=loose or True)


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_linear_dgrad_nan_surroundings(M, N, K, tile_variant):
    """Kind C: dy (k-contiguous, N + 8 wide), w (k-strided: the reduction runs down its rows, 256 NaN rows follow the last) and pre as
    column slices of NaN-filled buffers."""
    c, _ = _gemm_case(M, N, K)
    e = {k: NF.embed(v, TILE_PAD, 8) if v.dim() == 2 else NF.embed(v, 8, flat=True) for k, v in c.items()}
    for kind in (1, 2, 3):
        assert _plan(kind, K, M, N, K, N) == _plan(kind, K, M, N, K + 8, N + 8), "the leading dimension changes the launch plan"
    for form, (run, _, _, loose) in _dgrad_forms().items():
        clean, n_clean = _small_launches(lambda: run(c))
        got, n_got = _small_launches(lambda: run(e))
        assert n_got == n_clean, (form, n_got, n_clean)
        _same("gemm_dgrad", f"[{tile_variant}] {form} embedded", clean, got, bits=loose or True)


# ------------------------------------------------------------------------------------------------ dgrad + delta
_DELTA = {}


def _delta_case(B, H, N, HD):
    key = (B, H, N, HD)
    if key not in _DELTA:
        M, C = B * N, H * HD
        s = 7 * M + C
        _DELTA[key] = {k: t.to(LP).to(DEV) for k, t in (("dy", NF.draw((M, C), s + 1)), ("w", NF.draw((C, C), s + 2, C ** -0.5)),
                                                          ("o", NF.draw((M, C), s + 3)))}
    return _DELTA[key]


def _run_delta(t, H, HD, tile_variant):
    """-> outputs, and the path is the one the planner names: no delta exactly under the forced register-staged kernel or a -2"""
    M, C = t["dy"].shape
    dx, delta = ops.linear_dgrad_delta(t["dy"], t["w"], t["o"], H, HD)
    declined = tile_variant == "tile128" or _plan(4, C, M, C, t["w"].stride(0), t["dy"].stride(0))[0] == -2
    assert (delta is None) == declined, f"[{tile_variant}] delta {'missing' if delta is None else 'present'} against the planner's answer"
    return {"dx": dx} if delta is None else {"dx": dx, "delta": delta}


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("B,H,N,HD", [(1, 4, 300, 64), (2, 8, 513, 32)])
def test_linear_dgrad_delta_plants(B, H, N, HD, value, tile_variant):
    """ops.linear_dgrad_delta at the two shapes of test_attention_rows_fused_backward_with_the_proj_dgrad_delta: o[i, c] ->
    delta[i, c // hd] only, dx untouched; dy[i, n] -> row i of dx and of delta; w[n, k] -> column k of dx, head k // hd of delta.
    Under the variant the entry point declines, the plain dgrad it falls back to is held to the dx part of the rule."""
    c = _delta_case(B, H, N, HD)
    M, C = B * N, H * HD
    v = VALUES[value]
    clean, n_clean = _small_launches(lambda: _run_delta(c, H, HD, tile_variant))
    for what, idx in [("o", (0, 0)), ("o", (M - 1, C - 1)), ("o", (M // 2, HD)), ("dy", (0, 3)), ("dy", (M - 1, C - 1)), ("w", (C - 1, HD - 1)),
                      ("w", (0, C - 1))]:
        t = dict(c)
        t[what] = NF.plant(c[what], idx, v)
        bad, n_bad = _small_launches(lambda: _run_delta(t, H, HD, tile_variant))
        assert n_bad == n_clean and bad.keys() == clean.keys()
        rule = NF.rule_dgrad_delta(M, C, H, HD, what, idx)
        _judge("gemm_delta", f"[{tile_variant}] delta {what}{idx}={value}", v, clean, bad, {k: rule[k] for k in clean},
               lambda: NF.ref_dgrad_delta(t["dy"], t["w"], t["o"], H, HD))


@pytest.mark.parametrize("B,H,N,HD", [(1, 4, 300, 64), (2, 8, 513, 32)])
def test_linear_dgrad_delta_nan_surroundings(B, H, N, HD, tile_variant):
    c = _delta_case(B, H, N, HD)
    e = {k: NF.embed(v, TILE_PAD, 8) for k, v in c.items()}
    clean, n_clean = _small_launches(lambda: _run_delta(c, H, HD, tile_variant))
    got, n_got = _small_launches(lambda: _run_delta(e, H, HD, tile_variant))
    assert n_got == n_clean and got.keys() == clean.keys()
    _same("gemm_delta", f"[{tile_variant}] delta embedded", clean, got)


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad_run(t, splitk=None):
    """gw, gb start from the non-zero accumulators of the case.  splitk None: ops.linear_wgrad_accum (the planner's split)."""
    gw, gb = t["gw"].clone() if t["gw"].is_contiguous() else NF.embed(t["gw"], TILE_PAD, 8), t["gb"].clone()
    if splitk is None:
        ops.linear_wgrad_accum(t["dy"], t["x"], gw, gb)
    else:
        M, N = t["dy"].shape
        K = t["x"].shape[1]
        ops._gemm(t["dy"], t["x"], gw, N, K, M, t["dy"].stride(0), t["x"].stride(0), gw.stride(0), 1, 1, ops.EPI_ACCUM, C2=gb, splitk=splitk)
    return {"gw": gw, "gb": gb}


def _wgrad_plants(M, N, K):
    return [("dy", (0, 0)), ("dy", (M - 1, N - 1)), ("dy", (M // 2, 5)), ("x", (0, 0)), ("x", (M - 1, K - 1)), ("x", (M // 2, 9))]


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_linear_wgrad_plants(M, N, K, value, tile_variant):
    """ops.linear_wgrad_accum with gb on non-zero accumulators: dy[m, n] -> row n of gw and gb[n]; x[m, k] -> column k of gw, gb
    untouched.  Where the planner keeps the reduction on one k slice the rest is the clean accumulation bit for bit; a split over
    several slices adds by fp32 atomics and is compared by NaN set, and the same problem runs once more with splitk = 1 for the bits."""
    c, _ = _gemm_case(M, N, K)
    v = VALUES[value]
    for splitk in (None, 1):
        rc, plan = _plan(6, N, K, M, N, K, splitk or 0)
        assert rc == 0 and (splitk is None or plan[5] == 1)
        exact = plan[5] == 1
        clean = _wgrad_run(c, splitk)
        for what, idx in _wgrad_plants(M, N, K):
            t = dict(c)
            t[what] = NF.plant(c[what], idx, v)
            bad = _wgrad_run(t, splitk)
            _judge("gemm_wgrad", f"[{tile_variant}] wgrad splitk {splitk} ({plan[5]} slices) {what}{idx}={value}", v, clean, bad,
                   NF.rule_wgrad(N, K, what, idx), lambda: NF.ref_wgrad(t["dy"], t["x"], t["gw"], t["gb"]), bits=exact)


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_linear_wgrad_nan_surroundings(M, N, K, tile_variant):
    """Kind C: dy and x are k-strided here (the reduction runs down their M rows: the 256 NaN rows below are what a k-tile past M would
    read), gw is a column slice of a NaN-filled accumulator, gb sits between NaN elements."""
    c, _ = _gemm_case(M, N, K)
    e = {k: NF.embed(v, TILE_PAD, 8) if v.dim() == 2 else NF.embed(v, 8, flat=True) for k, v in c.items()}
    for splitk in (None, 1):
        plans = [_plan(6, N, K, M, N + p, K + p, splitk or 0) for p in (0, 8)]
        assert plans[0] == plans[1] and plans[0][0] == 0, "the leading dimension changes the launch plan"
        clean, got = _wgrad_run(c, splitk), _wgrad_run(e, splitk)
        assert got["gw"].stride(0) == K + 8
        _same("gemm_wgrad", f"[{tile_variant}] wgrad splitk {splitk} embedded", clean, got, bits=plans[0][1][5] == 1)


_PAIR = {}
PAIR_ROWS = [130, 600]          # the rows of the small-launch and of the two-tile GEMM shape


def _pair_case(M):
    if M not in _PAIR:
        probs = []
        for i, (N, K) in enumerate(((512, 256), (256, 512))):
            s = 31 * M + i
            probs.append({"dy": NF.draw((M, N), s + 1).to(LP).to(DEV), "x": NF.draw((M, K), s + 3).to(LP).to(DEV),
                          "gw": NF.draw((N, K), s + 5).to(DEV), "gb": NF.draw((N,), s + 7).to(DEV)})
        _PAIR[M] = probs
    return _PAIR[M]


def _pair_run(probs):
    outs = [(p["gw"].clone() if p["gw"].is_contiguous() else NF.embed(p["gw"], TILE_PAD, 8), p["gb"].clone()) for p in probs]
    n0 = ops.set_option("gemm_small_wgrad_launches", 0)
    ops.linear_wgrad_accum_pair(*[(p["dy"], p["x"], gw, gb) for p, (gw, gb) in zip(probs, outs)])
    took128 = ops.set_option("gemm_small_wgrad_launches", 0) - n0
    return {"gw0": outs[0][0], "gb0": outs[0][1], "gw1": outs[1][0], "gb1": outs[1][1]}, took128


def _pair_plan(M, tile_variant, pad=0):
    """(plan kernel, k slices) of the pair launch; under the forced register-staged kernel the pair runs as two single launches"""
    out = (ctypes.c_int * 14)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert load().octmae_wgrad_pair_plan(512, 256, 512 + pad, 256 + pad, 256, 512, 256 + pad, 512 + pad, M, 0, cus, out) == 0
    if tile_variant == "tile128":
        return 0, max(_plan(6, 512, 256, M, 512 + pad, 256 + pad)[1][5], _plan(6, 256, 512, M, 256 + pad, 512 + pad)[1][5])
    return out[0], out[2]


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("M", PAIR_ROWS)
def test_linear_wgrad_pair_plants(M, value, tile_variant):
    """ops.linear_wgrad_accum_pair of (512, 256) + (256, 512), a bias gradient on both: the wgrad rules on the problem that holds the
    plant, and the other problem's outputs untouched -- bit for bit where the pair runs on one k slice."""
    probs = _pair_case(M)
    v = VALUES[value]
    kernel, slices = _pair_plan(M, tile_variant)
    clean, took = _pair_run(probs)
    assert took == (1 if kernel == 3 else 0), (tile_variant, kernel, took)
    for which in (0, 1):
        N, K = probs[which]["gw"].shape
        for what, idx in [("dy", (0, N - 1)), ("dy", (M - 1, 0)), ("x", (M - 1, K - 1)), ("x", (0, 7))]:
            t = [dict(p) for p in probs]
            t[which][what] = NF.plant(probs[which][what], idx, v)
            bad, took_bad = _pair_run(t)
            assert took_bad == took
            r = NF.rule_wgrad(N, K, what, idx)
            o = 1 - which
            rule = {f"gw{which}": r["gw"], f"gb{which}": r["gb"], f"gw{o}": torch.zeros_like(clean[f"gw{o}"], dtype=torch.bool).cpu(),
                    f"gb{o}": torch.zeros_like(clean[f"gb{o}"], dtype=torch.bool).cpu()}

            def ref():
                out = {}
                for i, p in enumerate(t):
                    rr = NF.ref_wgrad(p["dy"], p["x"], p["gw"], p["gb"])
                    out[f"gw{i}"], out[f"gb{i}"] = rr["gw"], rr["gb"]
                return out
            _judge("gemm_wgrad_pair", f"[{tile_variant}] pair M {M} ({slices} slices) problem {which} {what}{idx}={value}", v, clean, bad,
                   rule, ref, bits=slices == 1)


@pytest.mark.parametrize("M", PAIR_ROWS)
def test_linear_wgrad_pair_nan_surroundings(M, tile_variant):
    probs = _pair_case(M)
    e = [{k: NF.embed(v, TILE_PAD, 8) if v.dim() == 2 else NF.embed(v, 8, flat=True) for k, v in p.items()} for p in probs]
    plan = _pair_plan(M, tile_variant)
    assert plan == _pair_plan(M, tile_variant, 8), "the leading dimension changes the launch plan"
    (clean, took), (got, took_e) = _pair_run(probs), _pair_run(e)
    assert took == took_e == (1 if plan[0] == 3 else 0)
    _same("gemm_wgrad_pair", f"[{tile_variant}] pair M {M} embedded", clean, got, bits=plan[1] == 1)


# ================================================================================================================== attention
ATTN_SHAPES = [(2, 3, 65, 64), (2, 3, 300, 64), (2, 3, 513, 32), (1, 2, 31, 32)]
_ATTN = {}


def _attn_case(B, H, N, HD):
    """qkv, dO drawn; o, lse of the default forward and of the online-max forward; delta = -rowsum(dO o) in fp32"""
    key = (B, H, N, HD)
    if key not in _ATTN:
        s = 17 * N + HD
        c = {"qkv": NF.draw((B * N, 3 * H * HD), s + 1).to(LP).to(DEV), "dO": NF.draw((B * N, H * HD), s + 2).to(LP).to(DEV)}
        c["o"], c["lse"] = ops.attn_fwd(c["qkv"], B, N, H, HD, HD ** -0.5)
        c["delta"] = -(c["dO"].float() * c["o"].float()).view(B * N, H, HD).sum(-1).contiguous()
        _ATTN[key] = c
    return _ATTN[key]


def _positions(B, H, N):
    """(b, h, row): sample 0, head 1 at row 0, at the last row of a full 64-row tile and at row N - 1 (the single query or key past the
    last full block at N = 65 and 513); and sample 1, head 0, row 0 -- where a kernel lands that runs one row past the end of sample 0"""
    full = (N - 1) // 64 * 64 - 1
    pos = [(0, 1, 0)] + ([(0, 1, full)] if full > 0 else []) + [(0, 1, N - 1)]
    return pos + ([(1, 0, 0)] if B > 1 else [])


def _fwd(t, dims, optimistic):
    B, H, N, HD = dims
    o, lse = ops.attn_fwd(t["qkv"], B, N, H, HD, HD ** -0.5, optimistic=optimistic)
    return {"o": o.view(B, N, H, HD), "lse": lse}


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("optimistic", [True, False, None])
@pytest.mark.parametrize("B,H,N,HD", ATTN_SHAPES)
def test_attn_fwd_plants(B, H, N, HD, optimistic, value):
    """ops.attn_fwd: q[b, n, h, d] -> o[b, n, h, :] and lse[b, h, n]; k[b, m, h, d] -> every o[b, :, h, :] and lse[b, h, :];
    v[b, m, h, d] -> o[b, :, h, d] only, lse untouched; every other (b, h) slice untouched.
    The clean result the rest is compared with is the ONLINE-MAX kernel's (optimistic=False) in all three forms: a non-finite row sum or
    accumulator of o raises the optimistic kernel's give-up flag (csrc/attn.hip, the test at the end of attn_fwd_kernel) and the
    online-max kernel, enqueued behind it, recomputes the whole launch; the half build runs that kernel only.
    One documented choice of that kernel is encoded (NF.attn_fwd_wave_rows): its rescale decision is wave-uniform, so the 31 query rows
    that share a wave with a planted q row may be rounded at another reference point -- they are held to the NaN set, not to the bits."""
    dims = (B, H, N, HD)
    c = _attn_case(*dims)
    v = VALUES[value]
    clean = _fwd(c, dims, False)
    for b, h, n in _positions(B, H, N):
        for which, what in enumerate("qkv"):
            d = (0, HD - 1, 5)[which]
            t = {"qkv": NF.plant(c["qkv"].view(B, N, 3, H, HD), (b, n, which, h, d), v).view_as(c["qkv"])}
            bad = _fwd(t, dims, optimistic)
            _judge("attn_fwd", f"attn_fwd optimistic={optimistic} {what}{(b, n, h, d)}={value}", v, clean, bad,
                   NF.rule_attn_fwd(B, H, N, HD, what, (b, n, h, d)), lambda: NF.ref_attn_fwd(t["qkv"], B, N, H, HD),
                   loose=NF.attn_fwd_wave_rows(B, H, N, HD, (b, n, h, d)) if what == "q" else None)


@pytest.mark.parametrize("optimistic", [True, False, None])
@pytest.mark.parametrize("B,H,N,HD", ATTN_SHAPES)
def test_attn_fwd_nan_surroundings(B, H, N, HD, optimistic):
    """Kind C, the flat form (qkv is a packed tensor with no leading dimension in the entry point): 256 rows of NaN before and after.
    For the last sample and head the keys >= N and the whole tiles past the last one (csrc/attn_tile.hpp) are that suffix."""
    dims = (B, H, N, HD)
    c = _attn_case(*dims)
    _same("attn_fwd", f"attn_fwd optimistic={optimistic} embedded", _fwd(c, dims, optimistic),
          _fwd({"qkv": NF.embed(c["qkv"], TILE_PAD, flat=True)}, dims, optimistic))


def _bwd_forms(HD):
    """the forms of tests/test_gpu_attention_rows.py::_Case.every_form, and the delta= form: name -> (fused, options, with delta)"""
    key = f"attn_bwd_hd{HD}_form"
    return {"pair": (False, {}, False), "fused_form1": (True, {key: 1, "attn_bwd_tail_fused": 1}, False),
            "fused_form0": (True, {key: 0, "attn_bwd_tail_fused": 1}, False), "fused_tail_unfused": (True, {key: 1, "attn_bwd_tail_fused": 0}, False),
            "fused_delta": (True, {key: 1, "attn_bwd_tail_fused": 1}, True)}


def _bwd(t, dims, fused, with_delta):
    B, H, N, HD = dims
    d = ops.attn_bwd(t["qkv"], t["o"], t["dO"], t["lse"], B, N, H, HD, HD ** -0.5, fused=fused, delta=t["delta"] if with_delta else None)
    return {"dqkv": d.view(B, N, 3, H, HD)}


class _options:
    def __init__(self, opts):
        self.opts, self.prev = opts, {}

    def __enter__(self):
        for k, v in self.opts.items():
            self.prev[k] = ops.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            ops.set_option(k, v)


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("form", list(_bwd_forms(64)))
@pytest.mark.parametrize("B,H,N,HD", ATTN_SHAPES)
def test_attn_bwd_plants(B, H, N, HD, form, value):
    """ops.attn_bwd for given qkv, o, lse: dO[b, n, h, d] -> dV[b, :, h, d], dQ[b, n, h, :] and every dK[b, :, h, :]; o[b, n, h, d] or
    lse[b, h, n] -> dQ[b, n, h, :] and dK[b, :, h, :], lse also dV[b, :, h, :]; in the delta= form delta[b N + n, h] as o (o itself is
    not read there).  Every other (b, h) slice untouched."""
    dims = (B, H, N, HD)
    c = _attn_case(*dims)
    v = VALUES[value]
    fused, opts, with_delta = _bwd_forms(HD)[form]
    with _options(opts):
        clean = _bwd(c, dims, fused, with_delta)
        for b, h, n in _positions(B, H, N):
            plants = [("dO", (b, n, h, 3)), ("lse", (b, h, n)), ("delta", (b * N + n, h)) if with_delta else ("o", (b, n, h, HD - 1))]
            for what, idx in plants:
                t = dict(c)
                shape = (B, N, H, HD) if what in ("dO", "o") else c[what].shape
                t[what] = NF.plant(c[what].view(shape), idx, v).view_as(c[what])
                bad = _bwd(t, dims, fused, with_delta)
                _judge("attn_bwd", f"attn_bwd {form} {what}{idx}={value}", v, clean, bad, {"dqkv": NF.rule_attn_bwd(B, H, N, HD, what, idx)},
                       lambda: {"dqkv": NF.ref_attn_bwd(t["qkv"], t["o"], t["dO"], t["lse"], B, N, H, HD, delta=t["delta"] if with_delta else None)})


@pytest.mark.parametrize("form", list(_bwd_forms(64)))
@pytest.mark.parametrize("B,H,N,HD", ATTN_SHAPES)
def test_attn_bwd_nan_surroundings(B, H, N, HD, form):
    """Kind C, the flat form (packed tensors; ops._chk refuses a strided delta): qkv, o, dO, lse and delta each between 256 rows of NaN.
    The padded query rows and keys of the last (b, h) slice (csrc/attn_bwd.hip: "a padded query row then gives P = exp2(-1e30) = 0 and
    dS = 0 whatever the zero-filled Q / dO rows produce") are that NaN suffix."""
    dims = (B, H, N, HD)
    c = _attn_case(*dims)
    fused, opts, with_delta = _bwd_forms(HD)[form]
    e = {k: NF.embed(v, TILE_PAD, flat=True) for k, v in c.items()}
    with _options(opts):
        _same("attn_bwd", f"attn_bwd {form} embedded", _bwd(c, dims, fused, with_delta), _bwd(e, dims, fused, with_delta))


# ================================================================================================================== LayerNorm
LN_SHAPES = [(7, 64), (33, 128), (300, 768)]
_LN = {}


def _ln_case(M, D):
    if (M, D) not in _LN:
        s = 13 * M + D
        c = {"x": NF.draw((M, D), s + 1), "gamma": NF.draw((D,), s + 2), "beta": NF.draw((D,), s + 3), "dy": NF.draw((M, D), s + 4).to(LP),
             "dres": NF.draw((M, D), s + 5), "dgamma": NF.draw((D,), s + 6), "dbeta": NF.draw((D,), s + 7), "dxsum": NF.draw((D,), s + 8)}
        _LN[(M, D)] = {k: v.to(DEV) for k, v in c.items()}
    return _LN[(M, D)]


def _ln_fwd(t):
    y, mean, rstd = ops.layernorm_fwd(t["x"], t["gamma"], t["beta"], EPS)
    return {"y": y, "mean": mean, "rstd": rstd}


def _ln_bwd(t, full=True):
    """the statistics are the forward kernel's on the same x; full: dres, the 16-bit copy and the three column sums on non-zero
    accumulators; else the bare form"""
    f = _ln_fwd(t)
    if not full:
        dx, _ = ops.layernorm_bwd(t["dy"], t["x"], f["mean"], f["rstd"], t["gamma"], None, None)
        return {"dx": dx}
    sums = {k: t[k].clone() for k in ("dgamma", "dbeta", "dxsum")}
    dx, dxb = ops.layernorm_bwd(t["dy"], t["x"], f["mean"], f["rstd"], t["gamma"], sums["dgamma"], sums["dbeta"], dres=t["dres"],
                                want_bf16=True, dxsum=sums["dxsum"])
    return {"dx": dx, "dxb": dxb, **sums}


def _corners(M, D):
    return [(0, 0), (0, D - 1), (M - 1, 0), (M - 1, D - 1)]


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("M,D", LN_SHAPES)
def test_layernorm_plants(M, D, value):
    """layernorm_fwd, ln_apply and layernorm_bwd (bare, and with dres, want_bf16, dxsum): the rules of NF.rule_ln_fwd / _apply / _bwd at
    the first and last row and column.  In the backward an x plant is made before the forward, as in training."""
    c = _ln_case(M, D)
    v = VALUES[value]
    clean_f, clean_b, clean_bare = _ln_fwd(c), _ln_bwd(c), _ln_bwd(c, False)
    clean_a = {"y": ops.ln_apply(c["x"], clean_f["mean"], clean_f["rstd"], c["gamma"], c["beta"])}
    assert torch.equal(clean_a["y"], clean_f["y"])
    plants = [("x", i) for i in _corners(M, D)] + [("dy", i) for i in _corners(M, D)] + [("gamma", (0,)), ("gamma", (D - 1,)),
             ("beta", (0,)), ("beta", (D - 1,)), ("dres", (0, 0)), ("dres", (M - 1, D - 1)), ("mean", (0,)), ("rstd", (M - 1,))]
    for what, idx in plants:
        t = {**c, **clean_f}
        t[what] = NF.plant(t[what], idx, v)
        tag = f"M{M} D{D} {what}{idx}={value}"
        if what in ("x", "gamma", "beta"):
            _judge("layernorm", "layernorm_fwd " + tag, v, clean_f, _ln_fwd(t), NF.rule_ln_fwd(M, D, what, idx),
                   lambda: NF.ref_ln_fwd(t["x"], t["gamma"], t["beta"], EPS))
        if what in ("x", "gamma", "beta", "mean", "rstd"):
            _judge("layernorm", "ln_apply " + tag, v, clean_a, {"y": ops.ln_apply(t["x"], t["mean"], t["rstd"], t["gamma"], t["beta"])},
                   NF.rule_ln_apply(M, D, what, idx), lambda: NF.ref_ln_apply(t["x"], t["mean"], t["rstd"], t["gamma"], t["beta"]))
        if what in ("x", "dy", "gamma", "dres"):
            rule = NF.rule_ln_bwd(M, D, what, idx)
            rule["dxb"] = rule["dx"]

            def ref(dres=True):
                f = NF.ref_ln_fwd(t["x"], t["gamma"], t["beta"], EPS)
                r = NF.ref_ln_bwd(t["dy"], t["x"], f["mean"], f["rstd"], t["gamma"], t["dres"] if dres else None)
                return {"dx": r["dx"], "dxb": r["dx"], "dgamma": t["dgamma"].double() + r["dgamma"], "dbeta": t["dbeta"].double() + r["dbeta"],
                        "dxsum": t["dxsum"].double() + r["dxsum"]}
            _judge("layernorm", "layernorm_bwd full " + tag, v, clean_b, _ln_bwd(t), rule, ref)
            if what != "dres":
                _judge("layernorm", "layernorm_bwd bare " + tag, v, clean_bare, _ln_bwd(t, False), {"dx": rule["dx"]}, lambda: ref(False))


@pytest.mark.parametrize("M,D", LN_SHAPES)
def test_layernorm_nan_surroundings(M, D):
    """Kind C, the flat form: the entry points take no leading dimension (and ops.ln_apply's _chk refuses a strided tensor), so x, dy,
    dres, gamma, beta, the row statistics and the accumulators each sit contiguous between NaN elements (8 rows of them)."""
    c = _ln_case(M, D)
    e = {k: NF.embed(v, 8, flat=True) for k, v in c.items()}
    clean_f, got_f = _ln_fwd(c), _ln_fwd(e)
    _same("layernorm", f"layernorm_fwd M{M} D{D} embedded", clean_f, got_f)
    stats = {k: NF.embed(clean_f[k], 8, flat=True) for k in ("mean", "rstd")}
    _same("layernorm", f"ln_apply M{M} D{D} embedded", {"y": clean_f["y"]}, {"y": ops.ln_apply(e["x"], stats["mean"], stats["rstd"], e["gamma"], e["beta"])})
    sums = {k: NF.embed(c[k], 8, flat=True) for k in ("dgamma", "dbeta", "dxsum")}
    dx, dxb = ops.layernorm_bwd(e["dy"], e["x"], stats["mean"], stats["rstd"], e["gamma"], sums["dgamma"], sums["dbeta"], dres=e["dres"],
                                want_bf16=True, dxsum=sums["dxsum"])
    _same("layernorm", f"layernorm_bwd M{M} D{D} embedded", _ln_bwd(c), {"dx": dx, "dxb": dxb, **sums})
    for k, s in sums.items():           # the accumulators' own surroundings were not written
        outside = torch.ones_like(s._base, dtype=torch.bool)
        pad = (s._base.numel() - D) // 2
        outside[pad:pad + D] = False
        assert bool(torch.isnan(s._base[outside]).all()), k


# ------------------------------------------------------------------------------------------------ slice pool
POOL_SHAPES = [(1, 7, 5, 64), (3, 11, 17, 128), (30, 10, 3, 768)]      # (B, S, T, D): 7, 33 and 300 pooled rows of the LayerNorm widths
_POOL = {}


def _pool_case(B, S, T, D):
    key = (B, S, T, D)
    if key not in _POOL:
        s = 3 * B + 5 * S + T + D
        c = {"x": NF.draw((B * S, T, D), s + 1), "gamma": NF.draw((D,), s + 2), "beta": NF.draw((D,), s + 3), "dout": NF.draw((B, D), s + 4),
             "dgamma": NF.draw((D,), s + 5), "dbeta": NF.draw((D,), s + 6), "dxsum": NF.draw((D,), s + 7)}
        _POOL[key] = {k: v.to(DEV) for k, v in c.items()}
    return _POOL[key]


def _pool_run(t, S, cls):
    """forward, then the backward on the forward's own pooled rows and statistics, the sums on non-zero accumulators"""
    T = t["x"].shape[1]
    out, pooled, mean, rstd = ops.slice_pool_fwd(t["x"], t["gamma"], t["beta"], EPS, S, cls)
    sums = {k: t[k].clone() if t[k]._base is None else NF.embed(t[k], 8, flat=True) for k in ("dgamma", "dbeta", "dxsum")}
    dx, dxb = ops.slice_pool_bwd(t["dout"], pooled, mean, rstd, t["gamma"], T, S, cls, sums["dgamma"], sums["dbeta"], want_bf16=True,
                                 dxsum=sums["dxsum"])
    return {"out": out, "pooled": pooled, "mean": mean, "rstd": rstd, "dx": dx, "dxb": dxb, **sums}


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("B,S,T,D", POOL_SHAPES)
def test_slice_pool_plants(B, S, T, D, cls, value):
    """slice_pool_fwd / slice_pool_bwd: the LayerNorm rules per pooled group, from the composition of tests/slicehead_ref.py (x through a
    token the pooling uses -> its pooled element, its statistics, its volume's row of out, its slice's dx rows and all of dgamma;
    through a token it skips -> nothing)."""
    c = _pool_case(B, S, T, D)
    v = VALUES[value]
    clean = _pool_run(c, S, cls)
    BS = B * S
    plants = [("x", (0, 0, 0)), ("x", (0, 1, D - 1)), ("x", (BS - 1, T - 1, 0)), ("x", (BS - 1, 0, D - 1)), ("gamma", (0,)), ("gamma", (D - 1,)),
              ("beta", (D - 1,)), ("dout", (0, 0)), ("dout", (B - 1, D - 1))]
    for what, idx in plants:
        t = dict(c)
        t[what] = NF.plant(c[what], idx, v)
        rule = {k: torch.zeros(clean[k].shape, dtype=torch.bool) for k in clean}
        if what != "dout":
            rule.update(NF.rule_slice_pool_fwd(B, S, T, D, cls, what, idx))
        if what != "beta":
            rule.update(NF.rule_slice_pool_bwd(B, S, T, D, cls, what, idx))
        rule["dxb"] = rule["dx"]

        def ref():
            r = NF.ref_slice_pool(t["x"], t["gamma"], t["beta"], t["dout"], S, cls, EPS)
            r["dxb"] = r["dx"]
            for k in ("dgamma", "dbeta", "dxsum"):
                r[k] = r[k] + t[k].double()
            return r
        _judge("slice_pool", f"slice_pool cls={cls} {(B, S, T, D)} {what}{idx}={value}", v, clean, _pool_run(t, S, cls), rule, ref)


@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("B,S,T,D", POOL_SHAPES)
def test_slice_pool_nan_surroundings(B, S, T, D, cls):
    """Kind C, the flat form (no leading dimensions in the entry points): 8 rows of NaN before and after every input."""
    c = _pool_case(B, S, T, D)
    e = {k: NF.embed(v, 8, flat=True) for k, v in c.items()}
    _same("slice_pool", f"slice_pool cls={cls} {(B, S, T, D)} embedded", _pool_run(c, S, cls), _pool_run(e, S, cls))


# ================================================================================================================== optimizer
HYPER = dict(step=3, lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.05)
GS = 0.5


def _optim_lengths():
    return [5, 4096 + 3, load().octmae_mt_chunk_elems() + 1]


def _optim_world(g=None, sentinel=None):
    from tests.test_gpu_optim_kernels import World
    lengths = _optim_lengths()
    w = World(lengths, sentinel=sentinel)
    w.P.load([NF.draw((n,), 100 + n).numpy() for n in lengths])
    w.G.load(g if g is not None else _optim_grads())
    w.M.load([NF.draw((n,), 200 + n, 0.1).numpy() for n in lengths])
    w.V.load([NF.draw((n,), 300 + n, 0.1).abs().numpy() for n in lengths])
    return w


def _optim_grads():
    return [NF.draw((n,), 400 + n).numpy() for n in _optim_lengths()]


def _optim_plants():
    """(tensor, element): the n & 3 tail of the shortest, the tail past the vector loop, both chunks of the tensor that spans two"""
    L = _optim_lengths()
    return [(0, 4), (0, 0), (1, 4096 + 2), (2, 0), (2, L[2] - 1)]


def _planted_grads(t, i, v):
    g = _optim_grads()
    g[t][i] = v
    return g


@pytest.mark.parametrize("value", list(VALUES))
def test_optimizer_norm_plants(value):
    """octmae_mt_sumsq and octmae_mt_finish_norm: a NaN or Inf in g of tensor t makes sumsq[t] non-finite and leaves the others bit for
    bit; the norm is non-finite; the clip coefficient is NaN for a NaN norm (`if (c > 1.f) c = 1.f` keeps it) and 0 for an Inf norm."""
    v = VALUES[value]
    clean = torch.from_numpy(_optim_world().sumsq())
    lengths = _optim_lengths()
    for t, i in _optim_plants():
        bad = torch.from_numpy(_optim_world(_planted_grads(t, i, v)).sumsq())
        NF.check(f"mt_sumsq g[{t}][{i}]={value}", clean, bad, NF.rule_optim(lengths, t, i)["sumsq"], nonfinite=True)
        out = torch.full((2,), 7.0, device=DEV)
        sq = bad.to(DEV)
        call("octmae_mt_finish_norm", sq.data_ptr(), len(lengths), 1.0, out.data_ptr(), out.data_ptr() + 4, _stream())
        norm, coef = (float(x) for x in out.cpu())
        assert not np.isfinite(norm), (value, norm)
        assert np.isnan(coef) if np.isnan(norm) else coef == 0.0, (value, norm, coef)
        assert np.isnan(norm) == (value == "nan")
    out = torch.full((2,), 7.0, device=DEV)
    sq = clean.to(DEV)
    call("octmae_mt_finish_norm", sq.data_ptr(), len(lengths), 1.0, out.data_ptr(), out.data_ptr() + 4, _stream())
    assert bool(torch.isfinite(out).all())


def _adamw(w, variant, gs=GS, embed_scale=False):
    """one launch; "unfused" is octmae_mt_adamw, the others octmae_mt_adamw_fused through World.adamw (with its guard checks).
    embed_scale: *gscale sits between NaN elements"""
    h = HYPER
    gs_t = torch.tensor([gs], dtype=torch.float32, device=DEV)
    if embed_scale:
        gs_t = NF.embed(gs_t, 8, flat=True)
    if variant == "unfused":
        tab = w.table()
        call("octmae_mt_adamw", tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(), tab.n_chunks, gs_t.data_ptr(),
             h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"], _stream())
        torch.cuda.synchronize()
    else:
        w.adamw(variant, gs_t, h["step"], h["lr"], h["b1"], h["b2"], h["eps"], h["wd"])
    from tests.test_gpu_optim_kernels import VARIANTS
    lp, sq = VARIANTS.get(variant, (False, False))
    out = {}
    for t in range(len(w.lengths)):
        out.update({f"p{t}": w.P.views[t].clone(), f"m{t}": w.M.views[t].clone(), f"v{t}": w.V.views[t].clone()})
        if lp:
            out[f"lp{t}"] = w.LP.views[t].clone()
    if sq:
        out["sumsq"] = w.SQ.views[0].clone()
    return out


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("variant", ["unfused", "plain", "lp", "sq", "lp_sq"])
def test_optimizer_update_plants(variant, value):
    """octmae_mt_adamw and the four octmae_mt_adamw_fused kernels: exactly the planted element of p, m, v and of the 16-bit mirror is
    non-finite (and sumsq[t] with SQ), every other element and tensor is the clean update bit for bit."""
    v = VALUES[value]
    lengths = _optim_lengths()
    clean = _adamw(_optim_world(), variant)
    for t, i in _optim_plants():
        bad = _adamw(_optim_world(_planted_grads(t, i, v)), variant)
        r = NF.rule_optim(lengths, t, i)
        rule = {k: (r["sumsq"] if k == "sumsq" else r["elements"][int(k[-1])]) for k in clean}
        _judge("optimizer", f"mt_adamw {variant} g[{t}][{i}]={value}", v, clean, bad, rule, nonfinite=True)


@pytest.mark.parametrize("variant", ["unfused", "plain", "lp", "sq", "lp_sq"])
def test_optimizer_nan_gradient_scale(variant):
    """every g finite, the NaN in *gscale: every element of p, m, v and of the 16-bit mirror is NaN (sumsq is of the raw gradient)"""
    bad = _adamw(_optim_world(), variant, gs=NAN)
    for k, t in bad.items():
        if k != "sumsq":
            assert bool(torch.isnan(t).all()), f"{variant}: {k} has {int((~torch.isnan(t)).sum())} elements that are not NaN"


def test_optimizer_nan_surroundings():
    """Kind C: the same tables with p, g, m, v between NaN elements in place of World's finite sentinels, and *gscale between NaN
    elements (the 16-bit mirror and sumsq are outputs) -- sumsq and all five updates hold the bits of the run between finite
    sentinels."""
    for variant in ("sumsq", "unfused", "plain", "lp", "sq", "lp_sq"):
        clean_w = _optim_world()
        clean = {"sumsq": torch.from_numpy(clean_w.sumsq())} if variant == "sumsq" else _adamw(clean_w, variant)
        w = _optim_world(sentinel=NAN)
        for role in (w.P, w.G, w.M, w.V):
            assert bool(torch.isnan(role.buf[role.outside]).all())
        got = {"sumsq": torch.from_numpy(w.sumsq())} if variant == "sumsq" else _adamw(w, variant, embed_scale=True)
        _same("optimizer", f"optimizer {variant} embedded", clean, got)


# ================================================================================================================== tokens and loss
# The kernels of tests/test_gpu_tokens.py, at the smallest shape of each list there.  The rules (NF.rule_enc_assemble ... NF.rule_mse) and the
# float64 evaluations (NF.ref_*) live in tests/nonfinite.py; tests/test_cpu_nonfinite.py holds the one against the other.  The index
# tables are never planted.
def _tok_run(family_tag, value, c, run, plants, rule, ref, embed_rows=8):
    """one clean run, one per plant (kind A or B), and one with every floating-point input between NaN elements (kind C, the flat
    form: these entry points take no leading dimension).  run / ref: dict of operands -> dict of outputs; rule(what, idx) -> masks."""
    v = VALUES[value]
    clean = run(c)
    for what, idx in plants:
        t = dict(c)
        t[what] = NF.plant(c[what], idx, v)
        _judge("tokens", f"{family_tag} {what}{idx}={value}", v, clean, run(t), rule(what, idx), lambda: ref(t))
    _same("tokens", f"{family_tag} embedded", clean, run({k: NF.embed(t, embed_rows, flat=True) for k, t in c.items()}))


def _perm_prefix(B, L, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(L, generator=g)[:n] for _ in range(B)]).contiguous()


def _restore(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.argsort(torch.argsort(torch.rand(B, L, generator=g), dim=1), dim=1).contiguous()


@pytest.mark.parametrize("value", list(VALUES))
def test_enc_assemble_plants(value):
    """octmae_enc_assemble at (B, nkeep, D) = (1, 1, 4) with 4 table rows: tok[r, k] -> x[1 + r, k]; pos[l, k] -> the rows whose
    ids_keep is l (none for a row no token keeps); cls[k], pos_cls[k] -> x[0, k]."""
    B, nkeep, D, L = 1, 1, 4, 4
    c = {"tok": NF.draw((B * nkeep, D), 1).to(LP).to(DEV), "pos": NF.draw((L, D), 2).to(DEV), "cls": NF.draw((D,), 3).to(DEV),
         "pos_cls": NF.draw((D,), 4).to(DEV)}
    ids = torch.tensor([[2]], dtype=torch.int64)
    ids_dev = ids.to(DEV)

    def run(t):
        x = torch.empty(B * (nkeep + 1), D, device=DEV)
        call("octmae_enc_assemble", t["tok"].data_ptr(), t["pos"].data_ptr(), t["cls"].data_ptr(), t["pos_cls"].data_ptr(), ids_dev.data_ptr(),
             x.data_ptr(), B, nkeep, D, _stream())
        return {"x": x}
    _tok_run("enc_assemble", value, c, run, [("tok", (0, 3)), ("pos", (2, 0)), ("pos", (3, 1)), ("pos", (0, 0)), ("cls", (1,)), ("pos_cls", (3,))],
             lambda what, idx: {"x": NF.rule_enc_assemble(B, nkeep, D, ids, what, idx)},
             lambda t: {"x": NF.ref_enc_assemble(t["tok"], t["pos"], t["cls"], t["pos_cls"], ids_dev)})


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("emb_has_cls", [0, 1])
def test_dec_assemble_plants(emb_has_cls, value):
    """octmae_dec_assemble at (B, nkeep, L, D) = (3, 10, 40, 64): emb row r of sample b -> the one row j with ids_restore[b, j] = r (the
    cls row with emb_has_cls); mask_token[k] -> column k of every masked row; dpos[j, k] -> x[b, 1 + j, k] of every sample; dcls /
    dpos_cls -> the cls rows."""
    B, nkeep, L, D = 3, 10, 40, 64
    erows = nkeep + emb_has_cls
    c = {"emb": NF.draw((B * erows, D), 1).to(LP).to(DEV), "mask_token": NF.draw((D,), 2).to(DEV), "dpos": NF.draw((L, D), 3).to(DEV),
         "dcls": NF.draw((D,), 4).to(DEV), "dpos_cls": NF.draw((D,), 5).to(DEV)}
    ids = _restore(B, L, 5)
    ids_dev = ids.to(DEV)

    def run(t):
        x = torch.empty(B * (L + 1), D, device=DEV)
        call("octmae_dec_assemble", t["emb"].data_ptr(), t["mask_token"].data_ptr(), t["dpos"].data_ptr(),
             None if emb_has_cls else t["dcls"].data_ptr(), t["dpos_cls"].data_ptr(), ids_dev.data_ptr(), x.data_ptr(), B, nkeep, L, D,
             emb_has_cls, _stream())
        return {"x": x}
    plants = [("emb", (emb_has_cls, 0)), ("emb", (B * erows - 1, D - 1)), ("mask_token", (7,)), ("dpos", (0, 0)), ("dpos", (L - 1, D - 1)),
              ("dpos_cls", (1,)), ("emb", (1 * erows, 5)) if emb_has_cls else ("dcls", (2,))]
    _tok_run(f"dec_assemble cls={emb_has_cls}", value, c, run, plants,
             lambda what, idx: {"x": NF.rule_dec_assemble(B, nkeep, L, D, ids, emb_has_cls, what, idx)},
             lambda t: {"x": NF.ref_dec_assemble(t["emb"], t["mask_token"], t["dpos"], t["dcls"], t["dpos_cls"], ids_dev, nkeep, emb_has_cls)})


@pytest.mark.parametrize("value", list(VALUES))
def test_patch_gather_and_row_gather_plants(value):
    """octmae_patch_gather at (B, C, T, H, W, tp, p, nkeep) = (3, 3, 6, 64, 64, 3, 16, 8): a voxel of a kept token -> its one element of
    that token's row, a voxel of a token ids_keep leaves out -> nothing.  octmae_gather_rows_cast at (B, n, rows, D) = (1, 1, 2, 8), with
    and without ids: src[b, 1 + ids] -> that element of the row, the cls row src[b, 0] -> nothing."""
    B, C, T, H, W, tp, p, nkeep = 3, 3, 6, 64, 64, 3, 16, 8
    gh, gw = H // p, W // p
    Lt, kdim = (T // tp) * gh * gw, C * tp * p * p
    ids = _perm_prefix(B, Lt, nkeep, 9)
    ids_dev = ids.to(DEV)

    def run(t):
        out = torch.empty(B * nkeep, kdim, dtype=LP, device=DEV)
        call("octmae_patch_gather", t["imgs"].data_ptr(), ids_dev.data_ptr(), 1, out.data_ptr(), B, C, T, H, W, tp, p, nkeep, _stream())
        return {"out": out}

    def voxel(b, l, c_, u, py, px):
        return (b, c_, (l // (gh * gw)) * tp + u, ((l // gw) % gh) * p + py, (l % gw) * p + px)
    dropped = next(l for l in range(Lt) if l not in ids[1].tolist())
    plants = [("imgs", voxel(0, int(ids[0, 0]), 0, 0, 0, 0)), ("imgs", voxel(2, int(ids[2, nkeep - 1]), C - 1, tp - 1, p - 1, p - 1)),
              ("imgs", voxel(1, dropped, 1, 1, 3, 4))]
    _tok_run("patch_gather", value, {"imgs": NF.draw((B, C, T, H, W), 1).to(DEV)}, run, plants,
             lambda what, idx: {"out": NF.rule_patch_gather(B, C, T, H, W, tp, p, nkeep, ids, idx)},
             lambda t: {"out": NF.ref_patch_gather(t["imgs"], ids_dev, tp, p)}, embed_rows=64)
    Bn, n, src_rows, D = 1, 1, 2, 8
    for ids2 in (None, torch.zeros(Bn, n, dtype=torch.int64)):
        ids2_dev = None if ids2 is None else ids2.to(DEV)

        def run2(t):
            out = torch.empty(Bn * n, D, dtype=LP, device=DEV)
            call("octmae_gather_rows_cast", t["src"].data_ptr(), None if ids2_dev is None else ids2_dev.data_ptr(), out.data_ptr(), Bn, n, src_rows,
                 D, _stream())
            return {"out": out}
        _tok_run("gather_rows_cast", value, {"src": NF.draw((Bn, src_rows, D), 2).to(DEV)}, run2, [("src", (0, 1, D - 1)), ("src", (0, 0, 3))],
                 lambda what, idx: {"out": NF.rule_gather_rows(Bn, n, D, ids2, idx)}, lambda t: {"out": NF.ref_gather_rows(t["src"], ids2_dev, n)})


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("norm_pix", [0, 1])
def test_mse_plants(norm_pix, value):
    """octmae_mse_fwd / octmae_mse_bwd at (B, C, T, S, tp) = (2, 1, 12, 32, 3): NF.rule_mse -- a plant in pred row 1 + l or in a voxel of
    token l -> loss_tok[b, l] and that element of dpred (with norm_pix a voxel reaches the whole row), the cls row of pred -> nothing.
    Kept rows and rows the mask removes alike: dpred = coef * mask * (pred - target), and 0 * NaN is NaN in the float64 gradient of
    forward_loss's (loss_tok * mask).sum() / mask.sum() too (tests/test_cpu_nonfinite.py::test_mse_rules_are_float64s_for_kept_and_masked_rows).
    In the surroundings run the mask and the coefficient are embedded as well."""
    from oracle import mae3d_ref as O
    B, C, T, S, tp, p = 2, 1, 12, 32, 3, 16
    cfg = O.MAEConfig(input_size=S, in_chans=C, num_frames=T, t_patch_size=tp, pred_t_dim=T, high_res_input_size=2 * S, norm_pix_loss=bool(norm_pix))
    u, L, PD = cfg.t_pred_patch_size, cfg.num_patches, cfg.patch_dim
    gh = gw = S // p
    mask = (torch.arange(B * L).view(B, L) % 3 != 1).float()
    l_kept, l_gone = 0, 1
    assert float(mask[0, l_kept]) == 1 and float(mask[0, l_gone]) == 0
    c = {"pred": NF.draw((B, L + 1, PD), 1).to(DEV), "imgs": (NF.draw((B, C, T, S, S), 2) / 6 + 0.5).to(DEV), "mask": mask.to(DEV),
         "coef": torch.full((1,), 2.0 / PD, dtype=torch.float32, device=DEV)}

    def run(t):
        loss_tok = torch.empty(B, L, device=DEV)
        call("octmae_mse_fwd", t["pred"].data_ptr(), t["imgs"].data_ptr(), None, loss_tok.data_ptr(), B, C, T, S, S, u, p, L, norm_pix, _stream())
        dpred = torch.empty(B * (L + 1), PD, dtype=LP, device=DEV)
        call("octmae_mse_bwd", t["pred"].data_ptr(), t["imgs"].data_ptr(), None, t["mask"].data_ptr(), t["coef"].data_ptr(), dpred.data_ptr(),
             B, C, T, S, S, u, p, L, norm_pix, _stream())
        return {"loss_tok": loss_tok, "dpred": dpred}

    def voxel(b, l, uu, py, px):
        return (b, 0, (l // (gh * gw)) * u + uu, ((l // gw) % gh) * p + py, (l % gw) * p + px)
    plants = [("pred", (0, 1 + l_kept, 0)), ("pred", (1, L, PD - 1)), ("pred", (0, 1 + l_gone, 7)), ("pred", (1, 0, 3)),
              ("imgs", voxel(0, l_kept, 0, 0, 0)), ("imgs", voxel(1, L - 1, u - 1, p - 1, p - 1)), ("imgs", voxel(0, l_gone, 1, 2, 3))]
    _tok_run(f"mse norm_pix={norm_pix}", value, c, run, plants, lambda what, idx: NF.rule_mse(B, C, T, S, S, u, p, norm_pix, what, idx),
             lambda t: NF.ref_mse(t["pred"], t["imgs"], t["mask"], t["coef"], cfg), embed_rows=64)


@pytest.mark.parametrize("value", list(VALUES))
def test_assembly_backward_plants(value):
    """octmae_scatter_add_rows (overwriting and accumulating) and octmae_dec_assemble_bwd at (B, L, nkeep, D) = (3, 40, 10, 64):
    src[b, 1 + r, k] -> out[l, k] for the one l with ids_restore[b, l] = r, the cls row src[b, 0] -> nothing; dx[b, 1 + l, k] ->
    ddpos[l, k], and the masked-token part[l, k] only if sample b masks l; the cls row of dx -> nothing."""
    B, L, nkeep, D = 3, 40, 10, 64
    ids = _restore(B, L, L)
    ids_dev = ids.to(DEV)
    c = {"src": NF.draw((B, 1 + nkeep, D), 1).to(DEV), "prior": NF.draw((L, D), 2).to(DEV)}
    for accumulate in (0, 1):
        def scatter(t):
            out = t["prior"].clone() if accumulate else torch.full((L, D), 7.0, device=DEV)
            call("octmae_scatter_add_rows", t["src"].data_ptr(), ids_dev.data_ptr(), out.data_ptr(), B, nkeep, L, D, 1 + nkeep, 1, accumulate, _stream())
            return {"out": out}
        _tok_run(f"scatter_add_rows accumulate={accumulate}", value, c, scatter, [("src", (0, 1, 0)), ("src", (2, nkeep, D - 1)), ("src", (1, 0, 5))],
                 lambda what, idx: {"out": NF.rule_scatter_add_rows(B, nkeep, L, D, ids, idx)},
                 lambda t: {"out": NF.ref_scatter_add_rows(t["src"], ids_dev, nkeep, t["prior"] if accumulate else None)})

    def dab(t):
        ddpos, part = torch.full((L, D), 7.0, device=DEV), torch.full((L, D), 7.0, device=DEV)
        call("octmae_dec_assemble_bwd", t["dx"].data_ptr(), ids_dev.data_ptr(), ddpos.data_ptr(), part.data_ptr(), B, nkeep, L, D, _stream())
        return {"ddpos": ddpos, "part": part}
    l_masked, l_kept = int((ids[0] >= nkeep).nonzero()[0]), int((ids[2] < nkeep).nonzero()[-1])
    _tok_run("dec_assemble_bwd", value, {"dx": NF.draw((B, 1 + L, D), 3).to(DEV)}, dab,
             [("dx", (0, 1 + l_masked, 0)), ("dx", (2, 1 + l_kept, D - 1)), ("dx", (1, 0, 9))],
             lambda what, idx: NF.rule_dec_assemble_bwd(B, nkeep, L, D, ids, idx), lambda t: NF.ref_dec_assemble_bwd(t["dx"], ids_dev, nkeep))
