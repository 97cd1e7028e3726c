"""GPU: the join kernels (octcubem_amd/csrc/join.hip through ops.join_fwd / ops.join_bwd / ops.JoinFn) at their dispatch edges, every
output element against the float64 reference and the derived bounds of tests/join_ref.py (tests/test_cpu_join.py shows what those bounds
pass and what they catch); determinism and accumulation of the parameter gradients; the refusals; the weight-gradient switch; autocast;
and the same cases on the half-operand build in a child process (tests/f16_worker.py)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import _lib, coem, ops
from tests import children
from tests import join_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")
DEV = "cuda"
ALL_KEYS = R.FWD_KEYS + R.BWD_KEYS

# (B, D, M, present_mask, dn_extra, dgamma / dbeta).  make_problem puts an all-zero feature into row 0, all features zero into row 1,
# 1e-20 x into row 2 and 1e18 x into row 3 of every case that has the rows.
CASES = {
    # the grid edge, one wave short of a workgroup, a whole number of workgroups, one wave over
    "B1": (1, 512, 3, 7, True, True), "B3": (3, 512, 3, 7, False, True), "B64": (64, 8, 2, 3, True, True), "B65": (65, 4, 2, 3, True, False),
    # one float4 per row; fewer float4s than lanes; a ragged last lane group; the shipped size; the 3072-float row; the largest legal row
    "D4": (5, 4, 3, 7, False, True), "D8": (5, 8, 3, 7, True, True), "D68": (7, 68, 3, 5, True, True), "D512": (65, 512, 3, 7, True, True),
    "D1024": (6, 1024, 3, 7, False, True), "D1364": (6, 1364, 3, 7, True, True),
    # chunk counts 3 (in the 4-chunk kernel) and 8 (M = 2 only)
    "D768": (5, 768, 2, 3, True, True), "D2048": (5, 2048, 2, 3, True, False),
    # more rows than waves in the grid (256 workgroups of 4): the row loop
    "rows": (1030, 8, 2, 1, True, True),
}
CASES.update({f"M2mask{m}": (9, 68, 2, m, bool(m & 1), True) for m in (1, 2, 3)})
CASES.update({f"M3mask{m}": (9, 512, 3, m, bool(m & 1), bool(m & 2)) for m in range(1, 8)})
WORKER_CASES = ("B1", "B65", "D68", "D512", "D1364", "D2048", "M3mask5", "M2mask2")


def problem(name):
    B, D, M, mask, use_extra, wg = CASES[name]
    feats, gamma, beta, dy, extra = R.make_problem(B, D, M, seed=31 + B + D)
    return (B, D, M, mask, wg), feats, gamma, beta, dy, (extra if use_extra else None)


def run(name):
    """the kernels on one case -> numpy arrays under the reference's keys (df of absent slots as NaN, dgamma / dbeta None when not asked for)"""
    (B, D, M, mask, wg), feats, gamma, beta, dy, extra = problem(name)
    t = lambda a: torch.from_numpy(a).to(DEV)
    fs = [t(f) if (mask >> k) & 1 else None for k, f in enumerate(feats)]
    g, b = t(gamma), t(beta)
    y, n, inv, mean, rstd = ops.join_fwd(fs, mask, g, b, R.LN_EPS)
    dg = torch.zeros(M * D, device=DEV) if wg else None
    db = torch.zeros(M * D, device=DEV) if wg else None
    df = ops.join_bwd(t(dy), None if extra is None else t(extra), fs, inv, mean, rstd, g, mask, dg, db)
    for k in range(M):
        if not (mask >> k) & 1:
            df[k] = float("nan")
    out = {"n": n, "inv_norm": inv, "mean": mean, "rstd": rstd, "y": y.float(), "df": df}
    if wg:
        out.update(dgamma=dg, dbeta=db)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(name, got, lp_is_f16):
    (B, D, M, mask, wg), feats, gamma, beta, dy, extra = problem(name)
    ref, bound = R.reference(feats, mask, gamma, beta, dy, extra, lp_is_f16=lp_is_f16)
    for key in ALL_KEYS:
        if key not in got:
            assert key in ("dgamma", "dbeta") and not wg
            continue
        w, at = R.worst(got[key], ref[key], bound[key], with_index=True)
        print(name, "f16" if lp_is_f16 else "bf16", key, "worst |err| / bound = %.3g at %d" % (w, at))
        assert w <= 1.0, (name, key, w, at)
    for k in range(M):      # absent slots are exact zeros
        if not (mask >> k) & 1:
            assert not got["n"][k].any() and not got["inv_norm"][:, k].any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_join_matches_the_reference_per_element(name):
    got = run(name)
    check(name, got, ops.LP_IS_F16)
    (B, D, M, mask, wg), feats, *_ = problem(name)
    for k in range(M):      # n_out against F.normalize run in float64, the bound the arithmetic gives a normalised element
        if (mask >> k) & 1:
            want = torch.nn.functional.normalize(torch.from_numpy(feats[k]).double(), dim=-1).numpy()
            assert (np.abs(got["n"][k] - want) <= np.abs(want) * (D / 2 + 4) * R.U + 2 * R.FLOOR).all(), (name, k)
    if B > 3:
        assert abs(got["rstd"][1] - float(np.float32(R.LN_EPS)) ** -0.5) <= 4 * R.U * 400         # every feature zero: variance 0
        if mask == (1 << M) - 1:
            assert np.isfinite(got["n"][:, 2:4]).all() and (np.abs(np.linalg.norm(got["n"][:, 3], axis=-1) - 1) < 1e-5).all()


def test_absent_slots_are_neither_read_nor_written():
    """through the C ABI: NULL feature pointers for absent modalities, and a df buffer whose absent slices keep their sentinel"""
    B, D, M, mask = 9, 68, 3, 5
    feats, gamma, beta, dy, extra = R.make_problem(B, D, M, seed=33)
    t = lambda a: torch.from_numpy(a).to(DEV)
    f0, f2, g, b = t(feats[0]), t(feats[2]), t(gamma), t(beta)
    n = torch.full((M, B, D), 7.0, device=DEV); inv = torch.full((B, M), 7.0, device=DEV)
    y = torch.empty((B, M * D), dtype=ops.BF16, device=DEV); mean = torch.empty(B, device=DEV); rstd = torch.empty(B, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("octmae_join_fwd", f0.data_ptr(), None, f2.data_ptr(), mask, g.data_ptr(), b.data_ptr(), n.data_ptr(), inv.data_ptr(),
              y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, D, M, R.LN_EPS, st)
    assert not n[1].any() and not inv[:, 1].any()
    df = torch.full((M, B, D), 7.0, device=DEV)
    dyt, ext = t(dy), t(extra)              # held in names: a temporary's memory is handed out again before the launch
    _lib.call("octmae_join_bwd", dyt.data_ptr(), ext.data_ptr(), f0.data_ptr(), None, f2.data_ptr(), inv.data_ptr(), mean.data_ptr(),
              rstd.data_ptr(), g.data_ptr(), mask, df.data_ptr(), None, None, None, B, D, M, st)
    assert bool((df[1] == 7.0).all()) and not bool((df[0] == 7.0).all())
    ref, bound = R.reference(feats, mask, gamma, beta, dy, extra, lp_is_f16=ops.LP_IS_F16)
    df[1] = float("nan")
    assert R.worst(df.cpu().numpy(), ref["df"], bound["df"]) <= 1.0


def test_parameter_gradients_are_bit_reproducible_and_accumulate():
    (B, D, M, mask, wg), feats, gamma, beta, dy, extra = problem("D512")
    t = lambda a: torch.from_numpy(a).to(DEV)
    fs, g, b, dyt = [t(f) for f in feats], t(gamma), t(beta), t(dy)
    y, n, inv, mean, rstd = ops.join_fwd(fs, mask, g, b, R.LN_EPS)
    runs = []
    for _ in range(2):
        dg, db = torch.zeros(M * D, device=DEV), torch.zeros(M * D, device=DEV)
        df = ops.join_bwd(dyt, None, fs, inv, mean, rstd, g, mask, dg, db)
        runs.append((dg.clone(), db.clone(), df))
    assert all(torch.equal(a, c) for a, c in zip(runs[0], runs[1]))
    ops.join_bwd(dyt, None, fs, inv, mean, rstd, g, mask, dg, db)          # a second backward into the same buffers: exactly twice
    assert torch.equal(dg, 2 * runs[0][0]) and torch.equal(db, 2 * runs[0][1])
    only_beta = torch.zeros(M * D, device=DEV)                                 # either buffer alone
    df2 = ops.join_bwd(dyt, None, fs, inv, mean, rstd, g, mask, None, only_beta)
    assert torch.equal(only_beta, runs[0][1]) and torch.equal(df2, runs[0][2])


def test_refusals_raise_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel entry point was reached")
    monkeypatch.setattr(ops, "call", no_launch)
    z = lambda B, D: torch.zeros(B, D, device=DEV)
    g = torch.ones(8192, device=DEV)
    for feats, mask in (([z(2, 6)] * 2, 3), ([z(2, 8)] * 4, 15), ([z(2, 2050)] * 2, 3), ([z(2, 2052)] * 2, 3), ([z(2, 8)] * 3, 0),
                        ([z(2, 8)] * 2, 4)):
        M, D = len(feats), feats[0].shape[1]
        with pytest.raises(ValueError):
            ops.join_fwd(feats, mask, g[:M * D], g[:M * D], 1e-5)
        with pytest.raises(ValueError):
            ops.JoinFn.apply(g[:M * D], g[:M * D], 1e-5, mask, *feats)
    odd = torch.zeros(2 * 8 + 1, device=DEV)[1:].view(2, 8)          # contiguous, but 4 bytes off a 16-byte boundary
    with pytest.raises(ValueError):
        ops.join_fwd([z(2, 8), odd], 3, g[:16], g[:16], 1e-5)
    with pytest.raises(ValueError):
        ops.join_fwd([z(2, 8), z(2, 8)], 3, g[1:17], g[:16], 1e-5)
    monkeypatch.undo()
    # the library itself: a non-zero code and no launch
    lib = _lib.load()
    p = g.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    for B, D, M, mask in ((2, 6, 2, 3), (2, 8, 4, 15), (2, 2052, 2, 3), (2, 1368, 3, 7), (2, 8, 3, 0), (2, 8, 2, 4), (0, 8, 2, 3)):
        assert lib.octmae_join_fwd(p, p, p, mask, p, p, p, p, p, p, p, B, D, M, 1e-5, st) != 0
        assert lib.octmae_join_bwd(p, None, p, p, p, p, p, p, p, mask, p, None, None, None, B, D, M, st) != 0
        assert lib.octmae_join_ws_floats(B, D, M) < 0 or mask in (0, 4)
    assert lib.octmae_join_fwd(None, p, p, 1, p, p, p, p, p, p, p, 2, 8, 2, 1e-5, st) != 0          # a present modality without features
    assert lib.octmae_join_fwd(p + 4, p, p, 3, p, p, p, p, p, p, p, 2, 8, 2, 1e-5, st) != 0          # a misaligned feature pointer
    assert lib.octmae_join_fwd(p, p, p, 3, p, p, p, p, p + 4, p, p, 2, 8, 2, 1e-5, st) != 0          # y_lp off an 8-byte boundary
    assert lib.octmae_join_bwd(p + 8, None, p, p, p, p, p, p, p, 3, p, None, None, None, 2, 8, 2, st) != 0
    assert lib.octmae_join_ws_floats(65, 512, 3) == 17 * 2 * 1536
    torch.cuda.synchronize()


def _joinfn(name, with_n):
    (B, D, M, mask, wg), feats, gamma, beta, dy, _ = problem(name)
    extra = R.make_problem(B, D, M, seed=31 + B + D)[4]          # the case's own dn_extra, whether or not the raw-kernel case uses it
    t = lambda a: torch.from_numpy(a).to(DEV)
    fs = [t(f).requires_grad_(True) if (mask >> k) & 1 else None for k, f in enumerate(feats)]
    g, b = torch.nn.Parameter(t(gamma)), torch.nn.Parameter(t(beta))
    y, *n = ops.JoinFn.apply(g, b, R.LN_EPS, mask, *fs)
    dy_lp = R.to_lp(dy, ops.LP_IS_F16)                       # y is a 16-bit tensor: its gradient arrives in that type
    loss = (y.float() * t(dy_lp)).sum()
    if with_n:
        loss = loss + sum((n[k] * t(extra[k])).sum() for k in range(M) if (mask >> k) & 1)
    return (B, D, M, mask), feats, gamma, beta, dy_lp, extra, fs, g, b, y, n, loss


@pytest.mark.parametrize("name,with_n", [("D512", True), ("M3mask5", False), ("M2mask2", True)])
def test_joinfn_routes_the_feature_gradients(name, with_n):
    (B, D, M, mask), feats, gamma, beta, dy_lp, extra, fs, g, b, y, n, loss = _joinfn(name, with_n)
    loss.backward()
    ref, bound = R.reference(feats, mask, gamma, beta, dy_lp, extra if with_n else None, lp_is_f16=ops.LP_IS_F16)
    df = np.stack([fs[k].grad.cpu().numpy() if fs[k] is not None else np.full((B, D), np.nan, np.float32) for k in range(M)])
    got = {"y": y.detach().float().cpu().numpy(), "n": torch.stack(n).detach().cpu().numpy(), "df": df, "dgamma": g.grad.cpu().numpy(),
           "dbeta": b.grad.cpu().numpy()}
    for key, v in got.items():
        w = R.worst(v, ref[key], bound[key])
        print(name, key, "worst |err| / bound =", w)
        assert w <= 1.0, (key, w)
    assert y.dtype == ops.BF16 and tuple(y.shape) == (B, M * D)


def test_joinfn_without_weight_grads_is_bit_equal_and_touches_no_buffer():
    *_, fs, g, b, y, n, loss = _joinfn("D512", True)
    loss.backward()
    want = [f.grad.clone() for f in fs]
    *_, fs2, g2, b2, y2, n2, loss2 = _joinfn("D512", True)
    g2.grad = torch.full_like(g2, 3.0)
    with ops.weight_grads(False):
        loss2.backward()
    assert all(torch.equal(f.grad, w) for f, w in zip(fs2, want))
    assert bool((g2.grad == 3.0).all()) and b2.grad is None and bool(g.grad.abs().sum() > 0)


@pytest.mark.parametrize("num_classes", [5, 8])
def test_head_is_bit_identical_inside_and_outside_autocast(num_classes):
    D, M, B = 64, 3, 5
    feats, *_ = R.make_problem(B, D, M, seed=35, special=False)
    outs = []
    for amp in (False, True):
        torch.manual_seed(0)
        head = coem.ClassificationHead(M * D, D, num_classes).to(DEV)
        fs = [torch.from_numpy(f).to(DEV).requires_grad_(True) for f in feats]
        with torch.cuda.amp.autocast(enabled=amp):
            logits, n = head.forward_joined(fs, 7)
            loss = (logits.float() ** 2).sum() + n[1].sum()
        loss.backward()
        outs.append([logits.detach()] + [f.grad for f in fs] + [p.grad.clone() for p in head.parameters()])
    assert outs[0][0].dtype == torch.float32
    for a, c in zip(*outs):
        assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ the half build
def worker_results():
    res = {}
    for name in WORKER_CASES:
        for key, v in run(name).items():
            res[f"{name}/{key}"] = v
    return res


def test_join_on_the_half_operand_build():
    """the same cases on liboctmae_f16.so in a fresh child process (a process binds one library): y against the bounds for one rounding to
    half; everything that never meets the 16-bit type is the same f32 code in both builds and must come back bit-equal"""
    assert os.path.exists(LIB_F16), f"{LIB_F16} is missing: __graft_entry__.build() makes it"
    children.spawn_f16_worker("join_f16", "tests.test_gpu_join:worker_results", ext="npz")
    theirs = children.f16_worker_result("join_f16")
    meta = json.loads(str(theirs["meta"]))
    assert meta["lib"] == "liboctmae_f16.so" and meta["lp_is_f16"] is True
    mine = worker_results()
    assert set(mine) | {"meta"} == set(theirs.files)
    for name in WORKER_CASES:
        check(name, {k.split("/", 1)[1]: theirs[k] for k in theirs.files if k.startswith(name + "/")}, True)
    if not ops.LP_IS_F16:
        for key, v in mine.items():
            if not key.endswith("/y"):
                assert np.array_equal(v, theirs[key], equal_nan=True), key
