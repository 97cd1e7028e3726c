"""GPU: ops.clip_pair_loss (csrc/cliploss.hip) -- the loss and its three gradients against the float64 reference of
tests/cliploss_ref.py, every row and every element within the bounds derived there, also where a forward workgroup walks several column
tiles and carries its (max, sum) along (cliploss_ref.TRIP_SHAPES, ordered scores); logits spanning +-3000; a NaN feature; bit
reproducibility; ClipLoss / ThreeModalityClipLoss fused against their ATen composition; the half-operand build; argument checks."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import children
from tests import cliploss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")
G_UP = 0.75          # the upstream gradient of every case

# (n, m, d, offset, column direction, zero fraction of the weights, scale): tile and k-step edges, the last rank of a local loss,
# a d past one 256-wide chunk of the backward and no multiple of it, and one case with every weight zero
CASES = ((1, 1, 1, 0, True, 0.0, 100.0), (63, 63, 31, 0, True, 0.2, 1 / 0.07), (64, 64, 32, 0, True, 0.2, 100.0),
         (65, 65, 33, 0, True, 0.2, 1 / 0.07), (129, 129, 512, 0, True, 0.2, 100.0), (8, 136, 512, 128, False, 0.0, 100.0),
         (33, 200, 65, 0, False, 0.2, 1 / 0.07), (33, 200, 65, 167, False, 0.2, 100.0), (33, 200, 65, 167, True, 0.2, 100.0),
         (65, 70, 300, 3, True, 0.2, 100.0), (65, 65, 33, 0, True, 1.0, 100.0))
# ... and R.TRIP_SHAPES, appended: there a workgroup of clip_lse_kernel walks several column tiles and carries its (max, sum) along
FIRST_TRIP_CASE = len(CASES)
CASES += tuple((n, m, d, off, True, 0.2, scale) for (n, m, d, off), scale in zip(R.TRIP_SHAPES, (100.0, 1 / 0.07, 100.0)))
TRIP_CASES = tuple(range(FIRST_TRIP_CASE, len(CASES)))
WORKER_CASES = (1, 3, 5, 8, 9, FIRST_TRIP_CASE)          # indices into CASES the half-build child repeats


def strided(x, pad=5):
    """x on the device as a row-strided slice of a wider buffer filled with NaN (a read past the row's d columns shows)"""
    x = torch.as_tensor(x)
    if x.dim() == 1:
        return x.to(DEV)
    wide = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=x.dtype, device=DEV)
    wide[:, 2:2 + x.shape[1]] = x.to(DEV)
    return wide[:, 2:2 + x.shape[1]]


@functools.lru_cache(maxsize=None)
def problem(k):
    n, m, d, off, col, zf, scale = CASES[k]
    a, b, wr, wc = R.make_problem(n, m, d, seed=20 + k, offset=off, zero_frac=zf)
    if zf >= 1.0:
        wr[:] = 0
        wc[:] = 0
    wc = wc if col else None
    return a, b, np.float32(scale), wr, wc, off, R.reference(a, b, np.float32(scale), wr, wc, off, g=G_UP)


def run(a, b, scale, wr, wc, off, g=G_UP):
    from octcubem_amd import ops
    A, B = strided(a).requires_grad_(True), strided(b).requires_grad_(True)
    S = torch.tensor(float(scale), dtype=torch.float32, device=DEV, requires_grad=True)
    L = ops.clip_pair_loss(A, B, S, strided(wr), None if wc is None else strided(wc), off)
    (L * g).backward()
    return {"loss": L.detach(), "da": A.grad, "db": B.grad, "dscale": S.grad}


@pytest.mark.parametrize("k", range(len(CASES)))
def test_loss_and_gradients_inside_the_bounds(k):
    a, b, scale, wr, wc, off, ref = problem(k)
    got = run(a, b, scale, wr, wc, off)
    torch.cuda.synchronize()
    for key in ("loss", "da", "db", "dscale"):
        w = R.worst(got[key], ref[key])
        print(CASES[k], key, "value", float(ref[key][0].abs().max()), "worst |err| / bound", w)
        assert w <= 1.0, (CASES[k], key, w)
    if CASES[k][5] >= 1.0:                       # every weight zero: exactly nothing
        assert float(got["loss"]) == 0.0 and not got["da"].any() and not got["db"].any() and float(got["dscale"]) == 0.0


@pytest.mark.parametrize("k", TRIP_CASES)
def test_trip_cases_lie_past_the_split(k):
    """The library's workspace answer equals the restated plan's, and under that plan a workgroup walks more than one tile."""
    from octcubem_amd._lib import load
    n, m = CASES[k][:2]
    p = R.plan(n, m)
    assert p == R.TRIP_PLANS[k - FIRST_TRIP_CASE]
    assert load().octmae_clip_loss_ws_floats(n, m) == 2 * (p["split_a"] * n + p["split_b"] * m) == R.ws_floats(n, m)
    trips_a, trips_b = -(-p["tiles_a"] // p["split_a"]), -(-p["tiles_b"] // p["split_b"])
    assert p["tiles_a"] > p["split_a"] and trips_a >= 2
    if k == TRIP_CASES[0]:
        assert p["split_a"] == R.MAX_SPLIT and trips_a == 3 and len(R.walked_tiles(p["tiles_a"], p["split_a"], 63)) == 2
    if k == TRIP_CASES[1]:
        assert R.plan(n, m, 2 * R.TARGET_WGS)["split_a"] < p["tiles_a"] and p["tiles_b"] > p["split_b"]
    if k == TRIP_CASES[2]:
        assert trips_a == 16 and p["split_b"] == 1 and trips_b == 3 and n - 2 * R.TILE == 2 and CASES[k][4]


@pytest.mark.parametrize("order", R.ORDERS)
def test_ordered_tile_maxima_across_the_trips_of_a_workgroup(order):
    """b[j] = c_j u + noise on the first trip shape (R.ordered_problem): the tile maxima of every row rise at every trip of a workgroup,
    never rise after its first, or rise and then fall"""
    a, b, scale, wr, wc, off = R.ordered_problem(order)
    R.assert_trip_order(order, R.trip_maxima(a, b, scale))      # a condition on the inputs, from float64 logits, before the kernel runs
    ref = R.reference(a, b, scale, wr, wc, off, g=G_UP)
    got = run(a, b, scale, wr, wc, off)
    torch.cuda.synchronize()
    for key in ("loss", "da", "db", "dscale"):
        w = R.worst(got[key], ref[key])
        print(order, key, "worst |err| / bound", w)
        assert w <= 1.0, (order, key, w)


def test_logits_spanning_thousands_with_equal_probabilities():
    n, d = 70, 40
    a, b, wr, wc = R.make_problem(n, n, d, seed=5, zero_frac=0.1)
    b = 30.0 * a                                    # z(i, i) = +3000
    b[1::2] = -b[1::2]                              # ... and -3000 on every other row
    b[10] = b[8]; b[11] = b[8]; b[40] = b[8]        # duplicated rows: equal probabilities in every row of the score matrix
    b = np.ascontiguousarray(b, dtype=np.float32)
    ref = R.reference(a, b, np.float32(100.0), wr, wc, 0, g=G_UP)
    z = 100.0 * a.astype(np.float64) @ b.astype(np.float64).T
    assert z.max() > 2990 and z.min() < -2990
    got = run(a, b, 100.0, wr, wc, 0)
    for key in ("loss", "da", "db", "dscale"):
        assert bool(torch.isfinite(got[key]).all()), key
        w = R.worst(got[key], ref[key])
        print(key, "worst |err| / bound", w)
        assert w <= 1.0, (key, w)


def test_a_nan_feature_gives_nan_and_the_next_call_is_clean():
    a, b, scale, wr, wc, off, ref = problem(7)                 # rectangular, row direction only
    bad = a.copy()
    bad[3, 5] = np.nan
    wr1 = np.where(wr == 0, np.float32(1e-3), wr)              # row 3 carries weight
    got = run(bad, b, scale, wr1, None, off)
    torch.cuda.synchronize()
    assert bool(torch.isnan(got["loss"])) and bool(torch.isnan(got["dscale"]))
    assert bool(torch.isnan(got["da"][3]).all()) and bool(torch.isnan(got["db"]).all())
    rest = torch.cat([got["da"][:3], got["da"][4:]])
    assert bool(torch.isfinite(rest).all())                    # the other rows of a never meet the NaN
    inf = a.copy()
    inf[0, 0] = np.inf
    assert bool(torch.isnan(run(inf, b, scale, wr1, None, off)["loss"]))
    clean = run(a, b, scale, wr, wc, off)
    for key in ("loss", "da", "db", "dscale"):
        assert R.worst(clean[key], ref[key]) <= 1.0, key


@pytest.mark.parametrize("k", [4, 8, FIRST_TRIP_CASE + 1])
def test_two_runs_are_bit_equal(k):
    a, b, scale, wr, wc, off, _ = problem(k)
    x, y = run(a, b, scale, wr, wc, off), run(a, b, scale, wr, wc, off)
    for key in x:
        assert torch.equal(x[key], y[key]), key


# ------------------------------------------------------------------------------------------------ the losses of coem.py
def _leaf(x):
    return torch.from_numpy(x).to(DEV).requires_grad_(True)


def test_clip_loss_fused_against_aten():
    from octcubem_amd import coem
    n, d = 65, 96
    a, b, _, _ = R.make_problem(n, n, d, seed=31)
    w = np.full(n, 0.5 / n, dtype=np.float32)
    ref = R.reference(a, b, np.float32(1 / 0.07), w, w, 0)
    out = {}
    for fused in (False, True):
        A, B = _leaf(a), _leaf(b)
        S = torch.tensor(1 / 0.07, dtype=torch.float32, device=DEV, requires_grad=True)
        L = coem.ClipLoss(fused=fused)(A, B, S)
        L.backward()
        out[fused] = {"loss": L.detach(), "da": A.grad, "db": B.grad, "dscale": S.grad}
    for key in ("loss", "da", "db", "dscale"):
        for fused in (False, True):                              # each path inside its own bound against float64 ...
            assert R.worst(out[fused][key], ref[key]) <= 1.0, (key, fused)
        diff = (out[True][key].double().cpu() - out[False][key].double().cpu()).abs().reshape(ref[key][1].shape)
        assert bool((diff <= 2.0 * ref[key][1]).all()), key      # ... hence within the sum of both against each other


@pytest.mark.parametrize("weights", ["mixed", "one_modality_absent", "all_absent"])
def test_three_modality_loss_fused_against_aten(weights):
    from octcubem_amd import coem
    n, d = 37, 48
    rng = np.random.default_rng(9)
    x, e1, _, _ = R.make_problem(n, n, d, seed=41)
    _, e2, _, _ = R.make_problem(n, n, d, seed=42)
    e2 = np.ascontiguousarray(e2 + 0.3 * x, dtype=np.float32)
    e2 /= np.linalg.norm(e2, axis=1, keepdims=True)
    w1 = (rng.random(n) < 0.7).astype(np.float32)
    w2 = (rng.random(n) < 0.5).astype(np.float32)
    if weights == "one_modality_absent":
        w2[:] = 0
    if weights == "all_absent":
        w1[:] = 0
        w2[:] = 0
    scales = (np.float32(1 / 0.07), np.float32(20.0), np.float32(5.5))
    share = lambda w: (w / (6 * w.sum()) if w.sum() > 0 else np.zeros_like(w)).astype(np.float32)
    refs = [R.reference(p, q, s, share(w), share(w), 0) for p, q, s, w in ((x, e1, scales[0], w1), (x, e2, scales[1], w2), (e1, e2, scales[2], w1 * w2))]
    want = {"loss": (sum(r["loss"][0] for r in refs), sum(r["loss"][1] for r in refs)),
            "x": (refs[0]["da"][0] + refs[1]["da"][0], refs[0]["da"][1] + refs[1]["da"][1]),
            "e1": (refs[0]["db"][0] + refs[2]["da"][0], refs[0]["db"][1] + refs[2]["da"][1]),
            "e2": (refs[1]["db"][0] + refs[2]["db"][0], refs[1]["db"][1] + refs[2]["db"][1]),
            "s0": refs[0]["dscale"], "s1": refs[1]["dscale"], "s2": refs[2]["dscale"]}
    out = {}
    for fused in (False, True):
        X, E1, E2 = _leaf(x), _leaf(e1), _leaf(e2)
        S = [torch.tensor(float(s), dtype=torch.float32, device=DEV, requires_grad=True) for s in scales]
        L = coem.ThreeModalityClipLoss(fused=fused)(X, E1, E2, *S, torch.from_numpy(w1).to(DEV), torch.from_numpy(w2).to(DEV))
        if L.requires_grad:                                      # the ATen path returns a constant 0 when every modality is absent
            L.backward()
        zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
        out[fused] = {"loss": L.detach(), "x": zero(X), "e1": zero(E1), "e2": zero(E2), "s0": zero(S[0]), "s1": zero(S[1]), "s2": zero(S[2])}
    assert out[True]["loss"].requires_grad is False and L.requires_grad     # the fused path always has a graph
    for key, rb in want.items():
        for fused in (False, True):
            assert R.worst(out[fused][key], rb) <= 1.0, (key, fused)
        diff = (out[True][key].double().cpu() - out[False][key].double().cpu()).abs().reshape(rb[1].shape)
        assert bool((diff <= 2.0 * rb[1]).all()), key
    if weights == "all_absent":
        assert float(out[True]["loss"]) == 0.0 and not out[True]["x"].any()


# ------------------------------------------------------------------------------------------------ the half build
def worker_results():
    res = {}
    for k in WORKER_CASES:
        a, b, scale, wr, wc, off, _ = problem(k)
        for key, v in run(a, b, scale, wr, wc, off).items():
            res[f"{k}/{key}"] = v.detach().cpu().numpy()
    return res


def test_half_build_gives_the_same_bits():
    """The entry points have no 16-bit operand: liboctmae_f16.so must return bit-equal results (a child process, one library each)."""
    assert os.path.exists(LIB_F16), "make -C octcubem_amd/csrc both"
    children.spawn_f16_worker("cliploss_f16", "tests.test_gpu_cliploss:worker_results", ext="npz")
    theirs = children.f16_worker_result("cliploss_f16")
    meta = json.loads(str(theirs["meta"]))
    assert meta["lib"] == "liboctmae_f16.so" and meta["lp_is_f16"] is True
    mine = worker_results()
    assert set(mine) | {"meta"} == set(theirs.files)
    for key, v in mine.items():
        assert v.tobytes() == theirs[key].tobytes(), key


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_raise_before_any_launch(monkeypatch):
    from octcubem_amd import ops
    launches = []
    monkeypatch.setattr(ops, "_launch", lambda *a, **k: launches.append(a[0]))
    a = torch.randn(6, 8, device=DEV)
    b = torch.randn(9, 8, device=DEV)
    s = torch.tensor(10.0, device=DEV)
    w = torch.full((6,), 1 / 6, device=DEV)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.clip_pair_loss(a.cpu(), b, s, w)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.clip_pair_loss(a, b, 10.0, w)
    with pytest.raises(TypeError, match="float32"):
        ops.clip_pair_loss(a.double(), b, s, w)
    with pytest.raises(TypeError, match="wr must be float32"):
        ops.clip_pair_loss(a, b, s, w.half())
    with pytest.raises(ValueError, match="strides"):
        ops.clip_pair_loss(torch.randn(8, 6, device=DEV).t(), b, s, w)
    with pytest.raises(ValueError, match=r"\[n, d\]"):
        ops.clip_pair_loss(a, torch.randn(9, 7, device=DEV), s, w)
    with pytest.raises(ValueError, match="wc must be"):
        ops.clip_pair_loss(a, b, s, w, torch.ones(5, device=DEV))
    with pytest.raises(ValueError, match="logit_scale must be one element"):
        ops.clip_pair_loss(a, b, torch.ones(2, device=DEV), w)
    for off in (-1, 4):
        with pytest.raises(ValueError, match="offset"):
            ops.clip_pair_loss(a, b, s, w, None, off)
    with pytest.raises(TypeError, match="offset"):
        ops.clip_pair_loss(a, b, s, w, None, 1.0)
    assert launches == []
    from octcubem_amd._lib import load
    lib = load()
    assert lib.octmae_clip_loss_ws_floats(0, 5) == -2
    # the C entry points refuse the same from host integers alone (-2, nothing launched)
    args = (a.data_ptr(), 8, b.data_ptr(), 8, s.data_ptr(), w.data_ptr(), None)
    outs = [torch.zeros(9, device=DEV) for _ in range(4)]
    ws = torch.zeros(4096, device=DEV)
    tail = lambda n, m, d: (outs[0].data_ptr(), None, outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(), 4096, n, m, d, 0)
    assert lib.octmae_clip_loss_fwd(*args, 4, *tail(6, 9, 8)) == -2            # n + offset > m
    assert lib.octmae_clip_loss_fwd(*args, -1, *tail(6, 9, 8)) == -2
    assert lib.octmae_clip_loss_fwd(*args, 0, *tail(0, 9, 8)) == -2
    assert lib.octmae_clip_loss_fwd(a.data_ptr(), 7, *args[2:], 0, *tail(6, 9, 8)) == -2      # stride below d
    assert lib.octmae_clip_loss_fwd(None, 8, *args[2:], 0, *tail(6, 9, 8)) == -2
    torch.cuda.synchronize()
    assert not ws.any() and not outs[2].any()
