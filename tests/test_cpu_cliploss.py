"""CPU tests of the fused contrastive loss and the COEM epoch loop: the float64 reference of tests/cliploss_ref.py against
F.cross_entropy, an f32 restatement of the kernel's arithmetic inside the derived bounds and four injected faults outside them, the ABI
of the new entry points, the learning-rate schedule, and the bookkeeping of the cached-feature accumulation on stub towers."""
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import cliploss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("octmae_clip_loss_ws_floats", "octmae_clip_loss_fwd", "octmae_clip_loss_bwd")
# (n, m, d, offset, scale): symmetric, rectangular with offset (the last rank of a local loss), rectangular without
CASES = ((129, 129, 512, 0, 1 / 0.07), (65, 200, 33, 135, 100.0), (65, 200, 33, 0, 100.0), (129, 129, 512, 0, 100.0))
KEYS = ("loss", "da", "db", "dscale")


def t64(x):
    return torch.from_numpy(np.asarray(x)).double()


@pytest.mark.parametrize("form", ["symmetric", "rect_offset", "weighted_zeros"])
def test_reference_equals_cross_entropy(form):
    n, m, d, off = {"symmetric": (40, 40, 16, 0), "rect_offset": (9, 31, 7, 22), "weighted_zeros": (23, 23, 5, 0)}[form]
    a, b, wr, wc = R.make_problem(n, m, d, seed=3, offset=off, zero_frac=0.4 if form == "weighted_zeros" else 0.0,
                                  equal_weights=form == "symmetric")
    if form == "weighted_zeros":
        assert (wr == 0).any() and (wc == 0).any()
    wc = None if form == "rect_offset" else wc
    scale = 14.3
    A, B = t64(a).requires_grad_(True), t64(b).requires_grad_(True)
    S = torch.tensor(scale, dtype=torch.float64, requires_grad=True)
    L = R.torch_losses(A, B, S, t64(wr), None if wc is None else t64(wc), off)
    (2.5 * L).backward()
    ref = R.reference(a, b, scale, wr, wc, off, g=2.5)
    if form == "symmetric":      # the reference's ClipLoss itself
        z = scale * t64(a) @ t64(b).t()
        lab = torch.arange(n)
        clip = (torch.nn.functional.cross_entropy(z, lab) + torch.nn.functional.cross_entropy(z.t(), lab)) / 2
        exact = np.full(n, 0.5 / n)                                   # float64 weights: 1 / (2 n) is no f32 number for n = 40
        assert abs(float(clip) - float(R.reference(a, b, scale, exact, exact, 0)["loss"][0])) <= 1e-12 * abs(float(clip))
    for key, got in (("loss", L.detach()), ("da", A.grad), ("db", B.grad), ("dscale", S.grad)):
        want = ref[key][0]
        assert float((got - want).abs().max()) <= 1e-11 * (float(want.abs().max()) + 1e-3), key


@pytest.mark.parametrize("case", CASES)
def test_f32_restatement_is_inside_the_bounds(case):
    n, m, d, off, scale = case
    a, b, wr, wc = R.make_problem(n, m, d, seed=11, offset=off, zero_frac=0.2)
    wc = None if (m != n and off == 0) else wc
    ref = R.reference(a, b, np.float32(scale), wr, wc, off, g=0.75)
    assert 0.1 <= float(ref["loss"][0]) <= 100.0                    # a loss of ordinary size, not a degenerate problem
    got = R.emulate(a, b, scale, wr, wc, off, g=0.75)
    for key in KEYS:
        w = R.worst(torch.from_numpy(np.asarray(got[key])), ref[key])
        print(case, key, "worst |err| / bound =", w)
        assert w <= 1.0, (key, w)


@pytest.mark.parametrize("fault", ["tile", "kstep", "partner", "weight"])
def test_injected_faults_leave_the_bounds(fault):
    n, m, d, off, scale = 129, 129, 512, 0, 100.0
    a, b, wr, wc = R.make_problem(n, m, d, seed=11, offset=off)
    ref = R.reference(a, b, np.float32(scale), wr, wc, off)
    got = R.emulate(a, b, scale, wr, wc, off, fault=fault)
    over = {key: R.worst(torch.from_numpy(np.asarray(got[key])), ref[key]) for key in KEYS}
    print(fault, over)
    assert over["loss"] > 1.0 and max(over["da"], over["db"]) > 1.0, over


def hip_constant(text, name):
    return int(re.search(rf"^constexpr int {name} = (\d+);", text, re.M).group(1))


def test_restated_plan_follows_the_kernel_constants_and_the_trip_shapes_lie_past_the_split():
    """Whoever changes a constant of the tile (csrc/simtile.hpp) or of csrc/cliploss.hip is told here to move R.TRIP_SHAPES
    (tests/test_gpu_cliploss.py runs them)."""
    src = open(os.path.join(ROOT, "octcubem_amd", "csrc", "cliploss.hip")).read()
    tile = open(os.path.join(ROOT, "octcubem_amd", "csrc", "simtile.hpp")).read()
    assert '#include "simtile.hpp"' in src and not re.search(r"^constexpr int CL_(ROWS|COLS|K|TARGET_WGS) ", src, re.M)
    assert hip_constant(tile, "SIM_TARGET_WGS") == R.TARGET_WGS and hip_constant(src, "CL_MAX_SPLIT") == R.MAX_SPLIT
    assert hip_constant(tile, "SIM_ROWS") == hip_constant(tile, "SIM_COLS") == R.TILE and hip_constant(tile, "SIM_K") == R.KSTEP
    # sim_split as written: ceil(target / row_blocks), then the two caps; both sides of the loss pass CL_MAX_SPLIT
    assert re.search(r"long long split = \(SIM_TARGET_WGS \+ row_blocks - 1\) / row_blocks;\s*if \(split > col_tiles\) split = col_tiles;\s*"
                     r"if \(split > cap\) split = cap;", tile)
    for side in "ab":
        assert re.search(rf"p->split_{side} = \(int\)sim_split\(p->row_blocks_{side}, p->tiles_{side}, CL_MAX_SPLIT\);", src), side
    assert re.search(r"return 2 \* \(\(long long\)p\.split_a \* n \+ \(long long\)p\.split_b \* m\);", src)
    assert R.split(1, 1) == 1 and R.split(1, 200) == 64 and R.split(40, 200) == 26 and R.split(4000, 9) == 1 and R.split(512, 9) == 2
    for (n, m, d, off), want in zip(R.TRIP_SHAPES, R.TRIP_PLANS):
        p = R.plan(n, m)
        assert p == want, (n, m, p)
        assert p["tiles_a"] > p["split_a"] and n + off <= m
        assert R.ws_floats(n, m) == 2 * (want["split_a"] * n + want["split_b"] * m)
    first, second, third = (R.plan(n, m) for n, m, _, _ in R.TRIP_SHAPES)
    assert first["split_a"] == R.MAX_SPLIT < first["tiles_a"] <= 3 * R.MAX_SPLIT                      # the cap itself; two or three trips
    assert second["split_a"] < R.plan(3001, 3001, 2 * R.TARGET_WGS)["split_a"] < second["tiles_a"]       # trips even at twice the target
    assert third["split_b"] == 1 and third["tiles_b"] == 3 and 130 % R.TILE == 2 and third["tiles_a"] == 16 * third["split_a"]
    # no earlier case of the GPU module leaves a workgroup more than one tile: the gap these shapes close
    for n, m in ((1, 1), (63, 63), (64, 64), (65, 65), (129, 129), (8, 136), (33, 200), (65, 70)):
        q = R.plan(n, m)
        assert q["split_a"] == q["tiles_a"] and q["split_b"] == q["tiles_b"]


@pytest.mark.parametrize("order", R.ORDERS)
def test_split_walk_restatement_on_ordered_scores(order):
    """The ordered problems of the GPU test: their condition holds, the f32 walk as launched (split 64, two or three trips, partials
    merged in order) keeps every row's log-sum-exp inside the derived bound, and a carried sum that is not rescaled, rescaled the wrong
    way or dropped does not -- wherever the order of the maxima lets that fault act at all."""
    a, b, scale, wr, wc, off = R.ordered_problem(order)
    R.assert_trip_order(order, R.trip_maxima(a, b, scale))
    ref = R.reference(a, b, scale, wr, wc, off)
    z = (scale * R._fma_scores(a, b)).astype(np.float32)
    p = R.plan(*z.shape)
    ok = R.worst(torch.from_numpy(R.split_lse(z, p["split_a"])), ref["lse_row"])
    over = {f: R.worst(torch.from_numpy(R.split_lse(z, p["split_a"], fault=f)), ref["lse_row"]) for f in ("no_rescale", "inverse", "restart")}
    print(order, "worst |err| / bound", ok, over)
    assert ok <= 1.0
    assert over["restart"] > 1.0 and over["inverse"] > 1.0      # a dropped sum always shows; exp(nm - -inf) at the first tile is 0 * inf
    assert (over["no_rescale"] > 1.0) == (order != "falling")   # a maximum that never rises is never rescaled: only the others see it


def test_abi_declares_the_clip_loss_entry_points():
    from octcubem_amd import _lib
    header = open(os.path.join(ROOT, "include", "octmae.h")).read()
    assert _lib.expected_abi_version() >= 24
    assert re.search(r"^ \* 24: octmae_clip_loss_fwd", header, re.M)
    for sym in SYMBOLS:
        assert re.search(rf"^int {sym}\(", header, re.M), sym
        assert sym in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["octmae_clip_loss_fwd"]) == 18 and len(_lib.SIGNATURES["octmae_clip_loss_bwd"]) == 22
    mk = open(os.path.join(ROOT, "octcubem_amd", "csrc", "Makefile")).read()
    assert "cliploss.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)
    for lib in ("liboctmae.so", "liboctmae_f16.so"):
        path = os.path.join(ROOT, "octcubem_amd", lib)
        if os.path.exists(path):
            names = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
            for sym in SYMBOLS:
                assert re.search(rf"\bT {sym}$", names, re.M), (lib, sym)


def test_scheduler_values_equal_the_reference_formula():
    from octcubem_amd import coem
    opts = [torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=9.0) for _ in range(3)]
    base, warm, steps = 3e-4, 10, 100
    sched = coem.cosine_lr(opts, base, warm, steps)
    want = {0: base * 1 / warm, warm - 1: base, warm: base, steps - 1: 0.5 * (1 + np.cos(np.pi * (steps - 1 - warm) / (steps - warm))) * base}
    for step, lr in want.items():
        got = sched(step)
        assert got == lr, (step, got, lr)
        assert all(g["lr"] == lr for o in opts for g in o.param_groups)
    one = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    coem.assign_learning_rate(one, 0.125)                      # a single optimizer, as the reference passes it
    assert one.param_groups[0]["lr"] == 0.125
    assert want[steps - 1] > 0 and sched(steps) == 0.0


# ------------------------------------------------------------------------------------------------ the loop on stub towers
class StubCLIP(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.visual = torch.nn.Linear(6, 4)
        self.text = torch.nn.Linear(5, 4)
        for p in self.parameters():
            p.data = torch.randn(p.shape, generator=g) * 0.5
        self.logit_scale = torch.nn.Parameter(torch.ones([]) * math.log(1 / 0.07))

    def forward(self, image, text):
        f = torch.nn.functional.normalize
        return f(self.visual(image), dim=-1), f(self.text(text), dim=-1), self.logit_scale.exp()


class Loader(list):
    pass


class SpyReducer:
    world = 1

    def __init__(self, log):
        self.log = log

    def begin_backward(self, sync=True):
        self.log.append(("begin", sync))

    def finish(self):
        self.log.append(("finish",))


class CountingSGD(torch.optim.SGD):
    steps = 0

    def step(self, *a, **k):
        self.steps += 1
        return super().step(*a, **k)


def loop_data(n_batches, bs, seed=4):
    g = torch.Generator().manual_seed(seed)
    loader = Loader((torch.randn(bs, 6, generator=g), torch.randn(bs, 5, generator=g)) for _ in range(n_batches))
    loader.num_batches, loader.num_samples = n_batches, n_batches * bs
    epochs = []
    return {"train": types.SimpleNamespace(dataloader=loader, set_epoch=epochs.append)}, epochs


def loop_args(**kw):
    base = dict(device="cpu", accum_freq=1, rank=0, world_size=1, batch_size=3, local_loss=False, gather_with_grad=False, horovod=False,
                correct_label=0, precision="amp", skip_scheduler=False, grad_clip_norm=None, log_every_n_steps=1, wandb=False,
                multimodal_type="default")
    base.update(kw)
    return types.SimpleNamespace(**base)


def reference_loop(model, batches, accum_freq, opt, loss, seen):
    """A restatement of train_retclip.train_one_epoch's accumulation branch (plain autograd, one optimizer)."""
    acc_in, acc_f = [], [[], []]
    for i, (x, y) in enumerate(batches):
        with torch.no_grad():
            fi, ft, _ = model(x, y)
        acc_f[0].append(fi); acc_f[1].append(ft); acc_in.append((x, y))
        if ((i + 1) % accum_freq) > 0:
            continue
        opt.zero_grad()
        for j in range(accum_freq):
            ci, ctx_, ls = model(*acc_in[j])
            fi = torch.cat(acc_f[0][:j] + [ci] + acc_f[0][j + 1:])
            ft = torch.cat(acc_f[1][:j] + [ctx_] + acc_f[1][j + 1:])
            seen.append((j, fi.detach().clone(), ft.detach().clone()))
            loss(fi, ft, ls).backward()
        opt.step()
        acc_in, acc_f = [], [[], []]
        with torch.no_grad():
            model.logit_scale.clamp_(0, math.log(100))


def test_accumulation_bookkeeping_on_stub_towers():
    from octcubem_amd import coem
    accum, bs, n_batches = 3, 3, 7                       # two groups of three, one batch dropped
    data, epochs = loop_data(n_batches, bs)
    base_loss = coem.ClipLoss(cache_labels=True)
    seen_a, seen_b, log, sched_steps = [], [], [], []

    def spy_loss(store):
        def f(fi, ft, ls):
            return base_loss(fi, ft, ls)
        def wrapped(fi, ft, ls):
            store.append((None, fi.detach().clone(), ft.detach().clone()))
            return f(fi, ft, ls)
        return wrapped

    m_a, m_b = StubCLIP(), StubCLIP()
    opt_a = CountingSGD(m_a.parameters(), lr=0.1)
    opt_b = CountingSGD(m_b.parameters(), lr=0.1)
    rec = coem.train_one_epoch(m_a, data, 5, [opt_a], None, sched_steps.append, loop_args(accum_freq=accum, batch_size=bs),
                               reducers=[SpyReducer(log), SpyReducer(log)], loss=spy_loss(seen_a))
    reference_loop(m_b, list(data["train"].dataloader), accum, opt_b, base_loss, seen_b)
    assert epochs == [5]
    assert rec["steps"] == n_batches // accum == 2 and opt_a.steps == opt_b.steps == 2          # one optimizer step per group, tail dropped
    assert [len(ml) for ml in rec["micro_losses"]] == [accum, accum]
    assert sched_steps == [2 * 5 + i // accum for i in range(n_batches)]                       # scheduler(step) on every batch
    # splice positions: the features every loss call saw are those of the restated loop, position by position
    assert len(seen_a) == len(seen_b) == 2 * accum
    for (_, fi, ft), (j, ri, rt) in zip(seen_a, seen_b):
        assert fi.shape == (accum * bs, 4) and torch.equal(fi, ri) and torch.equal(ft, rt)
    for pa, pb in zip(m_a.parameters(), m_b.parameters()):
        assert torch.equal(pa, pb)
    # sync only on the last micro-step, finish once per group, for each reducer
    per_group = [("begin", False)] * 2 * (accum - 1) + [("begin", True)] * 2 + [("finish",)] * 2
    assert log == per_group * 2, log


def test_loop_refusals_and_the_three_modality_stack():
    from octcubem_amd import coem
    data, _ = loop_data(2, 3)
    m = StubCLIP()
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    run = lambda **kw: coem.train_one_epoch(m, data, 0, opt, kw.pop("scaler", None), lambda s: None, loop_args(**kw), loss=coem.ClipLoss())
    with pytest.raises(NotImplementedError, match="oct_faf_ir"):
        run(multimodal_type="oct_faf_ir")
    with pytest.raises(NotImplementedError, match="default"):
        coem.train_one_epoch_3modalities(m, data, 0, opt, None, lambda s: None, loop_args(), loss=coem.ThreeModalityClipLoss())
    with pytest.raises(NotImplementedError, match="GradScaler"):
        run(scaler=object())
    with pytest.raises(NotImplementedError, match="horovod"):
        run(horovod=True)
    with pytest.raises(NotImplementedError, match="fp16"):
        run(precision="fp16")
    w = coem.stack_weight_modalities([[torch.ones(2), torch.tensor([1.0, 0.0]), torch.zeros(2)],
                                      [torch.ones(1), torch.tensor([0.0]), torch.ones(1)]])
    assert [x.tolist() for x in w] == [[1, 1, 1], [1, 0, 0], [0, 0, 1]]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coem.ClipLoss(fused=True)(torch.randn(4, 3), torch.randn(4, 3), torch.tensor(10.0))
    # fused=False is the composition it was: same bits as the explicit formula
    fi, ft = torch.nn.functional.normalize(torch.randn(5, 3), dim=-1), torch.nn.functional.normalize(torch.randn(5, 3), dim=-1)
    z = torch.tensor(10.0) * fi @ ft.T
    lab = torch.arange(5)
    want = (torch.nn.functional.cross_entropy(z, lab) + torch.nn.functional.cross_entropy((torch.tensor(10.0) * ft @ fi.T), lab)) / 2
    assert torch.equal(coem.ClipLoss()(fi, ft, torch.tensor(10.0)), want)
