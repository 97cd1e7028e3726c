"""GPU: activation recomputation (ops.BlockFn levels none / light / full) and tower locking.

The contract is bit equality throughout: ``ops.ln_apply`` against the ``y`` of ``ops.layernorm_fwd``, ``ops.gelu_apply`` against the
``act`` of the fc1 epilogue, and -- every launch being deterministic -- outputs, input gradients and accumulated parameter gradients of
a Block and of whole models at levels light and full against level none.  What each level keeps is counted in bytes through
``torch.autograd.graph.saved_tensors_hooks``.  The kernel checks run again on the half-operand build in a child process
(tests/f16_worker.py)."""
import os
import traceback
from functools import partial

import pytest
import torch

from tests import children

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import _lib, models_vit_2mod, models_vit_st, ops, optim as foptim, saliency, video_vit
    from octcubem_amd.arena import get_arena

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")
DEV = "cuda"
LN = partial(torch.nn.LayerNorm, eps=1e-6)
GUARD = 4096            # elements on either side of an output handed to the C entry points directly
SENTINEL = 0x5A5A


def bits(t):
    return t.detach().contiguous().view(torch.int16)


def guarded(n):
    """a 16-bit output of n elements between two guard zones filled with a sentinel: (whole buffer, the output's view)"""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(ops.BF16)


def guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ ln_apply
# D below, at and above one chunk per lane (256), the widest row of each kernel instance; M off the four-waves-per-block grain; and
# (ours) M beyond the 2048 waves of the largest grid, where a wave walks more than one row and the next row's prefetch is guarded
LN_CASES = [(M, D) for D in (4, 252, 256, 260, 1024, 2048) for M in (1, 3, 4, 5, 1025)] + [(4099, 256), (4099, 2048), (2049, 516)]


def check_ln_apply():
    for M, D in LN_CASES:
        g = torch.Generator().manual_seed(1000 * D + M)
        x = torch.randn(M, D, generator=g) * 3 + 1
        x[M // 2] = 2.5                                       # a constant row: variance 0, rstd = eps ** -0.5
        gamma, beta = torch.randn(D, generator=g) + 1, torch.randn(D, generator=g)
        x, gamma, beta = x.to(DEV), gamma.to(DEV), beta.to(DEV)
        y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, 1e-6)
        got = ops.ln_apply(x, mean, rstd, gamma, beta)
        assert got.dtype == ops.BF16 and torch.equal(bits(got), bits(y)), (M, D, int((bits(got) != bits(y)).sum()))
        buf, out = guarded(M * D)
        _lib.call("octmae_ln_apply", x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), M, D,
                  ops._stream())
        assert torch.equal(bits(out).view(M, D), bits(y)) and guards_intact(buf, M * D), (M, D)


def check_ln_apply_refusals():
    for M, D in ((4, 6), (4, 2052), (4, 4096), (3, 2)):
        x = torch.zeros(M, D, device=DEV)
        with pytest.raises(_lib.OctmaeError, match="bad argument"):
            ops.ln_apply(x, torch.zeros(M, device=DEV), torch.ones(M, device=DEV), torch.ones(D, device=DEV), torch.zeros(D, device=DEV))
    x = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.ln_apply(x, torch.zeros(3, device=DEV), torch.ones(4, device=DEV), torch.ones(8, device=DEV), torch.zeros(8, device=DEV))
    with pytest.raises(ValueError):
        ops.ln_apply(x, torch.zeros(4, device=DEV), torch.ones(4, device=DEV), torch.ones(4, device=DEV), torch.zeros(8, device=DEV))
    with pytest.raises(RuntimeError):
        ops.ln_apply(x.to(ops.BF16), torch.zeros(4, device=DEV), torch.ones(4, device=DEV), torch.ones(8, device=DEV), torch.zeros(8, device=DEV))


# ------------------------------------------------------------------------------------------------ gelu_apply
def check_gelu_apply_vs_fc1_epilogue():
    for M, K, N in ((5, 64, 256), (257, 128, 512)):
        g = torch.Generator().manual_seed(M)
        x = torch.randn(M, K, generator=g).to(ops.BF16).to(DEV)
        w = (torch.randn(N, K, generator=g) * 0.3).to(ops.BF16).to(DEV)
        b = torch.randn(N, generator=g).to(DEV)
        pre, act = ops.linear_fwd(x, w, b, "gelu")
        got = ops.gelu_apply(pre)
        assert got.shape == act.shape and torch.equal(bits(got), bits(act)), (M, K, N, int((bits(got) != bits(act)).sum()))


def check_gelu_apply_on_every_pattern():
    """all 65 536 bit patterns as a [256, 256] matrix through the identity-weight GEMM (tests/test_gpu_gemm_elements.py feeds its sweep
    the same way), the finite ones first and the infinities and NaNs behind them in rows of their own (255 + 1 rows of bfloat16, 248 + 8 of
    half): a row that holds an inf or a NaN comes out non-finite as a whole, every other row is the input bit for bit (but the one -0), so
    every FINITE value of the type is among the finite ``pre``"""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(ops.BF16)
    isfin = torch.isfinite(v.float())
    assert int(isfin.sum()) % 256 == 0
    xa = torch.cat([v[isfin], v[~isfin]]).view(256, 256)
    w = torch.eye(256).to(ops.BF16).to(DEV)
    pre, act = ops.linear_fwd(xa.to(DEV), w, torch.zeros(256, device=DEV), "gelu")
    got = ops.gelu_apply(pre)
    fin = torch.isfinite(pre.float())
    n_finite = int(torch.isfinite(xa.float()).sum())
    assert len(set(bits(pre)[fin].cpu().tolist())) >= n_finite - 1, "the finite pre-activations do not cover the type"
    assert torch.equal(bits(got)[fin], bits(act)[fin]), int((bits(got)[fin] != bits(act)[fin]).sum())


# one lane; below, at and above a wave; one past 64 x 304 x 4 lanes; and past the 512 x 256 lanes x 4 loads of this kernel's unrolled
# loop, with a tail that takes the single-load loop and ends inside a block
GELU_N = [8, 8 * 63, 8 * 64, 8 * 65, 8 * (64 * 304 * 4 + 1), 8 * (512 * 256 * 4 + 3 * 512 * 256 + 77)]


def check_gelu_apply_sizes():
    shift = 8 * 37
    for n in GELU_N:
        g = torch.Generator().manual_seed(n % 9973)
        data = (torch.randn(n + shift, generator=g) * 3).to(ops.BF16).to(DEV)
        whole = ops.gelu_apply(data)                                       # element i of the case sits at i + shift here ...
        buf, out = guarded(n)
        src = data[shift:].clone()
        _lib.call("octmae_gelu_apply", src.data_ptr(), out.data_ptr(), n, ops._stream())      # ... and at i here: another lane, another trip
        assert torch.equal(bits(out), bits(whole[shift:])) and guards_intact(buf, n), n
        if n >= 16:
            k = 8 * ((n // 8) // 3 + 1)
            parts = torch.cat([ops.gelu_apply(src[:k].clone()), ops.gelu_apply(src[k:].clone())])
            assert torch.equal(bits(parts), bits(out)), n
    for bad in (12, 7, 0):
        with pytest.raises(_lib.OctmaeError, match="bad argument"):
            ops.gelu_apply(torch.zeros(bad, dtype=ops.BF16, device=DEV))
    with pytest.raises(RuntimeError):
        ops.gelu_apply(torch.zeros(16, device=DEV))


def check_colsum_order():
    """the bias-gradient column sums ADDED to a gradient that is already there, beyond 256 rows (several row splits): the same bits call
    after call (atomic adds in finishing order gave (g + a) + b or (g + b) + a) -- what bit-equal accumulated gradients rest on"""
    g = torch.Generator().manual_seed(8)
    for M, N in ((260, 64), (260, 128), (5121, 1024), (40000, 64)):
        for dt in (torch.float32, ops.BF16):
            a = (torch.randn(M, N, generator=g) * 3).to(dt).to(DEV)
            start = torch.randn(N, generator=g).to(DEV) * 100
            outs = []
            for _ in range(8):
                out = start.clone()
                ops.colsum_accum(a, out)
                outs.append(out)
            assert all(torch.equal(o, outs[0]) for o in outs[1:]), (M, N, dt)
            bare = []                                   # the workspace-free entry point the library's own callers take
            for _ in range(8):
                out = start.clone()
                _lib.call("octmae_colsum_accum", a.data_ptr(), 1 if dt == ops.BF16 else 0, out.data_ptr(), M, N, N, ops._stream())
                bare.append(out)
            assert all(torch.equal(o, bare[0]) for o in bare[1:]), (M, N, dt, "without a workspace")
            outs.append(bare[0])
            want = start.double() + a.double().sum(0)
            for o in (outs[0], outs[-1]):
                assert float((o.double() - want).abs().max()) <= 1e-5 * float(a.double().abs().sum(0).max() + 100), (M, N, dt)


KERNEL_CHECKS = {"colsum_order": check_colsum_order, "ln_apply": check_ln_apply, "ln_apply_refusals": check_ln_apply_refusals, "gelu_vs_epilogue": check_gelu_apply_vs_fc1_epilogue,
                 "gelu_every_pattern": check_gelu_apply_on_every_pattern, "gelu_sizes": check_gelu_apply_sizes}


@pytest.mark.parametrize("name", list(KERNEL_CHECKS))
def test_kernels(name):
    KERNEL_CHECKS[name]()


def half_build_kernel_checks():
    """What tests/f16_worker.py runs on the half-operand build: every check, a failed one recorded with its traceback."""
    ran, failed = [], {}
    for name, fn in KERNEL_CHECKS.items():
        ran.append(name)
        try:
            fn()
            torch.cuda.synchronize()
        except AssertionError:
            failed[name] = traceback.format_exc()[-1500:]
    return {"ran": ran, "failed": failed}


def test_kernels_on_the_half_build():
    assert os.path.exists(LIB_F16), f"{LIB_F16} is missing: __graft_entry__.build() makes it"
    children.spawn_f16_worker("recompute_f16", "tests.test_gpu_recompute:half_build_kernel_checks")
    res = children.f16_worker_result("recompute_f16")
    assert res["lib"] == "liboctmae_f16.so" and res["lp_is_f16"] is True
    assert res["ran"] == list(KERNEL_CHECKS) and res["failed"] == {}, res["failed"]


# ------------------------------------------------------------------------------------------------ BlockFn levels
def randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n_, p_ in module.named_parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) * (0.05 if p_.dim() > 1 else 0.02) + (1.0 if "norm" in n_ and n_.endswith("weight") else 0.0))
    return module


def make_block(kind, C, dp):
    if kind == "block":
        blk = video_vit.Block(C, 2, 4.0, qkv_bias=True, norm_layer=LN, drop_path=dp)
    else:
        blk = video_vit.create_block(C, 2, 4.0, True, 0.0, 0.0, drop_path1=dp, drop_path2=dp, norm_layer=LN, act_layer=torch.nn.GELU,
                                     use_flash_attn=True, fused_bias_fc=False, fused_mlp=False, fused_dropout_add_ln=False)
    return randomize(blk, 3).to(DEV).train()


def run_block(blk, kind, mode, x, ws, wgrads=True):
    """two accumulated backwards at ``mode`` from zeroed gradients and a reset seed -> (outputs, input gradient, parameter gradients)"""
    blk.recompute = mode
    with torch.no_grad():
        blk(x) if kind == "block" else blk(x, None)             # binds the arena of a block that has not run yet
    arena = get_arena(blk)
    arena.zero_grad()
    torch.manual_seed(77)
    xg = x.clone().requires_grad_(True)
    outs = []
    for w in ws:
        if kind == "block":
            o = blk(xg)
            loss = (o * w[0]).sum()
            outs.append(o.detach().clone())
        else:                                                   # the pair of final_residual=False, both halves in the loss
            h, r = blk(xg, x * 0.5)
            loss = (h * w[0]).sum() + (r * w[1]).sum()
            outs += [h.detach().clone(), r.detach().clone()]
        with ops.weight_grads(wgrads):
            loss.backward()
    torch.cuda.synchronize()
    return outs, xg.grad.clone(), {n_: p_.grad.clone() for n_, p_ in blk.named_parameters()}, arena


@pytest.mark.parametrize("dp", [0.0, 0.5])
@pytest.mark.parametrize("N", [9, 130])
@pytest.mark.parametrize("C", [64, 128])            # two heads: head_dim 32 and 64
@pytest.mark.parametrize("kind", ["block", "flash"])
def test_block_levels_are_bit_equal(kind, C, N, dp):
    blk = make_block(kind, C, dp)
    g = torch.Generator().manual_seed(C + N)
    x = torch.randn(2, N, C, generator=g).to(DEV)
    ws = [(torch.randn(2, N, C, generator=g).to(DEV), torch.randn(2, N, C, generator=g).to(DEV)) for _ in range(2)]
    base_o, base_dx, base_g, _ = run_block(blk, kind, "none", x, ws)
    assert float(base_dx.abs().max()) > 0
    if dp == 0.0:       # (with stochastic depth a branch may be dropped for both samples; a k bias has a gradient of exactly zero in exact arithmetic)
        assert all(float(v.abs().max()) > 0 for n_, v in base_g.items() if ".k.bias" not in n_)
    off_o, off_dx, off_g, arena = run_block(blk, kind, "none", x, ws, wgrads=False)
    assert torch.equal(off_dx, base_dx) and float(arena.grad.abs().max()) == 0.0
    for mode in ("light", "full"):
        o, dx, gr, _ = run_block(blk, kind, mode, x, ws)
        assert len(o) == len(base_o) and all(torch.equal(a, b) for a, b in zip(o, base_o)), (mode, "outputs")
        assert torch.equal(dx, base_dx), (mode, "input gradient", float((dx - base_dx).abs().max()))
        for n_ in base_g:
            assert torch.equal(gr[n_], base_g[n_]), (mode, n_, float((gr[n_] - base_g[n_]).abs().max()))
        o, dx, gr, arena = run_block(blk, kind, mode, x, ws, wgrads=False)
        assert torch.equal(dx, base_dx), (mode, "input gradient without weight gradients")
        assert float(arena.grad.abs().max()) == 0.0, (mode, "the gradient arena was written with weight gradients off")


def test_block_rejects_an_unknown_mode():
    blk = make_block("block", 64, 0.0)
    blk.recompute = "heavy"
    with pytest.raises(ValueError):
        blk(torch.randn(2, 9, 64, device=DEV))


# ------------------------------------------------------------------------------------------------ what is saved
@pytest.mark.parametrize("kind", ["block", "flash"])
@pytest.mark.parametrize("C,N", [(64, 9), (128, 130)])
def test_saved_bytes_per_level(kind, C, N):
    """per token and block at width C, hidden 4 C, 16-bit operands -- everything BlockFn saves outside the parameter arena:
         none   x 4C + y1 2C + qkv 6C + o 2C + x2 4C + y2 2C + pre 8C + act 8C = 36 C, + mean / rstd of both norms (16 B) + lse (4 B per head)
         light  without y1, y2, act: 24 C + the same statistics
         full   x alone: 4 C"""
    B, H = 2, 2
    blk = make_block(kind, C, 0.0)
    x = torch.randn(B, N, C, device=DEV)
    with torch.no_grad():
        blk(x) if kind == "block" else blk(x, None)
    arena = get_arena(blk)
    own = {arena.flat.untyped_storage().data_ptr(), arena.lp.untyped_storage().data_ptr()}
    M = B * N
    stats = 16 * M + 4 * B * H * N
    for mode, want in (("none", M * 36 * C + stats), ("light", M * 24 * C + stats), ("full", M * 4 * C)):
        blk.recompute = mode
        total = [0]

        def pack(t):
            if t.untyped_storage().data_ptr() not in own:
                total[0] += t.numel() * t.element_size()
            return t

        xg = x.clone().requires_grad_(True)
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = blk(xg) if kind == "block" else blk(xg, None)
        print(kind, C, N, mode, "saved bytes", total[0], "expected", want)
        assert total[0] == want, (mode, total[0], want)
        out = out if kind == "block" else out[0]
        out.sum().backward()                 # and the backward runs off the hooked tensors


# ------------------------------------------------------------------------------------------------ models
def run_model(model, mode, step, n_steps=2):
    """``n_steps`` accumulated backwards of ``step(model, k) -> (loss, outputs)`` with the model at ``mode``: losses, outputs, gradients"""
    if mode == "none":
        model.set_grad_checkpointing(False)
    elif mode == "full":
        model.set_grad_checkpointing(True)
    else:
        model.set_grad_checkpointing(True, mode)
    model.arena.zero_grad()
    torch.manual_seed(5)
    losses, outs = [], []
    for k in range(n_steps):
        loss, out = step(model, k)
        loss.backward()
        losses.append(loss.detach().clone())
        outs.append(out.detach().clone())
    torch.cuda.synchronize()
    return losses, outs, {n_: p_.grad.clone() for n_, p_ in model.named_parameters() if p_.grad is not None}


def assert_modes_agree(model, step):
    model.train()
    with torch.no_grad():
        step(model, 0)                        # binds the arena
    base = run_model(model, "none", step)
    assert sum(float(v.abs().max()) > 0 for v in base[2].values()) >= len(list(model.parameters())) // 2      # (all but parameters the step does not use)
    for mode in ("full", "light"):
        got = run_model(model, mode, step)
        assert {b.recompute for b in model.modules() if isinstance(b, video_vit.Block)} == {mode}
        for a, b in zip(got[0] + got[1], base[0] + base[1]):
            assert torch.equal(a, b), (mode, "loss / outputs")
        assert got[2].keys() == base[2].keys()
        for n_ in base[2]:
            assert torch.equal(got[2][n_], base[2][n_]), (mode, n_, float((got[2][n_] - base[2][n_]).abs().max()))
    model.set_grad_checkpointing(False)


def assert_saliency_agrees(model, x):
    model.set_grad_checkpointing(False)
    a = saliency.input_gradient(model, x)
    model.set_grad_checkpointing(True)
    b = saliency.input_gradient(model, x)
    model.set_grad_checkpointing(False)
    assert float(a["grad"].abs().max()) > 0
    assert torch.equal(a["grad"], b["grad"]) and torch.equal(a["logits"], b["logits"]) and torch.equal(a["map"], b["map"])


def test_small_mae_modes_agree(golden_dir):
    from tests import test_gpu_model as TM
    z, cfg, P = TM.small(golden_dir)
    m = TM.build(cfg, P)
    imgs, noise = torch.from_numpy(z["imgs"]).to(DEV), torch.from_numpy(z["noise"]).to(DEV)

    def step(model, k):
        loss, pred, _ = model(imgs * (1.0 + 0.25 * k), mask_ratio=float(z["mask_ratio"]), noise=noise)
        return loss, pred

    assert_modes_agree(m, step)
    m.set_grad_checkpointing(True)
    assert {b.recompute for b in list(m.blocks) + list(m.decoder_blocks)} == {"full"}


def st_tower(depth, flash, C=64, drop_path_rate=0.0):
    m = models_vit_st.VisionTransformer(num_frames=4, t_patch_size=2, img_size=64, patch_size=16, in_chans=1, num_classes=8, embed_dim=C,
                                        depth=depth, num_heads=2, norm_layer=LN, sep_pos_embed=True, cls_embed=True, use_flash_attn=flash,
                                        drop_path_rate=drop_path_rate)
    return randomize(m, 11).to(DEV)


@pytest.mark.parametrize("flash", [True, False])
def test_oct_tower_modes_agree(flash):
    """33 tokens; flash blocks at width 128 (head_dim 64), timm-style blocks at width 64 (head_dim 32) with stochastic depth"""
    m = st_tower(3, flash, C=128 if flash else 64, drop_path_rate=0.0 if flash else 0.2)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 1, 4, 64, 64, generator=g).to(DEV)
    w = torch.randn(2, 3, 8, generator=g).to(DEV)

    def step(model, k):
        out = model(x)
        return (out * w[k]).sum(), out

    assert_modes_agree(m, step)
    assert_saliency_agrees(m, x)


def test_two_modality_tower_modes_agree():
    m = randomize(models_vit_2mod.VisionTransformer(image_size=64, out_dim=8, embed_dim=64, depth=2, num_heads=2, norm_layer=LN), 12).to(DEV)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 64, 64, generator=g).to(DEV)
    w = torch.randn(2, 2, 8, generator=g).to(DEV)

    def step(model, k):
        out = model(x, modality=k)
        return (out * w[k]).sum(), out

    assert_modes_agree(m, step)
    assert_saliency_agrees(m, x)


# ------------------------------------------------------------------------------------------------ locking, end to end
def test_lock_after_the_first_forward_keeps_locked_weights_still():
    """lock() AFTER the arena is bound: every frozen parameter had a gradient buffer; FusedAdamW steps whatever has one, and its weight
    decay alone would move the locked weights.  One step over model.parameters(): locked bit-unchanged, unlocked moved, and the same with
    recomputation on."""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 1, 4, 64, 64, generator=g).to(DEV)
    w = torch.randn(2, 8, generator=g).to(DEV)
    after = {}
    for mode in ("none", "full"):
        m = st_tower(4, True).train()
        torch.manual_seed(6)                             # the tower's dropout in front of its head draws the same masks in both runs
        (m(x) * w).sum().backward()                      # binds the arena; every parameter now holds a gradient
        assert all(p.grad is not None for p in m.parameters())
        m.lock(unlocked_groups=2)
        m.set_grad_checkpointing(mode == "full")
        open_ = {n_ for n_, p_ in m.named_parameters() if p_.requires_grad}
        assert open_ == {n_ for n_, _ in m.named_parameters() if n_.startswith(("blocks.3.", "norm.", "head."))}
        before = {n_: p_.detach().clone() for n_, p_ in m.named_parameters()}
        opt = foptim.FusedAdamW(m.parameters(), lr=1e-2, betas=(0.9, 0.95), weight_decay=0.05)
        opt.zero_grad()
        (m(x) * w).sum().backward()
        assert all((p_.grad is None) == (n_ not in open_) for n_, p_ in m.named_parameters())
        opt.step()
        torch.cuda.synchronize()
        for n_, p_ in m.named_parameters():
            if n_ in open_:
                assert not torch.equal(p_.detach(), before[n_]), f"{n_} is unlocked and did not move"
            else:
                assert torch.equal(p_.detach(), before[n_]), f"{n_} is locked and moved"
        m.eval()
        with torch.no_grad():                            # the operand copy of the next forward follows what moved
            after[mode] = ({n_: p_.detach().clone() for n_, p_ in m.named_parameters()}, m(x).clone())
    for n_ in after["none"][0]:
        assert torch.equal(after["none"][0][n_], after["full"][0][n_]), n_
    assert torch.equal(after["none"][1], after["full"][1])
