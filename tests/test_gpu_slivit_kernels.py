"""GPU: the ConvNeXt layer kernels (octcubem_amd/csrc/convnext.hip through ops.dwconv7_* / ops.layer_scale_*) element by element.

Reference: F.conv2d(groups=C) in float64 on the CPU.  Bounds (tests/slivit_ref.py; tests/test_cpu_slivit.py shows what they pass and what
they catch), no measured constant in any of them:
  * forward and input gradient, per element: |err| <= gamma_50 * (|bias| + sum |w x|), gamma_n = n u / (1 - n u), u = 2^-24 -- 50 fp32 terms
    in any order; the residual gradient is then added EXACTLY (one more rounding of the final sum: checked bit for bit against
    torch's fp32 add of the kernel's own result without it);
  * weight and bias gradient, per element: the same form with n = B H W + G + 5 -- one term per summed pixel (the products are fused
    multiply-adds), 3 additions that fold a workgroup's row quarters, G - 1 that fold the G per-workgroup partials (G read from the
    workspace query), one that adds into the gradient buffer, and one to spare; the magnitude includes the buffer's previous content;
  * layer scale: forward and dbranch bit-equal to torch's fp32 mul / add and one cast; the gamma gradient with n = M + RP + G + 2
    (rows, the RP row parts a workgroup folds, the G partials, the accumulation).
Shapes: maps narrower than the halo, equal to the filter, one past the 8 x 16 tile in each direction, several tiles; channel counts
below a wave's 64 lanes x 4, a non-power-of-two, and a tail after the 32-channel blocks; and the shapes of slivit_ref.DW_TRIP_SHAPES /
LS_TRIP_SHAPE, where the workgroups of the weight gradient and of the layer-scale backward outnumber their cap.  The same checks run on the half-operand build
in a child process (tests/f16_worker.py)."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import _lib, ops
from tests import children
from tests import slivit_ref as R

DEV = "cuda"
HW = [(1, 1), (2, 3), (3, 7), (7, 7), (8, 9), (17, 5), (33, 40)]
CS = [8, 32, 96, 136]
BS = [1, 3]
GUARD = 256          # floats in front of and behind every output (a multiple of 4: the 16-byte alignment survives)
SENTINEL = -7680.0     # exact in fp32, bfloat16 and half


def _guarded(n, dtype=torch.float32):
    """(whole buffer, the n elements in its middle)"""
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _problem(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H, W, C), generator=g)
    wt = torch.randn((C, 7, 7), generator=g) / 7.0
    bias = torch.randn((C,), generator=g)
    dz = torch.randn((B, H, W, C), generator=g)
    dres = torch.randn((B, H, W, C), generator=g)
    gw0 = torch.randn((C, 7, 7), generator=g)
    gb0 = torch.randn((C,), generator=g)
    return x, wt, bias, dz, dres, gw0, gb0


def _wgrad_ref64(dz, x):
    """(gw [C, 7, 7], sum |dz x| per tap, gb, sum |dz|) in float64: the weight gradient of the depthwise convolution"""
    B, H, W, C = x.shape
    xp = F.pad(x.double().permute(0, 3, 1, 2), (3, 3, 3, 3))
    d = dz.double().permute(0, 3, 1, 2)
    gw, mag = torch.zeros((C, 7, 7), dtype=torch.float64), torch.zeros((C, 7, 7), dtype=torch.float64)
    for i in range(7):
        for j in range(7):
            p = d * xp[:, :, i:i + H, j:j + W]
            gw[:, i, j] = p.sum(dim=(0, 2, 3))
            mag[:, i, j] = p.abs().sum(dim=(0, 2, 3))
    return gw, mag, d.sum(dim=(0, 2, 3)), d.abs().sum(dim=(0, 2, 3))


def check_dwconv(H, W, report=None, cs=CS, bs=BS):
    st = ops._stream()
    for C in cs:
        for B in bs:
            x, wt, bias, dz, dres, gw0, gb0 = _problem(B, H, W, C, seed=1000 * H + 10 * W + C + B)
            n = x.numel()
            xd, wd, bd, dzd, dresd = (t.to(DEV) for t in (x, wt, bias, dz, dres))
            tag = f"B{B} H{H} W{W} C{C}"
            # ---- forward, inside guard rows
            zbuf, z = _guarded(n)
            _lib.call("octmae_dwconv7_fwd", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), z.data_ptr(), B, H, W, C, st)
            z64, zmag = R.dwconv_ref64(x, wt, bias)
            err = (z.cpu().double().view(B, H, W, C) - z64).abs()
            ratio = float((err / R.dwconv_bound(zmag)).max())
            assert _guards_intact(zbuf, n), f"dwconv7_fwd wrote outside its output ({tag})"
            assert ratio <= 1.0, f"dwconv7_fwd {tag}: worst |err| / bound = {ratio:.3f}"
            assert torch.equal(ops.dwconv7_fwd(xd, wd, bd).view(-1), z), f"dwconv7_fwd: the wrapper and the raw call differ ({tag})"
            # ---- input gradient: the flipped filter; with dres = the result without + dres, exactly
            dbuf, dx = _guarded(n)
            _lib.call("octmae_dwconv7_bwd_input", dzd.data_ptr(), wd.data_ptr(), None, dx.data_ptr(), B, H, W, C, st)
            dx64, dmag = R.dwconv_ref64(dz, wt.flip(1, 2), None)
            err = (dx.cpu().double().view(B, H, W, C) - dx64).abs()
            ratio_i = float((err / R.dwconv_bound(dmag)).max()) if float(dmag.max()) > 0 else 0.0
            assert _guards_intact(dbuf, n), f"dwconv7_bwd_input wrote outside its output ({tag})"
            assert ratio_i <= 1.0, f"dwconv7_bwd_input {tag}: worst |err| / bound = {ratio_i:.3f}"
            dx_res = ops.dwconv7_bwd_input(dzd, wd, dresd)
            assert torch.equal(dx_res.view(-1), dx + dresd.view(-1)), f"dwconv7_bwd_input: dres is not added exactly ({tag})"
            # ---- weight gradient: accumulates into what the buffers hold, bit-equal twice, inside guards (the workspace too)
            nws = _lib.load().octmae_dwconv7_bwd_weight_ws_floats(B, H, W, C)
            assert nws > 0 and nws % (50 * C) == 0
            G = nws // (50 * C)
            runs = []
            for _ in range(2):
                gwbuf, gw = _guarded(C * 49)
                gbbuf, gb = _guarded(C)
                wsbuf, ws = _guarded(nws)
                gw.copy_(gw0.view(-1)); gb.copy_(gb0)
                _lib.call("octmae_dwconv7_bwd_weight", dzd.data_ptr(), xd.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), B, H, W, C, st)
                assert _guards_intact(gwbuf, C * 49) and _guards_intact(gbbuf, C) and _guards_intact(wsbuf, nws), \
                    f"dwconv7_bwd_weight wrote outside a buffer ({tag})"
                runs.append((gw.clone(), gb.clone()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"dwconv7_bwd_weight: two runs differ ({tag})"
            gw64, gwmag, gb64, gbmag = _wgrad_ref64(dz, x)
            gn = R.gamma_n(B * H * W + G + 5)
            rw = float(((runs[0][0].cpu().double().view(C, 7, 7) - (gw0.double() + gw64)).abs() / (gn * (gw0.double().abs() + gwmag))).max())
            rb_ = float(((runs[0][1].cpu().double() - (gb0.double() + gb64)).abs() / (gn * (gb0.double().abs() + gbmag))).max())
            assert rw <= 1.0 and rb_ <= 1.0, f"dwconv7_bwd_weight {tag}: worst |err| / bound = {rw:.3f} (gw), {rb_:.3f} (gb)"
            gw2, gb2 = gw0.to(DEV).clone(), gb0.to(DEV).clone()
            ops.dwconv7_bwd_weight(dzd, xd, gw2, gb2)
            assert torch.equal(gw2.view(-1), runs[0][0]) and torch.equal(gb2, runs[0][1])
            if report is not None:
                report[tag] = (ratio, ratio_i, rw, rb_)


def check_layer_scale(report=None, ms=(1, 5, 257, 1031), cs=CS + [1032]):
    st = ops._stream()
    for M in ms:
        for C in cs:
            g = torch.Generator().manual_seed(77 + M + C)
            res, branch, dout = (torch.randn((M, C), generator=g) for _ in range(3))
            gamma, gg0 = torch.rand((C,), generator=g) + 0.5, torch.randn((C,), generator=g)
            resd, brd, doutd, gmd = (t.to(DEV) for t in (res, branch, dout, gamma))
            tag = f"M{M} C{C}"
            obuf, out = _guarded(M * C)
            _lib.call("octmae_layer_scale_fwd", resd.data_ptr(), brd.data_ptr(), gmd.data_ptr(), out.data_ptr(), M, C, st)
            assert _guards_intact(obuf, M * C), f"layer_scale_fwd wrote outside its output ({tag})"
            assert torch.equal(out.cpu().view(M, C), res + gamma * branch), f"layer_scale_fwd is not torch's mul + add ({tag})"
            assert torch.equal(ops.layer_scale_fwd(resd, brd, gmd).view(-1), out)
            nws = _lib.load().octmae_layer_scale_bwd_ws_floats(M, C)
            assert nws > 0 and nws % C == 0
            G, RP = nws // C, 256 // min(C // 4, 256)
            runs = []
            for _ in range(2):
                dbuf, db = _guarded(M * C, ops.BF16)
                ggbuf, gg = _guarded(C)
                wsbuf, ws = _guarded(nws)
                gg.copy_(gg0)
                _lib.call("octmae_layer_scale_bwd", doutd.data_ptr(), brd.data_ptr(), gmd.data_ptr(), db.data_ptr(), gg.data_ptr(), ws.data_ptr(),
                          M, C, st)
                assert _guards_intact(dbuf, M * C) and _guards_intact(ggbuf, C) and _guards_intact(wsbuf, nws), \
                    f"layer_scale_bwd wrote outside a buffer ({tag})"
                runs.append((db.clone(), gg.clone()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"layer_scale_bwd: two runs differ ({tag})"
            assert torch.equal(runs[0][0].cpu().view(M, C), (gamma * dout).to(ops.BF16)), f"dbranch is not one rounding of gamma * dout ({tag})"
            p = dout.double() * branch.double()
            gn = R.gamma_n(M + RP + G + 2)
            r = float(((runs[0][1].cpu().double() - (gg0.double() + p.sum(0))).abs() / (gn * (gg0.double().abs() + p.abs().sum(0)))).max())
            assert r <= 1.0, f"layer_scale_bwd {tag}: gamma gradient worst |err| / bound = {r:.3f}"
            # without the gamma gradient: the same dbranch, nothing else touched
            assert torch.equal(ops.layer_scale_bwd(doutd, None, gmd, None).view(-1), runs[0][0])
            gg2 = gg0.to(DEV).clone()
            assert torch.equal(ops.layer_scale_bwd(doutd, brd, gmd, gg2).view(-1), runs[0][0]) and torch.equal(gg2, runs[0][1])
            if report is not None:
                report[tag] = r


def check_argument_checks():
    """-1 before any launch: the outputs keep their sentinel"""
    lib = _lib.load()
    st = ops._stream()
    x = torch.randn((1, 4, 4, 16), device=DEV)
    wt, bias = torch.randn((16, 7, 7), device=DEV), torch.randn((16,), device=DEV)
    out = torch.full((1, 4, 4, 16), SENTINEL, device=DEV)
    ws = torch.full((50 * 16 * 4,), SENTINEL, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    N = None
    calls = [
        lib.octmae_dwconv7_fwd(p(x), p(wt), p(bias), p(out), 1, 4, 4, 12, st),              # C % 8
        lib.octmae_dwconv7_fwd(p(x), p(wt), p(bias), p(out), 1, 4, 4, 4, st),
        lib.octmae_dwconv7_fwd(N, p(wt), p(bias), p(out), 1, 4, 4, 16, st),                 # null pointers
        lib.octmae_dwconv7_fwd(p(x), N, p(bias), p(out), 1, 4, 4, 16, st),
        lib.octmae_dwconv7_fwd(p(x), p(wt), N, p(out), 1, 4, 4, 16, st),
        lib.octmae_dwconv7_fwd(p(x), p(wt), p(bias), N, 1, 4, 4, 16, st),
        lib.octmae_dwconv7_fwd(p(x), p(wt), p(bias), p(out), 0, 4, 4, 16, st),              # empty
        lib.octmae_dwconv7_fwd(p(x), p(wt), p(bias), p(out), 1, 0, 4, 16, st),
        lib.octmae_dwconv7_fwd(ctypes.c_void_p(x.data_ptr() + 4), p(wt), p(bias), p(out), 1, 2, 2, 16, st),      # misaligned
        lib.octmae_dwconv7_bwd_input(p(x), p(wt), N, p(out), 1, 4, 4, 12, st),
        lib.octmae_dwconv7_bwd_input(N, p(wt), N, p(out), 1, 4, 4, 16, st),
        lib.octmae_dwconv7_bwd_input(p(x), p(wt), N, N, 1, 4, 4, 16, st),
        lib.octmae_dwconv7_bwd_weight(p(x), p(x), p(out), p(out), p(ws), 1, 4, 4, 12, st),
        lib.octmae_dwconv7_bwd_weight(p(x), p(x), p(out), p(out), N, 1, 4, 4, 16, st),
        lib.octmae_dwconv7_bwd_weight(p(x), p(x), N, p(out), p(ws), 1, 4, 4, 16, st),
        lib.octmae_dwconv7_bwd_weight(p(x), p(x), p(out), N, p(ws), 1, 4, 4, 16, st),
        lib.octmae_layer_scale_fwd(p(x), p(x), p(bias), p(out), 16, 12, st),
        lib.octmae_layer_scale_fwd(p(x), N, p(bias), p(out), 16, 16, st),
        lib.octmae_layer_scale_fwd(p(x), p(x), p(bias), N, 16, 16, st),
        lib.octmae_layer_scale_bwd(p(x), p(x), p(bias), p(out), p(out), p(ws), 16, 12, st),
        lib.octmae_layer_scale_bwd(p(x), N, p(bias), p(out), p(out), p(ws), 16, 16, st),   # a gamma gradient without branch
        lib.octmae_layer_scale_bwd(p(x), p(x), p(bias), p(out), p(out), N, 16, 16, st),    # ... without a workspace
        lib.octmae_layer_scale_bwd(p(x), p(x), p(bias), N, N, N, 16, 16, st),
    ]
    torch.cuda.synchronize()
    assert calls == [-1] * len(calls), calls
    assert lib.octmae_dwconv7_bwd_weight_ws_floats(1, 4, 4, 12) == -1 and lib.octmae_layer_scale_bwd_ws_floats(4, 12) == -1
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    with pytest.raises(RuntimeError):
        ops.dwconv7_fwd(x[..., :12].contiguous(), wt[:12].contiguous(), bias[:12].contiguous())
    with pytest.raises(RuntimeError):
        ops.dwconv7_fwd(x.double(), wt, bias)
    with pytest.raises(RuntimeError):
        ops.layer_scale_fwd(x.view(-1, 16), x.view(-1, 16)[:3].contiguous(), bias)


def check_dwconv_trips(shape, report=None):
    """A shape of R.DW_TRIP_SHAPES: by the library's own workspace answer G < ntiles, so workgroups of the weight gradient walk a second
    tile with their accumulators kept and both LDS images rewritten; then every check of check_dwconv at that shape."""
    B, H, W, C = shape
    ntiles, cblocks, G = R.dw_wgrad_plan(B, H, W, C)
    nws = _lib.load().octmae_dwconv7_bwd_weight_ws_floats(B, H, W, C)
    assert nws == 50 * C * G and nws // (50 * C) < ntiles, f"{shape}: {ntiles} tiles, workspace for {nws / (50 * C)} workgroups"
    check_dwconv(H, W, report, cs=[C], bs=[B])


def check_layer_scale_trips(report=None):
    """R.LS_TRIP_SHAPE: the small-C form (RP = 128 rows per workgroup, folded through s_red) with M > G RP by the library's own answer"""
    M, C = R.LS_TRIP_SHAPE
    CVB, RP, ncb, G = R.ls_bwd_plan(M, C)
    nws = _lib.load().octmae_layer_scale_bwd_ws_floats(M, C)
    assert nws == G * C and RP == 128 and M > (nws // C) * RP, f"M {M}: workspace for {nws / C} workgroups of {RP} rows"
    check_layer_scale(report, ms=(M,), cs=[C])
    check_layer_scale_exact(M, C, report)


def check_layer_scale_exact(M, C, report=None):
    """The gamma gradient on R.ls_dyadic_problem: every fp32 partial sum is exact, so the result EQUALS the float64 one -- each trip of
    each workgroup, each row part folded through s_red and each of the G partials is in it or the comparison fails (the bound of
    check_layer_scale, gamma_n of 260 000 terms, is thousands of times wider than one trip's share; tests/test_cpu_slivit.py drops trips
    and parts from the restated walk to show what this equality sees)."""
    st = ops._stream()
    dout, branch, gamma, gg0 = R.ls_dyadic_problem(M, C, seed=5)
    want = gg0.double() + (dout.double() * branch.double()).sum(0)
    assert torch.equal(want.float().double(), want)
    assert torch.equal(gg0.double() + R.ls_bwd_walk_sum(dout, branch), want)
    brd, doutd, gmd = (t.to(DEV) for t in (branch, dout, gamma))
    nws = _lib.load().octmae_layer_scale_bwd_ws_floats(M, C)
    dbuf, db = _guarded(M * C, ops.BF16)
    ggbuf, gg = _guarded(C)
    wsbuf, ws = _guarded(nws)
    gg.copy_(gg0)
    _lib.call("octmae_layer_scale_bwd", doutd.data_ptr(), brd.data_ptr(), gmd.data_ptr(), db.data_ptr(), gg.data_ptr(), ws.data_ptr(), M, C, st)
    assert _guards_intact(dbuf, M * C) and _guards_intact(ggbuf, C) and _guards_intact(wsbuf, nws)
    assert torch.equal(gg.cpu().double(), want), f"layer_scale_bwd M{M} C{C}: the exact gamma gradient differs by {(gg.cpu().double() - want).tolist()}"
    assert torch.equal(db.cpu().view(M, C), (gamma * dout).to(ops.BF16))
    # the workspace holds the G partials: each is its workgroup's exact share
    part = ws.cpu().double().view(nws // C, C)
    assert torch.equal(part.sum(0), want - gg0.double())
    if report is not None:
        report[f"M{M} C{C} exact"] = 0.0


def run_all_checks():
    rep = {}
    for H, W in HW:
        check_dwconv(H, W, rep)
    for shape in R.DW_TRIP_SHAPES:
        check_dwconv_trips(shape, rep)
    check_layer_scale(rep)
    check_layer_scale_trips(rep)
    check_argument_checks()
    return rep


@pytest.mark.parametrize("hw", HW, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_dwconv7_forward_and_gradients_per_element(hw):
    rep = {}
    check_dwconv(hw[0], hw[1], rep)
    print({k: tuple(round(v, 4) for v in r) for k, r in rep.items()})


@pytest.mark.parametrize("shape", R.DW_TRIP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv7_weight_gradient_past_the_workgroup_cap(shape):
    rep = {}
    check_dwconv_trips(shape, rep)
    print({k: tuple(round(v, 4) for v in r) for k, r in rep.items()})


def test_layer_scale_forward_and_backward():
    rep = {}
    check_layer_scale(rep)
    print({k: round(v, 4) for k, v in rep.items()})


def test_layer_scale_backward_past_the_workgroup_cap_with_folded_row_parts():
    rep = {}
    check_layer_scale_trips(rep)
    print({k: round(v, 4) for k, v in rep.items()})


def test_argument_checks_return_without_launching():
    check_argument_checks()


def half_build_cases():
    """What tests/f16_worker.py runs on the half-operand build; a failed check ends it with a traceback and a non-zero status."""
    return {"cases": len(run_all_checks())}


def test_same_checks_on_the_half_operand_build():
    children.spawn_f16_worker("slivit_f16", "tests.test_gpu_slivit_kernels:half_build_cases")
    meta = children.f16_worker_result("slivit_f16")
    assert meta["lib"] == "liboctmae_f16.so" and meta["lp_is_f16"] is True and meta["cases"] > 0
