"""CPU: the rules and helpers of tests/nonfinite.py are right -- every rule equals the NaN set of the same operation evaluated in float64
with plain torch ops (and autograd where the operation is a gradient) on the planted input; check() fails on a dropped NaN, on a
leaked NaN and on one flipped low bit outside the mask, and passes the untampered result; embed() gives the view it says."""
import pytest
import torch

from tests import nonfinite as NF

NAN = NF.NAN


def _holds(tag, ref_bad, rule):
    """the float64 NaN set equals the rule, tensor by tensor"""
    for name, m in rule.items():
        got = torch.isnan(ref_bad[name])
        assert got.shape == m.shape, (tag, name, got.shape, m.shape)
        assert torch.equal(got, m), f"{tag}/{name}: float64 has {int(got.sum())} NaN, the rule {int(m.sum())}; first difference at " \
                                    f"{NF._first(got != m)}"


# ------------------------------------------------------------------------------------------------------------------ GEMM
M_, N_, K_ = 37, 24, 16


def _gemm_inputs():
    return {"x": NF.draw((M_, K_), 1), "w": NF.draw((N_, K_), 2, 0.25), "bias": NF.draw((N_,), 3), "res": NF.draw((M_, N_), 4),
            "dy": NF.draw((M_, N_), 5), "pre": NF.draw((M_, K_), 6), "rowscale": torch.tensor([1.25, 2.0, 0.5] * 12 + [1.25])}


@pytest.mark.parametrize("what,idx", [("x", (0, 3)), ("x", (M_ - 1, K_ - 1)), ("w", (5, 0)), ("w", (N_ - 1, K_ - 1)), ("bias", (7,)),
                                      ("res", (3, 4)), ("rowscale", (2,))])
def test_forward_rule_is_float64s(what, idx):
    t = _gemm_inputs()
    t[what] = NF.plant(t[what], idx, NAN)
    rule = NF.rule_linear_fwd(M_, N_, what, idx)
    if what not in ("rowscale", "res"):
        _holds("plain", NF.ref_linear_fwd(t["x"], t["w"], t["bias"]), {"out": rule})
        _holds("gelu", NF.ref_linear_fwd(t["x"], t["w"], t["bias"], gelu=True), {"pre": rule, "act": rule})
    if what != "rowscale":
        _holds("resid", NF.ref_linear_fwd(t["x"], t["w"], t["bias"], res=t["res"]), {"out": rule})
    _holds("rowscale", NF.ref_linear_fwd(t["x"], t["w"], t["bias"], res=t["res"], rowscale=t["rowscale"]), {"out": rule})
    if what == "rowscale":                                        # one scale for all 37 rows
        _holds("one group", NF.ref_linear_fwd(t["x"], t["w"], t["bias"], res=t["res"], rowscale=torch.tensor([NAN]), rows_per_scale=M_),
               {"out": NF.rule_linear_fwd(M_, N_, "rowscale", (0,), M_)})


@pytest.mark.parametrize("what,idx", [("dy", (0, 3)), ("dy", (M_ - 1, N_ - 1)), ("w", (5, 2)), ("w", (N_ - 1, K_ - 1)), ("pre", (3, 4))])
def test_dgrad_rule_is_float64s(what, idx):
    t = _gemm_inputs()
    t[what] = NF.plant(t[what], idx, NAN)
    rule = NF.rule_linear_dgrad(M_, K_, what, idx)
    _holds("gelu'", NF.ref_linear_dgrad(t["dy"], t["w"], t["pre"]), rule)
    if what != "pre":
        _holds("plain", NF.ref_linear_dgrad(t["dy"], t["w"]), rule)
        # the same through autograd: dx is the gradient of sum(dy * (x w^T)) with respect to x
        x = t["x"].double().requires_grad_(True)
        ((x @ t["w"].double().t()) * t["dy"].double()).sum().backward()
        assert torch.equal(torch.isnan(x.grad), rule["dx"])


@pytest.mark.parametrize("what,idx", [("o", (3, 9)), ("dy", (M_ - 1, 0)), ("w", (2, 15))])
def test_delta_rule_is_float64s(what, idx):
    t = _gemm_inputs()
    t["o"] = NF.draw((M_, K_), 8)
    t[what] = NF.plant(t[what], idx, NAN)
    _holds("delta", NF.ref_dgrad_delta(t["dy"], t["w"], t["o"], 2, 8), NF.rule_dgrad_delta(M_, K_, 2, 8, what, idx))


@pytest.mark.parametrize("what,idx", [("dy", (0, 3)), ("dy", (M_ - 1, N_ - 1)), ("x", (4, 0)), ("x", (M_ - 1, K_ - 1))])
def test_wgrad_rule_is_float64s(what, idx):
    t = _gemm_inputs()
    t[what] = NF.plant(t[what], idx, NAN)
    _holds("wgrad", NF.ref_wgrad(t["dy"], t["x"], NF.draw((N_, K_), 9), NF.draw((N_,), 10)), NF.rule_wgrad(N_, K_, what, idx))


# ------------------------------------------------------------------------------------------------------------------ attention
B_, H_, L_, HD_ = 2, 3, 9, 4


def _attn_inputs():
    qkv = NF.draw((B_ * L_, 3 * H_ * HD_), 11)
    do = NF.draw((B_ * L_, H_ * HD_), 12)
    f = NF.ref_attn_fwd(qkv, B_, L_, H_, HD_)
    return qkv, do, f["o"].reshape(B_ * L_, H_ * HD_), f["lse"]


def test_attention_backward_formula_is_autograds():
    """ref_attn_bwd (from the saved o and lse, as the kernels are handed them) against autograd through the float64 forward"""
    qkv, do, o, lse = _attn_inputs()
    qd = qkv.double().requires_grad_(True)
    NF.ref_attn_fwd(qd, B_, L_, H_, HD_)["o"].backward(do.double().view(B_, L_, H_, HD_))
    got = NF.ref_attn_bwd(qkv, o, do, lse, B_, L_, H_, HD_)
    assert torch.allclose(got.reshape(qd.grad.shape), qd.grad, rtol=1e-10, atol=1e-12)
    delta = -(do.double() * o).view(B_ * L_, H_, HD_).sum(-1)
    assert torch.allclose(NF.ref_attn_bwd(qkv, None, do, lse, B_, L_, H_, HD_, delta=delta), got, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("what", ["q", "k", "v"])
@pytest.mark.parametrize("idx", [(0, 0, 1, 0), (0, L_ - 1, 1, HD_ - 1), (1, 0, 0, 2)])
def test_attention_forward_rule_is_float64s(what, idx):
    qkv, _, _, _ = _attn_inputs()
    b, n, h, d = idx
    bad = NF.plant(qkv.view(B_, L_, 3, H_, HD_), (b, n, "qkv".index(what), h, d), NAN).view_as(qkv)
    _holds(what, NF.ref_attn_fwd(bad, B_, L_, H_, HD_), NF.rule_attn_fwd(B_, H_, L_, HD_, what, idx))


def test_attention_forward_wave_rows_hold_the_planted_row_and_its_wave_only():
    w = NF.attn_fwd_wave_rows(2, 3, 70, 4, (1, 37, 2, 0))
    assert int(w["lse"].sum()) == 32 and bool(w["lse"][1, 2, 32:64].all()) and int(w["o"].sum()) == 32 * 4 and bool(w["o"][1, 32:64, 2].all())
    w = NF.attn_fwd_wave_rows(2, 3, 70, 4, (0, 69, 0, 0))
    assert int(w["lse"].sum()) == 6 and bool(w["lse"][0, 0, 64:].all())


@pytest.mark.parametrize("what,idx", [("dO", (0, 0, 1, 0)), ("dO", (1, L_ - 1, 0, HD_ - 1)), ("o", (0, 3, 1, 2)), ("o", (1, 0, 0, 0)),
                                      ("lse", (0, 1, L_ - 1)), ("lse", (1, 0, 0)), ("delta", (0 * L_ + 4, 1)), ("delta", (1 * L_, 0))])
def test_attention_backward_rule_is_float64s(what, idx):
    qkv, do, o, lse = _attn_inputs()
    delta = None
    if what == "dO":
        do = NF.plant(do.view(B_, L_, H_, HD_), idx, NAN).view_as(do)
    elif what == "o":
        o = NF.plant(o.view(B_, L_, H_, HD_), idx, NAN).view_as(o)
    elif what == "lse":
        lse = NF.plant(lse, idx, NAN)
    else:
        delta = NF.plant(-(do.double() * o).view(B_ * L_, H_, HD_).sum(-1), idx, NAN)
    got = NF.ref_attn_bwd(qkv, o, do, lse, B_, L_, H_, HD_, delta=delta)
    _holds(what, {"dqkv": got}, {"dqkv": NF.rule_attn_bwd(B_, H_, L_, HD_, what, idx)})


def test_attention_backward_dO_rule_through_autograd():
    """the dO rule once more, without the restated formula: autograd of the float64 forward with a NaN in the upstream gradient"""
    qkv, do, _, _ = _attn_inputs()
    idx = (0, 2, 1, 3)
    qd = qkv.double().requires_grad_(True)
    NF.ref_attn_fwd(qd, B_, L_, H_, HD_)["o"].backward(NF.plant(do.double().view(B_, L_, H_, HD_), idx, NAN))
    assert torch.equal(torch.isnan(qd.grad).view(B_, L_, 3, H_, HD_), NF.rule_attn_bwd(B_, H_, L_, HD_, "dO", idx))


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
R_, D_ = 7, 16
EPS = 1e-6


def _ln_inputs():
    return {"x": NF.draw((R_, D_), 21), "gamma": NF.draw((D_,), 22), "beta": NF.draw((D_,), 23), "dy": NF.draw((R_, D_), 24),
            "dres": NF.draw((R_, D_), 25)}


@pytest.mark.parametrize("what,idx", [("x", (0, 0)), ("x", (R_ - 1, D_ - 1)), ("gamma", (0,)), ("beta", (D_ - 1,))])
def test_layernorm_forward_rule_is_float64s(what, idx):
    t = _ln_inputs()
    t[what] = NF.plant(t[what], idx, NAN)
    _holds(what, NF.ref_ln_fwd(t["x"], t["gamma"], t["beta"], EPS), NF.rule_ln_fwd(R_, D_, what, idx))
    y, mean, rstd = torch.native_layer_norm(t["x"].double(), (D_,), t["gamma"].double(), t["beta"].double(), EPS)
    _holds(what + "/native", {"y": y, "mean": mean.flatten(), "rstd": rstd.flatten()}, NF.rule_ln_fwd(R_, D_, what, idx))


@pytest.mark.parametrize("what,idx", [("x", (2, 5)), ("mean", (0,)), ("rstd", (R_ - 1,)), ("gamma", (3,)), ("beta", (0,))])
def test_ln_apply_rule_is_float64s(what, idx):
    t = _ln_inputs()
    f = NF.ref_ln_fwd(t["x"], t["gamma"], t["beta"], EPS)
    t.update(mean=f["mean"], rstd=f["rstd"])
    t[what] = NF.plant(t[what], idx, NAN)
    _holds(what, NF.ref_ln_apply(t["x"], t["mean"], t["rstd"], t["gamma"], t["beta"]), NF.rule_ln_apply(R_, D_, what, idx))


@pytest.mark.parametrize("what,idx", [("x", (0, 0)), ("x", (R_ - 1, D_ - 1)), ("dy", (0, D_ - 1)), ("dy", (R_ - 1, 0)), ("gamma", (5,)),
                                      ("dres", (3, 4))])
def test_layernorm_backward_rule_is_float64s(what, idx):
    t = _ln_inputs()
    t[what] = NF.plant(t[what], idx, NAN)
    f = NF.ref_ln_fwd(t["x"], t["gamma"], t["beta"], EPS)           # the statistics of the planted x, as the forward kernel saves them
    rule = NF.rule_ln_bwd(R_, D_, what, idx)
    _holds(what, NF.ref_ln_bwd(t["dy"], t["x"], f["mean"], f["rstd"], t["gamma"], t["dres"]), rule)
    # and autograd of torch's own float64 layer_norm
    xd, gd, bd = (t[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
    torch.native_layer_norm(xd, (D_,), gd, bd, EPS)[0].backward(t["dy"].double())
    dx = xd.grad + t["dres"].double()
    _holds(what + "/autograd", {"dx": dx, "dgamma": gd.grad, "dbeta": bd.grad, "dxsum": dx.sum(0)}, rule)


@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("what,idx", [("x", (0, 0, 0)), ("x", (5, 1, 7)), ("x", (3, 4, 15)), ("gamma", (2,)), ("beta", (15,)),
                                      ("dout", (1, 3))])
def test_slice_pool_rules_are_float64s(what, idx, cls):
    Bv, S, T = 2, 3, 5
    t = {"x": NF.draw((Bv * S, T, D_), 31), "gamma": NF.draw((D_,), 32), "beta": NF.draw((D_,), 33), "dout": NF.draw((Bv, D_), 34)}
    t[what] = NF.plant(t[what], idx, NAN)
    ref = NF.ref_slice_pool(t["x"], t["gamma"], t["beta"], t["dout"], S, cls, EPS)
    if what != "dout":
        _holds(what + "/fwd", ref, NF.rule_slice_pool_fwd(Bv, S, T, D_, cls, what, idx))
    if what != "beta":
        _holds(what + "/bwd", ref, NF.rule_slice_pool_bwd(Bv, S, T, D_, cls, what, idx))
    assert bool((ref["dx"][:, ~NF._pool_used(T, cls)] == 0).all())      # the tokens the pooling skips: exact zeros


# ------------------------------------------------------------------------------------------------------------------ optimizer
@pytest.mark.parametrize("value", [NAN, NF.INF, -NF.INF])
def test_optimizer_rule_is_float64s(value):
    lengths = [5, 11]
    g = [NF.draw((n,), 40 + n) for n in lengths]
    p = [NF.draw((n,), 50 + n) for n in lengths]
    m = [NF.draw((n,), 60 + n, 0.1) for n in lengths]
    v = [NF.draw((n,), 70 + n, 0.1).abs() for n in lengths]
    g[1] = NF.plant(g[1], (4,), value)
    rule = NF.rule_optim(lengths, 1, 4)
    sumsq = torch.stack([(t.double() ** 2).sum() for t in g])
    assert torch.equal(~torch.isfinite(sumsq), rule["sumsq"])
    norm = sumsq.sum().sqrt()
    coef = torch.minimum(1.0 / (norm + 1e-6), torch.ones(()).double()) if norm == norm else norm      # min() as the kernel's `if (c > 1) c = 1`
    assert not bool(torch.isfinite(norm)) and (bool(torch.isnan(coef)) if value != value else float(coef) == 0.0)
    for t in range(2):
        out = NF.ref_adamw(p[t], g[t], m[t], v[t], 0.5, 1e-3, 0.9, 0.95, 1e-8, 0.05, 3)
        for k in ("p", "m", "v"):
            assert torch.equal(~torch.isfinite(out[k]), rule["elements"][t]), (t, k)
    out = NF.ref_adamw(p[0], g[0], m[0], v[0], NAN, 1e-3, 0.9, 0.95, 1e-8, 0.05, 3)       # a NaN in *gscale: everything
    assert all(bool(torch.isnan(out[k]).all()) for k in ("p", "m", "v"))


# ------------------------------------------------------------------------------------------------------------------ tokens and loss
def _perm_prefix(B, L, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(L, generator=g)[:n] for _ in range(B)]).contiguous()


def _restore(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.argsort(torch.argsort(torch.rand(B, L, generator=g), dim=1), dim=1).contiguous()


def test_enc_assemble_rule_is_float64s():
    B, nkeep, D, L = 3, 4, 8, 20
    ids = _perm_prefix(B, L, nkeep, 1)
    c = {"tok": NF.draw((B * nkeep, D), 1), "pos": NF.draw((L, D), 2), "cls": NF.draw((D,), 3), "pos_cls": NF.draw((D,), 4)}
    unused = next(l for l in range(L) if l not in ids.flatten().tolist())
    for what, idx in [("tok", (0, 3)), ("tok", (B * nkeep - 1, 0)), ("pos", (int(ids[1, 2]), 5)), ("pos", (unused, 1)), ("cls", (2,)), ("pos_cls", (7,))]:
        t = dict(c)
        t[what] = NF.plant(c[what], idx, NAN)
        rule = NF.rule_enc_assemble(B, nkeep, D, ids, what, idx)
        _holds(what, {"x": NF.ref_enc_assemble(t["tok"], t["pos"], t["cls"], t["pos_cls"], ids)}, {"x": rule})
        assert (what, idx) != ("pos", (unused, 1)) or not bool(rule.any())


@pytest.mark.parametrize("emb_has_cls", [0, 1])
def test_dec_assemble_rule_is_float64s(emb_has_cls):
    B, nkeep, L, D = 3, 4, 11, 8
    ids = _restore(B, L, 2)
    erows = nkeep + emb_has_cls
    c = {"emb": NF.draw((B * erows, D), 1), "mask_token": NF.draw((D,), 2), "dpos": NF.draw((L, D), 3), "dcls": NF.draw((D,), 4),
         "dpos_cls": NF.draw((D,), 5)}
    plants = [("emb", (0, 0)), ("emb", (emb_has_cls, 2)), ("emb", (B * erows - 1, D - 1)), ("mask_token", (3,)), ("dpos", (0, 0)), ("dpos", (L - 1, 7)),
              ("dpos_cls", (1,))] + ([] if emb_has_cls else [("dcls", (6,))])
    for what, idx in plants:
        t = dict(c)
        t[what] = NF.plant(c[what], idx, NAN)
        got = NF.ref_dec_assemble(t["emb"], t["mask_token"], t["dpos"], t["dcls"], t["dpos_cls"], ids, nkeep, emb_has_cls)
        _holds(what, {"x": got}, {"x": NF.rule_dec_assemble(B, nkeep, L, D, ids, emb_has_cls, what, idx)})


def test_gather_rules_are_float64s():
    B, C, T, H, W, tp, p, nkeep = 2, 3, 4, 8, 8, 2, 4, 3
    Lt = (T // tp) * (H // p) * (W // p)
    ids = _perm_prefix(B, Lt, nkeep, 3)
    imgs = NF.draw((B, C, T, H, W), 1)
    gh, gw = H // p, W // p

    def voxel(b, l, c, u, py, px):
        return (b, c, (l // (gh * gw)) * tp + u, ((l // gw) % gh) * p + py, (l % gw) * p + px)
    dropped = next(l for l in range(Lt) if l not in ids[1].tolist())
    for idx, hits in [(voxel(0, int(ids[0, 0]), 0, 0, 0, 0), 1), (voxel(1, int(ids[1, nkeep - 1]), C - 1, tp - 1, p - 1, p - 1), 1),
                      (voxel(0, int(ids[0, 1]), 1, 1, 2, 1), 1), (voxel(1, dropped, 1, 0, 3, 2), 0)]:
        rule = NF.rule_patch_gather(B, C, T, H, W, tp, p, nkeep, ids, idx)
        _holds(f"patch_gather{idx}", {"out": NF.ref_patch_gather(NF.plant(imgs, idx, NAN), ids, tp, p)}, {"out": rule})
        assert int(rule.sum()) == hits                       # a voxel of a kept token: one element; of a dropped token: nothing
    Bn, n, rows, D = 2, 3, 6, 8
    src = NF.draw((Bn, rows, D), 2)
    for ids2 in (None, _perm_prefix(Bn, rows - 1, n, 4)):
        for idx in [(0, 0, 3), (0, 1, 0), (1, 5, 7), (1, 2, 2)]:
            _holds(f"gather_rows{idx}", {"out": NF.ref_gather_rows(NF.plant(src, idx, NAN), ids2, n)},
                   {"out": NF.rule_gather_rows(Bn, n, D, ids2, idx)})


def test_assembly_backward_rules_are_float64s():
    B, L, nkeep, D = 3, 11, 4, 8
    ids = _restore(B, L, 5)
    src, prior, dx = NF.draw((B, 1 + nkeep, D), 1), NF.draw((L, D), 2), NF.draw((B, 1 + L, D), 3)
    for idx in [(0, 1, 0), (2, nkeep, D - 1), (1, 0, 5)]:
        for pr in (None, prior):
            _holds(f"scatter{idx}", {"out": NF.ref_scatter_add_rows(NF.plant(src, idx, NAN), ids, nkeep, pr)},
                   {"out": NF.rule_scatter_add_rows(B, nkeep, L, D, ids, idx)})
    l_masked, l_kept = int((ids[0] >= nkeep).nonzero()[0]), int((ids[2] < nkeep).nonzero()[-1])
    for idx in [(0, 1 + l_masked, 0), (2, 1 + l_kept, D - 1), (1, 0, 4)]:
        rule = NF.rule_dec_assemble_bwd(B, nkeep, L, D, ids, idx)
        _holds(f"dec_assemble_bwd{idx}", NF.ref_dec_assemble_bwd(NF.plant(dx, idx, NAN), ids, nkeep), rule)
    assert bool(NF.rule_dec_assemble_bwd(B, nkeep, L, D, ids, (0, 1 + l_masked, 0))["part"].any())
    assert not bool(NF.rule_dec_assemble_bwd(B, nkeep, L, D, ids, (2, 1 + l_kept, 0))["part"].any())


@pytest.mark.parametrize("norm_pix", [False, True])
def test_mse_rules_are_float64s_for_kept_and_masked_rows(norm_pix):
    """The backward through autograd of oracle/mae3d_ref.py::forward_loss, whose loss is (loss_tok * mask).sum() / mask.sum(): a NaN in
    a row the mask removes makes the loss NaN (0 * NaN) and reaches that row's gradient exactly as in a kept row -- the rule does not
    look at the mask.  The per-token losses and the stated formula coef * mask * (pred - target) give the same sets."""
    from oracle import mae3d_ref as O
    B, C, T, S, tp, p = 2, 1, 6, 8, 3, 4
    cfg = O.MAEConfig(input_size=S, patch_size=p, in_chans=C, num_frames=T, t_patch_size=tp, pred_t_dim=T, high_res_input_size=2 * S,
                      norm_pix_loss=norm_pix)
    u, L, PD = cfg.t_pred_patch_size, cfg.num_patches, cfg.patch_dim
    pred, imgs = NF.draw((B, L + 1, PD), 1), NF.draw((B, C, T, S, S), 2) / 6 + 0.5
    mask = (torch.arange(B * L).view(B, L) % 3 != 1).double()
    l_kept, l_gone = 0, 1
    assert float(mask[0, l_kept]) == 1 and float(mask[0, l_gone]) == 0
    plants = [("pred", (0, 1 + l_kept, 0)), ("pred", (0, 1 + l_gone, 5)), ("pred", (1, L, PD - 1)), ("pred", (1, 0, 3)),
              ("imgs", (0, 0, 0, 0, 0)), ("imgs", (0, 0, 1, 2, p + 1)), ("imgs", (1, 0, T - 1, S - 1, S - 1))]
    for what, idx in plants:
        t = {"pred": pred, "imgs": imgs}
        t[what] = NF.plant(t[what], idx, NAN)
        rule = NF.rule_mse(B, C, T, S, S, u, p, norm_pix, what, idx)
        _holds(f"{what}{idx}", NF.ref_mse(t["pred"], t["imgs"], mask, 2.0 / PD, cfg), rule)
        pr = t["pred"][:, 1:].double().requires_grad_(True)
        loss, _ = O.forward_loss(t["imgs"].double(), pr, mask, cfg)
        loss.backward()
        reached = bool(rule["loss_tok"].any())
        assert bool(torch.isnan(loss)) == reached                # kept or not: the masked loss is NaN once a token's loss is
        grad = torch.cat([torch.zeros(B, 1, PD, dtype=torch.float64), pr.grad], 1).view(-1, PD)
        _holds(f"{what}{idx}/autograd", {"dpred": grad}, {"dpred": rule["dpred"]})
    masked = NF.rule_mse(B, C, T, S, S, u, p, norm_pix, "pred", (0, 1 + l_gone, 5))
    assert bool(masked["loss_tok"][0, l_gone]) and bool(masked["dpred"][1 + l_gone, 5])


def test_wave_rows_constant_is_the_forward_kernels():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "octcubem_amd", "csrc", "attn.hip")).read()
    assert NF.ATTN_FWD_WAVE_ROWS_SOURCE in src and NF.ATTN_FWD_WAVE_ROWS_SOURCE.endswith(f"wid * {NF.ATTN_FWD_WAVE_ROWS};")
    assert "wave-uniform" in src and "!__all(ex <= RESCALE_SLACK)" in src


# ------------------------------------------------------------------------------------------------------------------ check()
def _clean_and_planted():
    t = _gemm_inputs()
    clean = NF.ref_linear_fwd(t["x"], t["w"], t["bias"])["out"]
    idx = (4, 2)
    bad = NF.ref_linear_fwd(NF.plant(t["x"], idx, NAN), t["w"], t["bias"])["out"]
    return clean, bad, NF.rule_linear_fwd(M_, N_, "x", idx)


def test_check_passes_the_untampered_result():
    clean, bad, rule = _clean_and_planted()
    NF.check("ok", clean, bad, rule)
    NF.check("ok", clean, bad, rule, nonfinite=True)
    NF.check_weak("ok", clean, bad, rule, True)
    NF.check("ok", clean, clean.clone(), torch.zeros_like(rule))


def test_check_fails_on_a_dropped_nan():
    clean, bad, rule = _clean_and_planted()
    bad = NF.plant(bad, (4, 7), 1.0)
    with pytest.raises(AssertionError, match=r"dropped.*\(4, 7\)"):
        NF.check("dropped", clean, bad, rule)
    with pytest.raises(AssertionError, match="the kernel has none"):
        NF.check_weak("dropped", clean, torch.where(rule, clean, bad), rule, True)


def test_check_fails_on_a_leaked_nan():
    clean, bad, rule = _clean_and_planted()
    bad = NF.plant(bad, (5, 7), NAN)
    with pytest.raises(AssertionError, match=r"leaked.*\(5, 7\)"):
        NF.check("leaked", clean, bad, rule)
    with pytest.raises(AssertionError, match=r"\(5, 7\)"):
        NF.check_weak("leaked", clean, bad, rule, True)
    with pytest.raises(AssertionError, match=r"leaked.*\(5, 7\)"):          # an Inf counts where the rule says "non-finite"
        NF.check("leaked", clean, NF.plant(bad, (5, 7), NF.INF), rule, nonfinite=True)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16, torch.float16])
def test_check_fails_on_one_flipped_low_bit_outside_the_mask(dtype):
    clean, bad, rule = _clean_and_planted()
    clean, bad = clean.to(dtype), bad.to(dtype)
    NF.check("ok", clean, bad, rule)
    flipped = NF._bits(bad).clone()
    flipped[6, 1] ^= 1
    with pytest.raises(AssertionError, match=r"\(6, 1\).*differs"):
        NF.check("bit", clean, flipped.view(dtype), rule)
    with pytest.raises(AssertionError, match=r"\(6, 1\).*differs"):
        NF.check_weak("bit", clean, flipped.view(dtype), rule, True)
    loose = torch.zeros_like(rule)
    loose[6] = True                                 # a documented choice lets row 6 differ in bits: the flip passes, a NaN there does not
    NF.check("loose", clean, flipped.view(dtype), rule, loose=loose)
    NF.check_weak("loose", clean, flipped.view(dtype), rule, True, loose=loose)
    with pytest.raises(AssertionError, match=r"leaked.*\(6, 1\)"):
        NF.check("loose", clean, NF.plant(bad, (6, 1), NAN), rule, loose=loose)
    inside = NF._bits(bad).clone()                  # the same flip inside the mask changes a NaN's payload: not a fault
    inside[4, 1] ^= 1
    NF.check("payload", clean, inside.view(dtype), rule)
    zero = NF.plant(clean, (6, 1), 0.0)             # -0 against +0 counts
    with pytest.raises(AssertionError, match=r"\(6, 1\)"):
        NF.check("zero", zero, torch.where(rule, bad, NF.plant(zero, (6, 1), -0.0)), rule)


# ------------------------------------------------------------------------------------------------------------------ embed()
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_embed_two_dimensional_form(dtype):
    x = NF.draw((7, 24), 81).to(dtype)
    v = NF.embed(x, pad_rows=3, pad_cols=16)
    assert torch.equal(v, x) and v.shape == x.shape and v.stride() == (40, 1) and not v.is_contiguous()
    buf = v._base
    assert buf.shape == (13, 40) and v.data_ptr() % 16 == 0 and v.data_ptr() == buf.data_ptr() + 3 * 40 * x.element_size()
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[3:10, :24] = False
    assert bool(torch.isnan(buf[outside]).all()) and int(outside.sum()) == 13 * 40 - 7 * 24
    x[0, 0] = 99.0
    assert float(v[0, 0]) != 99.0                              # a copy, not an alias of the input
    assert bool((NF.embed(x, 2, 8, fill=5.0)._base[0] == 5.0).all())
    with pytest.raises(AssertionError):
        NF.embed(x, 3, 4)                                      # pad_cols is a multiple of 8 elements


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 3, 31), (10, 24), (5,)])
def test_embed_flat_form(shape, dtype):
    x = NF.draw(shape, 82).to(dtype)
    v = NF.embed(x, pad_rows=2, flat=True)
    assert torch.equal(v, x) and v.is_contiguous() and v.shape == x.shape and v.data_ptr() % 16 == 0
    buf = v._base
    pad = (buf.numel() - x.numel()) // 2
    assert pad >= 2 * shape[-1] and pad % 64 == 0 and v.data_ptr() == buf.data_ptr() + pad * x.element_size()
    assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + x.numel():]).all())
    assert torch.equal(buf[pad:pad + x.numel()], x.flatten())


def test_plant_replaces_one_element_of_a_copy():
    x = NF.draw((4, 8), 83)
    y = NF.plant(x, (2, 3), NAN)
    assert bool(torch.isnan(y[2, 3])) and int(torch.isnan(y).sum()) == 1 and not bool(torch.isnan(x).any())
    assert torch.equal(NF._bits(torch.where(torch.isnan(y), x, y)), NF._bits(x))
