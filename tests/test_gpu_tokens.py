"""The token-assembly and loss kernels of csrc/tokens.hip, each called directly through the C ABI -- `pytest -m gpu` on an MI355X.

These kernels move rows by index: one wrong row is invisible in a model-level comparison, so every output here is compared
element by element (bit for bit where the kernel does one widening and one fp32 add) with plain torch indexing, and sits
between guard rows that must come back untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import ops
    from octcubem_amd._lib import call
from oracle import mae3d_ref as O

DEV = "cuda"
BF16 = ops.BF16 if torch.cuda.is_available() else torch.bfloat16   # the library's 16-bit operand type (OCTMAE_LIB)
GUARD = 3          # rows before and after every output
SENTINEL = 7.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """An output of `rows` x `width` elements between GUARD rows of SENTINEL on either side."""

    def __init__(self, rows, width, dtype):
        self.big = torch.full((rows + 2 * GUARD, width), SENTINEL, dtype=dtype, device=DEV)
        self.out = self.big[GUARD:GUARD + rows]

    def ptr(self):
        return self.out.data_ptr()

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.big[:GUARD] == SENTINEL).all()) and bool((self.big[-GUARD:] == SENTINEL).all())


def _perm_prefix(B, L, n, g, dtype=torch.int64):
    """[B, n]: the first n entries of a random permutation of L per sample -- every row has a distinct source."""
    return torch.stack([torch.randperm(L, generator=g)[:n] for _ in range(B)]).to(dtype).contiguous()


# ------------------------------------------------------------------------------------------------ encoder assembly
# The grid of the four walks below is capped at 8192 workgroups of 256 threads (2 097 152 items) and a thread strides on from there: the
# last shape of each list is the narrowest row (8 or 64 elements) with 259 to 448 items past the cap -- a second trip for one whole
# workgroup and a part of the next (docs/GRID_CAPS.md).
GRID_CAP_ITEMS = 8192 * 256


@pytest.mark.parametrize("B,nkeep,D", [(2, 1280, 1024), (3, 10, 64), (128, 80, 512), (1, 1, 4), (2, 524352, 8)])
def test_enc_assemble_equals_cat_and_gather(B, nkeep, D):
    """octmae_enc_assemble: x[b, 0] = cls + pos_cls, x[b, 1 + i] = float(tok[b, i]) + pos[ids_keep[b, i]] -- one 16-bit -> fp32
    widening and one fp32 add: torch.equal."""
    g = torch.Generator().manual_seed(B + nkeep + D)
    L = 4 * nkeep if nkeep < 100000 else nkeep + 5
    assert nkeep < 100000 or 256 < B * (nkeep + 1) * (D // 4) - GRID_CAP_ITEMS < 512
    tok = torch.randn(B * nkeep, D, generator=g).to(BF16).to(DEV)
    pos = torch.randn(L, D, generator=g).to(DEV)
    cls = torch.randn(D, generator=g).to(DEV)
    pos_cls = torch.randn(D, generator=g).to(DEV)
    ids_keep = _perm_prefix(B, L, nkeep, g).to(DEV)
    x = Guarded(B * (nkeep + 1), D, torch.float32)
    call("octmae_enc_assemble", tok.data_ptr(), pos.data_ptr(), cls.data_ptr(), pos_cls.data_ptr(), ids_keep.data_ptr(), x.ptr(),
         B, nkeep, D, _stream())
    exp = torch.cat([(cls + pos_cls).expand(B, 1, D), tok.float().view(B, nkeep, D) + pos[ids_keep]], 1)
    assert x.intact()
    assert torch.equal(x.out.view(B, nkeep + 1, D), exp)


# ------------------------------------------------------------------------------------------------ decoder assembly
@pytest.mark.parametrize("emb_has_cls", [0, 1])
@pytest.mark.parametrize("B,nkeep,L,D", [(2, 1280, 5120, 512), (3, 10, 40, 64), (5, 17, 17, 128), (2, 49, 196, 512), (2, 131088, 524352, 8)])
def test_dec_assemble_equals_gather_mask_token_and_dpos(B, nkeep, L, D, emb_has_cls):
    """octmae_dec_assemble: x[b, 1 + j] = (emb[b, r] if r = ids_restore[b, j] < nkeep else mask_token) + dpos[j]; the cls row is
    dcls + dpos_cls or, with emb_has_cls = 1 (the 2-D MAE: emb carries 1 + nkeep rows per sample, dcls = NULL), emb[b, 0] + dpos_cls."""
    g = torch.Generator().manual_seed(B + nkeep + L + D)
    assert L < 100000 or 256 < B * (L + 1) * (D // 4) - GRID_CAP_ITEMS < 512
    erows = nkeep + emb_has_cls
    emb = torch.randn(B * erows, D, generator=g).to(BF16).to(DEV)           # every row distinct
    mask_token = torch.randn(D, generator=g).to(DEV)
    dpos = torch.randn(L, D, generator=g).to(DEV)
    dcls = torch.randn(D, generator=g).to(DEV)
    dpos_cls = torch.randn(D, generator=g).to(DEV)
    ids_restore = torch.argsort(torch.argsort(torch.rand(B, L, generator=g), dim=1), dim=1).contiguous().to(DEV)
    x = Guarded(B * (L + 1), D, torch.float32)
    call("octmae_dec_assemble", emb.data_ptr(), mask_token.data_ptr(), dpos.data_ptr(), None if emb_has_cls else dcls.data_ptr(),
         dpos_cls.data_ptr(), ids_restore.data_ptr(), x.ptr(), B, nkeep, L, D, emb_has_cls, _stream())
    e = emb.float().view(B, erows, D)
    seq = torch.cat([e[:, emb_has_cls:], mask_token.expand(B, L - nkeep, D)], 1)
    body = torch.gather(seq, 1, ids_restore.unsqueeze(-1).expand(-1, -1, D)) + dpos
    first = (e[:, 0] if emb_has_cls else dcls.expand(B, D)) + dpos_cls
    assert x.intact()
    assert torch.equal(x.out.view(B, L + 1, D), torch.cat([first.unsqueeze(1), body], 1))


# ------------------------------------------------------------------------------------------------ patch gather
@pytest.mark.parametrize("B,C,T,H,W,tp,p,nkeep", [(2, 3, 1, 224, 224, 1, 16, 49), (3, 3, 6, 64, 64, 3, 16, 8),
                                                  (1, 1, 60, 256, 256, 3, 16, 1280), (3, 1, 22, 512, 512, 1, 8, 87400)])
def test_patch_gather_int64_and_int32_ids(B, C, T, H, W, tp, p, nkeep):
    """octmae_patch_gather with ids: out[b * nkeep + i][(c, u, py, px)] = imgs[b][c][t tp + u][hy p + py][wx p + px] for token
    ids[b][i] -> (t, hy, wx), rounded to 16 bits.  int64 ids (ids_is_i64 = 1) and int32 ids (0) agree bit for bit with each other
    and with the permute-built expectation; C = 3 is the RGB 2-D MAE's order."""
    g = torch.Generator().manual_seed(C * T + H)
    assert nkeep < 80000 or 256 < B * nkeep * (C * tp * p * p // 8) - GRID_CAP_ITEMS < 512
    imgs = torch.rand(B, C, T, H, W, generator=g).to(DEV)
    gt, gh, gw = T // tp, H // p, W // p
    L = gt * gh * gw
    ids = _perm_prefix(B, L, nkeep, g).to(DEV)
    kdim = C * tp * p * p
    full = imgs.view(B, C, gt, tp, gh, p, gw, p).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, L, kdim)
    exp = torch.gather(full, 1, ids.unsqueeze(-1).expand(-1, -1, kdim)).reshape(B * nkeep, kdim).to(BF16)
    outs = []
    for is_i64, idt in ((1, ids), (0, ids.to(torch.int32).contiguous())):     # int32 ids: ids_is_i64 = 0
        out = Guarded(B * nkeep, kdim, BF16)
        call("octmae_patch_gather", imgs.data_ptr(), idt.data_ptr(), is_i64, out.ptr(), B, C, T, H, W, tp, p, nkeep, _stream())
        assert out.intact(), is_i64
        assert torch.equal(out.out, exp), is_i64
        outs.append(out.out)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ row gather + cast
@pytest.mark.parametrize("B,n,src_rows,D", [(2, 1280, 5121, 512), (3, 10, 11, 64), (2, 1280, 1281, 1024), (1, 1, 2, 8), (3, 699137, 699140, 8)])
def test_gather_rows_cast_identity_and_permutation(B, n, src_rows, D):
    """octmae_gather_rows_cast: out[b n + i] = 16-bit(src[b][1 + ids[b][i]]); ids = NULL is the identity (the encoder assembly's
    backward), ids a permutation prefix the decoder assembly's."""
    g = torch.Generator().manual_seed(B + n + D)
    assert n < 100000 or 256 < B * n * (D // 8) - GRID_CAP_ITEMS < 512
    src = torch.randn(B, src_rows, D, generator=g).to(DEV)
    ids = _perm_prefix(B, src_rows - 1, n, g).to(DEV)
    for use_ids in (None, ids):
        out = Guarded(B * n, D, BF16)
        call("octmae_gather_rows_cast", src.data_ptr(), None if use_ids is None else use_ids.data_ptr(), out.ptr(), B, n, src_rows, D,
             _stream())
        idx = torch.arange(n, device=DEV).expand(B, n) if use_ids is None else use_ids
        exp = torch.gather(src[:, 1:], 1, idx.unsqueeze(-1).expand(-1, -1, D)).to(BF16)
        assert out.intact(), use_ids is None
        assert torch.equal(out.out.view(B, n, D), exp), use_ids is None


# ------------------------------------------------------------------------------------------------ patchify + masked MSE
def _ulp(ref: torch.Tensor) -> torch.Tensor:
    """One unit in the last place of the library's 16-bit type at the magnitude of `ref` (float64)."""
    mant, emin = (7, -126) if BF16 == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -200))).clamp_min(emin)
    return torch.exp2(e - mant)


@pytest.mark.parametrize("select_frames", [False, True])
@pytest.mark.parametrize("norm_pix", [0, 1])
@pytest.mark.parametrize("B,C,T,S,tp", [(2, 1, 12, 32, 3), (2, 3, 12, 32, 3), (1, 1, 60, 256, 3), (1, 1, 195, 256, 3)])
def test_mse_fwd_bwd_per_token_and_per_element(B, C, T, S, tp, norm_pix, select_frames):
    """octmae_mse_fwd / octmae_mse_bwd against oracle/mae3d_ref.py::forward_loss in float64: C = 1 (16-byte image reads) and C = 3
    (the scalar gather of the RGB 2-D MAE), with and without norm_pix_loss, with frame_idx = NULL and with a strictly increasing
    non-identity int32 frame selection (pred_t_dim < T); the third shape is the ViT-L one (p = 16, u = 3, 256 x 256, T = 60); the last
    has 65 x 256 = 16 640 tokens against the 4096 workgroups x 4 waves of either launch: 256 (forward) or 257 (backward, with the cls
    row) rows are a wave's second."""
    p = 16
    pred_t = T * 2 // 3 if select_frames else T
    cfg = O.MAEConfig(input_size=S, in_chans=C, num_frames=T, t_patch_size=tp, pred_t_dim=pred_t, high_res_input_size=2 * S,
                      norm_pix_loss=bool(norm_pix))
    u, L, PD = cfg.t_pred_patch_size, cfg.num_patches, cfg.patch_dim
    g = torch.Generator().manual_seed(C + T + S + norm_pix)
    imgs = torch.rand(B, C, T, S, S, generator=g)
    pred_full = torch.randn(B, L + 1, PD, generator=g)
    mask = (torch.rand(B, L, generator=g) > 0.3).float()
    frame_idx = None
    if select_frames:
        fi = torch.linspace(0, T - 1, pred_t).long()
        assert bool((fi[1:] > fi[:-1]).all()) and not torch.equal(fi, torch.arange(pred_t))
        frame_idx = fi.to(torch.int32).to(DEV)
    fip = None if frame_idx is None else frame_idx.data_ptr()
    # float64 reference: forward_loss's own scalar and its autograd gradient; the per-token losses are forward_loss's formula
    # (:317-329) token by token, pinned to that scalar
    pr = pred_full[:, 1:].double().requires_grad_(True)
    loss_ref, _ = O.forward_loss(imgs.double(), pr, mask.double(), cfg)
    loss_ref.backward()
    sel = imgs.double() if frame_idx is None else torch.index_select(imgs.double(), 2, fi)
    target = O.patchify(sel, cfg)
    if norm_pix:
        target = (target - target.mean(-1, keepdim=True)) / (target.var(-1, keepdim=True) + 1.0e-6) ** 0.5
    tok_ref = ((pr.detach() - target) ** 2).mean(-1)
    assert abs(float((tok_ref * mask).sum() / mask.sum()) - float(loss_ref.detach())) <= 1e-12 * float(loss_ref.detach())

    pd, im, mk = pred_full.to(DEV), imgs.to(DEV), mask.to(DEV)
    loss_tok = Guarded(B, L, torch.float32)
    call("octmae_mse_fwd", pd.data_ptr(), im.data_ptr(), fip, loss_tok.ptr(), B, C, T, S, S, u, p, L, norm_pix, _stream())
    assert loss_tok.intact()
    got = loss_tok.out.double().cpu()
    worst = float(((got - tok_ref).abs() / tok_ref).max())
    print(f"mse_fwd C={C} T={T} S={S} norm_pix={norm_pix} frames={select_frames}: worst token {worst:.2e}")
    assert bool(((got - tok_ref).abs() <= 1e-5 * tok_ref).all()), worst

    # backward: dpred = coef * mask * (pred - target); coef = 2 / PD is what PatchMSEFn passes, so the reference is forward_loss's
    # gradient times mask.sum()
    coef = torch.full((1,), 2.0 / PD, dtype=torch.float32, device=DEV)
    dpred = Guarded(B * (L + 1), PD, BF16)
    call("octmae_mse_bwd", pd.data_ptr(), im.data_ptr(), fip, mk.data_ptr(), coef.data_ptr(), dpred.ptr(), B, C, T, S, S, u, p, L,
         norm_pix, _stream())
    assert dpred.intact()
    d = dpred.out.view(B, L + 1, PD)
    assert bool((d[:, 0] == 0).all())                                       # cls rows: exact zeros
    body = d[:, 1:]
    assert bool((body[mk == 0] == 0).all())                                 # rows with mask = 0: exact zeros
    ref = pr.grad * float(mask.sum())
    err = (body.double().cpu() - ref).abs()
    assert bool((err <= _ulp(ref)).all()), float((err / _ulp(ref)).max())
    if not norm_pix:
        t32 = O.patchify(im if frame_idx is None else torch.index_select(im, 2, fi.to(DEV)), cfg)
        exp = ((coef * mk).unsqueeze(-1) * (pd[:, 1:] - t32)).to(BF16)
        assert torch.equal(body, exp)


# ------------------------------------------------------------------------------------------------ backward of the assemblies, row by row
def test_assembly_backward_rows_past_the_grid_cap():
    """octmae_scatter_add_rows and octmae_dec_assemble_bwd give one workgroup per table row l up to 65 535 of them; with L = 65 539 the
    workgroups 0 .. 3 walk on to a second row and rebuild their LDS list (the keepers / the masked flags) for it.  B = 3: every output
    element is ((0 + v_0) + v_1) + v_2 over the samples that take part, ascending b -- the same fp32 additions in torch, bit for bit."""
    B, L, nkeep, D = 3, 65535 + 4, 16385, 4
    g = torch.Generator().manual_seed(L)
    ids_restore = torch.argsort(torch.argsort(torch.rand(B, L, generator=g), dim=1), dim=1).contiguous().to(DEV)
    kept = ids_restore < nkeep
    assert bool(kept[:, 65535:].any()) and bool((~kept[:, 65535:]).any())          # the second-trip rows have keepers and masked samples
    src = torch.randn(B, 1 + nkeep, D, generator=g).to(DEV)
    prior = torch.randn(L, D, generator=g).to(DEV)
    for accumulate in (0, 1):
        out = Guarded(L, D, torch.float32)
        if accumulate:
            out.out.copy_(prior)
        call("octmae_scatter_add_rows", src.data_ptr(), ids_restore.data_ptr(), out.ptr(), B, nkeep, L, D, 1 + nkeep, 1, accumulate, _stream())
        exp = prior.clone() if accumulate else torch.zeros(L, D, device=DEV)
        for b in range(B):
            rows = src[b, 1 + ids_restore[b].clamp(max=nkeep - 1)]
            exp = torch.where(kept[b].unsqueeze(1), exp + rows, exp)
        assert out.intact(), accumulate
        assert torch.equal(out.out, exp), (accumulate, int((out.out != exp).any(1).sum()))
    dx = torch.randn(B, 1 + L, D, generator=g).to(DEV)
    ddpos, part = Guarded(L, D, torch.float32), Guarded(L, D, torch.float32)
    call("octmae_dec_assemble_bwd", dx.data_ptr(), ids_restore.data_ptr(), ddpos.ptr(), part.ptr(), B, nkeep, L, D, _stream())
    e_all, e_msk = torch.zeros(L, D, device=DEV), torch.zeros(L, D, device=DEV)
    for b in range(B):
        e_all = e_all + dx[b, 1:]
        e_msk = torch.where(kept[b].unsqueeze(1), e_msk, e_msk + dx[b, 1:])
    assert ddpos.intact() and part.intact()
    assert torch.equal(ddpos.out, e_all) and torch.equal(part.out, e_msk)
