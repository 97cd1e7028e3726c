"""GPU tests of attention rollout: ops.rollout_step (csrc/rollout.hip) against the float64 reference of tests/rollout_ref.py within
its derived per-element bounds, bit-reproducibility, batch independence, padding and non-finite operands; ops.capture_attention and
saliency.attention_rollout on two small models against the published matrix product computed from the captured qkv."""
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import _lib, models_vit_flash_attn, models_vit_st, ops, saliency
from tests import rollout_ref as R

DEV = "cuda"
NORM = partial(torch.nn.LayerNorm, eps=1e-6)
SHAPE_IDS = ["x".join(map(str, s)) for s in R.SHAPES]


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@lru_cache(maxsize=None)
def problem(shape):
    """(q, k on the host, scale, the chain's score bits): computed once per shape and never written"""
    B, N, H, HD = shape
    q, k, scale = R.make_problem(B, N, H, HD, seed=5)
    return q, k, scale, R.chain_scores(q, k, B, N, H, HD)


@lru_cache(maxsize=None)
def step_refs(shape, fusion):
    _, _, scale, s = problem(shape)
    return tuple(R.StepRef(s[b], scale, fusion) for b in range(shape[0]))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(shape, fusion, r, q=None, k=None):
    B, N, H, HD = shape
    qh, kh, scale, _ = problem(shape)
    return ops.rollout_step(dev(qh) if q is None else q, dev(kh) if k is None else k, B, N, H, HD, float(scale), r, fusion)


@pytest.mark.parametrize("fusion", R.FUSIONS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_step_lies_inside_the_derived_bounds(shape, fusion):
    B, N, H, HD = shape
    refs = step_refs(shape, fusion)
    q, k = dev(problem(shape)[0]), dev(problem(shape)[1])
    for start in R.STARTS:
        r = R.make_start(start, B, N)
        got = run(shape, fusion, dev(r), q, k)
        again = run(shape, fusion, dev(r), q, k)
        assert got.shape == (B, N) and got.dtype == torch.float32
        assert same_bits(got, again), "two launches differ"
        for b in range(B):
            ref = refs[b].apply(r[b])
            w = R.worst(got[b], ref)
            print(shape, fusion, start, b, "worst |err| / bound =", w)
            assert w < 1.0, (start, b, w)
            mass = float(got[b].double().sum().cpu())
            assert abs(mass - float(r[b].astype(np.float64).sum())) <= float(ref[1].sum())      # the rows of Ahat sum to 1


@pytest.mark.parametrize("fusion", R.FUSIONS)
@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[0] > 1], ids=lambda s: "x".join(map(str, s)))
def test_a_sample_alone_gives_the_bits_it_gives_in_the_batch(shape, fusion):
    B, N, H, HD = shape
    qh, kh, scale, _ = problem(shape)
    r = R.make_start("random", B, N)
    whole = run(shape, fusion, dev(r))
    for b in range(B):
        rows = slice(b * N, (b + 1) * N)
        alone = ops.rollout_step(dev(qh[rows]), dev(kh[rows]), 1, N, H, HD, float(scale), dev(r[b:b + 1]), fusion)
        assert same_bits(alone[0], whole[b]), b


@pytest.mark.parametrize("fusion", R.FUSIONS)
@pytest.mark.parametrize("shape", [(2, 129, 2, 32), (1, 130, 1, 40), (1, 1, 1, 32)], ids=lambda s: "x".join(map(str, s)))
def test_padding_is_never_read_and_nothing_else_is_written(shape, fusion):
    """q and k as the two thirds of a packed [B N, 3 C + 5] buffer (the layout attention_rollout hands over, plus an odd tail), r_in and
    r_out in the middle of longer buffers: NaN everywhere else, the bits of the contiguous run, and the NaN still there afterwards"""
    B, N, H, HD = shape
    W = H * HD
    qh, kh, scale, _ = problem(shape)
    r = R.make_start("zeros", B, N)
    want = run(shape, fusion, dev(r))
    packed = torch.full((B * N, 3 * W + 5), float("nan"), device=DEV)
    packed[:, :W] = dev(qh)
    packed[:, W:2 * W] = dev(kh)
    rbuf = torch.full((B * N + 37,), float("nan"), device=DEV)
    obuf = torch.full((B * N + 37,), float("nan"), device=DEV)
    rv, ov = rbuf[19:19 + B * N].view(B, N), obuf[19:19 + B * N].view(B, N)
    rv.copy_(dev(r))
    keep = (packed.clone(), rbuf.clone())
    got = ops.rollout_step(packed[:, :W], packed[:, W:2 * W], B, N, H, HD, float(scale), rv, fusion, out=ov)
    assert got.data_ptr() == ov.data_ptr() and same_bits(got, want)
    assert bool(torch.isnan(obuf[:19]).all()) and bool(torch.isnan(obuf[19 + B * N:]).all())
    assert same_bits(packed, keep[0]) and same_bits(rbuf, keep[1])


@pytest.mark.parametrize("fusion", R.FUSIONS)
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("operand", ["q", "k"])
def test_a_planted_non_finite_value_poisons_its_sample_and_no_other(operand, value, fusion):
    """One element of one sample: every probability of a row (q) or of a column and of every row whose score there is +inf or NaN (k) is
    NaN, every column sum of that sample holds such a row, so no element of r_out[b] comes out finite; the other samples keep their
    bits.  (ro_fuse keeps a NaN through max / min fusion, where fmaxf would drop it.)"""
    shape = (3, 70, 2, 32)
    B, N, H, HD = shape
    qh, kh, scale, _ = problem(shape)
    r = R.make_start("zeros", B, N)
    clean = run(shape, fusion, dev(r))
    assert bool(torch.isfinite(clean).all())
    for row, col in ((1 * N + 5, 3), (1 * N + 69, HD + 31)):
        q, k = dev(qh).clone(), dev(kh).clone()
        (q if operand == "q" else k)[row, col] = value
        got = run(shape, fusion, dev(r), q, k)
        assert not bool(torch.isfinite(got[1]).any()), (row, col)
        assert same_bits(got[0], clean[0]) and same_bits(got[2], clean[2])


def test_refusals_of_the_python_entry():
    shape = (2, 63, 2, 32)
    B, N, H, HD = shape
    qh, kh, scale, _ = problem(shape)
    q, k, r = dev(qh), dev(kh), dev(R.make_start("cls", B, N))
    with pytest.raises(ValueError):
        ops.rollout_step(q, k, B, N, H, HD, scale, r, "median")
    with pytest.raises(TypeError):
        ops.rollout_step(q.half(), k, B, N, H, HD, scale, r)
    with pytest.raises(ValueError):
        ops.rollout_step(q, k, B, N + 1, H, HD, scale, r)
    with pytest.raises(ValueError):
        ops.rollout_step(q.t().contiguous().t(), k, B, N, H, HD, scale, r)
    with pytest.raises(ValueError):
        ops.rollout_step(q, k, B, N, H, HD, scale, r, out=r)
    with pytest.raises(RuntimeError):
        ops.rollout_step(q.cpu(), k, B, N, H, HD, scale, r)
    # the C entry on valid arguments, and in place: -2 with r untouched
    ws = torch.empty(R.ws_bytes(B, N, H, 0), dtype=torch.uint8, device=DEV)
    before = r.clone()
    rc = _lib.load().octmae_rollout_step(q.data_ptr(), H * HD, k.data_ptr(), H * HD, B, N, H, HD, float(scale), 0, r.data_ptr(), r.data_ptr(),
                                         ws.data_ptr(), ws.numel(), ops._stream())
    torch.cuda.synchronize()
    assert rc == -2 and same_bits(r, before)


# ------------------------------------------------------------------------------------------------ the models
def _sharpen(m):
    """default-initialised attention is nearly uniform: scale the q | k rows of every qkv weight so that the maps have structure"""
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("qkv.weight") or name.endswith("Wqkv.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.35)
    return m


@lru_cache(maxsize=None)
def model(kind, global_pool):
    torch.manual_seed(11)
    if kind == "st":
        m = models_vit_st.VisionTransformer(num_frames=6, t_patch_size=3, img_size=32, patch_size=16, in_chans=1, num_classes=8, embed_dim=64,
                                            depth=3, num_heads=2, mlp_ratio=4, norm_layer=NORM, sep_pos_embed=True, cls_embed=True,
                                            global_pool=global_pool, drop_path_rate=0.0, dropout=0.0)
        x = torch.randn(2, 1, 6, 32, 32, generator=torch.Generator().manual_seed(21))
        return _sharpen(m).to(DEV).eval(), x.to(DEV), (2, 9, 2, 32), (2, 2, 2)
    m = models_vit_flash_attn.VisionTransformer(img_size=32, patch_size=16, in_chans=3, num_classes=8, embed_dim=64, depth=3, num_heads=1,
                                                norm_layer=NORM, global_pool=global_pool)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(22))
    return _sharpen(m).to(DEV).eval(), x.to(DEV), (2, 5, 1, 64), (2, 2)


@pytest.mark.parametrize("kind", ["st", "flash2d"])
def test_capture_attention_changes_no_bit_and_sees_every_block(kind):
    m, x, (B, N, H, HD), _ = model(kind, False)
    with torch.no_grad():
        plain = m(x)
        before = len(ops._ATTN_CAPTURE or ())
        with ops.capture_attention() as seen:
            captured = m(x)
        after = m(x)
    assert before == 0 and ops._ATTN_CAPTURE is None
    assert same_bits(plain.float(), captured.float()) and same_bits(plain.float(), after.float())
    assert len(seen) == len(m.blocks) == 3                           # and nothing was appended by the forward outside the context
    for qkv, b, n, h, hd, scale in seen:
        assert (b, n, h, hd) == (B, N, H, HD) and scale == pytest.approx(HD ** -0.5)
        assert qkv.dtype == ops.BF16 and qkv.numel() == B * N * 3 * H * HD and qkv.is_cuda
    assert len({e[0].data_ptr() for e in seen}) == 3                 # the tensors the kernels were given, one per block


def published_from_capture(seen, fusion, first_layer):
    """float64 attention matrices from the captured 16-bit qkv (scores: the f32 chain's bits), then the published product"""
    attn, scores, scales = [], [], []
    for qkv, B, N, H, HD, scale in seen:
        C = H * HD
        qk = qkv.detach().view(B * N, 3 * C).float().cpu().numpy()
        s = R.chain_scores(qk[:, :C], qk[:, C:2 * C], B, N, H, HD)
        scores.append(s)
        scales.append(np.float32(scale))
        attn.append(torch.softmax(float(np.float32(scale)) * torch.from_numpy(s).double(), dim=-1))
    return R.published_rollout(attn, fusion, first_layer), scores, scales


@pytest.mark.parametrize("first_layer", [0, 1])
@pytest.mark.parametrize("fusion", R.FUSIONS)
@pytest.mark.parametrize("global_pool", [False, True], ids=["cls", "global_pool"])
@pytest.mark.parametrize("kind", ["st", "flash2d"])
def test_attention_rollout_equals_the_published_product(kind, global_pool, fusion, first_layer):
    m, x, (B, N, H, HD), grid = model(kind, global_pool)
    with torch.no_grad(), ops.capture_attention() as seen:
        logits = m(x)
    res = saliency.attention_rollout(m, x, head_fusion=fusion, first_layer=first_layer)
    assert same_bits(res["logits"].float(), logits.float())
    Rm, scores, scales = published_from_capture(seen, fusion, first_layer)
    w = torch.zeros(B, N, dtype=torch.float64)
    if global_pool:
        w[:, 1:] = 1.0 / (N - 1)
    else:
        w[:, 0] = 1.0
    want = torch.einsum("bi,bij->bj", w, Rm)
    _, bound = R.chain_reference(scores, scales, w.float().numpy(), fusion, first_layer)
    tokens = res["tokens"]
    assert tokens.shape == (B, N) and tokens.dtype == torch.float32
    ratio = R.worst(tokens, (want, bound))
    print(kind, global_pool, fusion, first_layer, "worst |err| / bound =", ratio, "largest bound", float(bound.max()))
    assert ratio < 1.0
    assert res["rollout"].shape == (B, *grid) and same_bits(res["rollout"].reshape(B, -1), tokens[:, 1:])
    assert float(tokens.std()) > 1e-3                                 # a map with structure, not the uniform row
    # a given start row is used as given; the same call twice gives the same bits
    start = torch.rand(B, N, generator=torch.Generator().manual_seed(5))
    start[:, 2] = 0.0
    a = saliency.attention_rollout(m, x, head_fusion=fusion, first_layer=first_layer, start=start.to(DEV))
    b = saliency.attention_rollout(m, x, head_fusion=fusion, first_layer=first_layer, start=start.to(DEV))
    _, bound = R.chain_reference(scores, scales, start.numpy(), fusion, first_layer)
    assert same_bits(a["tokens"], b["tokens"])
    assert R.worst(a["tokens"], (torch.einsum("bi,bij->bj", start.double(), Rm), bound)) < 1.0


def test_attention_rollout_refusals_and_the_heatmap():
    m, x, (B, N, H, HD), grid = model("st", False)
    with pytest.raises(NotImplementedError, match="no token grid is known"):
        saliency.attention_rollout(torch.nn.Linear(4, 4).to(DEV), x)
    bad = torch.full((B, N), 0.1)
    bad[1, 3] = -0.5
    with pytest.raises(ValueError, match="non-negative"):
        saliency.attention_rollout(m, x, start=bad.to(DEV))
    bad[1, 3] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        saliency.attention_rollout(m, x, start=bad.to(DEV))
    with pytest.raises(ValueError):
        saliency.attention_rollout(m, x, start=torch.ones(B, N + 1, device=DEV))
    with pytest.raises(ValueError):
        saliency.attention_rollout(m, x, head_fusion="median")
    with pytest.raises(ValueError):
        saliency.attention_rollout(m, x, first_layer=3)
    flags, grads = [mod.training for mod in m.modules()], [p.grad for p in m.parameters()]
    res = saliency.attention_rollout(m, x)
    assert [mod.training for mod in m.modules()] == flags and all(p.grad is g for p, g in zip(m.parameters(), grads))
    heat = saliency.heatmap(res["rollout"], (6, 32, 32))
    assert heat.shape == (B, 6, 32, 32) and heat.dtype == torch.uint8
