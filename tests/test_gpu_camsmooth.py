"""GPU tests of the smoothed Grad-CAM paths: octmae_cam_eigen and octmae_cam_accumulate (csrc/saliency.hip) against the references of
tests/camsmooth_ref.py, and saliency.grad_cam(eigen_smooth / aug_smooth) and saliency.grad_cam_multimodal on the tiny towers of
tests/test_gpu_coem_3mod.py (rebuilt here) against passes written out by hand.  The worst measured error / bound ratio of every bounded check goes into the suite's measured-error
ledger (tests/conftest.py); profiles/camsmooth_bounds.txt holds those of one run."""
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import _lib, coem, models_vit_2mod, models_vit_3dhead, models_vit_st, ops, saliency
from oracle import vit_ref as V
from tests import camsmooth_ref as R
from tests import saliency_ref as S
from tests.conftest import parity
from tests.gemm_elem import worst

DEV = "cuda"
NORM = partial(torch.nn.LayerNorm, eps=1e-6)
FEAT_TOL = 1e-2                    # tests/test_gpu_coem_3mod.py: tower features against the oracle; 2 x between a pass at B and one at 2 B
E, OUT = 128, 64
RATIOS = {}                        # label -> worst measured / bound


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def note(label, ratio):
    RATIOS[label] = max(RATIOS.get(label, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _ratios_into_the_ledger():
    """each worst ratio as one entry of the suite's measured-error ledger (tests/conftest.py: parity), bound 1"""
    yield
    for k in sorted(RATIOS):
        parity(f"camsmooth worst error / bound: {k}", RATIOS[k], 1.0)


def gpu_eigen(A, w, npre, iters, relu=False):
    cam, res = ops.cam_eigen(torch.from_numpy(A).to(DEV), torch.from_numpy(w).to(DEV), npre, iters, relu)
    return cam, res


# ---- 1: the eigen map against the float64 SVD -----------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def eigen_case(L, C, npre, ratio=0.5):
    """inputs, oracles and the float32 model's maps, computed once per case and shared"""
    A, w, refs = R.decided_batch(3, L, C, ratio, npre)
    models = [R.eigen_model32(A[b], w[b], npre, 32) for b in range(3)]
    return A, w, refs, models


def check_map(label, cam, refs, models):
    """every sample's map within eigen_bound of the oracle; -> the worst ratio"""
    out = 0.0
    for b, (ref, mod) in enumerate(zip(refs, models)):
        p64 = ref[0]
        bound = R.eigen_bound(R.map_error(mod[0], p64))
        err = R.map_error(cam[b].cpu().numpy(), p64)
        print(f"{label} sample {b}: GPU error / max|p| {err:.3e}, model {R.map_error(mod[0], p64):.3e}, bound {bound:.3e}")
        out = max(out, err / bound)
    note(label.split(" [")[0], out)
    return out


@pytest.mark.parametrize("C", [4, 68, 1024])
@pytest.mark.parametrize("L", [2, 5, 257])
@pytest.mark.parametrize("npre", [0, 1])
def test_eigen_map_within_the_bound_of_the_float64_svd(C, L, npre):
    A, w, refs, models = eigen_case(L, C, npre)
    assert all(r[3] <= 0.55 and r[4] >= R.MIN_MARGIN for r in refs)            # 0.55^64 is far below fp32: the bound is rounding alone
    if npre:
        assert float(np.abs(A[:, 0]).min()) == np.float32(3e38)
    cam, res = gpu_eigen(A, w, npre, 32)
    assert cam.shape == (3, L) and res.shape == (3,) and cam.dtype == res.dtype == torch.float32
    assert check_map(f"eigen map vs SVD [{C}, {L}, {npre}]", cam, refs, models) <= 1.0
    assert bool((res < R.RES_MANY).all()) and bool((res >= 0).all())
    relu, res_relu = gpu_eigen(A, w, npre, 32, relu=True)
    assert same_bits(relu, cam.clamp_min(0.0)) and same_bits(res_relu, res)
    assert bool((cam < 0).any()) and bool((cam > 0).any())                     # a centred projection has both signs


# ---- 2: iters is honoured -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,C,seed", [R.ITER_CASES[1], R.ITER_CASES[2]])
def test_iteration_count_is_honoured(L, C, seed):
    A, w = R.planted_batch(3, L, C, 0.8, seed, 1)
    refs = [R.eigen_ref64(A[b], w[b], 1) for b in range(3)]
    assert all(0.72 <= r[3] <= 0.88 and r[4] >= R.MIN_MARGIN for r in refs)
    _, few = gpu_eigen(A, w, 1, 2)
    cam, many = gpu_eigen(A, w, 1, 32)
    print(f"gap 0.8, ({L}, {C}): residual after 2 iterations {few.tolist()}, after 32 {many.tolist()}")
    assert bool((few > R.RES_FEW).all()) and bool((many < R.RES_MANY).all())
    models = [R.eigen_model32(A[b], w[b], 1, 32) for b in range(3)]
    assert check_map(f"eigen map vs SVD, gap 0.8 [{C}, {L}]", cam, refs, models) <= 1.0
    for b in range(3):                                                         # the reported residual is the model's, to rounding
        assert abs(float(few[b]) - R.eigen_model32(A[b], w[b], 1, 2)[1]) <= 1e-3


# ---- 3 / 4: degenerate and non-finite samples ------------------------------------------------------------------------------------------
def test_degenerate_samples_give_zero_maps_beside_an_untouched_neighbour():
    g = np.random.default_rng(3)
    A, w = R.planted_batch(3, 6, 8, 0.5, 7, 1)
    A[0, 1:] = (g.integers(-8, 9, 8) / 4.0).astype(np.float32)               # constant columns whose mean is exact in float32
    w[1] = 0.0
    cam, res = gpu_eigen(A, w, 1, 8)
    for b in (0, 1):
        assert int((cam[b] != 0).sum()) == 0 and float(res[b]) == 0.0, b
    assert not bool(torch.isnan(cam).any()) and not bool(torch.isnan(res).any())
    alone, res_alone = gpu_eigen(A[2:3].copy(), w[2:3].copy(), 1, 8)
    assert same_bits(cam[2:3], alone) and same_bits(res[2:3], res_alone) and float(cam[2].abs().max()) > 0
    one, res_one = gpu_eigen(np.ascontiguousarray(A[:, :2]), w, 1, 8)          # L = 1
    assert int((one != 0).sum()) == 0 and int((res_one != 0).sum()) == 0 and one.shape == (3, 1)


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_non_finite_sample_is_flagged_and_the_others_are_untouched(value):
    A, w = R.planted_batch(3, 37, 16, 0.5, 8, 1)
    clean, res = gpu_eigen(A, w, 1, 8)
    assert bool(torch.isfinite(res).all())
    bad = A.copy()
    bad[1, 20, 5] = value
    cam_b, res_b = gpu_eigen(bad, w, 1, 8)
    assert bool(torch.isnan(res_b[1]))
    for b in (0, 2):
        assert same_bits(cam_b[b], clean[b]) and same_bits(res_b[b], res[b])
    wb = w.copy()
    wb[1, 3] = value                                                           # a non-finite weight
    cam_w, res_w = gpu_eigen(A, wb, 1, 8)
    assert bool(torch.isnan(res_w[1])) and same_bits(cam_w[0], clean[0]) and same_bits(cam_w[2], clean[2])
    assert same_bits(res_w[[0, 2]], res[[0, 2]])


# ---- 5: past the grid caps --------------------------------------------------------------------------------------------------------------
def test_eigen_rows_past_the_grid_cap_follow_the_model():
    """eig_rows_kernel: one wave per token row on at most 8192 workgroups of 4 (32 768 rows).  (3, 4, 10925): 32 775 rows, 7 of them a
    wave's second, and 64 row splits of 171 rows in the transposed product.  Two iterations, against the float32 model of the same two
    iterations; what separates the two is rounding, whose size on this input is the converged model's error against the SVD."""
    B, C, L = 3, 4, 10925
    assert B * L > 8192 * 4 and (B * L) % (8192 * 4) % 4 != 0
    A, w, refs = R.decided_batch(B, L, C, 0.5, 1)
    cam, res = gpu_eigen(A, w, 1, 2)
    worst_ratio = 0.0
    for b in range(B):
        m2, r2, _ = R.eigen_model32(A[b], w[b], 1, 2)
        bound = R.eigen_bound(R.map_error(R.eigen_model32(A[b], w[b], 1, 32)[0], refs[b][0]))
        err = R.map_error(cam[b].cpu().numpy(), m2.astype(np.float64))
        print(f"past the row cap, sample {b}: GPU against the model {err:.3e}, bound {bound:.3e}; residual {float(res[b]):.3e} / {r2:.3e}")
        worst_ratio = max(worst_ratio, err / bound)
        assert abs(float(res[b]) - r2) <= 1e-3
    note("eigen map vs model past the row cap", worst_ratio)
    assert worst_ratio <= 1.0


def test_eigen_on_a_large_batch_of_single_rows_is_zero():
    """(4100, 68, 1): 4100 workgroups of the per-sample fold, 17 column quads each; L = 1 centres every row away"""
    g = torch.Generator().manual_seed(5)
    A = torch.randn(4100, 2, 68, generator=g)
    A[:, 0] = 3e38
    cam, res = ops.cam_eigen(A.to(DEV), torch.randn(4100, 68, generator=g).to(DEV), 1, 2)
    assert cam.shape == (4100, 1) and int((cam != 0).sum()) == 0 and int((res != 0).sum()) == 0


def test_eigen_start_vector_past_the_grid_cap_equals_the_samples_alone():
    """eig_init_kernel: one thread per element of v on at most 4096 workgroups of 256 (1 048 576).  (16 400, 64, 2): 1 049 600 elements,
    1024 of them -- the start vectors of the last 16 samples -- on a second trip; those samples run alone must give the same bits."""
    B, C, L = 16400, 64, 2
    assert B * C > 4096 * 256 and (B * C - 4096 * 256) // C == 16
    g = torch.Generator().manual_seed(6)
    A, w = torch.randn(B, 1 + L, C, generator=g).to(DEV), torch.randn(B, C, generator=g).to(DEV)
    cam, res = ops.cam_eigen(A, w, 1, 3, relu=False)
    tail, res_tail = ops.cam_eigen(A[-20:].contiguous(), w[-20:].contiguous(), 1, 3, relu=False)
    assert same_bits(cam[-20:], tail) and same_bits(res[-20:], res_tail)
    assert bool(torch.isfinite(cam).all()) and bool(torch.isfinite(res).all()) and float(cam[-16:].abs().min()) > 0


# ---- 6: determinism and refusals ------------------------------------------------------------------------------------------------------
def test_eigen_is_deterministic_and_refuses_wrong_tensors():
    A, w, _, _ = eigen_case(257, 68, 1)
    a, ra = gpu_eigen(A, w, 1, 8)
    b, rb = gpu_eigen(A, w, 1, 8)
    assert same_bits(a, b) and same_bits(ra, rb)
    Z, z = torch.zeros(2, 6, 8, device=DEV), torch.zeros(2, 8, device=DEV)
    for bad in (lambda: ops.cam_eigen(Z[:, :, :6].contiguous(), z[:, :6].contiguous(), 1),        # C % 4
                lambda: ops.cam_eigen(Z, z, 6),                                                     # no patch row left
                lambda: ops.cam_eigen(Z, z, 1, iters=0),
                lambda: ops.cam_eigen(Z, z[:, :4].contiguous(), 1),
                lambda: ops.cam_eigen(Z.double(), z, 1),
                lambda: ops.cam_eigen(Z, z.cpu(), 1),
                lambda: ops.cam_eigen(Z.cpu(), z.cpu(), 1),
                lambda: ops.cam_eigen(Z.transpose(1, 2), z, 1),
                lambda: ops.cam_accumulate(torch.zeros(2, 30, device=DEV), torch.zeros(2, 30, device=DEV), 4, False, 1.0, True),   # n % width
                lambda: ops.cam_accumulate(torch.zeros(2, 30, device=DEV), torch.zeros(2, 32, device=DEV), 4, False, 1.0, True),
                lambda: ops.cam_accumulate(torch.zeros(2, 32, device=DEV).double(), torch.zeros(2, 32, device=DEV), 4, False, 1.0, True),
                lambda: ops.cam_accumulate(torch.zeros(2, 32), torch.zeros(2, 32), 4, False, 1.0, True),
                lambda: ops.cam_accumulate(torch.zeros(2, 32, device=DEV), torch.zeros(2, 32, device=DEV), 0, False, 1.0, True)):
        with pytest.raises(RuntimeError):
            bad()
    same = torch.zeros(2, 32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.cam_accumulate(same, same, 4, False, 1.0, True)


# ---- 7: the augmentation fold ---------------------------------------------------------------------------------------------------------
def check_accumulate(B, n, width, flip, first, label):
    g = np.random.default_rng(B + n + width)
    cam = g.standard_normal((B, n)).astype(np.float32)
    cam[-1] = cam[-1] * 50 - 20                                               # per-sample ranges
    acc0 = g.standard_normal((B, n)).astype(np.float32)
    weight = 1.0 / 6.0
    acc = torch.full((B, n), float("nan"), device=DEV) if first else torch.from_numpy(acc0).to(DEV)
    out = ops.cam_accumulate(acc, torch.from_numpy(cam).to(DEV), width, flip, weight, first)
    assert out is acc
    ref = R.accumulate_ref64(acc0, cam, width, flip, weight, first)
    ratio = float((np.abs(out.cpu().numpy().astype(np.float64) - ref) / R.accumulate_bound(acc0, cam, weight, first)).max())
    note(label, ratio)
    return ratio


@pytest.mark.parametrize("B,n,width", [(1, 4, 4), (3, 6 * 5, 5), (2, 8 * 8 * 20, 8)])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("first", [False, True])
def test_accumulate_within_a_few_roundings_of_float64(B, n, width, flip, first):
    assert check_accumulate(B, n, width, flip, first, "cam_accumulate vs float64") <= 1.0


def test_accumulate_past_the_grid_cap():
    """cam_accum_kernel: one thread per element on at most 4096 workgroups of 256 (1 048 576); 817 x 1284 = 1 049 028 elements, 452 of
    them (one workgroup and 196 threads of the next) on a second trip"""
    assert 817 * 1284 > 4096 * 256 and (817 * 1284 - 4096 * 256) % 256 != 0
    assert check_accumulate(817, 1284, 12, True, False, "cam_accumulate past the grid cap") <= 1.0


def test_accumulate_constant_map_and_the_flip_of_a_flipped_map():
    acc = torch.full((2, 12), 0.75, device=DEV)
    out = ops.cam_accumulate(acc, torch.full((2, 12), 3.25, device=DEV), 4, True, 0.5, False)
    assert bool((out == 0.75).all())                                           # a constant map contributes exactly 0
    assert int((ops.cam_accumulate(torch.empty(2, 12, device=DEV), torch.full((2, 12), -2.0, device=DEV), 3, False, 0.5, True) != 0).sum()) == 0
    for width in (5, 8, 1):
        g = torch.Generator().manual_seed(width)
        m = torch.randn(3, 6, width, generator=g)
        md, fd = m.to(DEV).reshape(3, -1), m.flip(-1).contiguous().to(DEV).reshape(3, -1)
        acc = ops.cam_accumulate(torch.empty(3, 6 * width, device=DEV), md, width, False, 0.25, True)
        ops.cam_accumulate(acc, fd, width, True, 0.25, False)                  # the flip of the flipped map is the map
        ref = 2.0 * R.accumulate_ref64(None, m.reshape(3, -1).numpy(), width, False, 0.25, True)
        assert float((np.abs(acc.cpu().numpy().astype(np.float64) - ref) / (2 * R.accumulate_bound(None, None, 0.25, True))).max()) <= 1.0


# ---- models -----------------------------------------------------------------------------------------------------------------------------
def tower2():
    c2 = V.ViT2DConfig(img_size=64, patch_size=16, in_chans=3, num_classes=E, embed_dim=E, depth=2, num_heads=2, global_pool=True)
    P2 = V.init_from_shapes(V.vit2d_param_shapes(c2), seed=52)
    g = torch.Generator().manual_seed(58)
    for i in range(2):
        P2[f"mod_head_{i}.weight"] = torch.randn(OUT, E, generator=g) * 0.05
        P2[f"mod_head_{i}.bias"] = torch.randn(OUT, generator=g) * 0.02
    t = models_vit_2mod.VisionTransformer(image_size=64, out_dim=OUT, embed_dim=E, depth=2, num_heads=2, mlp_ratio=4, norm_layer=NORM,
                                          flash_compat=False)
    t.load_state_dict(P2, strict=True)
    return t.to(DEV)


def tower3():
    c3 = V.ViTSTConfig(num_frames=6, t_patch_size=3, img_size=64, patch_size=16, in_chans=1, num_classes=OUT, embed_dim=E, depth=2,
                       num_heads=2, global_pool=True)
    P3 = V.init_from_shapes(V.vit_st_param_shapes(c3), seed=51)
    m3 = models_vit_st.VisionTransformer(num_frames=6, t_patch_size=3, img_size=64, patch_size=16, in_chans=1, num_classes=OUT, embed_dim=E,
                                         depth=2, num_heads=2, sep_pos_embed=True, cls_embed=True, global_pool=True, dropout=0.0,
                                         mlp_ratio=4, norm_layer=NORM)
    m3.load_state_dict(P3, strict=True)
    return m3.to(DEV)


def cls_model(three=True, pair=True, num_classes=8):
    """the same weights at every call: the towers from fixed parameters, the head from a fixed seed"""
    m3, t2 = tower3(), tower2()
    torch.manual_seed(7)
    if three:
        return coem.CustomTextCLIP3ModClassification(m3, t2, num_classes, pair=pair).to(DEV)
    return coem.CustomTextCLIPClassification(m3, t2, num_classes).to(DEV)


def inputs(three=True):
    g = torch.Generator().manual_seed(16)
    x = {"image": torch.rand(2, 1, 6, 64, 64, generator=g).to(DEV), "text1": torch.randn(2, 3, 64, 64, generator=g).to(DEV),
         "text2": torch.randn(2, 3, 64, 64, generator=g).to(DEV)}
    if not three:
        x = {"image": x["image"], "text": x["text2"]}
    return x, torch.tensor([5, 2], device=DEV)


GRID = {"image": (2, 4, 4), "text": (4, 4), "text1": (4, 4), "text2": (4, 4)}


def first(h):
    return h[0] if isinstance(h, (tuple, list)) else h


def by_hand(model, x, tgt, lv, lt, three):
    """hooks, one forward, one autograd.grad, the two reductions: {name: (A, G, cam)} and the logits"""
    seen = {"visual": [], "text": []}
    hs = [model.visual.blocks[lv].register_forward_hook(lambda m, i, o: seen["visual"].append(first(o))),
          model.text.blocks[lt].register_forward_hook(lambda m, i, o: seen["text"].append(first(o)))]
    model.eval()
    try:
        with torch.enable_grad(), ops.weight_grads(False):
            args = [x[k].clone().requires_grad_(True) for k in (("image", "text1", "text2") if three else ("image", "text"))]
            logits = model(*args)[0]
            flat = seen["visual"] + seen["text"]
            grads = torch.autograd.grad(logits.gather(1, tgt[:, None]).sum(), flat)
    finally:
        for h in hs:
            h.remove()
    parts = {"image": (seen["visual"][0], grads[0])}
    if not three:
        parts["text"] = (seen["text"][0], grads[1])
    elif len(seen["text"]) == 1:
        parts["text1"] = (seen["text"][0][:2], grads[1][:2])
        parts["text2"] = (seen["text"][0][2:], grads[1][2:])
    else:
        parts["text1"], parts["text2"] = (seen["text"][0], grads[1]), (seen["text"][1], grads[2])
    out = {}
    for k, (A, G) in parts.items():
        A, G = A.detach().float().contiguous(), G.float().contiguous()
        out[k] = (A, G, ops.cam_tokens(A, ops.cam_weights(G, 1), 1).view(2, *GRID[k]))
    return logits.detach(), out


def cosine(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a * b).sum() / (a.norm() * b.norm()))


# ---- 8: multimodal plumbing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("three,pair", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("layers", [-1, (0, 1)])
def test_multimodal_streams_gradients_and_maps_equal_a_pass_by_hand(three, pair, layers):
    x, tgt = inputs(three)
    lv, lt = (layers, layers) if isinstance(layers, int) else layers
    model = cls_model(three, pair).train()
    res = saliency.grad_cam_multimodal(model, x, tgt, layers=layers, return_streams=True)
    assert model.training and all(m.training for m in model.modules())
    names = ("image", "text1", "text2") if three else ("image", "text")
    assert set(res) == {"logits", "target", "cam", "activations", "gradients"} and torch.equal(res["target"], tgt)
    assert all(set(res[k]) == set(names) for k in ("cam", "activations", "gradients"))
    logits, hand = by_hand(cls_model(three, pair), x, tgt, lv, lt, three)
    assert same_bits(res["logits"], logits)
    for k in names:
        A, G, cam = hand[k]
        assert res["cam"][k].shape == (2,) + GRID[k] and res["cam"][k].dtype == torch.float32
        assert same_bits(res["activations"][k], A) and same_bits(res["gradients"][k], G) and same_bits(res["cam"][k], cam), k
        _, _, cam64, cb = S.cam_ref64(res["activations"][k], res["gradients"][k], 1)
        val, idx = worst(res["cam"][k].reshape(2, -1), cam64, cb)
        assert val <= 1.0 and float(cam64.max()) > 0 and float(G.abs().sum()) > 0, (k, val, idx)
    # the streams are what the towers hand on: the hidden states of the same passes
    ev = model.eval()
    with torch.no_grad():
        assert same_bits(res["activations"]["image"], first(ev.visual(x["image"], hidden_states=True)[lv]).float().contiguous())
        if not three:
            assert same_bits(res["activations"]["text"], first(ev.text(x["text"], hidden_states=True)[lt]).float().contiguous())
        elif pair:
            h = first(ev.text(torch.cat((x["text1"], x["text2"])), hidden_states=True)[lt]).float()
            assert same_bits(res["activations"]["text1"], h[:2].contiguous()) and same_bits(res["activations"]["text2"], h[2:].contiguous())
        else:
            for i, k in enumerate(("text1", "text2")):
                assert same_bits(res["activations"][k], first(ev.text(x[k], hidden_states=True, modality=i)[lt]).float().contiguous())
    # the default target is the arg-max class; without return_streams the three keys
    auto = saliency.grad_cam_multimodal(model, x, layers=layers)
    assert set(auto) == {"logits", "target", "cam"} and torch.equal(auto["target"], res["logits"].argmax(1))
    heat = saliency.heatmap(res["cam"]["image"], (6, 64, 64))
    assert heat.dtype == torch.uint8 and heat.shape == (2, 6, 64, 64)
    assert saliency.heatmap(res["cam"][names[-1]], (64, 64)).shape == (2, 64, 64)


def test_paired_and_unpaired_en_face_maps_agree_and_are_not_swapped():
    x, tgt = inputs()
    a = saliency.grad_cam_multimodal(cls_model(pair=True), x, tgt)["cam"]
    b = saliency.grad_cam_multimodal(cls_model(pair=False), x, tgt)["cam"]
    own = {k: cosine(a[k], b[k]) for k in ("image", "text1", "text2")}
    cross = {"text1": cosine(a["text1"], b["text2"]), "text2": cosine(a["text2"], b["text1"])}
    print("pair against two passes, cosine of the maps:", own, "against the other modality's:", cross)
    for k in ("text1", "text2"):
        assert own[k] >= 1.0 - 2 * FEAT_TOL and own[k] > cross[k], (k, own, cross)
    assert same_bits(a["image"], b["image"]) or own["image"] >= 1.0 - 2 * FEAT_TOL


@pytest.mark.parametrize("three", [True, False])
def test_single_modality_leaves_the_other_maps_out(three):
    x, tgt = inputs(three)
    model = cls_model(three)
    names = ("image", "text1", "text2") if three else ("image", "text")
    for only in names:
        res = saliency.grad_cam_multimodal(model, {only: x[only]}, tgt, single_modality=only, eigen_smooth=True, return_streams=True)
        for k in names:
            if k == only:
                assert res["cam"][k].shape == (2,) + GRID[k] and res["residual"][k].shape == (2,) and res["activations"][k] is not None
            else:
                assert res["cam"][k] is None and res["residual"][k] is None and res["activations"][k] is None and res["gradients"][k] is None
        full = model.eval()(*[x[k] for k in names], single_modality=only)[0]
        assert same_bits(res["logits"], full.detach())
    with pytest.raises(ValueError):
        saliency.grad_cam_multimodal(model, x, tgt, single_modality="text3")
    with pytest.raises(ValueError):
        saliency.grad_cam_multimodal(model, {"image": x["image"]}, tgt)


def test_multimodal_pass_leaves_the_model_alone():
    x, tgt = inputs()
    model = cls_model().train()
    model(*x.values())[0].sum().backward()                         # binds every p.grad to its arena
    arenas = (model.visual.arena, model.text.arena, model.classification_head.arena)
    for a in arenas:
        a.grad.view(torch.int32).fill_(0x3F8ACE01)
    before = [a.grad.clone() for a in arenas]
    flat = [a.flat.clone() for a in arenas]
    grads = [(p, p.grad) for p in model.parameters()]
    count = [0]
    owner = object()
    ops.add_grad_ready_callback(owner, lambda ps: count.__setitem__(0, count[0] + len(ps) + 1))
    try:
        saliency.grad_cam_multimodal(model, x, tgt, eigen_smooth=True, aug_smooth=True)
        torch.cuda.synchronize()
    finally:
        ops.remove_grad_ready_callback(owner)
    assert model.training and all(m.training for m in model.modules()) and count[0] == 0
    assert all(p.grad is g for p, g in grads)
    for a, g, f in zip(arenas, before, flat):
        assert same_bits(a.grad, g) and same_bits(a.flat, f)


def test_classes_without_a_grid_are_refused_by_name():
    m3, t2 = tower3(), tower2()
    with pytest.raises(NotImplementedError, match="CustomTextCLIP3Mod"):
        saliency.grad_cam_multimodal(coem.CustomTextCLIP3Mod(m3, t2).to(DEV), inputs()[0])
    head3d = models_vit_3dhead.VisionTransformerWith3DPoolingHead(img_size=64, patch_size=16, in_chans=3, num_classes=OUT, embed_dim=E,
                                                                  depth=1, num_heads=2, norm_layer=NORM).to(DEV)
    with pytest.raises(NotImplementedError, match="VisionTransformerWith3DPoolingHead"):
        saliency.grad_cam_multimodal(coem.CustomTextCLIPClassification(m3, head3d, 8, embed_dim=OUT).to(DEV), inputs(False)[0])


def test_grad_cam_knows_the_en_face_tower():
    t2 = tower2()
    x, _ = inputs()
    res = saliency.grad_cam(t2, x["text1"], torch.tensor([5, 2], device=DEV), return_streams=True)
    assert res["cam"].shape == (2, 4, 4) and res["activations"].shape == (2, 17, E)
    _, _, cam64, cb = S.cam_ref64(res["activations"], res["gradients"], 1)
    assert worst(res["cam"].reshape(2, -1), cam64, cb)[0] <= 1.0 and float(cam64.max()) > 0


# ---- 9: smoothing through the model ---------------------------------------------------------------------------------------------------
def st_inputs():
    return torch.rand(2, 1, 6, 64, 64, generator=torch.Generator().manual_seed(21)).to(DEV), torch.tensor([3, 40], device=DEV)


def test_eigen_smooth_is_cam_eigen_on_the_returned_streams():
    m, (x, tgt) = tower3(), st_inputs()
    res = saliency.grad_cam(m, x, tgt, eigen_smooth=True, return_streams=True)
    assert set(res) == {"logits", "target", "cam", "residual", "activations", "gradients"}
    cam, residual = ops.cam_eigen(res["activations"], ops.cam_weights(res["gradients"], 1), 1, 32)
    assert same_bits(res["cam"], cam.view(2, 2, 4, 4)) and same_bits(res["residual"], residual) and float(cam.max()) > 0
    plain = saliency.grad_cam(m, x, tgt, return_streams=True)
    assert set(plain) == {"logits", "target", "cam", "activations", "gradients"}
    assert same_bits(plain["activations"], res["activations"]) and same_bits(plain["gradients"], res["gradients"])
    few = saliency.grad_cam(m, x, tgt, eigen_smooth=True, eigen_iters=1)
    assert not same_bits(few["cam"], res["cam"])
    # the float64 oracle on the same streams: the residual says whether the map is to be trusted, and where it does, it is
    wd = ops.cam_weights(res["gradients"], 1)
    signed, _ = ops.cam_eigen(res["activations"], wd, 1, 32, relu=False)
    assert same_bits(signed.clamp_min(0.0), cam)
    A, w = res["activations"].cpu().numpy(), wd.cpu().numpy()
    for b in range(2):
        p64, _, _, rho, margin = R.eigen_ref64(A[b], w[b], 1)
        err = R.map_error(signed[b].cpu().numpy(), p64)
        print(f"model streams, sample {b}: sigma2 / sigma1 {rho:.3f}, sign margin {margin:.3f}, residual {float(residual[b]):.2e}, "
              f"map error {err:.2e}")
        if margin >= R.MIN_MARGIN and rho <= 0.55:
            assert err <= R.eigen_bound(R.map_error(R.eigen_model32(A[b], w[b], 1, 32)[0], p64))


@pytest.mark.parametrize("eigen", [False, True])
def test_aug_smooth_is_the_fold_of_six_explicit_passes(eigen):
    m, (x, tgt) = tower3(), st_inputs()
    res = saliency.grad_cam(m, x, tgt, aug_smooth=True, eigen_smooth=eigen)
    plain = saliency.grad_cam(m, x, tgt, eigen_smooth=eigen)
    acc, worst_res = torch.empty(2, 32, device=DEV), None
    k = 0
    for flip in (False, True):
        for factor in (0.9, 1.0, 1.1):
            xa = x.flip(-1) if flip else x
            one = saliency.grad_cam(m, xa if factor == 1.0 else xa * factor, tgt, eigen_smooth=eigen)
            ops.cam_accumulate(acc, one["cam"].reshape(2, -1), 4, flip, 1.0 / 6.0, k == 0)
            if eigen:
                worst_res = one["residual"] if worst_res is None else torch.maximum(worst_res, one["residual"])
            k += 1
    assert same_bits(res["cam"], acc.view(2, 2, 4, 4))
    assert float(res["cam"].min()) >= 0.0 and float(res["cam"].max()) <= 1.0 and float(res["cam"].max()) > 0.0
    assert same_bits(res["logits"], plain["logits"]) and torch.equal(res["target"], tgt)
    assert set(res) == ({"logits", "target", "cam", "residual"} if eigen else {"logits", "target", "cam"})
    if eigen:
        assert same_bits(res["residual"], worst_res)
    auto = saliency.grad_cam(m, x, aug_smooth=True)
    assert torch.equal(auto["target"], plain["logits"].argmax(1))


def test_smoothed_saliency_is_autocast_invariant():
    m, (x, tgt) = tower3(), st_inputs()
    xs, t2 = inputs()
    model = cls_model()

    def run():
        return (saliency.grad_cam(m, x, tgt, eigen_smooth=True, aug_smooth=True),
                saliency.grad_cam_multimodal(model, xs, t2, eigen_smooth=True, aug_smooth=True, return_streams=True))
    plain = run()
    with torch.cuda.amp.autocast():
        cast = run()

    def flat(d, prefix=""):
        for k, v in d.items():
            if isinstance(v, dict):
                yield from flat(v, prefix + k + ".")
            else:
                yield prefix + k, v
    for a, b in zip(plain, cast):
        fa, fb = dict(flat(a)), dict(flat(b))
        assert fa.keys() == fb.keys()
        for k in fa:
            assert same_bits(fa[k], fb[k]), k
    mm = plain[1]
    for k in ("image", "text1", "text2"):
        assert float(mm["cam"][k].min()) >= 0.0 and float(mm["cam"][k].max()) <= 1.0 and mm["residual"][k].shape == (2,)
