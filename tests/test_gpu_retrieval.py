"""GPU tests of the COEM validation: octmae_retrieval_ranks (ops.retrieval_ranks, csrc/retrieval.hip) and coem.get_metrics /
get_metrics_3modalities / get_corrected_metrics / evaluate on top of it.

R / C / K below are the kernel's RR_ROWS / RR_COLS / RR_K (64 rows of a per workgroup, 64 columns per tile, 32 k per LDS step; an MFMA
step is 2 k).  Sizes: n, m from {1, 2, R-1, R, R+1, C-1, C+1, 2C+3} = {1, 2, 63, 64, 65, 131}, d from {1, 2, 3, K-1, K, K+1, 512, 515},
paired (not the full product) so that the largest n m d = 131 * 131 * 515 keeps the numpy references well under a second.  On top of
them the three shapes of retrieval_ref.TRIP_SHAPES, where a workgroup walks more than one column tile (d of 2 or 3).

Families.  ``dyadic``: entries in {-2 .. 2} / 4, every product a multiple of 1/16 and every partial sum below 2^10, so the f32 chain is
exact and the expected counts are integer numpy arithmetic -- all four outputs EQUAL; ties everywhere, which pins the tie rule, keep and
the groups.  ``equal``: all rows identical -> out0 == 0, out1 == the kept columns before the target.  ``duplicates``: normalised normal
features with a tenth of b's rows bit copies of other rows: a copy of the target row ties (out1 if its index is lower, never out0), which
fails when t_i is not the tile's own value.  ``continuous``: with float64 scores and beta_ij = d 2^-23 sum_k |a_ik b_jk| (twice the
gamma_d bound of an f32 chain of d terms, unit roundoff 2^-24) the position must lie in [lo_i, hi_i]; at most 5 % of the rows may have
lo != hi and R@1 must be neither 0 nor 1, both asserted, so the case cannot be hollow."""
import functools
import json
import os
import types
from functools import partial

import numpy as np
import pytest
import torch

from tests import children
from tests import retrieval_ref as R
from tests import test_cpu_retrieval as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")
RR, CC, KK = 64, 64, 32

# (n, m, d): every n, m of {1, 2, R-1, R, R+1, C-1, C+1, 2C+3} and every d of {1, 2, 3, K-1, K, K+1, 512, 515} occurs
SIZES = ((1, 1, 1), (2, 2, 2), (63, 63, 3), (64, 64, 31), (65, 65, 32), (131, 131, 33), (64, 131, 512), (131, 65, 515), (1, 131, 32),
         (131, 1, 33), (2, 63, 515), (65, 2, 1), (63, 64, 512), (131, 131, 515))
assert {s[0] for s in SIZES} | {s[1] for s in SIZES} == {1, 2, RR - 1, RR, RR + 1, CC - 1, CC + 1, 2 * CC + 3}
assert {s[2] for s in SIZES} == {1, 2, 3, KK - 1, KK, KK + 1, 512, 515}
DYADIC_CASES = [(n, m, d, full) for (n, m, d) in SIZES for full in (False, True) if full or n == m]
# ... and R.TRIP_SHAPES, appended: a workgroup walks several column tiles there (it keeps its four counters and rewrites flg / cgs per
# tile): split 1024 of 1025 tiles, 22 of 47, and 1 of 3 under 1024 row blocks.  full = a target table, keep and the groups, each time.
TRIP_CASES = [(n, m, d, full) for (n, m, d) in R.TRIP_SHAPES for full in (False, True) if full or n == m]
DYADIC_CASES += TRIP_CASES


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def side_inputs(rng, n, m, full):
    """full: explicit target, a keep mask (targets kept), two groups; otherwise all None (needs n == m)"""
    if not full:
        return None, None, None, None
    target = rng.integers(0, m, size=n).astype(np.int32)
    if n > 8 * m and m > 8:                  # far more rows than columns: targets from half of the columns, or every column is one
        cols = rng.permutation(m)[:m // 2]
        target = cols[rng.integers(0, len(cols), size=n)].astype(np.int32)
    keep = (rng.random(m) < 0.7).astype(np.uint8)
    keep[target] = 1
    return target, keep, rng.integers(0, 4, size=n).astype(np.int32), rng.integers(0, 4, size=m).astype(np.int32)


@functools.lru_cache(maxsize=None)
def dyadic_case(n, m, d, full):
    rng = np.random.default_rng([n, m, d, int(full), 1])
    ia, ib = rng.integers(-2, 3, size=(n, d)), rng.integers(-2, 3, size=(m, d))
    target, keep, rg, cg = side_inputs(rng, n, m, full)
    want = R.counts(ia @ ib.T, target, keep, rg, cg)                     # integer scores, 16 x the f32 ones: exact
    a, b = (ia / 4).astype(np.float32), (ib / 4).astype(np.float32)
    for x in (a, b, want):
        x.setflags(write=False)
    return a, b, target, keep, rg, cg, want


def launch(a, b, target=None, keep=None, rg=None, cg=None):
    from octcubem_amd import ops
    got = ops.retrieval_ranks(dev(a), dev(b), dev(target), dev(keep), dev(rg), dev(cg))
    assert got.dtype == torch.int32 and tuple(got.shape) == (a.shape[0], 4) and got.is_contiguous()
    return got.cpu().numpy().astype(np.int64)


def check_dyadic(n, m, d, full):
    a, b, target, keep, rg, cg, want = dyadic_case(n, m, d, full)
    got = launch(a, b, target, keep, rg, cg)
    assert np.array_equal(got, want), f"n={n} m={m} d={d} full={full}: {int((got != want).sum())} of {want.size} counts differ"


@pytest.mark.parametrize("n,m,d,full", DYADIC_CASES)
def test_dyadic_counts_are_equal(n, m, d, full):
    check_dyadic(n, m, d, full)


def test_dyadic_cases_have_ties_and_groups():
    a, b, target, keep, rg, cg, want = dyadic_case(131, 131, 515, True)
    assert (want[:, 1] > 0).any() and (want[:, 0] > 0).any() and (want[:, 3] > want[:, 2]).any() and (want[:, 2] > 0).any() and not keep.all()
    for n, m, d in R.TRIP_SHAPES:              # ... and counts that no single tile can hold: every tile's share has to arrive
        _, _, _, keep, _, _, want = dyadic_case(n, m, d, True)
        assert (want[:, 1] > 0).any() and (want[:, 0] > 0).any() and (want[:, 3] > want[:, 2]).any() and (want[:, 2] > 0).any()
        tiles = [keep[j0:j0 + CC] for j0 in range(0, m, CC)]
        assert not keep.all() and sum(0 < t.sum() < len(t) for t in tiles) >= min(len(tiles), 3) - 1      # the keep bits differ from tile to tile
        assert m < 1000 or want[:, 3].min() > CC


@pytest.mark.parametrize("n,m,d", ((65, 65, 3), (64, 131, 33), (131, 63, 512)))
def test_equal_rows_tie_by_column_index(n, m, d):
    rng = np.random.default_rng([n, m, d, 2])
    v = rng.standard_normal(d).astype(np.float32)
    a, b = np.tile(v, (n, 1)), np.tile(v, (m, 1))
    target, keep, rg, cg = side_inputs(rng, n, m, True)
    got = launch(a, b, target, keep, rg, cg)
    before = np.array([int(keep[:t].sum()) for t in target])
    assert np.array_equal(got[:, 0], np.zeros(n, dtype=np.int64)) and np.array_equal(got[:, 1], before)
    same = (cg[None, :] == rg[:, None]).sum(1)
    assert np.array_equal(got[:, 3], same) and np.array_equal(got[:, 2], same)          # s = sum v^2 > 0


def normalize(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def bounds(a, b, target, exclude=None):
    """(lo, hi, s64, beta): lo_i counts the j != target with s64 - beta > t64 + beta_t, hi_i the j with s64 + beta >= t64 - beta_t minus the
    target itself; columns with exclude[i, j] take part in neither."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    s = a64 @ b64.T
    beta = a.shape[1] * 2.0 ** -23 * (np.abs(a64) @ np.abs(b64).T)
    rows = np.arange(a.shape[0])
    t, bt = s[rows, target][:, None], beta[rows, target][:, None]
    other = np.ones(s.shape, dtype=bool)
    other[rows, target] = False
    if exclude is not None:
        other &= ~exclude
    lo = (other & (s - beta > t + bt)).sum(1)
    hi = (other & (s + beta >= t - bt)).sum(1)
    return lo, hi, s, beta


@pytest.mark.parametrize("n,m,d", ((131, 131, 33), (65, 131, 515), (64, 64, 512)))
def test_bit_copies_of_the_target_row_tie(n, m, d):
    rng = np.random.default_rng([n, m, d, 3])
    a = normalize(rng.standard_normal((n, d)))
    b = normalize(0.5 * np.resize(a, (m, d)) + normalize(rng.standard_normal((m, d))))
    copies = rng.choice(m, size=max(m // 10, 2), replace=False)
    src = np.array([rng.choice(np.setdiff1d(np.arange(m), copies)) for _ in copies])
    b[copies] = b[src]
    cls = np.arange(m)
    cls[copies] = src                                                         # the class of a row: the row it is a bit copy of
    target = np.concatenate([copies, src, rng.integers(0, m, size=n)])[:n].astype(np.int32)      # targets with copies above and below
    got = launch(a, b, target)
    twin = cls[None, :] == cls[target][:, None]                               # [n, m]: j holds the same bits as the target row
    twins_before = (twin & (np.arange(m)[None, :] < target[:, None])).sum(1)
    assert twins_before.max() >= 1 and (twin.sum(1) > 1).sum() >= 2
    lo, hi, s, beta = bounds(a, b, target, exclude=twin)
    t, bt = s[np.arange(n), target][:, None], beta[np.arange(n), target][:, None]
    near = (~twin & (np.arange(m)[None, :] < target[:, None]) & (np.abs(s - t) <= beta + bt)).sum(1)     # ties the bound leaves open
    assert (got[:, 1] >= twins_before).all() and (got[:, 1] <= twins_before + near).all(), (got[:, 1], twins_before)
    pos = got[:, 0] + got[:, 1]
    assert (pos >= lo + twins_before).all() and (pos <= hi + twins_before).all()
    assert (got[:, 0] <= hi).all()                                            # a twin is never counted as greater


CONTINUOUS = ((63, 63, 31, 0.25), (131, 131, 32, 0.25), (65, 131, 33, 0.25), (131, 131, 512, 0.15), (64, 131, 515, 0.15)) + \
    (R.TRIP_SHAPES[1] + (20.0,),)


@pytest.mark.parametrize("n,m,d,c", CONTINUOUS)
def test_continuous_positions_lie_within_the_f32_bound(n, m, d, c):
    """b = normalize(c a + unit noise); c = 0.25, lowered to 0.15 at d >= 512 where 0.25 gives R@1 above 0.9 (float64 on the CPU: R@1
    0.18 / 0.09 / 0.11 at d = 31 / 32 / 33, 0.72 / 0.80 at 512 / 515; rows with lo != hi: none, and 1.6 % at d = 515).  The trip shape
    3001 x 3001, d = 3 -- 3001 points on a sphere, the nearest about 0.036 rad away -- takes c = 20 (R@1 0.35, lo != hi in 0.07 % of the rows)"""
    rng = np.random.default_rng([n, m, d, 4])
    a = normalize(rng.standard_normal((n, d)))
    target = rng.permutation(m)[:n].astype(np.int32)
    b = normalize(rng.standard_normal((m, d)))
    b[target] = normalize(c * a + normalize(rng.standard_normal((n, d))))
    lo, hi, _, _ = bounds(a, b, target)
    assert (lo != hi).mean() <= 0.05
    got = launch(a, b, target)
    pos = got[:, 0] + got[:, 1]
    r1 = float((pos < 1).mean())
    print(f"n={n} m={m} d={d}: R@1 {r1:.3f}, rows with lo != hi {(lo != hi).mean():.4f}, out of bounds {int(((pos < lo) | (pos > hi)).sum())}")
    assert 0.0 < r1 < 0.9
    assert ((pos >= lo) & (pos <= hi)).all(), f"{int(((pos < lo) | (pos > hi)).sum())} rows outside [lo, hi]"
    if n == m:                                                                # the diagonal default equals an explicit arange
        inv = np.argsort(target)
        assert np.array_equal(launch(a[inv], b), launch(a[inv], b, np.arange(m, dtype=np.int32)))


def test_two_launches_give_the_same_bits():
    a, b, target, keep, rg, cg, _ = dyadic_case(131, 131, 515, True)
    rng = np.random.default_rng(9)
    a2, b2 = normalize(rng.standard_normal((131, 515))), normalize(rng.standard_normal((131, 515)))
    assert np.array_equal(launch(a2, b2, target, keep, rg, cg), launch(a2, b2, target, keep, rg, cg))


@pytest.mark.parametrize("n,m,d", ((65, 131, 33), (131, 65, 515)))
def test_strided_views_of_wider_buffers(n, m, d):
    from octcubem_amd import ops
    a, b, target, keep, rg, cg, want = dyadic_case(n, m, d, True)
    rng = np.random.default_rng(5)
    wa = (rng.integers(-2, 3, size=(2 * n, d + 5)) / 4).astype(np.float32)
    wb = (rng.integers(-2, 3, size=(m, d + 3)) / 4).astype(np.float32)
    wa[::2, 3:3 + d] = a
    wb[:, 1:1 + d] = b
    va, vb = dev(wa)[::2, 3:3 + d], dev(wb)[:, 1:1 + d]
    assert not va.is_contiguous() and va.stride(0) == 2 * (d + 5) and vb.stride(0) == d + 3
    got = ops.retrieval_ranks(va, vb, dev(target), dev(keep).bool(), dev(rg), dev(cg)).cpu().numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k", range(G.N_GOLDEN))
def test_public_functions_equal_the_golden_fixture(k):
    p = {key: (v if isinstance(v, tuple) else torch.from_numpy(np.asarray(v)).to(DEV)) for key, v in G.golden_problem(k).items()}
    from octcubem_amd import coem
    if k == 0:
        got = coem.get_metrics(p["image"], p["text"], p["logit_scale"])
    elif k == 1:
        got = coem.get_metrics_3modalities(p["image"], p["text1"], p["text2"], p["logit_scale"], p["logit_scale1"], p["logit_scale2"],
                                           p["w1"], p["w2"])
    else:
        got = coem.get_corrected_metrics(p["image"], p["text"], p["logit_scale"], list(p["labels"]))
    G.assert_close(got, G.expected(G.golden(), k))


def test_bad_arguments_raise_before_any_launch():
    from octcubem_amd import ops
    a, b, target, keep, rg, cg, _ = dyadic_case(65, 65, 32, True)
    da, db, dt, dk, drg, dcg = dev(a), dev(b), dev(target), dev(keep), dev(rg), dev(cg)
    for bad_value in (float("nan"), float("inf"), float("-inf")):
        bad = da.clone()
        bad[7, 1] = bad_value
        with pytest.raises(ValueError, match="a contains non-finite"):
            ops.retrieval_ranks(bad, db)
        with pytest.raises(ValueError, match="b contains non-finite"):
            ops.retrieval_ranks(da, bad)
    with pytest.raises(TypeError, match="a must be float32"):
        ops.retrieval_ranks(da.double(), db)
    with pytest.raises(TypeError, match="b must be float32"):
        ops.retrieval_ranks(da, db.half())
    with pytest.raises(TypeError, match="target must be int32"):
        ops.retrieval_ranks(da, db, dt.long())
    with pytest.raises(TypeError, match="keep must be bool or uint8"):
        ops.retrieval_ranks(da, db, dt, dk.int())
    with pytest.raises(RuntimeError, match="a must be a GPU tensor"):
        ops.retrieval_ranks(torch.from_numpy(a), db)
    with pytest.raises(RuntimeError, match="target must be a GPU tensor"):
        ops.retrieval_ranks(da, db, torch.from_numpy(target))
    with pytest.raises(ValueError, match="n == m"):
        ops.retrieval_ranks(da[:64], db)
    with pytest.raises(ValueError, match="together"):
        ops.retrieval_ranks(da, db, row_group=drg)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.retrieval_ranks(da.t().contiguous().t(), db)
    with pytest.raises(ValueError, match="expected a"):
        ops.retrieval_ranks(da, db[:, :31])
    with pytest.raises(ValueError, match="empty"):
        ops.retrieval_ranks(da[:0], db[:0])
    with pytest.raises(ValueError, match=r"target must lie in"):
        ops.retrieval_ranks(da, db, torch.full_like(dt, 65))
    k2 = dk.clone()
    k2[int(target[3])] = 0
    with pytest.raises(ValueError, match="kept"):
        ops.retrieval_ranks(da, db, dt, k2)


def test_the_entry_point_refuses():
    from octcubem_amd import _lib
    a = torch.zeros(4, 8, device=DEV)
    b = torch.zeros(6, 8, device=DEV)
    out = torch.zeros(4, 4, dtype=torch.int32, device=DEV)
    tg = torch.zeros(4, dtype=torch.int32, device=DEV)
    g4, g6 = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(6, dtype=torch.int32, device=DEV)
    fn = _lib.load().octmae_retrieval_ranks
    A, B, O, T = a.data_ptr(), b.data_ptr(), out.data_ptr(), tg.data_ptr()
    for args in ((None, 8, B, 8, T, None, None, None, O, 4, 6, 8), (A, 8, None, 8, T, None, None, None, O, 4, 6, 8),
                 (A, 8, B, 8, T, None, None, None, None, 4, 6, 8), (A, 8, B, 8, T, None, None, None, O, 0, 6, 8),
                 (A, 8, B, 8, T, None, None, None, O, 4, 0, 8), (A, 8, B, 8, T, None, None, None, O, 4, 6, 0),
                 (A, 7, B, 8, T, None, None, None, O, 4, 6, 8), (A, 8, B, 7, T, None, None, None, O, 4, 6, 8),
                 (A, 8, B, 8, T, None, None, None, O, 4, 2 ** 31, 8), (A, 8, B, 8, None, None, None, None, O, 4, 6, 8),
                 (A, 8, B, 8, T, None, g4.data_ptr(), None, O, 4, 6, 8), (A, 8, B, 8, T, None, None, g6.data_ptr(), O, 4, 6, 8)):
        assert fn(*args, None) == -2, args
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0
    keep = torch.ones(6, dtype=torch.uint8, device=DEV)
    keep[0] = 0                                                               # the target column is not kept
    assert fn(A, 8, B, 8, T, keep.data_ptr(), None, None, O, 4, 6, 8, None) == -2
    tg[2] = 6                                                                 # no column of b
    assert fn(A, 8, B, 8, T, None, None, None, O, 4, 6, 8, None) == -2
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0


def test_retrieval_ranks_ignore_autocast():
    from octcubem_amd import ops
    a, b, target, keep, rg, cg, want = dyadic_case(65, 65, 32, True)
    with torch.autocast("cuda", dtype=torch.float16):
        got = ops.retrieval_ranks(dev(a), dev(b), dev(target), dev(keep), dev(rg), dev(cg))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)


def test_launch_is_accounted_with_its_flops():
    from octcubem_amd import ops
    a, b, *_ = dyadic_case(65, 65, 32, False)
    seen = []
    prev = ops.KTIMER
    ops.KTIMER = types.SimpleNamespace(launch=lambda kind, flops, nbytes, fn, exec_flops=None: (seen.append((kind, flops)), fn()))
    try:
        ops.retrieval_ranks(dev(a), dev(b))
    finally:
        ops.KTIMER = prev
    assert seen == [("retrieval_ranks", 2.0 * 65 * 65 * 32)]


# ---------------------------------------------------------------------------------------------- end to end
BATCHES = (5, 5, 3)


def tiny_clip(seed):
    from octcubem_amd import coem, models_vit, models_vit_st
    torch.manual_seed(seed)
    kw = dict(mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    m3 = models_vit_st.VisionTransformer(num_frames=6, t_patch_size=3, img_size=64, patch_size=16, in_chans=1, num_classes=64, embed_dim=128,
                                         depth=2, num_heads=2, sep_pos_embed=True, cls_embed=True, global_pool=True, dropout=0.0, **kw)
    m2 = models_vit.VisionTransformer(img_size=64, patch_size=16, in_chans=3, num_classes=64, embed_dim=128, depth=2, num_heads=2,
                                      qkv_bias=True, global_pool=True, **kw)
    for m in (m3, m2):
        torch.nn.init.normal_(m.head.weight, std=0.2)                         # a projection that spreads the samples
    return coem.CustomTextCLIP(m3, m2).to(DEV)


def val_loader():
    g = torch.Generator().manual_seed(8)
    n = sum(BATCHES)
    vol = torch.rand(n, 1, 6, 64, 64, generator=g) * torch.linspace(0.2, 3.0, n).view(n, 1, 1, 1, 1)
    ir = torch.randn(n, 3, 64, 64, generator=g) + torch.linspace(-1.5, 1.5, n).view(n, 1, 1, 1)
    out, i = [], 0
    for bsz in BATCHES:
        out.append((vol[i:i + bsz], ir[i:i + bsz]))
        i += bsz
    return out


def test_evaluate_end_to_end(tmp_path):
    from octcubem_amd import coem
    model = tiny_clip(21)
    loader = val_loader()
    assert [b[0].shape[0] for b in loader] == list(BATCHES)
    data = {"val": types.SimpleNamespace(dataloader=loader)}
    scalars = []
    tb = types.SimpleNamespace(add_scalar=lambda name, val, step: scalars.append((name, val, step)))
    args = types.SimpleNamespace(device=DEV, val_frequency=1, epochs=4, save_logs=True, checkpoint_path=str(tmp_path),
                                 save_retrieval_results=True, multimodal_type="default", return_metainfo=False, correct_label=0)
    got = coem.evaluate(model, data, 2, args, tb_writer=tb)
    assert not model.training and got["epoch"] == 2 and got["num_samples"] == 13 and len(got) == 13
    # the same features, batch by batch
    feats, loss = [], 0.0
    with torch.no_grad():
        for vol, ir in loader:
            fi, ft, ls = model(vol.to(DEV), ir.to(DEV))
            fi64, ft64 = fi.double().cpu(), ft.double().cpu()
            logits = float(ls) * fi64 @ ft64.T
            tg = torch.arange(fi.shape[0])
            loss += float((torch.nn.functional.cross_entropy(logits, tg) + torch.nn.functional.cross_entropy(logits.T, tg)) / 2) * fi.shape[0]
            feats.append((fi.cpu().numpy(), ft.cpu().numpy()))
    print(f"val_loss {got['val_loss']!r} / {loss / 13!r}")
    assert abs(got["val_loss"] - loss / 13) <= 1e-6
    fi, ft = np.concatenate([f[0] for f in feats]), np.concatenate([f[1] for f in feats])
    diag = np.arange(13)
    for name, x, y in (("image_to_text", fi, ft), ("text_to_image", ft, fi)):
        lo, hi, s, _ = bounds(x, y, diag)
        assert np.array_equal(lo, hi), f"{name}: the inputs leave a rank open within the f32 bound"
        assert np.array_equal(lo, R.stable_preds(s))
        for key, v in R.rank_metrics(name, lo).items():
            assert got[key] == v, (key, got[key], v)
    # the files
    lines = open(os.path.join(str(tmp_path), "results.jsonl")).read().splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == got
    assert sorted(scalars) == sorted((f"val/{k}", v, 2) for k, v in got.items())
    z = np.load(os.path.join(str(tmp_path), "retrieval_results_2.npz"))
    assert set(z.files) == {"image_features", "text_features", "logit_scale"} and z["logit_scale"].shape == (3,)
    assert z["image_features"].shape == (13, 64) and np.array_equal(z["image_features"], fi) and np.array_equal(z["text_features"], ft)
    # the same inside autocast; not due -> {}
    args.save_logs = False
    with torch.autocast("cuda", dtype=torch.float16):
        again = coem.evaluate(model, data, 4, args)
    assert again["epoch"] == 4 and abs(again["val_loss"] - got["val_loss"]) <= 1e-6
    assert {k: v for k, v in again.items() if k not in ("epoch", "val_loss")} == {k: v for k, v in got.items() if k not in ("epoch", "val_loss")}
    args.val_frequency = 3
    assert coem.evaluate(model, data, 2, args) == {}
    # duplicate-report targets: BCE against the same-feature matrix
    args.val_frequency, args.correct_label = 1, 1
    bce = coem.evaluate(model, data, 1, args)
    want = 0.0
    for (x, y) in feats:
        logits = float(model.logit_scale.exp()) * torch.from_numpy(x).double() @ torch.from_numpy(y).double().T
        f = torch.nn.functional.binary_cross_entropy_with_logits
        want += float((f(logits, torch.eye(len(x), dtype=torch.float64)) + f(logits.T, torch.eye(len(x), dtype=torch.float64))) / 2) * len(x)
    print(f"val_loss with correct_label {bce['val_loss']!r} / {want / 13!r}")
    assert abs(bce["val_loss"] - want / 13) <= 1e-6 * max(1.0, want / 13)


# ---------------------------------------------------------------------------------------------- the half build
def half_build_cases():
    """What tests/f16_worker.py runs on the half-operand build."""
    for case in DYADIC_CASES:
        check_dyadic(*case)
    return {"passed": [list(c) for c in DYADIC_CASES]}


def start_children():
    """tests/conftest.py calls this once the collection holds a test of this module, before this process has touched the GPU;
    tests/children.py releases the worker when the GPU has room for it."""
    if os.path.exists(LIB_F16):
        children.spawn_f16_worker("retrieval_f16", "tests.test_gpu_retrieval:half_build_cases")


def test_half_build_runs_the_same_retrieval_kernel():
    """The entry point has no 16-bit operand: liboctmae_f16.so must give the same counts on every dyadic case."""
    assert os.path.exists(LIB_F16), "make -C octcubem_amd/csrc both"
    start_children()
    res = children.f16_worker_result("retrieval_f16")
    assert res["lib"] == "liboctmae_f16.so" and res["lp_is_f16"] is True
    assert res["passed"] == [list(c) for c in DYADIC_CASES], res
