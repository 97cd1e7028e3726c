"""CPU side of mixup / cutmix: the exported symbol and the argument errors of octmae_mix_batch (reported before any launch), the host
checks of ops.mix_batch's tables, the decision logic of octcubem_amd.mixup.Mixup on seeded streams -- checked as PROPERTIES of the rule,
not as values taken from the code under test -- and mixup_target against the restatement (tests/mix_ref.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from octcubem_amd import Mixup, _lib, mixup as M, ops
from tests import mix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_both_libraries_export_the_symbol_at_abi_20():
    assert _lib.expected_abi_version() >= 20 and "octmae_mix_batch" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "octmae_mix_batch")
    f16 = ctypes.CDLL(os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so"))
    assert hasattr(f16, "octmae_mix_batch") and f16.octmae_abi_version() == _lib.load().octmae_abi_version() == _lib.expected_abi_version()


def test_mix_batch_reports_argument_errors_without_a_gpu():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    q = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: every call below is refused before a launch

    def call(x=q, kind=q, lam=q, oml=q, box=q, B=4, S=3 * 8 * 8, H=8, W=8):
        return lib.octmae_mix_batch(x, kind, lam, oml, box, B, S, H, W, None)

    for null in ("x", "kind", "lam", "oml", "box"):
        assert call(**{null: None}) == -1, null
    for bad in (dict(B=3), dict(B=1), dict(B=0), dict(B=-2), dict(S=0), dict(S=-64), dict(H=0), dict(W=-8)):
        assert call(**bad) == -1, bad
    assert call(S=3 * 64 + 1) == -1 and call(S=100) == -1 and call(S=32) == -1      # H * W does not divide S / exceeds it
    assert call(x=q + 2) == -1                                                      # not a float pointer
    assert call(S=(1 << 30) + 64) == -2                                             # element offsets of a sample are 32-bit
    with pytest.raises(_lib.OctmaeError, match="bad argument"):
        _lib.call("octmae_mix_batch", None, None, None, None, None, 2, 4, 2, 2, None)
    # the kernel has no CPU form: CPU tensors are an error, not a fall-back
    with pytest.raises(RuntimeError):
        ops.mix_batch(torch.zeros(2, 1, 4, 4), [1, 1], [0.5, 0.5], [0.5, 0.5], np.zeros((2, 4)), 4, 4)


def test_host_tables_are_checked_before_the_upload():
    ok = dict(kind=[2, 0, 1, 2], lam=[1, 1, 0.25, 1], oml=[0, 0, 0.75, 0], box=[[0, 9, 0, 10], [-5, 99, 7, 3], [9, 1, 1, 0], [4, 4, 10, 10]])
    kind, lam, oml, box = ops.mix_tables(Bn=4, H=9, W=10, **ok)      # boxes of samples that do not cut are not looked at
    assert kind.dtype == np.int32 and lam.dtype == np.float32 and oml.dtype == np.float32 and box.dtype == np.int32 and box.shape == (4, 4)
    for bad in ([-1, 9, 0, 10], [0, 10, 0, 10], [5, 4, 0, 10], [0, 9, -1, 10], [0, 9, 0, 11], [0, 9, 6, 5]):
        with pytest.raises(ValueError, match="box"):
            ops.mix_tables(Bn=4, H=9, W=10, **dict(ok, box=[bad] + ok["box"][1:]))
    with pytest.raises(ValueError, match="kind"):
        ops.mix_tables(Bn=4, H=9, W=10, **dict(ok, kind=[3, 0, 1, 2]))
    for short in ("kind", "lam", "oml", "box"):
        with pytest.raises(ValueError, match="entries"):
            ops.mix_tables(Bn=4, H=9, W=10, **dict(ok, **{short: ok[short][:3]}))
    # bytes: pair (0, 3) cuts 90 + 0 elements per plane, pair (1, 2) mixes one side; 3 planes of [9, 10]
    assert ops.mix_bytes(kind, box, 270, 9, 10) == 4.0 * (2 * (270 + 0) + (2 * 270 + 270))


# ---- decisions --------------------------------------------------------------------------------------------------------
def decisions(n_calls, B, H, W, seed, **kw):
    m = Mixup(num_classes=7, rng=np.random.RandomState(seed), **kw)
    return [m.decide(B, H, W) for _ in range(n_calls)]


@pytest.mark.parametrize("mode", ["batch", "elem", "pair"])
def test_boxes_lie_inside_the_image_and_corrected_lam_is_the_uncut_share(mode):
    H, W, B = 37, 50, 6
    seen_cut = 0
    for p in decisions(200, B, H, W, 11, mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, prob=0.9):
        kind, box = p["kind"], p["box"]
        lam = np.broadcast_to(np.asarray(p["lam"]), (B,))
        cut = np.broadcast_to(np.asarray(p["use_cutmix"]), (B,))
        assert set(kind.tolist()) <= {0, 1, 2}
        for i in range(B):
            yl, yh, xl, xh = (int(v) for v in box[i])
            if kind[i] == M.KIND_CUTMIX:
                seen_cut += 1
                assert cut[i] and 0 <= yl <= yh <= H and 0 <= xl <= xh <= W
                want = 1.0 - ((yh - yl) * (xh - xl)) / float(H * W)                 # exact in double
                assert lam[i] == (want if mode == "batch" else np.float32(want))    # elem / pair keep their lams in float32
            elif kind[i] == M.KIND_MIXUP:
                assert not cut[i] and p["lam32"][i] == np.float32(lam[i]) and lam[i] != 1.0
                oml = np.float32(1.0 - lam[i]) if mode == "batch" else np.float32(1) - np.float32(lam[i])
                assert p["oml32"][i] == oml
            else:
                assert lam[i] == 1.0
        ops.mix_tables(kind, p["lam32"], p["oml32"], box, B, H, W)                   # and the tables pass the launch's own check
    assert seen_cut > 100


def test_uncorrected_lam_is_the_drawn_one():
    for p in decisions(50, 4, 32, 32, 5, mixup_alpha=0.0, cutmix_alpha=1.0, correct_lam=False):
        assert p["use_cutmix"] is True and p["lam"] == p["lam_mix"] and (p["kind"] == M.KIND_CUTMIX).all()
        # the box of rand_bbox: sides int(H * sqrt(1 - lam)) before clipping, so never larger
        cut = int(32 * np.sqrt(1 - p["lam_mix"]))
        yl, yh, xl, xh = p["box"][0]
        assert yh - yl <= cut and xh - xl <= cut and (p["box"] == p["box"][0]).all()


@pytest.mark.parametrize("mode", ["batch", "elem", "pair"])
def test_closed_gate_means_lam_one_and_nothing_to_do(mode):
    for p in decisions(20, 6, 16, 16, 3, mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, prob=0.0):
        assert (np.asarray(p["lam"]) == 1.0).all() and (np.asarray(p["lam_mix"]) == 1.0).all() and not p["kind"].any()
    m = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, rng=np.random.RandomState(0))
    m.mixup_enabled = False
    p = m.decide(4, 8, 8)
    assert (np.asarray(p["lam"]) == 1.0).all() and not p["kind"].any()
    # half-open gate: the untouched samples are exactly those with lam == 1
    for p in decisions(50, 6, 16, 16, 4, mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, prob=0.5):
        lam_mix = np.broadcast_to(np.asarray(p["lam_mix"]), (6,))
        assert ((p["kind"] == M.KIND_NONE) == (lam_mix == 1.0)).all()


@pytest.mark.parametrize("mode", ["batch", "elem", "pair"])
def test_cutmix_minmax_forces_cutmix_and_the_corrected_lam(mode):
    H, W = 40, 30
    for p in decisions(100, 4, H, W, 9, mixup_alpha=0.0, cutmix_alpha=0.0, cutmix_minmax=(0.2, 0.8), correct_lam=False, mode=mode):
        assert (p["kind"] == M.KIND_CUTMIX).all() and np.asarray(p["use_cutmix"]).all()
        lam = np.broadcast_to(np.asarray(p["lam"]), (4,))
        for i in range(4):
            yl, yh, xl, xh = (int(v) for v in p["box"][i])
            assert int(H * 0.2) <= yh - yl < int(H * 0.8) and int(W * 0.2) <= xh - xl < int(W * 0.8)
            assert 0 <= yl and yh <= H and 0 <= xl and xh <= W
            want = 1.0 - ((yh - yl) * (xh - xl)) / float(H * W)
            assert lam[i] == (want if mode == "batch" else np.float32(want))
    assert Mixup(cutmix_minmax=(0.2, 0.8)).cutmix_alpha == 1.0
    with pytest.raises(ValueError):
        Mixup(cutmix_minmax=(0.2, 0.5, 0.8))


def test_pair_mode_mirrors_its_decisions_and_elem_mode_does_not():
    mirrored = 0
    for p in decisions(50, 8, 20, 24, 21, mixup_alpha=0.8, cutmix_alpha=1.0, mode="pair"):
        for k in ("kind", "lam32", "oml32", "box", "lam", "lam_mix", "use_cutmix"):
            assert np.array_equal(p[k], p[k][::-1]), k
        assert len(p["lam"]) == 8
    for p in decisions(50, 8, 20, 24, 21, mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem"):
        mirrored += int(np.array_equal(p["lam"], p["lam"][::-1]))
    assert mirrored == 0
    # batch mode: one decision for all
    for p in decisions(20, 8, 20, 24, 21, mixup_alpha=0.8, cutmix_alpha=1.0, mode="batch"):
        assert isinstance(p["lam"], float) and len(set(p["kind"].tolist())) == 1 and (p["box"] == p["box"][0]).all()


def test_switch_prob_chooses_between_the_two_alphas():
    n = 4000
    ps = decisions(n, 2, 16, 16, 2, mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.25)
    share = sum(bool(p["use_cutmix"]) for p in ps) / n
    assert abs(share - 0.25) < 5 * np.sqrt(0.25 * 0.75 / n)                     # 5 sigma of a binomial share
    assert not any(p["use_cutmix"] for p in decisions(50, 2, 16, 16, 2, mixup_alpha=0.8, cutmix_alpha=0.0))
    assert all(p["use_cutmix"] for p in decisions(50, 2, 16, 16, 2, mixup_alpha=0.0, cutmix_alpha=1.0))
    with pytest.raises(ValueError):
        Mixup(mixup_alpha=0.0, cutmix_alpha=0.0).decide(2, 8, 8)


def test_mean_lam_of_alpha_one_is_one_half():
    """Beta(1, 1) is uniform: mean 1/2, standard deviation 1/sqrt(12); over 20 000 draws the standard error of the mean is 0.002, so
    0.01 is a 5 sigma band."""
    m = Mixup(mixup_alpha=1.0, cutmix_alpha=0.0, mode="elem", rng=np.random.RandomState(1234))
    lam = np.concatenate([m.decide(200, 8, 8)["lam"] for _ in range(100)])
    assert lam.shape == (20000,) and abs(float(lam.astype(np.float64).mean()) - 0.5) < 0.01
    m = Mixup(mixup_alpha=1.0, cutmix_alpha=0.0, mode="batch", rng=np.random.RandomState(4321))
    lam = np.array([m.decide(2, 8, 8)["lam"] for _ in range(20000)])
    assert abs(float(lam.mean()) - 0.5) < 0.01


def test_global_numpy_state_is_the_default_stream():
    np.random.seed(77)
    a = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem").decide(6, 12, 12)
    b = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", rng=np.random.RandomState(77)).decide(6, 12, 12)
    for k in ("kind", "lam32", "oml32", "box", "lam"):
        assert np.array_equal(a[k], b[k]), k


def test_bad_inputs_raise_value_error():
    m = Mixup(num_classes=3, rng=np.random.RandomState(0))
    t = torch.zeros(4, dtype=torch.long)
    for x in (torch.zeros(4, 1, 8, 8),                               # not on the GPU
              torch.zeros(3, 1, 8, 8),                               # odd batch
              torch.zeros(4, 1, 8, 8, dtype=torch.float16),          # dtype
              torch.zeros(4, 8, 8), torch.zeros(4, 1, 1, 2, 8, 8),   # rank
              np.zeros((4, 1, 8, 8), dtype=np.float32)):
        with pytest.raises(ValueError):
            m(x, t)
    with pytest.raises(ValueError):
        m.decide(3, 8, 8)
    with pytest.raises(ValueError):
        Mixup(mode="sample")
    assert m.last_params is None


def test_decisions_match_timm_draw_for_draw():
    timm_mixup = pytest.importorskip("timm.data.mixup", reason="timm is not installed: stream equality with timm is intended but unverified")
    H, W, B = 32, 48, 6
    for mode in ("batch", "elem", "pair"):
        for kw in (dict(mixup_alpha=0.8, cutmix_alpha=1.0), dict(mixup_alpha=0.0, cutmix_alpha=1.0, correct_lam=False),
                   dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=(0.2, 0.8), prob=0.7)):
            np.random.seed(5)
            theirs = timm_mixup.Mixup(mode=mode, num_classes=7, **kw)
            ours = Mixup(mode=mode, num_classes=7, rng=np.random.RandomState(5), **kw)
            for _ in range(10):
                x = torch.arange(B * 2 * H * W, dtype=torch.float32).reshape(B, 2, H, W)
                lam = {"batch": theirs._mix_batch, "elem": theirs._mix_elem, "pair": theirs._mix_pair}[mode](x)
                p = ours.decide(B, H, W)
                got = p["lam"] if mode == "batch" else torch.from_numpy(p["lam"]).unsqueeze(1)
                assert (lam == got) if mode == "batch" else torch.equal(lam, got)
                assert torch.equal(x, R.apply_params(torch.arange(B * 2 * H * W, dtype=torch.float32).reshape(B, 2, H, W),
                                                     torch.zeros(B, dtype=torch.long), p, 7, 0.1)[0])


# ---- targets -----------------------------------------------------------------------------------------------------------
def test_mixup_target_equals_the_restatement_and_is_a_distribution():
    g = torch.Generator().manual_seed(0)
    t = torch.randint(0, 7, (6,), generator=g)
    lam_vec = np.array([0.3, 1.0, 0.0, 0.6888889, 0.5, 1.0 - 2.0 ** -24], dtype=np.float32)
    for lam in (0.3, 1.0, 0.0, 0.7123456789, lam_vec):
        for s in (0.0, 0.1):
            dev_lam = lam if isinstance(lam, float) else torch.from_numpy(lam).unsqueeze(1)
            got = M.mixup_target(t, 7, dev_lam, s)
            assert got.dtype == torch.float32 and got.shape == (6, 7)
            assert torch.equal(got, R.mixup_target(t, 7, lam, s))
            assert float((got.sum(-1) - 1).abs().max()) <= 1e-6 and float(got.min()) >= 0.0
    # the rule itself, in double, on one row: classes a != b, lam, smoothing
    y = M.mixup_target(torch.tensor([2, 5]), 7, 0.25, 0.1)
    off, on = 0.1 / 7, 1 - 0.1 + 0.1 / 7
    assert abs(float(y[0, 2]) - (on * 0.25 + off * 0.75)) <= 1e-6 and abs(float(y[0, 5]) - (off * 0.25 + on * 0.75)) <= 1e-6
    assert abs(float(y[0, 0]) - off) <= 1e-6 and torch.equal(y[1], M.mixup_target(torch.tensor([5, 2]), 7, 0.25, 0.1)[0])
