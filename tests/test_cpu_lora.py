"""Low-rank adapters without a GPU: the float64 references and bounds of tests/lora_ref.py hold for the stated arithmetic in another
order of additions and catch planted faults; the C ABI of csrc/lora.hip is bound in both libraries under ABI 35, answers its plan and
workspace queries and refuses bad arguments before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import gemm_elem as GE
from tests import lora_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
LPS = [torch.bfloat16, torch.float16]
# (O, I, r, M): one rank, a rank that is no multiple of 16 (two column tiles), square layers (the swap fault), several chunks of 32 rows
SHAPES = [(96, 32, 1, 17), (64, 64, 4, 65), (64, 64, 17, 97), (128, 128, 64, 33)]


def _draw(O, I, r, M, lp, seed, pad=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, I), generator=g).to(lp)
    dy = (0.1 * torch.randn((M, O), generator=g)).to(lp)
    A, B = torch.randn((r, I), generator=g) / I ** 0.5, 0.3 * torch.randn((O, r), generator=g)
    A_lp, B_lp = LR.pad_operands(A, B, lp)
    rp = A_lp.shape[0]
    if pad and rp > r:
        A_lp[r:] = 1.0
        B_lp[:, r:] = 1.0
    gA0, gB0 = torch.randn((rp, I), generator=g), torch.randn((O, rp), generator=g)
    return x, dy, A_lp, B_lp, gA0, gB0


def _worst(lp, shape, fault=None, pad=False, seed=0):
    O, I, r, M = shape
    s = 0.5
    x, dy, A_lp, B_lp, gA0, gB0 = _draw(O, I, r, M, lp, 100 + seed, pad)
    gA, gB = LR.emulate_wgrad(x, dy, A_lp, B_lp, s, gA0, gB0, lp, chunk=32, seed=seed, fault=fault)
    (ra, ba), (rb, bb) = LR.wgrad_ref(x, dy, A_lp, B_lp, s, r, gA0[:r], gB0[:, :r], GE.LP_U[lp], torch.finfo(lp).tiny)
    wa, _, same_a = LR.check(gA, ra, ba, gA0, r, 0)
    wb, _, same_b = LR.check(gB, rb, bb, gB0, r, 1)
    return wa, wb, same_a and same_b


@pytest.mark.parametrize("lp", LPS, ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_stated_arithmetic_in_another_order_stays_inside_the_bounds(lp, shape):
    for seed in range(3):
        wa, wb, same = _worst(lp, shape, seed=seed)
        print(f"{shape} {lp}: worst gA {wa:.3f}, gB {wb:.3f}")
        assert wa <= 1.0 and wb <= 1.0 and same


@pytest.mark.parametrize("lp", LPS, ids=["bf16", "f16"])
@pytest.mark.parametrize("fault", ["row", "chunk", "rank", "scale", "swap"])
def test_planted_faults_leave_the_bounds(lp, fault):
    for shape in SHAPES[1:]:                          # the square layers
        wa, wb, _ = _worst(lp, shape, fault=fault)
        print(f"{fault} {shape} {lp}: worst gA {wa:.1f}, gB {wb:.1f}")
        assert wa > 1.0 and wb > 1.0, (fault, shape, wa, wb)


@pytest.mark.parametrize("lp", LPS, ids=["bf16", "f16"])
def test_padding_that_is_not_zero_shows_in_the_rows_behind_the_rank(lp):
    for shape in SHAPES[:3]:                          # r < rp
        assert _worst(lp, shape)[2]
        assert not _worst(lp, shape, pad=True)[2]


@pytest.mark.parametrize("O,I,r", [(96, 32, 1), (64, 256, 16), (256, 64, 17), (128, 128, 64)])
def test_merge_by_fused_multiply_adds_stays_inside_its_bound(O, I, r):
    g = torch.Generator().manual_seed(O + r)
    W, A, B = 0.02 * torch.randn((O, I), generator=g), torch.randn((r, I), generator=g) / I ** 0.5, 0.3 * torch.randn((O, r), generator=g)
    s = 0.5                                           # never 1: a forgotten scale must show
    Wn, An, Bn = W.numpy(), A.numpy(), B.numpy()
    delta = np.zeros((O, I), dtype=np.float32)
    for k in range(r):
        delta = GE._fma(Bn[:, k:k + 1], An[k:k + 1, :], delta)
    v = torch.from_numpy(GE._fma(np.float32(s), delta, Wn))
    ref, bound = LR.merge_ref(W, A, B, s)
    w, _ = GE.worst(v, ref, bound)
    assert w <= 1.0, w
    # a forgotten scale and a dropped rank do not stay inside
    assert GE.worst(torch.from_numpy(GE._fma(np.float32(1.0), delta, Wn)), ref, bound)[0] > 1.0
    short = np.zeros((O, I), dtype=np.float32)
    for k in range(r - 1):
        short = GE._fma(Bn[:, k:k + 1], An[k:k + 1, :], short)
    assert GE.worst(torch.from_numpy(GE._fma(np.float32(s), short, Wn)), ref, bound)[0] > 1.0


NAMES = ("octmae_lora_merge", "octmae_lora_wgrad", "octmae_lora_plan", "octmae_lora_ws_bytes")


def test_bindings_history_and_both_libraries():
    from octcubem_amd import _lib
    for name in NAMES:
        assert name in _lib.SIGNATURES
    assert not any(name in _lib.RESTYPES for name in NAMES) and len(_lib.SIGNATURES["octmae_lora_ws_bytes"]) == 5
    assert len(_lib.SIGNATURES["octmae_lora_merge"]) == 12 and len(_lib.SIGNATURES["octmae_lora_wgrad"]) == 18
    assert _lib.SIGNATURES["octmae_lora_wgrad"][16] is ctypes.c_longlong                          # the workspace size
    with open(os.path.join(ROOT, "include", "octmae.h")) as f:
        hdr = f.read()
    history = hdr[:hdr.index("#define OCTMAE_ABI_VERSION")]
    assert all(name in history for name in NAMES) and "csrc/lora.hip" in history
    assert _lib.expected_abi_version() == 35
    with open(os.path.join(ROOT, "octcubem_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert "lora.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert re.search(r"^\$\(O\)lora\.o:.*\n.*\n.*-ffp-contract=off", mk, re.M)
    for lib in (_lib.load(), ctypes.CDLL(os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so"))):
        assert all(hasattr(lib, name) for name in NAMES)
        assert lib.octmae_abi_version() == 35


def test_plan_and_workspace_answer_without_a_gpu():
    from octcubem_amd import ops
    for M, I, O, rp in [(1, 32, 96, 16), (65, 64, 192, 16), (5121, 1024, 3072, 16), (4 * 5121, 1024, 4096, 32), (32 * 1281, 4096, 1024, 64)]:
        chunk, nchunks, tx, ty = ops.lora_plan(M, I, O, rp)
        assert chunk % 32 == 0 and chunk >= 256 and (nchunks - 1) * chunk < M <= nchunks * chunk
        assert tx == -(-I // 64) and ty == -(-O // 64) and nchunks <= 65535
        ws = ops.lora_ws_bytes(M, I, O, rp)
        # T, U, the transposed B and one fp32 slab per chunk, each part rounded up to 256 bytes
        parts = 2 * (-(-M * rp * 2 // 256) * 256) + -(-rp * O * 2 // 256) * 256
        assert ws == parts + nchunks * (I + O) * rp * 4
    assert ops.lora_plan(5121, 1024, 3072, 16)[1] > 1 and ops.lora_plan(256, 64, 64, 16)[:2] == (256, 1)
    assert ops.lora_plan(257, 64, 64, 16)[1] == 2
    lib = __import__("octcubem_amd._lib", fromlist=["load"]).load()
    out = (ctypes.c_int * 4)()
    for bad in [(0, 64, 64, 16), (8, 60, 64, 16), (8, 64, 0, 16), (8, 64, 64, 0), (8, 64, 64, 8), (8, 64, 64, 80)]:
        assert lib.octmae_lora_plan(*bad, out) == -1 and lib.octmae_lora_ws_bytes(*bad, ctypes.byref(ctypes.c_longlong())) == -1, bad
    assert lib.octmae_lora_plan(8, 64, 64, 16, None) == -1 and lib.octmae_lora_ws_bytes(8, 64, 64, 16, None) == -1


def test_entry_points_report_argument_errors_without_a_gpu():
    from octcubem_amd import _lib, ops
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    q = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned; never dereferenced: every call below is refused before a launch
    big = 1 << 40

    def merge(W=q, A=q, B=q, s=2.0, O=64, I=64, r=8, out=q, f32=0, A_lp=q, B_lp=q):
        return lib.octmae_lora_merge(W, A, B, s, O, I, r, out, f32, A_lp, B_lp, None)

    def wgrad(X=q, ldx=64, dY=q, ldy=64, A_lp=q, B_lp=q, s=2.0, M=16, I=64, O=64, r=8, gA=q, lda=64, gB=q, ldb=8, ws=q, ws_bytes=big):
        return lib.octmae_lora_wgrad(X, ldx, dY, ldy, A_lp, B_lp, s, M, I, O, r, gA, lda, gB, ldb, ws, ws_bytes, None)

    for fn in (merge, wgrad):
        for bad in (dict(r=0), dict(r=-1), dict(r=65), dict(I=0), dict(O=0), dict(I=60), dict(O=68), dict(I=-64)):
            assert fn(**bad) == -1, (fn.__name__, bad)
    for null in ("W", "A", "B", "out"):
        assert merge(**{null: None}) == -1, null
    assert merge(W=q + 4) == -1 and merge(A=q + 8) == -1 and merge(B=q + 2) == -1 and merge(out=q + 8) == -1
    assert merge(A_lp=q + 1) == -1 and merge(B_lp=q + 1) == -1 and merge(f32=2) == -1 and merge(s=float("nan")) == -1
    for null in ("X", "dY", "A_lp", "B_lp", "ws"):
        assert wgrad(**{null: None}) == -1, null
    assert wgrad(gA=None, gB=None) == -1
    assert wgrad(X=q + 8) == -1 and wgrad(dY=q + 2) == -1 and wgrad(A_lp=q + 8) == -1 and wgrad(B_lp=q + 4) == -1 and wgrad(ws=q + 8) == -1
    assert wgrad(gA=q + 2) == -1 and wgrad(gB=q + 1) == -1
    assert wgrad(ldx=56) == -1 and wgrad(ldx=68) == -1 and wgrad(ldy=60) == -1 and wgrad(lda=63) == -1 and wgrad(ldb=7) == -1
    assert wgrad(M=0) == -1 and wgrad(ws_bytes=ops.lora_ws_bytes(16, 64, 64, 16) - 1) == -1 and wgrad(s=float("nan")) == -1
    with pytest.raises(_lib.OctmaeError, match="bad argument"):
        _lib.call("octmae_lora_merge", None, None, None, 1.0, 64, 64, 8, None, 0, None, None, None)
    # no CPU form, and the Python wrappers refuse first, naming the argument
    with pytest.raises(RuntimeError, match="W"):
        ops.lora_merge(torch.zeros(64, 64), torch.zeros(8, 64), torch.zeros(64, 8), 2.0, torch.zeros(64, 64))
    with pytest.raises(RuntimeError, match="x"):
        ops.lora_wgrad(torch.zeros(16, 64, dtype=ops.BF16), torch.zeros(16, 64, dtype=ops.BF16), torch.zeros(16, 64, dtype=ops.BF16),
                       torch.zeros(64, 16, dtype=ops.BF16), 2.0, 8, torch.zeros(8, 64), torch.zeros(64, 8))


# ------------------------------------------------------------------------------------------------ the public module, without a GPU
def _vit(depth=3, C=64):
    from functools import partial
    from octcubem_amd import models_vit
    return models_vit.VisionTransformer(img_size=32, patch_size=16, in_chans=3, num_classes=8, embed_dim=C, depth=depth, num_heads=2,
                                        mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), global_pool=True)


def test_attach_names_requires_grad_and_layer_decay_scales():
    import octcubem_amd
    from octcubem_amd import lora, lr_decay, video_vit
    assert octcubem_amd.lora is lora and "lora" in octcubem_amd.__all__
    m = _vit()
    keys_before = set(m.state_dict())
    new = lora.attach(m, rank=4, alpha=8, targets=("qkv", "fc2"), blocks=[0, 2])
    names = {n for n, _ in m.named_parameters()}
    added = names - keys_before
    assert added == {f"blocks.{i}.lora.{t}_{w}" for i in (0, 2) for t in ("qkv", "fc2") for w in "AB"} and len(new) == 8
    P = dict(m.named_parameters())
    assert tuple(P["blocks.0.lora.qkv_A"].shape) == (4, 64) and tuple(P["blocks.0.lora.qkv_B"].shape) == (192, 4)
    assert tuple(P["blocks.2.lora.fc2_A"].shape) == (4, 256) and tuple(P["blocks.2.lora.fc2_B"].shape) == (64, 4)
    assert float(P["blocks.0.lora.qkv_B"].detach().abs().max()) == 0.0
    bound = 1.0 / 64 ** 0.5                                   # kaiming-uniform with a = sqrt(5): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
    a = P["blocks.0.lora.qkv_A"]
    assert 0.5 * bound < float(a.detach().abs().max()) <= bound
    for n, p in P.items():
        adapted = n.startswith(("blocks.0.", "blocks.2."))
        assert p.requires_grad == (".lora." in n or not adapted), n
        assert p.grad is None
    assert m.blocks[0].lora.scale == 2.0
    # block i's layer-decay scale, unchanged code
    groups = lr_decay.param_groups_lrd(m, 0.05, m.no_weight_decay(), 0.75)
    scale_of = {id(p): g["lr_scale"] for g in groups for p in g["params"]}
    for i in (0, 2):
        assert scale_of[id(P[f"blocks.{i}.lora.qkv_A"])] == 0.75 ** (4 - (i + 1))
    assert scale_of[id(P["blocks.1.attn.qkv.weight"])] == 0.75 ** 2 and id(P["blocks.0.attn.qkv.weight"]) not in scale_of
    # refusals
    with pytest.raises(RuntimeError, match="already"):
        lora.attach(m, blocks=[0])
    with pytest.raises(ValueError):
        lora.attach(_vit(), targets=("head",))
    with pytest.raises(ValueError):
        lora.attach(_vit(), rank=65)
    with pytest.raises(AssertionError):
        lora.attach(_vit(), lora_dropout=0.1)
    from functools import partial
    unfused = video_vit.Block(64, 2, norm_layer=partial(torch.nn.GroupNorm, 1))
    with pytest.raises(NotImplementedError, match="unfused"):
        lora.attach(unfused)
    # both key layouts
    for blk, qkv in ((video_vit.Block(64, 2, qkv_bias=True), (192, 64)), (video_vit.FlashBlock(128, 2), (384, 128))):
        lora.attach(blk, rank=16)
        assert tuple(blk.lora.qkv_B.shape) == (qkv[0], 16) and tuple(blk.lora.qkv_A.shape) == (16, qkv[1])
        assert not any(p.requires_grad for n, p in blk.named_parameters() if not n.startswith("lora."))


def test_state_dict_filter_round_trip_and_trainable_marking():
    from octcubem_amd import lora
    m = _vit(depth=2)
    lora.attach(m, rank=4)
    train = lora.mark_only_lora_trainable(m)
    want = {n for n, _ in m.named_parameters() if ".lora." in n or n.split(".")[0] in ("head", "fc_norm")}
    assert {n for n, p in m.named_parameters() if p.requires_grad} == want and len(train) == len(want)
    assert not m.patch_embed.proj.weight.requires_grad and not m.pos_embed.requires_grad
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n in want:
                p.copy_(torch.randn(p.shape))
    sd = lora.lora_state_dict(m)
    assert set(sd) == want
    assert set(lora.lora_state_dict(m, also=())) == {n for n in want if ".lora." in n}
    m2 = _vit(depth=2)
    lora.attach(m2, rank=4)
    lora.load_lora_state_dict(m2, sd)
    own = m2.state_dict()
    assert all(torch.equal(own[k], v) for k, v in sd.items())
    with pytest.raises(RuntimeError, match="unexpected"):
        lora.load_lora_state_dict(m2, dict(sd, bogus=torch.zeros(1)))
    with pytest.raises(RuntimeError, match="missing"):
        lora.load_lora_state_dict(m2, {k: v for k, v in sd.items() if not k.endswith("proj_A")})
    lora.load_lora_state_dict(m2, {k: v for k, v in sd.items() if not k.endswith("proj_A")}, strict=False)
    # a pretrained checkpoint into an adapted model: the adapters stay, their keys are not asked for
    from octcubem_amd import checkpoint, models_vit_st
    from functools import partial
    kw = dict(num_frames=6, t_patch_size=3, img_size=32, patch_size=16, in_chans=1, num_classes=8, embed_dim=64, depth=2, num_heads=2,
              mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), sep_pos_embed=True, cls_embed=True, global_pool=True, dropout=0.0)
    pre, st = models_vit_st.VisionTransformer(**kw), models_vit_st.VisionTransformer(**kw)
    lora.attach(st, rank=4)
    with torch.no_grad():
        st.blocks[0].lora.qkv_B.fill_(0.25)
    before = {k: v.clone() for k, v in st.state_dict().items() if ".lora." in k}
    missing, unexpected = checkpoint.load_pretrained(st, pre.state_dict(), strict=True)
    assert not missing and not unexpected
    now = st.state_dict()
    assert all(torch.equal(now[k], v) for k, v in before.items())
    assert all(torch.equal(now[k], v) for k, v in pre.state_dict().items())
