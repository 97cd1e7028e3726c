"""CPU-side tests: the C-ABI library loads and exports every symbol include/octmae.h declares, host logic of the
drop-in modules (constructor contract, state_dict keys, schedules, grouping), loud failure without a GPU."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

from oracle import mae3d_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    """_lib binds what include/octmae.h declares, by parsing it: both builds of the library export every parsed name."""
    from octcubem_amd import _lib
    lib = _lib.load()
    f16 = ctypes.CDLL(os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so"))
    assert len(_lib.SIGNATURES) >= 111
    for s in _lib.SIGNATURES:
        assert hasattr(lib, s) and hasattr(f16, s), s
    assert set(_lib.RESTYPES) <= set(_lib.SIGNATURES)
    assert lib.octmae_abi_version() == _lib.expected_abi_version() == _lib.CONSTANTS["OCTMAE_ABI_VERSION"] and lib.octmae_mt_chunk_elems() == 65536


def test_header_parser_on_literal_declarations():
    """_lib.parse_header is a pure function of the header text: declarations over several lines, comments stripped first, the pointer
    rule with its one exception, both spellings of a 64-bit return, integer #defines and enum members; a spelling outside the
    header's vocabulary is an error that names the function, never a guess."""
    from octcubem_amd import _lib
    vp, i, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    sigs, res, consts = _lib.parse_header("""
        #define OCTMAE_ABI_VERSION 7
        #define OCTMAE_H_
        enum { OCTMAE_X_A = 0, OCTMAE_X_B = 3 /* the last */ };
        /* int octmae_in_a_comment(int a); */
        // int octmae_in_a_line_comment(void);
        typedef struct { int kind, mode; } octmae_desc;
        int octmae_first(void);
        int octmae_second(const float* x, long long x_stride,
                          const octmae_desc* desc, void** out,
                          int n, float eps,   /* between two parameters */
                          void* stream);
        int octmae_option(const char* key, int value);  long long octmae_bytes(long long n, int k);
        long long int octmae_doubles(long long);
    """)
    assert sigs == {"octmae_first": [], "octmae_second": [vp, ll, vp, vp, i, f, vp], "octmae_option": [ctypes.c_char_p, i],
                    "octmae_bytes": [ll, i], "octmae_doubles": [ll]}
    assert res == {"octmae_bytes": ll, "octmae_doubles": ll}
    assert consts == {"OCTMAE_ABI_VERSION": 7, "OCTMAE_X_A": 0, "OCTMAE_X_B": 3}
    for bad, what in (("int octmae_sized(const float* x, size_t n);", "size_t n"), ("int octmae_wide(double x);", "double x"),
                      ("unsigned octmae_count(void);", "unsigned"), ("void* octmae_handle(int a);", "void*")):
        with pytest.raises(_lib.OctmaeError) as e:
            _lib.parse_header("int octmae_fine(int a);\n" + bad)
        assert re.search(r"octmae_(sized|wide|count|handle)", str(e.value)) and what in str(e.value), str(e.value)


def test_header_mapping_pins():
    """A few argument lists of the real header written out by hand: they guard the parser's mapping (a long long read as int would
    truncate a stride without an error), not a second table."""
    from octcubem_amd import _lib
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    sig = _lib.SIGNATURES
    assert sig["octmae_set_option"] == [ctypes.c_char_p, i]
    assert sig["octmae_gemm_bf16_ws"] == [vp] * 6 + [i] * 11 + [vp, ll, vp] and _lib._ll is ll
    assert sig["octmae_linear_dgrad_dgelu"][-3:] == [vp, ll, vp]
    assert sig["octmae_rank_counts"] == [vp, ll, vp, ll, vp, ll, i, vp]                      # the two row strides and n
    assert sig["octmae_retrieval_pair_ranks"] == [vp, ll] * 6 + [i, vp, vp, ll, ll, i, vp]   # six strides, ws_bytes, n
    assert sig["octmae_image_augment"] == [vp, i, i, i] + [vp] * 6                           # struct pointers
    assert _lib.RESTYPES == {n: ll for n in ("octmae_retrieval_topk_ws", "octmae_retrieval_pair_ws", "octmae_bootstrap_moments_ws")}


def test_comm_constants_are_the_headers():
    from octcubem_amd import _lib, comm
    assert (comm.F32, comm.BF16, comm.F64, comm.F16) == (0, 1, 2, 3) == tuple(_lib.CONSTANTS[f"OCTMAE_COMM_{n}"] for n in ("F32", "BF16", "F64", "F16"))
    assert (comm.SUM, comm.AVG, comm.MAX) == (0, 1, 2) == tuple(_lib.CONSTANTS[f"OCTMAE_COMM_{n}"] for n in ("SUM", "AVG", "MAX"))
    assert comm.ID_BYTES == 128 == _lib.CONSTANTS["OCTMAE_COMM_ID_BYTES"]


def test_half_build_exports_the_same_abi_and_reports_its_operand_type():
    """liboctmae_f16.so (make F16=1; the verification build of tests/test_gpu_f16_parity.py) is the SAME source: every declared
    symbol, the same ABI number, octmae_lp_dtype() == 1 where the product library says 0; and the host side maps that to the torch
    dtype it allocates 16-bit buffers with (in a child process: a process binds ONE library)."""
    import subprocess
    from octcubem_amd import _lib
    path = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")
    assert os.path.exists(path), "make -C octcubem_amd/csrc both"
    lib = ctypes.CDLL(path)
    for s in _lib.SIGNATURES:
        assert hasattr(lib, s), s
    assert lib.octmae_abi_version() == _lib.expected_abi_version()
    assert lib.octmae_lp_dtype() == 1 and _lib.load().octmae_lp_dtype() == 0
    code = "from octcubem_amd import ops; print(ops.BF16, ops.LP_IS_F16, ops.ATTN_OPTIMISTIC)"
    for lp, want in ((path, "torch.float16 True False"), (_lib.LIB_PATH, "torch.bfloat16 False True")):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, OCTMAE_LIB=lp))
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == want, (r.stdout, r.stderr)


def test_argument_errors_are_reported_without_a_gpu():
    from octcubem_amd import _lib
    lib = _lib.load()
    # NULL pointers / bad sizes are rejected before any launch
    assert lib.octmae_gemm_bf16(None, None, None, None, None, None, 8, 8, 8, 8, 8, 8, 0, 0, 0, 0, 1, None) == -1
    assert lib.octmae_attn_fwd(None, None, None, None, 1, 1, 1, 64, 0.125, None) == -1
    assert lib.octmae_layernorm_fwd(None, None, None, None, None, None, 1, 64, 1e-6, None) == -1
    assert lib.octmae_random_masking_ids(None, None, None, None, None, 1, 8, 2, None) == -1
    with pytest.raises(_lib.OctmaeError):
        _lib.call("octmae_cast_f32_bf16", None, None, 8, None)


def test_weight_gradient_split_plan_tiles_the_rows_exactly_once():
    """octmae_wgrad_split_plan (csrc/gemm.hip: the host-side copy of the arithmetic the weight-gradient kernels run, split_range_of +
    wgrad_stagger_for): whatever the row count, the requested split, the tile count and the stagger option, the k slices must
    cover [0, ceil(M / 64)) contiguously, none empty; staggered slices rise linearly and the shortest keeps at least half the mean
    length and 8 k-tiles; the rule applies only to >= 8 slices of <= 96 k-tiles; option 0 switches it off."""
    from octcubem_amd import _lib
    lib = _lib.load()
    import random
    rng = random.Random(4)
    prev = lib.octmae_set_option(b"wgrad_stagger", 29)
    try:
        seen_staggered = 0
        for v in (29, 0, 200, 100000):
            assert lib.octmae_set_option(b"wgrad_stagger", v) >= 0
            for _ in range(400):
                M = rng.choice([1, 63, 64, 65, 700, 40992, 163968, 655488, rng.randrange(1, 700000)])
                splitk = rng.choice([1, 2, 3, 4, 5, 8, 9, 16, 21, 64, rng.randrange(1, 300)])
                tiles = rng.choice([1, 4, 12, 16, 48, 64, 128])
                slices = ctypes.c_int(0)
                bounds = (ctypes.c_int * (splitk + 2))()
                d = lib.octmae_wgrad_split_plan(M, splitk, tiles, ctypes.byref(slices), bounds)
                S, ktiles = slices.value, (M + 63) // 64
                b = list(bounds[:S + 1])
                assert 1 <= S <= max(1, min(splitk, ktiles)), (M, splitk, S)
                assert b[0] == 0 and b[-1] == ktiles, (M, splitk, tiles, v, b)
                lens = [b[i + 1] - b[i] for i in range(S)]
                assert min(lens) >= 1, (M, splitk, tiles, v, lens)
                if d == 0:                                   # equal slices: all but the last have the same length
                    assert len(set(lens[:-1])) <= 1 and lens[-1] <= lens[0]
                else:
                    seen_staggered += 1
                    assert v > 0 and S >= 8 and ktiles <= 96 * S
                    mean = ktiles / S
                    assert min(lens) >= min(mean / 2, mean - 8) - 1.01 and min(lens) >= 7, (lens, mean)
                    # rising by d / 256 k-tiles per slice; each bound carries two floors (error in (-1, 1)), a length two bounds,
                    # a difference of lengths three
                    step = d / 256.0
                    assert all(abs((lens[i + 1] - lens[i]) - step) < 4.0 for i in range(S - 1)), (lens, step)
                    assert abs((lens[-1] - lens[0]) - step * (S - 1)) < 4.0, (lens, step)
                if v == 0:
                    assert d == 0
        assert seen_staggered > 50
        assert lib.octmae_wgrad_split_plan(0, 4, 16, None, None) == -1
    finally:
        lib.octmae_set_option(b"wgrad_stagger", prev)


def test_model_contract_and_state_dict_keys():
    from octcubem_amd import models_mae
    from functools import partial
    cfg = O.MAEConfig(input_size=64, in_chans=1, embed_dim=128, depth=2, num_heads=2, decoder_embed_dim=64, decoder_depth=2,
                      decoder_num_heads=2, num_frames=12, t_patch_size=3, pred_t_dim=12, high_res_input_size=128)
    m = models_mae.MaskedAutoencoderViT(input_size=64, patch_size=16, in_chans=1, embed_dim=128, depth=2, num_heads=2,
                                        decoder_embed_dim=64, decoder_depth=2, decoder_num_heads=2,
                                        norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_frames=12, t_patch_size=3,
                                        sep_pos_embed=True, cls_embed=True, pred_t_dim=12, high_res_input_size=128)
    shapes = O.param_shapes(cfg)
    sd = m.state_dict()
    assert set(sd) == set(shapes)
    assert all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    # attributes downstream reference code reads (video_vit.py:49-67, models_mae…:83-84,503-507)
    pe = m.patch_embed
    assert (pe.num_patches, pe.input_size, pe.patch_size, pe.grid_size, pe.t_grid_size, pe.frames, pe.t_patch_size) == \
        (64, (4, 4, 4), (16, 16), 4, 4, 12, 3)
    assert m.t_pred_patch_size == 3 and m.high_res_input_size == (4, 8, 8)
    # the flash-layout checkpoint keys are accepted (reverse of the reference's remap, models_mae…:693-724)
    P = O.init_params(cfg, seed=1)
    flash = {}
    for k, v in P.items():
        mm = re.match(r"(.*blocks\.\d+)\.attn\.(q|k|v)\.(weight|bias)$", k)
        if mm:
            continue
        flash[k.replace(".attn.proj.", ".mixer.out_proj.")] = v
    for pre in [f"blocks.{i}" for i in range(2)] + [f"decoder_blocks.{i}" for i in range(2)]:
        for kind in ("weight", "bias"):
            flash[f"{pre}.mixer.Wqkv.{kind}"] = torch.cat([P[f"{pre}.attn.{n}.{kind}"] for n in "qkv"], 0)
    res = m.load_state_dict_to_backbone(flash, strict=True)
    for k in P:
        assert torch.equal(m.state_dict()[k], P[k]), k
    # patchify / unpatchify round trip (visualiser helpers)
    x = torch.rand(2, 1, 12, 64, 64)
    assert torch.equal(m.unpatchify(m.patchify(x)), x)
    assert torch.allclose(m.patchify(x), O.patchify(x, cfg))


def test_product_path_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from octcubem_amd import models_mae
    from functools import partial
    m = models_mae.MaskedAutoencoderViT(input_size=64, patch_size=16, in_chans=1, embed_dim=128, depth=1, num_heads=2,
                                        decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2,
                                        norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_frames=6, t_patch_size=3,
                                        sep_pos_embed=True, cls_embed=True, pred_t_dim=6, high_res_input_size=128)
    with pytest.raises(RuntimeError, match="GPU only|no CPU fallback|cuda"):
        m(torch.rand(1, 1, 6, 64, 64))


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "octcubem_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in src.replace("the oracle", "").replace("oracle's", ""), fn


def test_lr_schedule_and_weight_decay_groups():
    from octcubem_amd import lr_sched, misc, models_mae

    class A: pass
    a = A(); a.lr = 1.6e-3; a.min_lr = 1e-6; a.warmup_epochs = 5; a.epochs = 50

    class Opt:
        def __init__(self): self.param_groups = [{"lr": 0.0}, {"lr": 0.0, "lr_scale": 0.5}]
    for e in (0.0, 0.37, 4.999, 5.0, 17.3, 49.99):
        o = Opt()
        lr = lr_sched.adjust_learning_rate(o, e, a)
        assert abs(lr - O.cosine_lr(e, 1.6e-3, 1e-6, 5, 50)) < 1e-15
        assert o.param_groups[0]["lr"] == lr and o.param_groups[1]["lr"] == lr * 0.5
    from functools import partial
    m = models_mae.MaskedAutoencoderViT(input_size=64, patch_size=16, in_chans=1, embed_dim=128, depth=1, num_heads=2,
                                        decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2,
                                        norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_frames=6, t_patch_size=3,
                                        sep_pos_embed=True, cls_embed=True, pred_t_dim=6, high_res_input_size=128)
    groups = misc.add_weight_decay(m, 0.05)
    names = {id(p): n for n, p in m.named_parameters()}
    nd, d = O.weight_decay_groups([(n, tuple(p.shape)) for n, p in m.named_parameters()], 0.05)
    assert [names[id(p)] for p in groups[0]["params"]] == nd and [names[id(p)] for p in groups[1]["params"]] == d
    assert groups[0]["weight_decay"] == 0.0 and groups[1]["weight_decay"] == 0.05


def test_arena_ordering_makes_qkv_adjacent():
    from octcubem_amd.arena import _ordered
    names = ["a.norm1.weight", "a.attn.q.weight", "a.attn.q.bias", "a.attn.k.weight", "a.attn.k.bias", "a.attn.v.weight",
             "a.attn.v.bias", "a.attn.proj.weight", "a.attn.proj.bias"]
    out = [n for n, _ in _ordered([(n, None) for n in names])]
    assert out == ["a.norm1.weight", "a.attn.q.weight", "a.attn.k.weight", "a.attn.v.weight", "a.attn.q.bias", "a.attn.k.bias",
                   "a.attn.v.bias", "a.attn.proj.weight", "a.attn.proj.bias"]


def test_lr_decay_groups_match_reference_golden(golden_dir):
    """octcubem_amd.lr_decay on a parameter-only stand-in for the ST ViT (no GPU) vs the groups the reference built."""
    import json
    import numpy as np
    import torch
    from octcubem_amd import lr_decay
    from oracle import vit_ref as V
    z = np.load(os.path.join(golden_dir, "finetune_small.npz"))
    cfg = V.ViTSTConfig(**json.loads(str(z["cfg"])))
    shapes = V.vit_st_param_shapes(cfg)

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.blocks = [None] * cfg.depth
            self._names = {}
            for n, s in shapes.items():
                key = n.replace(".", "__")
                self.register_parameter(key, torch.nn.Parameter(torch.zeros(s)))
                self._names[key] = n

        def named_parameters(self, *a, **k):
            for key, p in super().named_parameters(*a, **k):
                yield self._names[key], p
    m = Stub()
    groups = lr_decay.param_groups_lrd(m, 0.05, no_weight_decay_list=("cls_token", "pos_embed", "pos_embed_spatial",
                                                                    "pos_embed_temporal", "pos_embed_class"), layer_decay=0.75)
    id2name = {id(p): n for n, p in m.named_parameters()}
    ref = json.loads(str(z["groups"]))
    key = lambda g: (g["lr_scale"], g["weight_decay"])
    assert len(groups) == len(ref)
    for a, b in zip(sorted(groups, key=key), sorted(ref, key=key)):
        assert sorted(id2name[id(p)] for p in a["params"]) == sorted(b["params"])
        assert a["weight_decay"] == b["weight_decay"] and abs(a["lr_scale"] - b["lr_scale"]) < 1e-15
    for n, lid in json.loads(str(z["layer_ids"])).items():
        assert lr_decay.get_layer_id_for_vit(n, cfg.depth + 1) == lid


def test_graft_entry_build_compiles_and_agrees_on_the_abi_number():
    """__graft_entry__.build() must run clean from this tree: make (a no-op when up to date), import, and the ABI number
    the library reports == OCTMAE_ABI_VERSION in include/octmae.h (the one place it is written)."""
    import __graft_entry__ as g
    from octcubem_amd import _lib
    g.build()
    hdr = open(os.path.join(ROOT, "include", "octmae.h")).read()
    assert int(re.search(r"#define\s+OCTMAE_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.load().octmae_abi_version()
    src = open(os.path.join(ROOT, "octcubem_amd", "csrc", "probe.hip")).read()
    assert "return OCTMAE_ABI_VERSION" in src


def test_generated_attention_bodies_are_current():
    """csrc/attn_bwd1w_body.inc and attn_bwd1w_body_hd64.inc (the placed tile bodies of the one-wave-per-SIMD attention backward
    kernels) are committed so that a build needs no Python; they must be what tools/gen_attn_bwd1w.py produces."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_attn_bwd1w.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_native_comm_bootstrap_over_a_store(monkeypatch):
    """comm.NativeComm.from_store: rank 0 publishes the 128-byte RCCL unique id under one key of the launcher's store and every
    rank -- rank 0 included -- constructs its communicator from the bytes it reads back (the communicator itself needs GPUs:
    its constructor and the id source are replaced; octmae_comm_* argument errors are checked in
    test_argument_errors_are_reported_without_a_gpu)."""
    import threading
    import torch.distributed as dist
    from octcubem_amd import comm as ocomm
    made = {}
    the_id = bytes(range(128))
    monkeypatch.setattr(ocomm.NativeComm, "unique_id", staticmethod(lambda: the_id))
    monkeypatch.setattr(ocomm.NativeComm, "__init__", lambda self, idb, rank, world, device: made.__setitem__(rank, (bytes(idb), world, device)))
    monkeypatch.setattr(ocomm.NativeComm, "__del__", lambda self: None, raising=False)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    store = dist.HashStore()
    ths = [threading.Thread(target=ocomm.NativeComm.from_store, args=(store, r, 3, r)) for r in (2, 1, 0)]   # rank 0 arrives last
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=30)
    assert made == {r: (the_id, 3, r) for r in range(3)}
    assert len(the_id) == ocomm.ID_BYTES == 128


def test_bench_board_sampler_without_hwmon_reports_nothing(tmp_path, monkeypatch):
    """bench.BoardSampler reads the amdgpu hwmon files by plain file reads (no child process after the GPU is initialised); on a
    host without them -- this container -- it must start, stop and report None instead of failing the benchmark."""
    import glob
    import bench
    monkeypatch.setattr(glob, "glob", lambda pat, **kw: [])
    b = bench.BoardSampler(0, period=0.01)
    assert b.cards == {}
    b.start()
    assert b.stop() is None


def test_bench_board_sampler_reads_power_and_clock(tmp_path, monkeypatch):
    import glob
    import time
    import bench
    h = tmp_path / "card0" / "device" / "hwmon" / "hwmon3"
    h.mkdir(parents=True)
    (h / "power1_input").write_text("1350000000\n"); (h / "freq1_input").write_text("1950000000\n"); (h / "power1_cap").write_text("1400000000\n")
    monkeypatch.setattr(glob, "glob", lambda pat, **kw: [str(h)])
    b = bench.BoardSampler(0, period=0.01)
    b.start(); time.sleep(0.1)
    st = b.stop()
    assert st is not None and st["samples"] >= 2
    assert abs(st["power_w_avg"] - 1350.0) < 1e-6 and abs(st["sclk_mhz_avg"] - 1950.0) < 1e-6 and st["power_cap_w"] == 1400.0


def test_device_prefetcher_is_a_pass_through_on_the_cpu():
    from octcubem_amd import misc
    batches = [(torch.full((2, 3), float(i)), {"id": i, "t": torch.tensor([i])}) for i in range(5)]
    assert misc.prefetched(batches, "cpu") is batches                      # no GPU: the loader itself
    pf = misc.DevicePrefetcher(batches, "cpu", only=(0,))
    assert len(pf) == 5
    out = list(pf)
    assert all(a is b for a, b in zip(out, batches))
    assert list(misc.DevicePrefetcher([], "cpu")) == []


def test_autocast_invariant_decorator_switches_the_context_off_for_forward_methods_only():
    """octcubem_amd/_autocast.py on the CPU (the GPU side is tests/test_gpu_autocast.py): a decorated module's forward / forward_* /
    encode_* run with autocast off -- an fp32 matmul stays fp32 inside `torch.autocast("cpu", dtype=torch.bfloat16)` -- other methods
    and undecorated modules are untouched, and outside autocast the wrapper adds nothing."""
    from octcubem_amd._autocast import autocast_invariant

    class Plain(torch.nn.Module):
        def forward(self, a, b):
            return a @ b

        def forward_features(self, a, b):
            return a @ b

        def encode_image(self, a, b):
            return a @ b

        def helper(self, a, b):
            return a @ b

    Inv = autocast_invariant(type("Inv", (Plain,), dict(Plain.__dict__)))
    a, b = torch.randn(8, 8), torch.randn(8, 8)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert Plain()(a, b).dtype == torch.bfloat16                      # what autocast does to an ATen island
        m = Inv()
        for out in (m(a, b), m.forward_features(a, b), m.encode_image(a, b)):
            assert out.dtype == torch.float32
        assert m.helper(a, b).dtype == torch.bfloat16                     # not a forward-like method: untouched
        assert torch.is_autocast_enabled("cpu")                           # the caller's context is restored
    exact = a @ b
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert torch.equal(Inv()(a, b), exact)
    assert torch.equal(Inv()(a, b), exact)
    assert getattr(Inv.forward, "_octmae_no_autocast", False) and not hasattr(Inv.helper, "_octmae_no_autocast")


def test_small_launch_plan():
    """The cost model that sends a forward / dgrad GEMM to the small-launch kernel (csrc/gemm.hip plan128, reached without a GPU through
    octmae_gemm_small_plan).  Properties the kernel relies on: 1 <= slices <= 4, no EMPTY slice (its workgroup would publish a zero
    tile -- harmless -- but a tile whose counter never reaches `slices` would never be written: (S - 1) * ceil(ktiles / S) < ktiles),
    a split only with the workspace lent and within its 1024 slots, a ring of 4 or 2 stages.  Policy: the Linear shapes of ONE
    volume (the reference's shipped recipe) take it and the long reductions are split; the shapes of the headline step (32 / 64 / 128
    volumes per micro-batch) never do."""
    from octcubem_amd import _lib
    lib = _lib.load()
    S, st = ctypes.c_int(0), ctypes.c_int(0)

    def plan(NA, NB, K, cus=256, ws=1, big=1):
        use = lib.octmae_gemm_small_plan(NA, NB, K, cus, ws, big, ctypes.byref(S), ctypes.byref(st))
        assert use in (0, 1)
        return use, S.value, st.value

    for cus in (256, 304, 64):
        for NA in (512, 1024, 1536, 2048, 3072, 4096):
            for NB in (1, 64, 1281, 2562, 5121, 4 * 1281, 8 * 5121, 32 * 1281, 128 * 5121):
                for K in (64, 512, 768, 1024, 2048, 3072, 4096):
                    for ws in (0, 1):
                        use, s_, n_ = plan(NA, NB, K, cus, ws, int(NA >= 256 and NB >= 256))
                        kt = K // 64
                        assert 1 <= s_ <= 4 and n_ in (2, 4)
                        if not use:
                            assert s_ == 1
                            continue
                        assert ws or s_ == 1
                        if s_ > 1:
                            assert (s_ - 1) * -(-kt // s_) < kt and kt // s_ >= 8
                            assert -(-NA // 128) * -(-NB // 128) * s_ <= 1024
    # one volume per step: every forward / dgrad Linear of the encoder (1281 rows, D 1024) and decoder (5121 rows, D 512)
    for NA, NB, K in ((3072, 1281, 1024), (1024, 1281, 1024), (4096, 1281, 1024), (1024, 1281, 4096), (1024, 1281, 3072),
                      (1536, 5121, 512), (512, 5121, 512), (512, 5121, 2048)):
        assert plan(NA, NB, K)[0] == 1, (NA, NB, K)
    assert plan(1024, 1281, 4096)[1] > 1 and plan(1024, 1281, 4096, ws=0)[1] == 1       # the long reductions are split when they can be
    # the headline step never takes it
    for vols in (32, 64, 128):
        for NA, rows, K in ((3072, 1281, 1024), (1024, 1281, 1024), (4096, 1281, 1024), (1024, 1281, 4096), (1024, 1281, 3072),
                            (1536, 5121, 512), (512, 5121, 512), (2048, 5121, 512), (512, 5121, 2048), (512, 5121, 1536)):
            assert plan(NA, vols * rows, K)[0] == 0, (vols, NA, rows, K)
    prev = lib.octmae_set_option(b"gemm_small", 0)
    try:
        assert plan(1024, 1281, 4096)[0] == 0                                              # switched off: never
    finally:
        lib.octmae_set_option(b"gemm_small", prev)


def test_bench_parity_compliant_child_failure_is_recorded_not_raised():
    """bench.py's `parity_compliant` record comes from a child process on the half-operand build; whatever goes wrong there (here: no GPU
    in this container, so the child exits with an error) must end up IN the record -- the headline run goes on."""
    import argparse
    import bench
    rec = bench.run_parity_compliant_child(argparse.Namespace(global_batch=256, micro_batch=0), steps=1, warmup=0)
    assert rec["dtype"] == "f16" and rec["lib"] == "liboctmae_f16.so" and rec["value"] is None
    assert "error" in rec and rec["error"]


def test_bench_dump_outputs_writes_a_fixed_float32_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: loss, pred, mask and sampled parameters / gradients as float32 .npy files; the sample positions are
    seeded and depend on the shapes only, so two runs (two builds) write element-for-element comparable files."""
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_PRED_SAMPLES", 1000)
    monkeypatch.setattr(bench, "DUMP_PER_TENSOR", 64)
    g = torch.Generator().manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 2))
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g)
    loss, pred, mask = torch.tensor(0.25), torch.randn(3, 50, 20, generator=g), (torch.rand(3, 50, generator=g) > 0.5)
    shapes = bench.dump_outputs(str(tmp_path / "a"), loss, pred, mask, model)
    bench.dump_outputs(str(tmp_path / "b"), loss, pred * 2, mask, model)
    assert shapes == {"loss": [], "mask": [3, 50], "pred": [1000], "params": [64 + 30 + 2 + 60], "grads": [64 + 30 + 2 + 60]}
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in shapes}
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in shapes}
    assert all(v.dtype == np.float32 for v in a.values())
    assert float(a["loss"]) == 0.25 and np.array_equal(a["mask"], mask.float().numpy())
    assert np.array_equal(b["pred"], 2 * a["pred"])                 # same positions, whatever the values
    assert set(a["pred"].tolist()) <= set(pred.reshape(-1).tolist())
    assert np.array_equal(a["params"][64:94], model[0].bias.detach().numpy())          # small tensors whole, in parameter order
    assert np.array_equal(a["grads"][-2:], model[1].bias.grad.numpy())


# ------------------------------------------------------------------------------------------------ the GEMM launch planner
PLAN_FWD, PLAN_DGRAD, PLAN_DGELU, PLAN_DGELU_WS, PLAN_DELTA, PLAN_WGRAD, PLAN_WGRAD_BIAS = range(7)       # `kind` of octmae_gemm_plan
TILE128, TWOSTAGE256, PHASED256, SMALL128D = range(4)                                                     # out[0]: the kernel family
PLAN_FIELDS = ("kernel", "grid", "tiles_a", "tiles_b", "cgroup", "slices", "per", "kstagger", "atomic1", "nst", "small_S", "ws_rows", "colsum")


def _both_libraries():
    from octcubem_amd import _lib
    return [_lib.load(), ctypes.CDLL(os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so"))]


def _gemm_plan(lib, kind, NA, NB, K, lda=None, ldb=None, variant=0, splitk=1, ws=1, cus=256):
    """(rc, fields) for X[a][b] = sum_k A[a][k] B[b][k]; the default leading dimensions are those of packed operands"""
    a_ks = kind != PLAN_FWD
    b_ks = kind in (PLAN_WGRAD, PLAN_WGRAD_BIAS)
    out = (ctypes.c_int * 13)()
    rc = lib.octmae_gemm_plan(kind, NA, NB, K, lda or (NA if a_ks else K), ldb or (NB if b_ks else K), variant, splitk, ws, cus, out)
    return rc, dict(zip(PLAN_FIELDS, out))


def _fits_256(NA, NB, K, kind):
    return NA >= 256 and NB >= 256 and (kind in (PLAN_WGRAD, PLAN_WGRAD_BIAS) or K % 64 == 0)


PAIR_FIELDS = ("kernel", "grid", "slices", "per", "kstagger", "atomic1", "nst", "colsum", "tiles_a0", "tiles_b0", "cgroup0", "tiles_a1", "tiles_b1", "cgroup1")
# (N0, K0, N1, K1) of the four weight-gradient pairs of a ViT-L Block: encoder fc2 + fc1 (128 output tiles of 256 x 256) and proj + qkv (64),
# decoder fc2 + fc1 (32) and proj + qkv (16)
ENC_FC, ENC_QKV, DEC_FC, DEC_QKV = (1024, 4096, 4096, 1024), (1024, 1024, 3072, 1024), (512, 2048, 2048, 512), (512, 512, 1536, 512)


def _pair_plan(lib, pair, M, splitk=0, cus=256):
    """(rc, fields) of octmae_wgrad_pair_plan for packed operands"""
    N0, K0, N1, K1 = pair
    out = (ctypes.c_int * 14)()
    rc = lib.octmae_wgrad_pair_plan(N0, K0, N0, K0, N1, K1, N1, K1, M, splitk, cus, out)
    return rc, dict(zip(PAIR_FIELDS, out))


def _splitk_for(n_out_tiles: int, ktiles: int, target_blocks: int) -> int:
    """The rule as octcubem_amd/ops.py held it before the planner took it over (auto_wgrad_split in csrc/gemm_plan.hpp), verbatim: the
    reference of test_auto_weight_gradient_split_is_the_rule_ops_had."""
    # as many k-slices as keep tiles x slices within ONE round of workgroups over the chip (a second, partly filled
    # round costs more than the slightly lower fill), and >= 8 k-tiles (512 token rows) per slice
    s = max(1, target_blocks // n_out_tiles)
    s = max(1, min(s, ktiles // 8 if ktiles >= 8 else 1))
    if s > 1 and target_blocks == 256:
        def cost(k):
            return 1.4 * -(-ktiles // k) + 0.22 * n_out_tiles * k
        s = min(range(1, s + 1), key=cost)
    return s


def test_weight_gradient_split_rule():
    """The planner's own k split of a weight gradient (splitk = 0; auto_wgrad_split, host arithmetic): as many k slices as keep tiles x
    slices within one round of 256 workgroups with >= 8 k-tiles each -- unless the fp32-atomic epilogues of the slices (0.22 us per tile
    and slice) cost more than the main-loop time they save (1.4 us per k-tile): one or two volumes per step stay unsplit where round 5
    split two ways; from 8 volumes on nothing changes (the headline's choices are those of rounds 2-5).  Read off the plans on 256 CUs:
    the four pairs of a Block through octmae_wgrad_pair_plan, single launches through octmae_gemm_plan."""
    import json
    pins = {r[0]: r for r in json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_plan_pins.json")))["pair"]}
    for lib in _both_libraries():
        slices = lambda pair, rows: _pair_plan(lib, pair, rows)[1]["slices"]     # noqa: E731
        for small in (1, 0):                                    # 0: the 256-tile pair is the kernel at every size
            prev = lib.octmae_set_option(b"gemm_small", small)
            try:
                for vols in (8, 16, 32, 64, 128):               # unchanged from the old rule
                    assert all(_pair_plan(lib, pr, vols * rows)[1]["kernel"] == PHASED256
                               for pr, rows in ((ENC_FC, 1281), (ENC_QKV, 1281), (DEC_FC, 5121), (DEC_QKV, 5121)))
                    assert slices(ENC_FC, vols * 1281) == 2
                    assert slices(ENC_QKV, vols * 1281) == 4
                    assert slices(DEC_FC, vols * 5121) == 8
                    assert slices(DEC_QKV, vols * 5121) in (15, 16)
                if small:                                       # one volume: the 128-tile pair, with the slices the pins saw it launch
                    for name, pr, rows in (("B1_enc_fc2+fc1", ENC_FC, 1281), ("B1_enc_proj+qkv", ENC_QKV, 1281), ("B1_dec_fc2+fc1", DEC_FC, 5121),
                                           ("B1_dec_proj+qkv", DEC_QKV, 5121)):
                        rc, p = _pair_plan(lib, pr, rows)
                        assert (rc, p["kernel"], p["grid"], p["slices"], p["nst"]) == (0, *pins[name][7:11]) and p["kernel"] == SMALL128D, name
                    continue
                assert _pair_plan(lib, ENC_FC, 1281)[1]["kernel"] == PHASED256
                assert slices(ENC_FC, 1281) == 1 and slices(ENC_QKV, 1281) == 1                   # one volume: no atomics
                assert slices(ENC_FC, 2 * 1281) == 1 and slices(ENC_QKV, 2 * 1281) == 2
                assert 3 <= slices(DEC_FC, 5121) <= 5 and 5 <= slices(DEC_QKV, 5121) <= 7
            finally:
                lib.octmae_set_option(b"gemm_small", prev)
        for N, K in ((256, 256), (256, 1792), (1024, 1024), (2048, 2048), (2048, 4096), (3840, 5120)):     # 1, 7, 16, 64, 128, 300 tiles: always a legal split
            tiles = (N // 256) * (K // 256)
            for ktiles in (1, 5, 8, 21, 81, 2562):
                rc, p = _gemm_plan(lib, PLAN_WGRAD, N, K, 64 * ktiles, variant=0x4000, splitk=0)
                s_ = p["slices"]
                assert rc == 0 and p["kernel"] == PHASED256 and p["grid"] == tiles * s_
                assert 1 <= s_ <= max(1, 256 // tiles) and (s_ == 1 or ktiles // s_ >= 8)
        for ktiles in (1, 5, 8, 21, 81, 2562):                  # the 128-tile register-staged kernel's target (1024 blocks): the old rule
            rc, p = _gemm_plan(lib, PLAN_WGRAD, 128, 384, 64 * ktiles, variant=0x4000, splitk=0)
            assert rc == 0 and p["kernel"] == TILE128 and p["grid"] == 3 * p["slices"]
            assert 1 <= p["slices"] <= max(1, ktiles // 8) and (p["slices"] > 1) == (ktiles >= 16)


def test_auto_weight_gradient_split_is_the_rule_ops_had():
    """splitk = 0 (the planner chooses: auto_wgrad_split) gives, field for field, the plan of the split that ops._splitk_for chose
    before the rule moved into the planner -- for single weight gradients over a grid of shapes and kernel variants and for the
    pinned pairs on three CU counts.  ops.py took a problem for 256-tiled from N, K >= 256 alone; the planner also asks that each
    operand lies inside a 32-bit buffer range (fits_256) and computes the split for the tiles it launches: for the 4096-wide operands
    at 128 x 5121 rows, the one place of this grid where the two differ, the reference is given the 128-tiles the library runs."""
    import json
    kt = lambda rows: (rows + 63) // 64     # noqa: E731
    for lib in _both_libraries():
        for N in (128, 136, 256, 384, 512, 1024, 1536, 3072, 4096):
            for K in (128, 136, 256, 384, 512, 1024, 1536, 3072, 4096):
                for M in (64, 500, 1281, 2 * 1281, 5121, 4 * 1281, 32 * 1281, 32 * 5121, 128 * 5121):
                    for variant in (0, 0x100, 0x4000):
                        in_range = 2 * M * max(N, K) < 0xFFF00000           # packed operands: M rows of N and of K 16-bit elements
                        assert in_range or (M == 128 * 5121 and 4096 in (N, K))     # 5.4 GB: the only operands of this grid beyond the range
                        big = N >= 256 and K >= 256 and not variant & 0x100 and in_range
                        t = 256 if big else 128
                        ref = _splitk_for(-(-N // t) * -(-K // t), kt(M), 256 if big else 1024)
                        auto, asked = (_gemm_plan(lib, PLAN_WGRAD_BIAS, N, K, M, variant=variant, splitk=s_) for s_ in (0, ref))
                        assert auto == asked and auto[0] == 0, (N, K, M, variant, ref, auto, asked)
        for name, N0, K0, N1, K1, M, *_ in json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_plan_pins.json")))["pair"]:
            ref = _splitk_for(-(-N0 // 256) * -(-K0 // 256) + -(-N1 // 256) * -(-K1 // 256), kt(M), 256)
            for cus in (64, 256, 304):
                auto, asked = (_pair_plan(lib, (N0, K0, N1, K1), M, splitk=s_, cus=cus) for s_ in (0, ref))
                assert auto == asked and auto[0] == 0, (name, cus, ref, auto, asked)


def test_gemm_plan_variant_bits_mean_what_they_say():
    """octmae_gemm_plan on both libraries: bit 8 gives the 128-tile register-staged kernel; bits 9 / 10 the two-stage / phased
    256-tile kernel wherever the problem takes 256-tiles and never the small-launch kernel (dgrad + delta is built for the phased
    main loop only: bit 9 gives that one there); bit 14 never the small-launch kernel; bits 12 / 13 the small-launch kernel with
    that ring depth wherever its operands allow (NA % 8 == 0, whole k-tiles), its split clamped so that no slice is empty and
    slices x tiles fit the workspace's 1024 slots; and no plan splits a small launch without a workspace."""
    for lib in _both_libraries():
        for NA, NB, K in [(N, M, K) for M in (64, 200, 256, 1281, 5121, 8 * 5121) for N in (136, 384, 512, 1024, 4096) for K in (64, 72, 512, 4096)]:
            kt = -(-K // 64)
            for kind in (PLAN_FWD, PLAN_DGRAD, PLAN_DGELU, PLAN_DGELU_WS, PLAN_DELTA, PLAN_WGRAD, PLAN_WGRAD_BIAS):
                wgrad = kind in (PLAN_WGRAD, PLAN_WGRAD_BIAS)
                if (wgrad and NB % 8) or (not wgrad and K % 8):
                    continue                                                 # the entry points reject these operands
                big, small_ok = _fits_256(NA, NB, K, kind), not wgrad and NA % 8 == 0 and K % 64 == 0
                for ws in (0, 1):
                    plan = lambda bits, splitk=1: _gemm_plan(lib, kind, NA, NB, K, variant=bits, splitk=splitk, ws=ws)    # noqa: E731
                    rc, p = plan(0x100)
                    assert (rc, p["kernel"]) == ((0, TILE128) if kind != PLAN_DELTA else (-2, 0))
                    for bits, fam in ((0x200, TWOSTAGE256), (0x400, PHASED256), (0x600, PHASED256)):
                        rc, p = plan(bits)
                        if kind == PLAN_DELTA:
                            assert (rc, p["kernel"]) == ((0, PHASED256) if big else (-2, 0))
                        else:
                            assert rc == 0 and p["kernel"] == (fam if big else TILE128)
                    rc, p = plan(0x4000)
                    assert p["kernel"] != SMALL128D and (rc == 0 or (kind == PLAN_DELTA and not big))
                    rc, p = plan(0)
                    assert rc == -2 or p["small_S"] == 1 or (ws and p["kernel"] == SMALL128D)
                    for bits, nst in ((0x1000, 4), (0x2000, 2)):
                        for S, via_bits in ((1, 0), (2, 0), (3, 1), (4, 1), (7, 1)):
                            rc, p = plan(bits | (S << 16 if via_bits else 0), splitk=1 if via_bits else S)
                            if not small_ok:
                                assert p["kernel"] != SMALL128D
                                continue
                            assert rc == 0 and p["kernel"] == SMALL128D and p["nst"] == nst
                            s_ = p["small_S"]
                            nt = -(-NA // 128) * -(-NB // 128)
                            assert 1 <= s_ <= min(S, 4) and p["slices"] == s_ and p["grid"] == nt * s_ and p["per"] == -(-kt // s_)
                            assert s_ == 1 or (ws and (s_ - 1) * -(-kt // s_) < kt and nt * s_ <= 1024)
                            # the largest split <= the request that meets the three conditions
                            assert all(not (ws and (t - 1) * -(-kt // t) < kt and nt * t <= 1024) for t in range(s_ + 1, min(S, 4) + 1))


def test_gemm_plan_agrees_with_the_two_older_plan_queries():
    """octmae_gemm_small_plan / octmae_wgrad_split_plan are implemented over the same planner: on every case of test_small_launch_plan
    the small-launch decision, split and ring depth of octmae_gemm_plan are theirs, and a weight-gradient plan has the slices and the
    stagger octmae_wgrad_split_plan reports."""
    S, st = ctypes.c_int(0), ctypes.c_int(0)
    for lib in _both_libraries():
        for cus in (256, 304, 64):
            for NA in (512, 1024, 1536, 2048, 3072, 4096):
                for NB in (1, 64, 1281, 2562, 5121, 4 * 1281, 8 * 5121, 32 * 1281, 128 * 5121):
                    for K in (64, 512, 768, 1024, 2048, 3072, 4096):
                        for ws in (0, 1):
                            use = lib.octmae_gemm_small_plan(NA, NB, K, cus, ws, int(NA >= 256 and NB >= 256), ctypes.byref(S), ctypes.byref(st))
                            for kind in (PLAN_FWD, PLAN_DGRAD):
                                rc, p = _gemm_plan(lib, kind, NA, NB, K, ws=ws, cus=cus)
                                assert rc == 0 and (p["kernel"] == SMALL128D) == bool(use)
                                if use:
                                    assert (p["small_S"], p["nst"]) == (S.value, st.value)
        bounds = (ctypes.c_int * 65)()
        for M in (64, 1281, 5121, 4 * 1281, 32 * 1281, 32 * 5121, 128 * 5121):
            for N, K in ((1024, 1024), (3072, 1024), (1024, 4096), (512, 512), (512, 2048), (384, 128)):
                for splitk in (1, 2, 3, 8, 16, 64):
                    rc, p = _gemm_plan(lib, PLAN_WGRAD_BIAS, N, K, M, variant=0x4000, splitk=splitk)
                    d = lib.octmae_wgrad_split_plan(M, splitk, p["tiles_a"] * p["tiles_b"], ctypes.byref(S), bounds)
                    assert rc == 0 and p["slices"] == S.value and p["grid"] == p["tiles_a"] * p["tiles_b"] * S.value
                    assert p["kstagger"] == (d if p["kernel"] != TILE128 else 0)


def test_gemm_plans_of_the_model_shapes_are_those_the_previous_dispatch_launched():
    """tests/golden/gemm_plan_pins.json: kernel family, workgroups, k slices and ring depth of every forward / dgrad / dgrad x GELU' /
    dgrad + delta launch and weight-gradient pair of the ViT-L encoder and decoder Linears at 1, 4, 32 and 128 volumes and of the
    GEMM_SHAPES of tests/test_gpu_kernels.py, on 256 CUs with and without the split-K workspace.  The values were NOT produced by this
    planner: they were read off a rocprofv3 kernel trace of tools/gemm_dispatch_sweep.py on an MI355X running the commit BEFORE the
    planner existed (kernel name -> family, its ring-depth template argument -> ring depth, grid / workgroup -> workgroups and
    slices; profiles/gemm_dispatch_sweep_parent_vs_branch.txt).  cgroup is a kernel argument and not visible in a trace: its
    columns (one per problem for a pair) are that commit's rule in gemm_impl / octmae_wgrad_accum_pair, transcribed by hand into the
    script that wrote the file -- a second statement of the rule, not an observation."""
    import json
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_plan_pins.json")))
    assert len(pins["gemm"]) >= 340 and len(pins["pair"]) == 16
    for lib in _both_libraries():
        for name, kind, NA, NB, K, splitk, ws, family, grid, cgroup, slices, nst in pins["gemm"]:
            for s_ in (splitk, 0) if kind in (PLAN_WGRAD, PLAN_WGRAD_BIAS) else (splitk,):     # 0: the planner's own split must be that commit's
                rc, p = _gemm_plan(lib, kind, NA, NB, K, splitk=s_, ws=ws)
                assert (rc, p["kernel"], p["grid"], p["cgroup"], p["slices"], p["nst"]) == (0, family, grid, cgroup, slices, nst), (name, ws, s_, p)
        out = (ctypes.c_int * 14)()
        for name, N0, K0, N1, K1, M, splitk, family, grid, slices, nst, cgroup0, cgroup1 in pins["pair"]:
            for s_ in (splitk, 0):                                                             # 0: as above
                rc = lib.octmae_wgrad_pair_plan(N0, K0, N0, K0, N1, K1, N1, K1, M, s_, 256, out)
                assert (rc, out[0], out[1], out[2], out[6], out[10], out[13]) == (0, family, grid, slices, nst, cgroup0, cgroup1), (name, s_, list(out))
