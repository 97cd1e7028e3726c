"""GPU: deterministic mode ("deterministic" of octmae_set_option; ops.set_deterministic).

Kernel level, for every kernel family that reaches the slab-storing weight-gradient epilogue:
  (a) BIT equality with the slice-by-slice oracle the mode is specified by -- unsplit launches (splitk = 1, option off) of the SAME
      kernel family over the row ranges the plan query reports, in ascending order, onto the same non-zero accumulator.  This is the
      assertion that fails without the feature (and would fail for any other order of the additions);
  (b) 60 repeated launches are bit-identical to the first while a side stream keeps HBM busy (mismatches counted on the device, one
      synchronisation) -- a guard: small launches often finish in order even where the order is not fixed;
  (c) every element within the weight-gradient bound of tests/test_gpu_gemm_elements.py, (M + slices + 4) 2^-23 (|dY|^T |X| + |gW0|),
      against float64.
Operands and accumulators are views into NaN-filled buffers with leading dimensions of their own (tests/nonfinite.py: embed), and the
accumulator's buffer must keep its bits outside the matrix.  The bias gradient's oracle is ONE launch of the fixed-order column sums
over dY (ops.colsum_accum), which is what the mode runs in front of the GEMM.

Shapes that moved from the issue's list, and why:
  * the 128-tile pair (gemm128d_wgrad_kernel) at widths (256, 512) + (512, 256): the planner takes no k-split launch of that family at
    those widths for any M on 256 CUs (its cost model prices the 256-tile pair lower); the nearest pair it does split there is
    (512, 1024) + (1024, 512) at M = 3264 (3 slices, 4-stage ring).  One ring depth is run because one exists: the cost model never
    prefers the 2-stage ring for a split launch (one more slice on the 4-stage ring is always priced lower), so in this mode the
    planner does not offer it and the library builds no slab form of it (csrc/gemm_plan.hpp: plan_wgrad_pair).
  * "M = 8192, N = K = 256" plans 16 equal slices in the default mode (not 8 staggered ones); the staggered default plans are covered
    by the planner sweep of tests/test_cpu_deterministic.py.
The half-operand build is not run: its child launcher lists its suites inside an existing test file.

Model level: three optimizer steps of the small 3-D MAE with clipping, twice from one seed (the second time beside a busy side stream)
-- losses, gradient norms and every parameter bit-equal; a Block of width 256 on 4096 rows at the three recomputation levels."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import misc, ops, optim as foptim, video_vit
    from octcubem_amd._lib import call, load
    from octcubem_amd.arena import get_arena
    from octcubem_amd.optim import _MultiTensorTable
    LP = ops.BF16
else:
    LP = torch.bfloat16
from tests import deterministic_ref as D
from tests import gemm_elem as GE
from tests import nonfinite as NF

DEV = "cuda"
REPEATS = 60


class mode:
    """with mode(True): ... -- deterministic mode on (off) inside, the previous setting afterwards"""

    def __init__(self, flag, **options):
        self.flag, self.options, self.prev = flag, options, {}

    def __enter__(self):
        self.prev_flag = ops.set_deterministic(self.flag)
        for k, v in self.options.items():
            self.prev[k] = ops.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            ops.set_option(k, v)
        ops.set_deterministic(self.prev_flag)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ws_bytes():
    return D.split_ws_bytes(load())


def bits(t):
    return t.detach().contiguous().view(torch.int32)


class Pressure:
    """a side stream that keeps HBM busy: kick() every few launches (the pattern of test_attention_is_bit_reproducible_under_memory_pressure)"""

    def __init__(self):
        self.side = torch.cuda.Stream()
        self.junk = torch.empty(64 * 1024 * 1024, dtype=torch.float32, device=DEV).fill_(1.0)
        self.n = 0

    def kick(self):
        if self.n % 4 == 0:
            with torch.cuda.stream(self.side):
                self.junk.mul_(1.0001)
        self.n += 1


# ---- weight-gradient cases ---------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(N, K, M):
    """16-bit operands, non-zero fp32 accumulators (CPU), the float64 reference and the bound's magnitudes: computed once, read-only"""
    key = (N, K, M)
    if key not in _CASES:
        g = torch.Generator().manual_seed(7 * N + 3 * K + M)
        c = {"dy": torch.randn(M, N, generator=g).to(LP), "x": torch.randn(M, K, generator=g).to(LP),
             "gw0": torch.randn(N, K, generator=g), "gb0": torch.randn(N, generator=g)}
        dyd, xd = c["dy"].double(), c["x"].double()
        c["gw"] = c["gw0"].double() + dyd.t() @ xd
        c["gw_abs"] = dyd.abs().t() @ xd.abs() + c["gw0"].double().abs()
        c["gb"] = c["gb0"].double() + dyd.sum(0)
        c["gb_abs"] = c["gb0"].double().abs() + dyd.abs().sum(0)
        _CASES[key] = c
    return _CASES[key]


def _device_operands(c):
    """(dy, x) on the device inside NaN-filled buffers: leading dimensions N + 8 and K + 8, NaN rows above and below"""
    return NF.embed(c["dy"], device=DEV), NF.embed(c["x"], device=DEV)


def _accumulators(c, bias=True):
    gw = NF.embed(c["gw0"], device=DEV)
    gb = NF.embed(c["gb0"], device=DEV) if bias else None
    return gw, gb


def _outside_intact(view, before):
    """the buffer around an embedded accumulator holds the bits it held before the launches (`before`: a clone of view._base)"""
    now = view._base.clone()
    m = torch.ones_like(now, dtype=torch.bool)
    lo = (view.data_ptr() - view._base.data_ptr()) // view.element_size()
    if view.dim() == 2:
        r0, ld = divmod(lo, view._base.shape[1])
        m[r0:r0 + view.shape[0], :view.shape[1]] = False
    else:
        m[lo:lo + view.numel()] = False
    return bool((bits(now)[m] == bits(before)[m]).all())


def _wgrad(dy, x, gw, gb, splitk):
    N, K, M = dy.shape[1], x.shape[1], dy.shape[0]
    ops._gemm(dy, x, gw, N, K, M, dy.stride(0), x.stride(0), gw.stride(0), 1, 1, ops.EPI_ACCUM, C2=gb, splitk=splitk)


def _check_bound(c, gw, gb, M, slices, what):
    r, at = GE.worst(gw, c["gw"], (M + slices + 4) * GE.EPS32 * c["gw_abs"])
    print(f"deterministic/{what}: gW worst |got - ref| / bound = {r:.4f} at {at}")
    assert r <= 1.0, (what, r, at)
    if gb is not None:
        r, at = GE.worst(gb, c["gb"], (M + slices + 4) * GE.EPS32 * c["gb_abs"])
        print(f"deterministic/{what}: gb worst |got - ref| / bound = {r:.4f} at {at}")
        assert r <= 1.0, (what, "bias", r, at)


def _gb_oracle(c, dy):
    gb = NF.embed(c["gb0"], device=DEV)
    ops.colsum_accum(dy, gb)
    return gb


@pytest.mark.parametrize("N,K,M,splitk,family", [
    (256, 256, 8192, 0, 2),      # one 256-tile, the planner's split (16 slices by default)
    (512, 264, 8192, 0, 2),      # 2 x 2 tiles of 256 with a ragged tile column
    (136, 200, 1000, 3, 0),      # register-staged 128-tile family, an explicit split whose last k-tile is ragged (1000 = 15 x 64 + 40)
    (136, 200, 4100, 0, 0),      # the same family, the planner's split
])
def test_wgrad_matches_the_slice_by_slice_oracle(N, K, M, splitk, family):
    lib = load()
    c = _case(N, K, M)
    dy, x = _device_operands(c)
    with mode(True):
        rc, p = D.gemm_plan(lib, 6, N, K, M, _ws_bytes(), _cus(), ops._variant_bits(), splitk, dy.stride(0), x.stride(0))
        assert rc == 0 and p["kernel"] == family and p["slices"] > 1 and p["atomic1"] == D.ROUTE_SLABS and p["kstagger"] == 0 and p["colsum"] == 3, p
        d, bounds = D.split_bounds(lib, M, p["slices"], p["tiles_a"] * p["tiles_b"])
        rows = D.slice_rows(bounds, M)
        assert d == 0 and rows[-1][1] == M and rows[-1][1] > rows[-1][0], "the last slice is not empty"
        gw, gb = _accumulators(c)
        before_w, before_b = gw._base.clone(), gb._base.clone()
        _wgrad(dy, x, gw, gb, splitk)
        first_w, first_b = gw.clone(), gb.clone()
        # (b) repeats under memory pressure
        bad = torch.zeros((), dtype=torch.int64, device=DEV)
        pr = Pressure()
        gw0, gb0 = c["gw0"].to(DEV), c["gb0"].to(DEV)
        for _ in range(REPEATS):
            pr.kick()
            gw.copy_(gw0); gb.copy_(gb0)
            _wgrad(dy, x, gw, gb, splitk)
            bad += (bits(gw) != bits(first_w)).sum() + (bits(gb) != bits(first_b)).sum()
        torch.cuda.synchronize()
        assert int(bad) == 0, f"{int(bad)} elements differed between repeated launches"
        assert _outside_intact(gw, before_w) and _outside_intact(gb, before_b), "bytes outside the accumulators were written"
        if splitk > 0:      # the knob that forces the small-launch kernel's own split on forward / dgrad launches leaves a weight gradient's alone
            old = ops.FORCE_SMALL_LAUNCH, ops.FORCE_SPLITK
            ops.FORCE_SMALL_LAUNCH, ops.FORCE_SPLITK = 4, 1
            try:
                gw.copy_(gw0); gb.copy_(gb0)
                _wgrad(dy, x, gw, gb, splitk)
            finally:
                ops.FORCE_SMALL_LAUNCH, ops.FORCE_SPLITK = old
            assert torch.equal(bits(gw), bits(first_w)) and torch.equal(bits(gb), bits(first_b))
    # (a) the oracle: unsplit launches of the same family over the slices' rows, in order, option off
    with mode(False):
        ow, _ = _accumulators(c, bias=False)
        for r0, r1 in rows:
            rc, q = D.gemm_plan(lib, 5, N, K, r1 - r0, _ws_bytes(), _cus(), ops._variant_bits(), 1, dy.stride(0), x.stride(0))
            assert rc == 0 and q["kernel"] == family and q["slices"] == 1, q
            _wgrad(dy[r0:r1], x[r0:r1], ow, None, 1)
        ob = _gb_oracle(c, dy)
    torch.cuda.synchronize()
    diff = int((bits(first_w) != bits(ow)).sum())
    assert diff == 0, f"{diff} of {N * K} elements differ from the slice-by-slice oracle ({p['slices']} slices)"
    assert torch.equal(bits(first_b), bits(ob)), "the bias gradient is not the one fixed-order column-sum launch"
    # (c)
    _check_bound(c, first_w, first_b, M, p["slices"], f"single {N}x{K}x{M}")


def _pair_call(probs, M, splitk, ws=None):
    args = []
    for dy, x, gw, gb in probs:
        args += [dy.data_ptr(), x.data_ptr(), gw.data_ptr(), gb.data_ptr() if gb is not None else None, dy.shape[1], x.shape[1],
                 dy.stride(0), x.stride(0), gw.stride(0)]
    if ws is None:
        call("octmae_wgrad_accum_pair", *args, M, splitk, ops._stream())
    else:
        call("octmae_wgrad_accum_pair_ws", *args, M, splitk, ws.data_ptr(), ws.numel(), ops._stream())


@pytest.mark.parametrize("shapes,M,family,oracle_options", [
    (((256, 512), (512, 256)), 4096, 2, {"gemm_small": 0}),     # phased 256-tile pair; the oracle's short launches are kept on that family
    (((512, 1024), (1024, 512)), 3264, 3, {}),                  # 128-tile pair with a k split (see the module docstring)
])
def test_wgrad_pair_matches_the_slice_by_slice_oracle(shapes, M, family, oracle_options):
    lib = load()
    cs = [_case(N, K, M) for N, K in shapes]
    ops_dev = [_device_operands(c) for c in cs]
    with mode(True):
        rc, p = D.pair_plan(lib, shapes[0], shapes[1], M, _ws_bytes(), _cus())
        assert rc == 0 and p["kernel"] == family and p["slices"] > 1 and p["atomic1"] == D.ROUTE_SLABS and p["kstagger"] == 0 and p["colsum"] == 3, p
        d, bounds = D.split_bounds(lib, M, p["slices"], p["ta0"] * p["tb0"] + p["ta1"] * p["tb1"])
        rows = D.slice_rows(bounds, M)
        acc = [_accumulators(c) for c in cs]
        before = [(gw._base.clone(), gb._base.clone()) for gw, gb in acc]
        probs = [(dy, x, gw, gb) for (dy, x), (gw, gb) in zip(ops_dev, acc)]
        n0 = ops.set_option("gemm_small_wgrad_launches", 0)
        ops.linear_wgrad_accum_pair(probs[0], probs[1])
        assert ops.set_option("gemm_small_wgrad_launches", 0) - n0 == (1 if family == 3 else 0)
        first = [(gw.clone(), gb.clone()) for gw, gb in acc]
        bad = torch.zeros((), dtype=torch.int64, device=DEV)
        pr = Pressure()
        starts = [(c["gw0"].to(DEV), c["gb0"].to(DEV)) for c in cs]
        for _ in range(REPEATS):
            pr.kick()
            for (gw0, gb0), (gw, gb) in zip(starts, acc):
                gw.copy_(gw0); gb.copy_(gb0)
            ops.linear_wgrad_accum_pair(probs[0], probs[1])
            for (gw, gb), (fw, fb) in zip(acc, first):
                bad += (bits(gw) != bits(fw)).sum() + (bits(gb) != bits(fb)).sum()
        torch.cuda.synchronize()
        assert int(bad) == 0, f"{int(bad)} elements differed between repeated launches"
        for (gw, gb), (bw, bb) in zip(acc, before):
            assert _outside_intact(gw, bw) and _outside_intact(gb, bb)
    with mode(False, **oracle_options):
        oacc = [_accumulators(c, bias=False)[0] for c in cs]
        for r0, r1 in rows:
            rc, q = D.pair_plan_old(lib, shapes[0], shapes[1], r1 - r0, _cus(), 1)
            assert rc == 0 and q["kernel"] == family and q["slices"] == 1, q
            _pair_call([(dy[r0:r1], x[r0:r1], ow, None) for (dy, x), ow in zip(ops_dev, oacc)], r1 - r0, 1)
        obs = [_gb_oracle(c, dy) for c, (dy, _) in zip(cs, ops_dev)]
    torch.cuda.synchronize()
    for i, (c, (fw, fb), ow, ob) in enumerate(zip(cs, first, oacc, obs)):
        diff = int((bits(fw) != bits(ow)).sum())
        assert diff == 0, f"output {i}: {diff} elements differ from the slice-by-slice oracle ({p['slices']} slices)"
        assert torch.equal(bits(fb), bits(ob)), f"output {i}: bias gradient"
        _check_bound(c, fw, fb, M, p["slices"], f"pair[{i}] {shapes[i]} M={M}")


def test_a_workspace_too_small_for_the_planned_split():
    """8+ slices are planned at M = 8192, N = K = 256; a lent workspace that holds 2 slabs runs 2 -- the plan the query then reports --
    and the result is that plan's oracle.  Without any workspace the launch is unsplit, and still no atomics: bits of one unsplit launch."""
    lib = load()
    N = K = 256
    M = 8192
    c = _case(N, K, M)
    dy, x = _device_operands(c)
    small = torch.full((2 * N * K * 4 + 512,), 0xFF, dtype=torch.uint8, device=DEV)        # NaN-patterned, never initialised by us
    with mode(True):
        assert D.gemm_plan(lib, 5, N, K, M, _ws_bytes(), _cus())[1]["slices"] >= 8
        rc, p = D.gemm_plan(lib, 5, N, K, M, small.numel(), _cus(), 0, 0, dy.stride(0), x.stride(0))
        assert rc == 0 and p["slices"] == 2 and p["atomic1"] == D.ROUTE_SLABS, p
        _, bounds = D.split_bounds(lib, M, 2, 1)
        rows = D.slice_rows(bounds, M)
        gw, _ = _accumulators(c, bias=False)
        before = gw._base.clone()

        def launch(out, ws, ws_bytes):
            call("octmae_gemm_bf16_ws", dy.data_ptr(), x.data_ptr(), out.data_ptr(), None, None, None, N, K, M, dy.stride(0), x.stride(0),
                 out.stride(0), 0, 1, 1, ops.EPI_ACCUM, 0, ws, ws_bytes, ops._stream())

        launch(gw, small.data_ptr(), small.numel())
        assert _outside_intact(gw, before)
        g1, _ = _accumulators(c, bias=False)
        launch(g1, None, 0)                                                                # no workspace: unsplit
        assert D.gemm_plan(lib, 5, N, K, M, 0, _cus())[1]["slices"] == 1
    with mode(False):
        ow, _ = _accumulators(c, bias=False)
        for r0, r1 in rows:
            _wgrad(dy[r0:r1], x[r0:r1], ow, None, 1)
        o1, _ = _accumulators(c, bias=False)
        _wgrad(dy, x, o1, None, 1)
    torch.cuda.synchronize()
    assert torch.equal(bits(gw), bits(ow)) and torch.equal(bits(g1), bits(o1))
    _check_bound(c, gw, None, M, 2, "small workspace")


# ---- the fold kernel alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3, 8])
@pytest.mark.parametrize("NA,NB,ldc,ld_slab", [
    (37, 50, 56, 52),            # rows of 50: not a multiple of 4 -- the element-by-element form
    (37, 52, 64, 56),            # 16-byte form, ldc > NB
    (1030, 2048, 2052, 2048),    # 527 360 groups of 4: past the fold's grid cap of 2048 x 256 threads (a thread makes a second trip)
])
def test_fold_kernel_alone(NA, NB, ldc, ld_slab, S):
    g = np.random.default_rng(NA + NB + S)
    gw0 = g.standard_normal((NA, NB)).astype(np.float32)
    parts = [(g.standard_normal((NA, NB)) * 10.0 ** g.integers(-2, 2)).astype(np.float32) for _ in range(S)]
    stride = NA * ld_slab + 64                                             # NaN between the slabs as well
    slabs = torch.full((S * stride,), float("nan"), dtype=torch.float32, device=DEV)
    for z, p in enumerate(parts):
        slabs[z * stride:z * stride + NA * ld_slab].view(NA, ld_slab)[:, :NB] = torch.from_numpy(p).to(DEV)
    buf = torch.full((NA + 6, ldc), float("nan"), dtype=torch.float32, device=DEV)
    gw = buf[3:3 + NA, :NB]
    gw.copy_(torch.from_numpy(gw0))
    before = buf.clone()
    call("octmae_wgrad_fold", gw.data_ptr(), slabs.data_ptr(), S, NA, NB, ldc, ld_slab, stride, ops._stream())
    torch.cuda.synchronize()
    want = D.fold(gw0, parts)
    assert np.array_equal(gw.cpu().numpy().view(np.int32), want.view(np.int32)), "the fold is not ((gW + P_0) + P_1) ... in fp32"
    assert _outside_intact(gw, before), "gW outside the matrix changed"
    assert bool(torch.isnan(slabs).any()) and not bool(torch.isnan(gw).any())


# ---- fc1's bias gradient of the dgrad x GELU' launch without a column-sum workspace -----------------------------------------------------
def test_dgelu_bias_gradient_without_a_workspace():
    lib = load()
    M, K, N = 4096, 256, 256
    g = torch.Generator().manual_seed(11)
    dy = NF.embed(torch.randn(M, N, generator=g).to(LP), device=DEV)
    w = NF.embed((torch.randn(N, K, generator=g) * N ** -0.5).to(LP), device=DEV)
    pre = NF.embed(torch.randn(M, K, generator=g).to(LP), device=DEV)
    cs0 = torch.randn(K, generator=g)
    out = (ctypes.c_int * 13)()
    with mode(False):
        assert lib.octmae_gemm_plan(2, K, M, N, w.stride(0), dy.stride(0), ops._variant_bits(), 1, 1, _cus(), out) == 0 and out[12] == 1
    with mode(True):
        assert lib.octmae_gemm_plan(2, K, M, N, w.stride(0), dy.stride(0), ops._variant_bits(), 1, 1, _cus(), out) == 0 and out[12] == 4
        cs0d = cs0.to(DEV)
        cs = cs0d.clone()
        dx0 = ops.linear_dgrad(dy, w, pre=pre, colsum=cs, atomic_colsum=True)
        first = cs.clone()
        bad = torch.zeros((), dtype=torch.int64, device=DEV)
        pr = Pressure()
        for _ in range(REPEATS):
            pr.kick()
            cs.copy_(cs0d)
            dx = ops.linear_dgrad(dy, w, pre=pre, colsum=cs, atomic_colsum=True)
            bad += (bits(cs) != bits(first)).sum() + (dx.view(torch.int16) != dx0.view(torch.int16)).sum()
        torch.cuda.synchronize()
    assert int(bad) == 0
    dsd = dx0.double().cpu()
    r, at = GE.worst(first, cs0.double() + dsd.sum(0), (M + 8) * GE.EPS32 * (cs0.double().abs() + dsd.abs().sum(0)))
    print(f"deterministic/dgelu_colsum: worst |got - ref| / bound = {r:.4f} at {at}")
    assert r <= 1.0, (r, at)


# ---- gradient norm ---------------------------------------------------------------------------------------------------------------------
def _norm_tensors():
    """one tensor of 5 x 65536 + 123 elements at a 4-byte- but not 16-byte-aligned address, and tensors of 1, 7 and 65536 elements;
    p, g, m, v share the layout (the AdamW kernel's 16-byte form looks at all four addresses)"""
    chunk = load().octmae_mt_chunk_elems()
    assert chunk == 65536
    lengths = [5 * chunk + 123, 1, 7, chunk]
    g = torch.Generator().manual_seed(5)
    roles = {}
    for r in "pgmv":
        views = []
        for n in lengths:
            buf = torch.randn(n + 9, generator=g).abs_().to(DEV) if r == "v" else torch.randn(n + 9, generator=g).to(DEV)
            views.append(buf[1:1 + n] if n > chunk else buf[4:4 + n])
        roles[r] = views
    assert roles["g"][0].data_ptr() % 16 == 4 and roles["g"][3].data_ptr() % 16 == 0
    return chunk, lengths, roles


def _chunk_views(chunk, views):
    return [v[o:o + chunk] for v in views for o in range(0, v.numel(), chunk)]


def _sumsq(tab, n, partial=None):
    sq = torch.zeros(n, dtype=torch.float32, device=DEV)
    if partial is None:
        call("octmae_mt_sumsq", tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(), tab.n_chunks, sq.data_ptr(), ops._stream())
    else:
        call("octmae_mt_sumsq_ws", tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(), tab.n_chunks, sq.data_ptr(),
             partial.data_ptr(), ops._stream())
    return sq


def _adamw_sumsq(tab, n, partial=None):
    sq = torch.zeros(n, dtype=torch.float32, device=DEV)
    head = (tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(), tab.n_chunks, None, None, sq.data_ptr())
    tail = (1e-3, 0.9, 0.95, 1e-8, 0.05, 1, ops._stream())
    if partial is None:
        call("octmae_mt_adamw_fused", *head, *tail)
    else:
        call("octmae_mt_adamw_fused_ws", *head, partial.data_ptr(), *tail)
    return sq


@pytest.mark.parametrize("kernel", ["sumsq", "adamw"])
def test_gradient_norm_adds_its_chunks_in_order(kernel):
    chunk, lengths, R = _norm_tensors()
    run = _sumsq if kernel == "sumsq" else _adamw_sumsq
    whole = _MultiTensorTable(R["p"], R["g"], R["m"], R["v"])
    assert whole.n_chunks == 6 + 3
    # every chunk as a tensor of its own, default mode: the value the kernel adds for it today (one addend onto zero)
    pieces = _MultiTensorTable(*[_chunk_views(chunk, R[r]) for r in "pgmv"])
    assert pieces.n_chunks == pieces.n_tensors == whole.n_chunks
    with mode(False):
        per_chunk = run(pieces, pieces.n_tensors).cpu().numpy()
    want = np.float32([D.chunk_sum(per_chunk[:6]), per_chunk[6], per_chunk[7], per_chunk[8]])
    with mode(True):
        partial = torch.full((whole.n_chunks,), float("nan"), dtype=torch.float32, device=DEV)
        first = run(whole, whole.n_tensors, partial)
        bad = torch.zeros((), dtype=torch.int64, device=DEV)
        pr = Pressure()
        for _ in range(REPEATS):
            pr.kick()
            bad += (bits(run(whole, whole.n_tensors, partial)) != bits(first)).sum()
        torch.cuda.synchronize()
        # the mode never falls back to adding in finishing order: without the workspace the call is refused
        with pytest.raises(Exception, match="bad argument"):
            run(whole, whole.n_tensors)
    assert int(bad) == 0
    assert np.array_equal(partial.cpu().numpy().view(np.int32), per_chunk.view(np.int32)), "a chunk's partial is not today's one-chunk value"
    assert np.array_equal(first.cpu().numpy().view(np.int32), want.view(np.int32)), (first.cpu().numpy(), want)
    exact = np.float64([float((v.double() ** 2).sum()) for v in R["g"]])
    assert np.all(np.abs(first.cpu().numpy() - exact) <= (np.float64(lengths) + 8) * GE.EPS32 * exact)


def test_grad_norm_and_coef_uses_the_workspace_under_the_option():
    _, lengths, R = _norm_tensors()
    ps = [torch.nn.Parameter(p.clone()) for p in R["p"]]
    for p, g in zip(ps, R["g"]):
        p.grad = g.clone()
    with mode(True):
        a = foptim.grad_norm_and_coef(ps, 1.0, {})
        b = foptim.grad_norm_and_coef(ps, 1.0, {})
    with mode(False):
        c = foptim.grad_norm_and_coef(ps, 1.0, {})
    torch.cuda.synchronize()
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    assert abs(float(a[0]) - float(c[0])) <= 1e-5 * float(c[0])


# ---- model level -------------------------------------------------------------------------------------------------------------------------
def _train_three_steps(golden_dir, batch, pressure):
    from tests import test_gpu_model as TM
    z, cfg, P = TM.small(golden_dir)
    m = TM.build(cfg, P).train()
    opt = foptim.FusedAdamW(misc.add_weight_decay(m, 0.05), lr=1e-3, betas=(0.9, 0.95))
    scaler = misc.NativeScalerWithGradNormCount(fp32=True)
    torch.manual_seed(3)
    losses, norms = [], []
    for step in range(3):
        imgs = torch.rand(batch, 1, cfg.num_frames, cfg.input_size, cfg.input_size, generator=torch.Generator().manual_seed(10 + step)).to(DEV)
        noise = torch.rand(batch, cfg.num_patches, generator=torch.Generator().manual_seed(20 + step)).to(DEV)
        if pressure is not None:
            pressure.n = 0
            pressure.kick()
        opt.zero_grad()
        loss, _, _ = m(imgs, mask_ratio=0.75, noise=noise)
        norm = scaler(loss, opt, clip_grad=0.5, parameters=m.parameters())
        losses.append(loss.detach().clone())
        norms.append(torch.as_tensor(norm).detach().clone())
    torch.cuda.synchronize()
    return losses, norms, {k: v.detach().clone() for k, v in m.state_dict().items()}, cfg


def test_three_optimizer_steps_are_bit_reproducible(golden_dir):
    lib = load()
    batch = 61                               # 61 x (16 kept patches + cls) = 1037 kept rows
    with mode(True):
        a = _train_three_steps(golden_dir, batch, None)
        cfg = a[3]
        rows = batch * (cfg.num_patches // 4 + 1)
        assert rows >= 1024
        C = cfg.embed_dim
        # the plans of the launches a Block's backward issues: a pair (ops.linear_wgrad_accum_pair) where the library takes one,
        # else -- as at this width, below the 256-tile kernels -- the two single launches the wrapper falls back to
        plans = []
        for a_, b_ in (((3 * C, C), (C, C)), ((4 * C, C), (C, 4 * C))):
            rc, p = D.pair_plan(lib, a_, b_, rows, _ws_bytes(), _cus())
            assert rc in (0, -2)
            plans += [p] if rc == 0 else [D.gemm_plan(lib, 6, N, K, rows, _ws_bytes(), _cus())[1] for N, K in (a_, b_)]
        assert any(p["slices"] > 1 and p["atomic1"] == D.ROUTE_SLABS for p in plans), f"no weight gradient of the step is split: {plans}"
        b = _train_three_steps(golden_dir, batch, Pressure())
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(bits(x.float()), bits(y.float())), "loss / gradient norm"
    print("deterministic/model: gradient norms of the three steps", [float(n) for n in a[1]], "(clip at 0.5)")
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def _run_block(blk, level, x, w):
    blk.recompute = level
    with torch.no_grad():
        blk(x)
    arena = get_arena(blk)
    arena.zero_grad()
    xg = x.clone().requires_grad_(True)
    out = blk(xg)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), xg.grad.clone(), {n: p.grad.clone() for n, p in blk.named_parameters()}


def test_block_recomputation_levels_are_bit_equal_at_full_size():
    """width 256, 4096 rows: the qkv + proj and fc1 + fc2 weight-gradient pairs are split there, so without the mode the three levels
    agree only up to the order of the fp32 atomics (README, recomputation)."""
    lib = load()
    C, B, N = 256, 8, 512
    blk = video_vit.Block(C, 4, 4.0, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n_, p_ in blk.named_parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) * (0.05 if p_.dim() > 1 else 0.02) + (1.0 if "norm" in n_ and n_.endswith("weight") else 0.0))
    blk = blk.to(DEV).train()
    x = torch.randn(B, N, C, generator=g).to(DEV)
    w = torch.randn(B, N, C, generator=g).to(DEV)
    with mode(True):
        for a, b in (((3 * C, C), (C, C)), ((4 * C, C), (C, 4 * C))):
            rc, p = D.pair_plan(lib, a, b, B * N, _ws_bytes(), _cus())
            assert rc == 0 and p["slices"] > 1 and p["atomic1"] == D.ROUTE_SLABS, p
        base = _run_block(blk, "none", x, w)
        assert all(float(v.abs().max()) > 0 for n_, v in base[2].items() if ".k.bias" not in n_ and "k_bias" not in n_)
        for level in ("light", "full", "none"):
            got = _run_block(blk, level, x, w)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), level
            for n_ in base[2]:
                assert torch.equal(got[2][n_], base[2][n_]), (level, n_, float((got[2][n_] - base[2][n_]).abs().max()))


def test_option_off_afterwards_is_the_default_plan_again():
    """after everything above: the option is off, a weight gradient plans as the release does (16 slices, the batched read-modify-write
    route for unsplit launches, the bias gradient inside the kernel) and its launch meets the bound"""
    lib = load()
    assert ops.is_deterministic() is False
    N = K = 256
    M = 8192
    rc, p = D.gemm_plan(lib, 6, N, K, M, _ws_bytes(), _cus())
    assert rc == 0 and (p["kernel"], p["slices"], p["per"], p["atomic1"], p["colsum"]) == (2, 16, 8, 2, 1), p
    assert D.gemm_plan_old(lib, 6, N, K, M, 1, _cus()) == (rc, p)
    c = _case(N, K, M)
    dy, x = _device_operands(c)
    gw, gb = _accumulators(c)
    ops.linear_wgrad_accum(dy, x, gw, gb)
    torch.cuda.synchronize()
    _check_bound(c, gw, gb, M, p["slices"], "default mode")
