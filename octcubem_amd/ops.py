"""Operators of the 3-D MAE hot path: thin wrappers over the C ABI (liboctmae.so) and the
torch.autograd.Function glue that strings them into forward/backward.

Numerics policy: fp32 residual stream / LayerNorm statistics / softmax statistics /
accumulators / master weights and weight gradients; bf16 GEMM and attention operands.

Weight gradients are accumulated by the wgrad GEMM (fp32, split-K) DIRECTLY into ``param.grad`` (the
model pre-binds ``param.grad`` to views of one flat gradient arena, see models_mae._ParamArena), so the
Functions below return ``None`` for parameters and call ``notify_grad_ready`` instead -- that is the hook
the data-parallel reducer uses to overlap the RCCL all-reduce with backward.
"""
from __future__ import annotations

import math
import os
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from ._lib import OctmaeError, call, load


def _lp_dtype():
    """The torch dtype of the library's 16-bit operand type (octmae_lp_dtype): bfloat16 for liboctmae.so, float16 for the
    verification build liboctmae_f16.so (OCTMAE_LIB).  A library that is missing or cannot be loaded here (a CPU-only box) is
    reported by the first compute call, not by the import; bfloat16 is assumed until then and CHECKED when the library does load."""
    try:
        return torch.float16 if load().octmae_lp_dtype() == 1 else torch.bfloat16
    except OctmaeError:
        return torch.bfloat16


BF16 = _lp_dtype()                 # named for the shipped build; every "bf16" below means "the library's 16-bit operand type"
LP_IS_F16 = BF16 == torch.float16


def _check_lp_dtype(lib):
    got = torch.float16 if lib.octmae_lp_dtype() == 1 else torch.bfloat16
    if got != BF16:
        raise OctmaeError(f"the library computes on {got} operands but octcubem_amd.ops was imported assuming {BF16} (the library was "
                          "built or selected after the import): restart the process with OCTMAE_LIB set before importing octcubem_amd")


from . import _lib as _libmod  # noqa: E402
_libmod._on_load.append(_check_lp_dtype)
F32 = torch.float32
_CHECK_IDS = os.environ.get("OCTMAE_CHECK_IDS", "0") == "1"    # verify the permutation contract of the assembly ops per call

EPI_BF16, EPI_F32, EPI_GELU, EPI_RESID, EPI_DGELU, EPI_ACCUM = range(6)


def _stream():
    # the raw handle of the current stream of the current device: 0.3 us, against 8 us for torch.cuda.current_stream().cuda_stream
    # (a Stream object per call) -- per launch, ~240 times per forward + backward (tools/host_overhead_profile.py)
    try:
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    except AttributeError:      # a PyTorch without these private accessors
        return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    return t


# ------------------------------------------------------------------------------------------------
# grad-ready notification (used by parallel.FlatGradReducer)
# ------------------------------------------------------------------------------------------------
# Several reducers may listen during one backward (the COEM step drives one FlatGradReducer per tower): every subscriber sees
# every notification and picks out the parameters of its own arena.  Keyed by owner so that a reducer replaces / removes only
# its own entry (a single global callback let the second reducer's begin_backward() silence the first).
_grad_ready_subs: dict = {}


def add_grad_ready_callback(owner, cb: Callable[[Sequence[torch.nn.Parameter]], None]):
    _grad_ready_subs[id(owner)] = cb


def remove_grad_ready_callback(owner):
    _grad_ready_subs.pop(id(owner), None)


def set_grad_ready_callback(cb):
    """Single-subscriber form kept for callers that own the whole backward: replaces every subscription (None: clears)."""
    _grad_ready_subs.clear()
    if cb is not None:
        _grad_ready_subs[0] = cb


def notify_grad_ready(params):
    if _grad_ready_subs:
        ps = [p for p in params if p is not None]
        for cb in list(_grad_ready_subs.values()):
            cb(ps)


# ------------------------------------------------------------------------------------------------
# weight-gradient switch (saliency passes: only the activation gradients are wanted)
# ------------------------------------------------------------------------------------------------
_weight_grads = True       # module-level, not thread-local: a backward runs on autograd's worker thread


def weight_grads_enabled() -> bool:
    return _weight_grads


class weight_grads:
    """Context manager: ``with ops.weight_grads(False):`` -- a backward that RUNS inside launches no weight-gradient GEMM, no bias
    column sum, no LayerNorm parameter gradient and no positional / cls / mask-token gradient from any Function of this file, touches no
    gradient buffer (``ctx.grads()`` is not called) and notifies no reducer.  The activation-gradient launches are the same ones, so
    the input gradient is bit-identical either way.  Read when a backward runs, not when the forward ran; nests, and restores the
    previous state on exit, also when the body raises."""

    def __init__(self, enabled: bool):
        self.enabled = bool(enabled)
        self._prev: List[bool] = []

    def __enter__(self):
        global _weight_grads
        self._prev.append(_weight_grads)
        _weight_grads = self.enabled
        return self

    def __exit__(self, *exc):
        global _weight_grads
        _weight_grads = self._prev.pop()
        return False


def grad_buf(p: torch.nn.Parameter) -> torch.Tensor:
    """The fp32 buffer weight gradients are accumulated into (``p.grad``; created zeroed if absent)."""
    if p.grad is None:
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return p.grad


# ------------------------------------------------------------------------------------------------
# per-launch timing (bench.py): HIP events on the stream the kernels are launched on
# ------------------------------------------------------------------------------------------------
class KernelTimer:
    """Brackets single-kernel launches with events on the launch stream; kind -> [(start, end)] plus per-kind launch counts
    and algorithmic flop / byte totals.  Only every ``stride``-th launch of a kind is bracketed (two event records per
    launch cost ~3 % of a step when every one of the ~7000 launches is timed); totals are scaled up by count / sampled.
    The stride is 5 -- coprime with the periods (2, 3, 4) in which differently-shaped GEMMs of one kind alternate inside a
    Block, so every shape is sampled in proportion (a stride of 4 only ever timed one of the four weight-gradient shapes)."""

    def __init__(self, stride: int = 5):
        self.stride = max(1, int(stride))
        self.records = {}
        self.stats = {}

    def launch(self, kind, flops, nbytes, fn, exec_flops=None):
        """flops: ALGORITHMIC (attention forward 4 B H N^2 hd, backward 8 B H N^2 hd = x3 in total);
        exec_flops: what the kernel executes (recomputed products included), defaults to flops.
        fn returning False: nothing was launched (the library's -2; the caller goes another way), so nothing is counted."""
        st = self.stats.setdefault(kind, [0, 0.0, 0.0, 0.0])
        sampled = st[0] % self.stride == 0
        if sampled:
            s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
            s.record()
        if fn() is False:
            return
        st[0] += 1; st[1] += flops; st[2] += nbytes; st[3] += flops if exec_flops is None else exec_flops
        if sampled:
            e.record()
            self.records.setdefault(kind, []).append((s, e))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kind, recs in self.records.items():
            n, flops, nbytes, xflops = self.stats[kind]
            ms = sum(s.elapsed_time(e) for s, e in recs)
            avg_us = 1e3 * ms / len(recs)
            out[kind] = {"launches": n, "sampled": len(recs), "total_ms": avg_us * n * 1e-3, "avg_us": avg_us, "flops": flops,
                         "bytes": nbytes, "exec_flops": xflops}
        return out


KTIMER: Optional[KernelTimer] = None


def _launch(kind, flops, nbytes, fn, exec_flops=None):
    if KTIMER is None:
        fn()
    else:
        KTIMER.launch(kind, flops, nbytes, fn, exec_flops)


# ------------------------------------------------------------------------------------------------
# raw ops
# ------------------------------------------------------------------------------------------------
def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    if x.dtype == BF16:
        return x.contiguous()
    x = x.contiguous()
    _chk(x, F32, "cast_bf16")
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    call("octmae_cast_f32_bf16", x.data_ptr(), out.data_ptr(), x.numel(), _stream())
    return out


def cast_bf16_rowscale(x2d: torch.Tensor, rowscale: torch.Tensor, rows_per_scale: int) -> torch.Tensor:
    """bf16(rowscale[r // rows_per_scale] * x2d[r]) for fp32 x2d [R, D] (the gradient entering a stochastic-depth branch)."""
    _chk(x2d, F32, "cast_bf16_rowscale"); _chk(rowscale, F32, "rowscale")
    R, D = x2d.shape
    assert rowscale.numel() * rows_per_scale == R
    out = torch.empty((R, D), dtype=BF16, device=x2d.device)
    call("octmae_cast_rowscale_f32_bf16", x2d.data_ptr(), rowscale.data_ptr(), out.data_ptr(), R, D, rows_per_scale, _stream())
    return out


def cast_bf16_into(src: torch.Tensor, dst: torch.Tensor):
    call("octmae_cast_f32_bf16", src.data_ptr(), dst.data_ptr(), src.numel(), _stream())


def colsum_accum(x2d: torch.Tensor, out: torch.Tensor):
    """out[c] += sum_r x2d[r][c] (fp32 accumulate).  The additions have a fixed order (octmae_colsum_accum_ws: beyond 256 rows the row
    splits leave their sums in a workspace and a second launch folds them), so a gradient accumulated over several backwards does not
    depend on the order the workgroups finish in."""
    M, N = x2d.shape
    rows = load().octmae_colsum_ws_rows(M)
    ws = torch.empty((rows, N), dtype=F32, device=x2d.device) if rows else None
    call("octmae_colsum_accum_ws", x2d.data_ptr(), 1 if x2d.dtype == BF16 else 0, out.data_ptr(), _p(ws), M, N, x2d.stride(0), _stream())


_GEMM_KIND = {(0, 0): "gemm_fwd", (1, 0): "gemm_dgrad", (1, 1): "gemm_wgrad"}


FORCE_SMALL_TILE = False    # tests: route every GEMM through the 128-tile register-staged kernel
FORCE_TWO_STAGE = False     # tests / A-B: the un-phased two-stage main loop of the 256-tile kernel
FORCE_PHASED = False        # tests / A-B: the phased main loop also where the two-stage one is the default
FORCE_SMALL_LAUNCH = 0      # tests / A-B: 4 or 2 = every forward / dgrad GEMM through gemm128d_kernel with that ring depth (its k split:
FORCE_SPLITK = 1            #   FORCE_SPLITK, 1 .. 4); -1 = never that kernel (the pre-round-6 choice)


# The fc1 forward's epilogue stores gelu'(pre) in place of pre and the fc2 dgrad's epilogue multiplies with it (VERDICT r05 item 3,
# route i): one more 16-bit rounding point (gelu' itself), no transcendental in the backward epilogue.  bench.py --set
# ops.GELU_PRIME_FWD=1 for the same-box A/B of the step; the flag a forward ran with travels with its saved tensor.
GELU_PRIME_FWD = os.environ.get("OCTMAE_GELU_PRIME_FWD", "0") == "1"


def _variant_bits():
    return (0x100 if FORCE_SMALL_TILE else 0) | (0x200 if FORCE_TWO_STAGE else 0) | (0x400 if FORCE_PHASED else 0) | \
        (0x1000 if FORCE_SMALL_LAUNCH == 4 else 0x2000 if FORCE_SMALL_LAUNCH == 2 else 0x4000 if FORCE_SMALL_LAUNCH < 0 else 0) | \
        (((FORCE_SPLITK & 7) << 16) if FORCE_SMALL_LAUNCH > 0 else 0)


# Split-K workspace of the small-launch forward / dgrad kernel (octmae_gemm_bf16_ws): one per (device, stream) -- launches on one
# stream run one after the other and may share it, launches on different streams may not.  64 MiB of partial-tile slots + 16 KiB of
# arrival counters, zeroed once (every launch leaves the counters zero).  ON by default since round 6: a long reduction on few
# tiles (the fc2 forward of ONE volume: 88 tiles of 128 x 128, K = 4096) is split 2-4 ways, deterministically (csrc/gemm.hip,
# gemm128d_kernel).  OCTMAE_SPLIT_WS=0 / bench.py --set ops.SPLIT_WS=0: never lend it (no launch is split).
SPLIT_WS = os.environ.get("OCTMAE_SPLIT_WS", "1") != "0"
_split_ws = {}


def _split_ws_for(st: int):
    """(pointer, bytes) of the current device's workspace for stream handle `st`, or (None, 0)."""
    if not SPLIT_WS:
        return None, 0
    key = (torch.cuda.current_device(), st)
    ws = _split_ws.get(key)
    if ws is None:
        if len(_split_ws) >= 8:                     # a process that keeps creating streams: do not hoard 64 MiB for each
            _split_ws.clear()
        ws = _split_ws[key] = torch.zeros(load().octmae_gemm_split_ws_kib() * 1024, dtype=torch.uint8, device="cuda")
    return ws.data_ptr(), ws.numel()


def _gemm(A, B, C, NA, NB, K, lda, ldb, ldc, a_ks, b_ks, epi, C2=None, bias=None, aux=None, ldaux=0, splitk=0):
    st = _stream()
    # forward / dgrad kinds: lend the split-K workspace; weight gradients: in deterministic mode, for the slabs of their k slices
    if ((epi & 0xff) != EPI_ACCUM and not FORCE_SMALL_TILE) or ((epi & 0xff) == EPI_ACCUM and is_deterministic()):
        skp, skn = _split_ws_for(st)
        args = (A.data_ptr(), B.data_ptr(), C.data_ptr(), _p(C2), _p(bias), _p(aux), NA, NB, K, lda, ldb, ldc, ldaux, a_ks, b_ks,
                epi | _variant_bits(), FORCE_SPLITK if FORCE_SMALL_LAUNCH > 0 and (epi & 0xff) != EPI_ACCUM else splitk, skp, skn, st)
        fn = "octmae_gemm_bf16_ws"
    else:
        args = (A.data_ptr(), B.data_ptr(), C.data_ptr(), _p(C2), _p(bias), _p(aux), NA, NB, K, lda, ldb, ldc, ldaux, a_ks, b_ks,
                epi | _variant_bits(), splitk, st)
        fn = "octmae_gemm_bf16"
    if KTIMER is None:
        call(fn, *args)
    else:
        kind = f"{_GEMM_KIND.get((a_ks, b_ks), 'gemm')}_epi{epi & 0xff}"
        # algorithmic bytes: both operands once, the output, the second output of the GELU epilogue (2), the residual (3) or
        # pre-activation (4) the epilogue reads
        nbytes = 2.0 * (NA * K + NB * K) + C.element_size() * NA * NB
        if (epi & 0xff) == 2 and C2 is not None:
            nbytes += C2.element_size() * NA * NB
        if (epi & 0xff) in (3, 4) and aux is not None:
            nbytes += aux.element_size() * NA * NB
        KTIMER.launch(kind, 2.0 * NA * NB * K, nbytes, lambda: call(fn, *args))


def linear_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], mode: str = "bf16",
               res: Optional[torch.Tensor] = None, rowscale: Optional[torch.Tensor] = None, rows_per_scale: int = 1,
               store_dgelu: bool = False):
    """y = x @ w.T + bias.  x bf16 [M,K], w bf16 [N,K], bias f32 [N].
    mode: 'bf16' | 'f32' | 'gelu' (returns (pre, act)) | 'resid' (f32: res + y, or res + rowscale[m // rows_per_scale] * y)."""
    M, K = x.shape
    N = w.shape[0]
    dev = x.device
    if rowscale is not None:
        assert mode == "resid" and rowscale.dtype == F32 and rowscale.numel() * rows_per_scale == M
        out = torch.empty((M, N), dtype=F32, device=dev)
        st = _stream()
        args = (w.data_ptr(), x.data_ptr(), out.data_ptr(), _p(bias), res.data_ptr(), rowscale.data_ptr(), rows_per_scale, N, M, K,
                w.stride(0), x.stride(0), N, res.stride(0), _variant_bits(), *_split_ws_for(st), st)
        _launch(f"gemm_fwd_epi{EPI_RESID}", 2.0 * N * M * K, 2.0 * (N * K + M * K) + 8.0 * N * M,
                lambda: call("octmae_linear_resid_rowscale", *args))
        return out
    if mode == "bf16":
        out = torch.empty((M, N), dtype=BF16, device=dev)
        _gemm(w, x, out, N, M, K, w.stride(0), x.stride(0), N, 0, 0, EPI_BF16, bias=bias)
        return out
    if mode == "f32":
        out = torch.empty((M, N), dtype=F32, device=dev)
        _gemm(w, x, out, N, M, K, w.stride(0), x.stride(0), N, 0, 0, EPI_F32, bias=bias)
        return out
    if mode == "gelu":
        pre = torch.empty((M, N), dtype=BF16, device=dev)
        act = torch.empty((M, N), dtype=BF16, device=dev)
        # store_dgelu: `pre` receives gelu'(pre-activation) -- what linear_dgrad(..., pre_is_dgelu=True) multiplies with
        _gemm(w, x, pre, N, M, K, w.stride(0), x.stride(0), N, 0, 0, EPI_GELU | (0x8000 if store_dgelu else 0), C2=act, bias=bias)
        return pre, act
    if mode == "resid":
        out = torch.empty((M, N), dtype=F32, device=dev)
        _gemm(w, x, out, N, M, K, w.stride(0), x.stride(0), N, 0, 0, EPI_RESID, bias=bias, aux=res, ldaux=res.stride(0))
        return out
    raise ValueError(mode)


def linear_dgrad(dy: torch.Tensor, w: torch.Tensor, pre: Optional[torch.Tensor] = None,
                 colsum: Optional[torch.Tensor] = None, atomic_colsum: bool = False, pre_is_dgelu: bool = False,
                 fold_entry: bool = False) -> torch.Tensor:
    """dx[M,K] = dy[M,N] @ w[N,K]  (optionally * gelu'(pre[M,K])), bf16.  With ``pre``, ``colsum`` (fp32 [K]) receives
    += the column sums of dx -- the bias gradient of the Linear that produced ``pre`` -- from the same call: per-slab partial
    sums through a workspace and a folding launch (octmae_linear_dgrad_dgelu); ``atomic_colsum`` selects the
    fp32-atomic form of octmae_gemm_bf16's epilogue 4 instead (kept for comparison)."""
    M, N = dy.shape
    K = w.shape[1]
    dx = torch.empty((M, K), dtype=BF16, device=dy.device)
    if pre is None:
        assert colsum is None
        _gemm(w, dy, dx, K, M, N, w.stride(0), dy.stride(0), K, 1, 0, EPI_BF16)
    elif (colsum is None and not fold_entry) or atomic_colsum:
        _gemm(w, dy, dx, K, M, N, w.stride(0), dy.stride(0), K, 1, 0, EPI_DGELU | (0x8000 if pre_is_dgelu else 0), C2=colsum, aux=pre,
              ldaux=pre.stride(0))
    else:
        # fold_entry without colsum (weight gradients switched off, and the Linear that produced ``pre`` has a bias): the entry point
        # the switched-on backward takes, the side output a null pointer.  A bias-free Linear takes the branch above either way.
        ws = None
        if colsum is not None:
            rows = load().octmae_dgelu_colsum_ws_rows(M)
            ws = torch.empty((rows, K), dtype=F32, device=dy.device)
        st = _stream()
        args = (w.data_ptr(), dy.data_ptr(), dx.data_ptr(), pre.data_ptr(), _p(ws), _p(colsum), M, N, K, w.stride(0),
                dy.stride(0), K, pre.stride(0), _variant_bits() | (0x8000 if pre_is_dgelu else 0), *_split_ws_for(st), st)
        if KTIMER is None:
            call("octmae_linear_dgrad_dgelu", *args)
        else:   # two launches (GEMM + the fold of the partial sums), timed together
            KTIMER.launch("gemm_dgrad_epi4", 2.0 * K * M * N, 2.0 * (K * N + M * N) + 2.0 * K * M + 2.0 * K * M,      # + the pre-activation read
                          lambda: call("octmae_linear_dgrad_dgelu", *args))
    return dx


DGRAD_DELTA = True     # the proj dgrad also produces the attention backward's delta (octmae_linear_dgrad_delta); A/B: bench.py --set ops.DGRAD_DELTA=0


def linear_dgrad_delta(dy: torch.Tensor, w: torch.Tensor, o: torch.Tensor, H: int, HD: int):
    """dx[M,K] = dy[M,N] @ w[N,K] (bf16) and delta[M,H] (fp32) = -sum over each head's HD columns of dx * o -- the attention
    backward's per-query constant, from the epilogue of the GEMM that produces dO (no separate pass over O and dO).
    Returns (dx, None) when the shape does not take the fused kernel (the caller then lets octmae_attn_bwd_fused compute it)."""
    M, N = dy.shape
    K = w.shape[1]
    if not (DGRAD_DELTA and not FORCE_SMALL_TILE and M >= 256 and K >= 256 and N % 64 == 0 and K % 8 == 0 and H * HD == K and H <= 64
            and HD in (32, 64)):
        return linear_dgrad(dy, w), None
    dx = torch.empty((M, K), dtype=BF16, device=dy.device)
    delta = torch.empty((M, H), dtype=F32, device=dy.device)
    st = _stream()
    args = (w.data_ptr(), dy.data_ptr(), dx.data_ptr(), o.data_ptr(), delta.data_ptr(), M, N, K, w.stride(0), dy.stride(0), K, o.stride(0),
            H, HD, _variant_bits(), *_split_ws_for(st), st)
    rc = [0]

    def run():
        rc[0] = load().octmae_linear_dgrad_delta(*args)
        return rc[0] != -2

    _launch("gemm_dgrad_epi6", 2.0 * K * M * N, 2.0 * (K * N + M * N) + 2.0 * K * M + 2.0 * K * M, run)
    if rc[0] == -2:           # the library's own applicability test (plan_gemm, EPI_DELTA) said no (e.g. an operand beyond a 32-bit buffer range): plain dgrad
        return linear_dgrad(dy, w), None
    if rc[0] != 0:
        raise RuntimeError(f"octmae_linear_dgrad_delta failed (rc={rc[0]})")
    return dx, delta


def linear_wgrad_accum(dy: torch.Tensor, x: torch.Tensor, gw: torch.Tensor, gb: Optional[torch.Tensor] = None):
    """gw[N,K] (f32) += dy[M,N].T @ x[M,K]; with ``gb`` (f32 [N]) also gb += dy.sum(0) -- the bias gradient, taken from the
    dY tiles the weight-gradient kernel stages anyway (one extra MFMA per k-step in the first column of tiles) instead of a
    separate pass over dY."""
    M, N = dy.shape
    K = x.shape[1]
    _gemm(dy, x, gw, N, K, M, dy.stride(0), x.stride(0), gw.stride(0), 1, 1, EPI_ACCUM, C2=gb)    # k split: the planner's (auto_wgrad_split)


# fc1 + fc2 and qkv + proj weight gradients of a Block as one launch each (octmae_wgrad_accum_pair); OCTMAE_WGRAD_PAIR=0: same-box A/B
WGRAD_PAIR = os.environ.get("OCTMAE_WGRAD_PAIR", "1") != "0"


def linear_wgrad_accum_pair(first, second):
    """Two linear_wgrad_accum calls over the same token rows -- (dy, x, gw, gb) each -- as ONE launch: the tiles of both outputs
    share the split over the rows, so there are half as many fp32-atomic epilogues and the k-loops are twice as long (measured on
    the combined shape, profiles/r04_wgrad_pair.txt: -12 ... -15 % at 32 volumes, -2 ... -7 % at 128).  Falls back to two launches when
    the library says the pair does not apply (-2) or WGRAD_PAIR is off."""
    (dy0, x0, gw0, gb0), (dy1, x1, gw1, gb1) = first, second
    M = dy0.shape[0]
    # the pair entry point has no variant argument, hence the switch tests; whether the shapes take it is the library's answer (-2)
    if WGRAD_PAIR and not FORCE_SMALL_TILE and dy1.shape[0] == M and x0.shape[0] == M and x1.shape[0] == M:
        rc = [0]
        args = []
        for dy, x, gw, gb in (first, second):
            for t_, dt_, nm_ in ((dy, BF16, "dy"), (x, BF16, "x"), (gw, F32, "gw")):       # rows may be slices of wider tensors
                if not (t_.is_cuda and t_.dtype == dt_ and t_.dim() == 2 and t_.stride(1) == 1):
                    raise RuntimeError(f"linear_wgrad_accum_pair: {nm_} must be a GPU {dt_} matrix with contiguous rows")
            args += [dy.data_ptr(), x.data_ptr(), gw.data_ptr(), _p(gb), dy.shape[1], x.shape[1], dy.stride(0), x.stride(0), gw.stride(0)]
        det = is_deterministic()                         # the slabs of the k slices live in the stream's split-K workspace
        st = _stream()
        args += [M, 0] + (list(_split_ws_for(st)) if det else []) + [st]     # k split 0: the planner's (auto_wgrad_split)
        pair = load().octmae_wgrad_accum_pair_ws if det else load().octmae_wgrad_accum_pair

        def run():
            rc[0] = pair(*args)
            return rc[0] != -2

        fl = 2.0 * M * (dy0.shape[1] * x0.shape[1] + dy1.shape[1] * x1.shape[1])
        nb = 2.0 * M * (dy0.shape[1] + x0.shape[1] + dy1.shape[1] + x1.shape[1]) + 4.0 * (gw0.numel() + gw1.numel())
        _launch("gemm_wgrad_epi5", fl, nb, run)
        if rc[0] == 0:
            return
        if rc[0] != -2:
            raise RuntimeError(f"octmae_wgrad_accum_pair failed (rc={rc[0]})")
    linear_wgrad_accum(dy0, x0, gw0, gb0)
    linear_wgrad_accum(dy1, x1, gw1, gb1)


def layernorm_fwd(x: torch.Tensor, gamma, beta, eps: float):
    M, D = x.shape
    y = torch.empty((M, D), dtype=BF16, device=x.device)
    mean = torch.empty((M,), dtype=F32, device=x.device)
    rstd = torch.empty((M,), dtype=F32, device=x.device)
    # algorithmic HBM bytes: 4 B read + 2 B written per element (the row statistics are 8 B per row)
    _launch(f"ln_fwd_d{D}", 0.0, 6.0 * M * D + 8.0 * M,
            lambda: call("octmae_layernorm_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(),
                         rstd.data_ptr(), M, D, float(eps), _stream()))
    return y, mean, rstd


def ln_apply(x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gamma, beta) -> torch.Tensor:
    """The ``y`` of ``layernorm_fwd(x, gamma, beta, eps)`` rebuilt from the row statistics that call returned: bit-equal, one pass
    without reductions (octmae_ln_apply).  What a Block that runs at recompute level "light" does instead of keeping y1 / y2."""
    M, D = _chk(x, F32, "ln_apply input").shape
    if _chk(mean, F32, "ln_apply mean").numel() != M or _chk(rstd, F32, "ln_apply rstd").numel() != M:
        raise ValueError(f"ln_apply: {mean.numel()} / {rstd.numel()} row statistics for {M} rows")
    if gamma.numel() != D or beta.numel() != D:
        raise ValueError(f"ln_apply: gamma / beta of {gamma.numel()} / {beta.numel()} elements for rows of {D}")
    y = torch.empty((M, D), dtype=BF16, device=x.device)
    _launch(f"ln_apply_d{D}", 0.0, 6.0 * M * D + 8.0 * M,
            lambda: call("octmae_ln_apply", x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                         y.data_ptr(), M, D, _stream()))
    return y


def gelu_apply(pre: torch.Tensor) -> torch.Tensor:
    """The ``act`` of ``pre, act = linear_fwd(..., "gelu")`` rebuilt from ``pre`` (the stored, 16-bit-rounded pre-activation): bit-equal
    to the GEMM epilogue's (octmae_gelu_apply).  The element count must be a multiple of 8."""
    _chk(pre, BF16, "gelu_apply input")
    act = torch.empty_like(pre)
    n = pre.numel()
    _launch("gelu_apply", 0.0, 4.0 * n, lambda: call("octmae_gelu_apply", pre.data_ptr(), act.data_ptr(), n, _stream()))
    return act


def layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, dres=None, want_bf16=False, dxsum=None):
    M, D = x.shape
    dx = torch.empty((M, D), dtype=F32, device=x.device)
    dxb = torch.empty((M, D), dtype=BF16, device=x.device) if want_bf16 else None
    ws = torch.empty((load().octmae_layernorm_bwd_ws_floats(M, D),), dtype=F32, device=x.device)
    # algorithmic HBM bytes: dy bf16 + x fp32 read, dx fp32 written, + the incoming residual-stream gradient (fp32) and the bf16
    # copy of dx when the fused forms are used
    nbytes = (2.0 + 4.0 + 4.0 + (4.0 if dres is not None else 0.0) + (2.0 if want_bf16 else 0.0)) * M * D + 8.0 * M
    _launch(f"ln_bwd_d{D}", 0.0, nbytes,
            lambda: call("octmae_layernorm_bwd", dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), _p(dres),
                         dx.data_ptr(), _p(dxb), _p(dgamma), _p(dbeta), _p(dxsum), ws.data_ptr(), M, D, _stream()))
    return dx, dxb



# ------------------------------------------------------------------------------------------------
# ConvNeXt layer (csrc/convnext.hip): depthwise 7x7 convolution and layer scale, channels-last fp32
# ------------------------------------------------------------------------------------------------
def _chk_nhwc(t: torch.Tensor, name: str):
    _chk(t, F32, name)
    if t.dim() != 4:
        raise RuntimeError(f"{name}: expected a channels-last [B, H, W, C] tensor, got {tuple(t.shape)}")
    if t.shape[3] % 8:
        raise RuntimeError(f"{name}: C = {t.shape[3]} is not a multiple of 8")
    return tuple(int(v) for v in t.shape)


def _chk_dw_weight(wt: torch.Tensor, C: int, name: str):
    _chk(wt, F32, name)
    if wt.numel() != C * 49 or wt.shape[0] != C or tuple(wt.shape[-2:]) != (7, 7):
        raise RuntimeError(f"{name}: expected [{C}, 7, 7] (or [{C}, 1, 7, 7]), got {tuple(wt.shape)}")


def _chk_vec(v: torch.Tensor, C: int, name: str):
    _chk(v, F32, name)
    if v.numel() != C:
        raise RuntimeError(f"{name}: expected {C} elements, got {tuple(v.shape)}")


def dwconv7_fwd(x: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """z[b,h,w,c] = bias[c] + sum_ij wt[c,i,j] x[b, h+i-3, w+j-3, c] (zero padding): nn.Conv2d(C, C, 7, padding=3, groups=C) on a
    channels-last fp32 map [B, H, W, C], C % 8 == 0, any H, W >= 1."""
    B, H, W, C = _chk_nhwc(x, "dwconv7_fwd x")
    _chk_dw_weight(wt, C, "dwconv7_fwd weight"); _chk_vec(bias, C, "dwconv7_fwd bias")
    z = torch.empty_like(x)
    n = float(x.numel())
    _launch(f"dwconv7_fwd_c{C}", 2.0 * 49 * n, 8.0 * n,
            lambda: call("octmae_dwconv7_fwd", x.data_ptr(), wt.data_ptr(), bias.data_ptr(), z.data_ptr(), B, H, W, C, _stream()))
    return z


def dwconv7_bwd_input(dz: torch.Tensor, wt: torch.Tensor, dres: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx = dres + sum_ij wt[c,i,j] dz[b, h-i+3, w-j+3, c]; ``dres`` (fp32, the shape of dz) is added last, exactly."""
    B, H, W, C = _chk_nhwc(dz, "dwconv7_bwd_input dz")
    _chk_dw_weight(wt, C, "dwconv7_bwd_input weight")
    if dres is not None and _chk(dres, F32, "dwconv7_bwd_input dres").shape != dz.shape:
        raise RuntimeError(f"dwconv7_bwd_input: dres {tuple(dres.shape)} for dz {tuple(dz.shape)}")
    dx = torch.empty_like(dz)
    n = float(dz.numel())
    _launch(f"dwconv7_bwd_input_c{C}", 2.0 * 49 * n, (8.0 if dres is None else 12.0) * n,
            lambda: call("octmae_dwconv7_bwd_input", dz.data_ptr(), wt.data_ptr(), _p(dres), dx.data_ptr(), B, H, W, C, _stream()))
    return dx


def dwconv7_bwd_weight(dz: torch.Tensor, x: torch.Tensor, gw: torch.Tensor, gb: torch.Tensor):
    """gw[c,i,j] += sum dz[b,h,w,c] x[b, h+i-3, w+j-3, c], gb[c] += sum dz: fp32 accumulation in a fixed order (two launches: partial sums
    per workgroup, then their fold), so two runs are bit-equal."""
    B, H, W, C = _chk_nhwc(dz, "dwconv7_bwd_weight dz")
    if _chk_nhwc(x, "dwconv7_bwd_weight x") != (B, H, W, C):
        raise RuntimeError(f"dwconv7_bwd_weight: x {tuple(x.shape)} for dz {tuple(dz.shape)}")
    _chk_dw_weight(gw, C, "dwconv7_bwd_weight gw"); _chk_vec(gb, C, "dwconv7_bwd_weight gb")
    nws = load().octmae_dwconv7_bwd_weight_ws_floats(B, H, W, C)
    if nws <= 0:
        raise RuntimeError(f"dwconv7_bwd_weight: unsupported shape {(B, H, W, C)}")
    ws = torch.empty((nws,), dtype=F32, device=dz.device)
    n = float(dz.numel())
    _launch(f"dwconv7_bwd_weight_c{C}", 2.0 * 49 * n, 8.0 * n + 8.0 * nws,
            lambda: call("octmae_dwconv7_bwd_weight", dz.data_ptr(), x.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), B, H, W, C,
                         _stream()))


def _chk_rows(t: torch.Tensor, dtype, name: str):
    _chk(t, dtype, name)
    if t.dim() != 2 or t.shape[1] % 8:
        raise RuntimeError(f"{name}: expected [M, C] rows with C % 8 == 0, got {tuple(t.shape)}")
    return int(t.shape[0]), int(t.shape[1])


def layer_scale_fwd(res: torch.Tensor, branch: torch.Tensor, gamma: torch.Tensor) -> torch.Tensor:
    """out = res + gamma[c] * branch on fp32 rows [M, C]: bit-equal to torch's fp32 mul followed by add."""
    M, C = _chk_rows(res, F32, "layer_scale_fwd res")
    if _chk_rows(branch, F32, "layer_scale_fwd branch") != (M, C):
        raise RuntimeError(f"layer_scale_fwd: branch {tuple(branch.shape)} for res {tuple(res.shape)}")
    _chk_vec(gamma, C, "layer_scale_fwd gamma")
    out = torch.empty_like(res)
    _launch(f"layer_scale_fwd_c{C}", 2.0 * M * C, 12.0 * M * C,
            lambda: call("octmae_layer_scale_fwd", res.data_ptr(), branch.data_ptr(), gamma.data_ptr(), out.data_ptr(), M, C, _stream()))
    return out


def layer_scale_bwd(dout: torch.Tensor, branch: Optional[torch.Tensor], gamma: torch.Tensor, ggamma: Optional[torch.Tensor] = None):
    """dbranch = gamma[c] * dout in the 16-bit operand type (one rounding); with ``ggamma`` (fp32 [C]) also
    ggamma[c] += sum_m dout[m,c] * branch[m,c], in a fixed order."""
    M, C = _chk_rows(dout, F32, "layer_scale_bwd dout")
    _chk_vec(gamma, C, "layer_scale_bwd gamma")
    ws = None
    if ggamma is not None:
        _chk_vec(ggamma, C, "layer_scale_bwd ggamma")
        if branch is None or _chk_rows(branch, F32, "layer_scale_bwd branch") != (M, C):
            raise RuntimeError("layer_scale_bwd: the gamma gradient needs branch, fp32 and of dout's shape")
        ws = torch.empty((load().octmae_layer_scale_bwd_ws_floats(M, C),), dtype=F32, device=dout.device)
    dbranch = torch.empty((M, C), dtype=BF16, device=dout.device)
    _launch(f"layer_scale_bwd_c{C}", 2.0 * M * C, (6.0 if ggamma is None else 10.0) * M * C,
            lambda: call("octmae_layer_scale_bwd", dout.data_ptr(), _p(branch) if ggamma is not None else None, gamma.data_ptr(),
                         dbranch.data_ptr(), _p(ggamma), _p(ws), M, C, _stream()))
    return dbranch


def slice_pool_fwd(x: torch.Tensor, gamma, beta, eps: float, S: int, cls: bool):
    """x fp32 [B*S, T, D] -> out fp32 [B, D] = mean over the S slices of LayerNorm(mean of tokens 1..T-1, or token 0); with the
    pooled rows and their LayerNorm statistics (saved for the backward)."""
    BS, T, D = x.shape
    if BS % S:
        raise RuntimeError(f"slice_pool: {BS} rows are not a whole number of volumes of {S} slices")
    B = BS // S
    out = torch.empty((B, D), dtype=F32, device=x.device)
    pooled = torch.empty((BS, D), dtype=F32, device=x.device)
    mean = torch.empty((BS,), dtype=F32, device=x.device)
    rstd = torch.empty((BS,), dtype=F32, device=x.device)
    ws = torch.empty((load().octmae_slice_pool_ws_floats(BS, T, D),), dtype=F32, device=x.device)
    # algorithmic HBM bytes: x read (mean mode: every patch token; cls mode: one row per slice)
    _launch(f"pool_fwd_d{D}", 0.0, 4.0 * BS * (1 if cls else T - 1) * D,
            lambda: call("octmae_slice_pool_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), pooled.data_ptr(),
                         mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), B, S, T, D, int(cls), float(eps), _stream()))
    return out, pooled, mean, rstd


def slice_pool_bwd(dout, pooled, mean, rstd, gamma, T: int, S: int, cls: bool, dgamma, dbeta, want_bf16=False, dxsum=None):
    B, D = dout.shape
    BS = B * S
    dx = torch.empty((BS, T, D), dtype=F32, device=dout.device)
    dxb = torch.empty((BS, T, D), dtype=BF16, device=dout.device) if want_bf16 else None
    ws = torch.empty((load().octmae_slice_pool_ws_floats(BS, T, D),), dtype=F32, device=dout.device)
    # algorithmic HBM bytes: the dense dx written (fp32, + the 16-bit copy)
    _launch(f"pool_bwd_d{D}", 0.0, (4.0 + (2.0 if want_bf16 else 0.0)) * BS * T * D,
            lambda: call("octmae_slice_pool_bwd", dout.data_ptr(), pooled.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                         dx.data_ptr(), _p(dxb), _p(dgamma), _p(dbeta), _p(dxsum), ws.data_ptr(), B, S, T, D, int(cls), _stream()))
    return dx, dxb


def _join_check(name, feats, present_mask):
    """The refusals of csrc/join.hip restated on the host, so that a bad call raises ValueError before any tensor is made or launched."""
    M = len(feats)
    if M not in (2, 3):
        raise ValueError(f"{name}: {M} modalities, the kernel is built for 2 or 3")
    if isinstance(present_mask, bool) or not isinstance(present_mask, (int, np.integer)) or not 0 < int(present_mask) < (1 << M):
        raise ValueError(f"{name}: present_mask must have at least one of its low {M} bits set and none above them, got {present_mask!r}")
    present_mask = int(present_mask)
    ref = None
    for k, f in enumerate(feats):
        if not (present_mask >> k) & 1:
            continue
        if f is None:
            raise ValueError(f"{name}: modality {k} is marked present and has no features")
        _chk(f, F32, f"{name}: features of modality {k}")
        if f.data_ptr() % 16:
            raise ValueError(f"{name}: features of modality {k} start at an address that is not 16-byte aligned (a view at an odd "
                             "storage offset): the kernel moves rows in 16-byte pieces -- pass a copy (.clone())")
        if f.dim() != 2 or (ref is not None and (f.shape != ref.shape or f.device != ref.device)):
            raise ValueError(f"{name}: expected [B, D] features of one shape on one device, got {tuple(f.shape)}")
        ref = f
    B, D = ref.shape
    if B < 1 or D % 4 != 0 or M * D > 4096:
        raise ValueError(f"{name}: B = {B}, D = {D}, M = {M}: the kernel needs B >= 1, D % 4 == 0 and M * D <= 4096")
    return M, B, D, present_mask, ref.device


def _join_aligned(name, **tensors):
    for nm, t in tensors.items():
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"{name}: {nm} starts at an address that is not 16-byte aligned: the kernel moves rows in 16-byte pieces")


def join_fwd(feats, present_mask: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    """feats: M = 2 or 3 raw tower outputs f32 [B, D] (None where absent) -> y (16-bit operand type) [B, M * D] = LayerNorm(concat of
    the L2-normalised features, zeros in absent slots), n_out f32 [M, B, D] (the normalised features), inv_norm f32 [B, M], mean, rstd [B]
    (csrc/join.hip)."""
    M, B, D, present_mask, dev = _join_check("join_fwd", feats, present_mask)
    if gamma.numel() != M * D or beta.numel() != M * D:
        raise ValueError(f"join_fwd: gamma / beta need {M * D} elements, got {gamma.numel()} and {beta.numel()}")
    _chk(gamma, F32, "join_fwd: gamma"); _chk(beta, F32, "join_fwd: beta")
    _join_aligned("join_fwd", gamma=gamma, beta=beta)
    y = torch.empty((B, M * D), dtype=BF16, device=dev)
    n_out = torch.empty((M, B, D), dtype=F32, device=dev)
    inv_norm = torch.empty((B, M), dtype=F32, device=dev)
    mean = torch.empty((B,), dtype=F32, device=dev)
    rstd = torch.empty((B,), dtype=F32, device=dev)
    f = [(_p(x) if (present_mask >> k) & 1 else None) for k, x in enumerate(feats)] + [None] * (3 - M)
    P = bin(present_mask).count("1")
    # algorithmic HBM bytes: the present features read, the normalised features (fp32) and the 16-bit row written
    _launch(f"join_fwd_d{M * D}", 0.0, (4.0 * P + 6.0 * M) * B * D + (8.0 + 4.0 * M) * B,
            lambda: call("octmae_join_fwd", f[0], f[1], f[2], present_mask, gamma.data_ptr(), beta.data_ptr(), n_out.data_ptr(),
                         inv_norm.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, D, M, float(eps), _stream()))
    return y, n_out, inv_norm, mean, rstd


def join_bwd(dy: torch.Tensor, dn_extra: Optional[torch.Tensor], feats, inv_norm, mean, rstd, gamma, present_mask: int,
             dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> df f32 [M, B, D]: the gradient at the raw tower outputs (slices of absent modalities are NOT written); ``dy`` f32 [B, M * D],
    ``dn_extra`` f32 [M, B, D] or None; ``dgamma`` / ``dbeta`` (f32 [M * D]) are accumulated into when given, deterministically."""
    M, B, D, present_mask, dev = _join_check("join_bwd", feats, present_mask)
    _chk(dy, F32, "join_bwd: dy")
    if tuple(dy.shape) != (B, M * D) or (dn_extra is not None and tuple(dn_extra.shape) != (M, B, D)):
        raise ValueError(f"join_bwd: dy must be [{B}, {M * D}] and dn_extra [{M}, {B}, {D}]")
    if dn_extra is not None:
        _chk(dn_extra, F32, "join_bwd: dn_extra")
    for t, nm in ((dgamma, "dgamma"), (dbeta, "dbeta")):
        if t is not None and (_chk(t, F32, f"join_bwd: {nm}").numel() != M * D):
            raise ValueError(f"join_bwd: {nm} needs {M * D} elements")
    _join_aligned("join_bwd", dy=dy, dn_extra=dn_extra, gamma=gamma)
    df = torch.empty((M, B, D), dtype=F32, device=dev)
    ws = None
    if dgamma is not None or dbeta is not None:
        ws = torch.empty((load().octmae_join_ws_floats(B, D, M),), dtype=F32, device=dev)
    f = [(_p(x) if (present_mask >> k) & 1 else None) for k, x in enumerate(feats)] + [None] * (3 - M)
    P = bin(present_mask).count("1")
    _launch(f"join_bwd_d{M * D}", 0.0, (4.0 * M + (8.0 + (4.0 if dn_extra is not None else 0.0)) * P) * B * D + (8.0 + 4.0 * M) * B,
            lambda: call("octmae_join_bwd", dy.data_ptr(), _p(dn_extra), f[0], f[1], f[2], inv_norm.data_ptr(), mean.data_ptr(),
                         rstd.data_ptr(), gamma.data_ptr(), present_mask, df.data_ptr(), _p(dgamma), _p(dbeta), _p(ws), B, D, M, _stream()))
    return df


# ------------------------------------------------------------------------------------------------
# slab LayerNorm (csrc/slabnorm.hip): the SLIViT head's first LayerNorm off the spatio-temporal token stream
# ------------------------------------------------------------------------------------------------
def _slab_check(name, x: torch.Tensor, T: int, L: int, n_prefix: int, **vectors):
    """The refusals of csrc/slabnorm.hip restated on the host, so that a bad call raises ValueError before anything is allocated."""
    _chk(x, F32, f"{name}: token stream")
    if x.dim() != 3:
        raise ValueError(f"{name}: expected the token stream [N, n_prefix + T * L, C], got {tuple(x.shape)}")
    N, tokens, C = x.shape
    if T < 1 or L < 1 or n_prefix < 0 or N < 1 or tokens != n_prefix + T * L:
        raise ValueError(f"{name}: {tokens} tokens are not n_prefix = {n_prefix} + T = {T} slices of L = {L}")
    if C % 8 != 0 or C < 8:
        raise ValueError(f"{name}: C = {C} is not a multiple of 8")
    K = C * L
    for nm, v in vectors.items():
        if v is None:
            continue
        if _chk(v, F32, f"{name}: {nm}").numel() != K:
            raise ValueError(f"{name}: {nm} needs C * L = {K} elements, got {v.numel()}")
    for nm, v in dict(x=x, **vectors).items():
        if v is not None and v.data_ptr() % 16:
            raise ValueError(f"{name}: {nm} starts at an address that is not 16-byte aligned: the kernel moves it in 16-byte pieces")
    return N, C, K


def _slab_ws(N: int, T: int, L: int, C: int, dev) -> torch.Tensor:
    n = load().octmae_slabnorm_ws_floats(N, T, L, C)
    if n < 0:
        raise ValueError(f"slab_norm: N = {N}, T = {T}, L = {L}, C = {C} is outside the kernel's domain (include/octmae.h)")
    return torch.empty((max(n, 4),), dtype=F32, device=dev)


def slab_norm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, T: int, L: int, n_prefix: int):
    """x f32 [N, n_prefix + T * L, C] -> A (16-bit operand type) [N * T, C * L], mean, rstd f32 [N * T]: row n * T + t of A is
    LayerNorm(C * L) of slice t's L tokens transposed to [C, L] and flattened (element c * L + l), gamma / beta f32 [C * L] in that
    order -- models_slivit_head.py:37-38 in front of vit-pytorch's to_patch_embedding[1], without a transposed copy of the stream."""
    N, C, K = _slab_check("slab_norm_fwd", x, T, L, n_prefix, gamma=gamma, beta=beta)
    rows = N * T
    A = torch.empty((rows, K), dtype=BF16, device=x.device)
    mean = torch.empty((rows,), dtype=F32, device=x.device)
    rstd = torch.empty((rows,), dtype=F32, device=x.device)
    ws = _slab_ws(N, T, L, C, x.device)
    # algorithmic HBM bytes: the slab read once (fp32), the row written (16 bits), gamma and beta once, the statistics
    _launch(f"slab_norm_fwd_k{K}", 0.0, 6.0 * rows * K + 8.0 * K + 8.0 * rows,
            lambda: call("octmae_slab_norm_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), A.data_ptr(), mean.data_ptr(),
                         rstd.data_ptr(), ws.data_ptr(), N, T, L, C, n_prefix, float(eps), _stream()))
    return A, mean, rstd


def slab_norm_bwd(dA: torch.Tensor, x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gamma: torch.Tensor, T: int, L: int,
                  n_prefix: int, dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> dx f32 of x's shape (the n_prefix leading token rows of every volume are zeros) for dA (16-bit) [N * T, C * L]; ``dgamma`` /
    ``dbeta`` (f32 [C * L]) are accumulated into when given, in a fixed order."""
    N, C, K = _slab_check("slab_norm_bwd", x, T, L, n_prefix, gamma=gamma, dgamma=dgamma, dbeta=dbeta)
    rows = N * T
    _chk(dA, BF16, "slab_norm_bwd: dA")
    if tuple(dA.shape) != (rows, K) or dA.data_ptr() % 16:
        raise ValueError(f"slab_norm_bwd: dA must be a 16-byte aligned [{rows}, {K}] matrix, got {tuple(dA.shape)}")
    if _chk(mean, F32, "slab_norm_bwd: mean").numel() != rows or _chk(rstd, F32, "slab_norm_bwd: rstd").numel() != rows:
        raise ValueError(f"slab_norm_bwd: {mean.numel()} / {rstd.numel()} row statistics for {rows} rows")
    dx = torch.empty_like(x)
    ws = _slab_ws(N, T, L, C, x.device)
    pgrads = (dgamma is not None) + (dbeta is not None)
    _launch(f"slab_norm_bwd_k{K}", 0.0, 10.0 * rows * K + 4.0 * K * (1 + 2 * pgrads) + 4.0 * N * n_prefix * C + 8.0 * rows,
            lambda: call("octmae_slab_norm_bwd", dA.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                         dx.data_ptr(), _p(dgamma), _p(dbeta), ws.data_ptr(), N, T, L, C, n_prefix, _stream()))
    return dx


_VOL_DTYPES = {torch.uint8: 0, torch.float32: 1}


def volume_box(vol: torch.Tensor) -> torch.Tensor:
    """The bounding box of the voxels > 0 of one [D, H, W] uint8 / float32 volume (MONAI CropForegroundd's default select_fn, margin
    0): int32 [6] = {d0, d1, h0, h1, w0, w1}, half-open, left on the GPU.  No voxel > 0: the full extent."""
    if vol.dim() != 3 or vol.dtype not in _VOL_DTYPES:
        raise RuntimeError(f"volume_box: expected a [D, H, W] uint8 or float32 volume, got {tuple(vol.shape)} {vol.dtype}")
    _chk(vol, vol.dtype, "volume_box")
    D, H, W = vol.shape
    box = torch.empty((6,), dtype=torch.int32, device=vol.device)
    _launch("volume_box", 0.0, float(vol.numel() * vol.element_size()),
            lambda: call("octmae_volume_box", vol.data_ptr(), _VOL_DTYPES[vol.dtype], D, H, W, box.data_ptr(), _stream()))
    return box


def volume_resample(vol: torch.Tensor, size, box: Optional[torch.Tensor] = None, flip_d: bool = False, flip_w: bool = False,
                    normalize=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.interpolate(mode="trilinear", align_corners=False) of one [D, H, W] uint8 / float32 volume (of the sub-volume ``box`` names:
    volume_box's six device ints) to ``size`` = (T, OH, OW), the result's first / last axis reversed by ``flip_d`` / ``flip_w``, then
    ``normalize`` = (subtrahend, divisor) applied where the value is not 0.  ``out``: a contiguous float32 [T, OH, OW] tensor, which
    may be a slice of a batch tensor."""
    if vol.dim() != 3 or vol.dtype not in _VOL_DTYPES:
        raise RuntimeError(f"volume_resample: expected a [D, H, W] uint8 or float32 volume, got {tuple(vol.shape)} {vol.dtype}")
    _chk(vol, vol.dtype, "volume_resample")
    T, OH, OW = (int(s) for s in size)
    if out is None:
        out = torch.empty((T, OH, OW), dtype=F32, device=vol.device)
    else:
        _chk(out, F32, "volume_resample out")
        if tuple(out.shape) != (T, OH, OW) or out.device != vol.device:
            raise RuntimeError(f"volume_resample: out is {tuple(out.shape)} on {out.device}, expected {(T, OH, OW)} on {vol.device}")
    if box is not None:
        _chk(box, torch.int32, "volume_resample box")
        if box.numel() != 6 or box.device != vol.device:
            raise RuntimeError("volume_resample: box must be six int32 on the volume's device")
    sub, div = (0.0, 1.0) if normalize is None else (float(normalize[0]), float(normalize[1]))
    D, H, W = vol.shape
    # algorithmic HBM bytes: the (boxed) volume read once, the output written once
    _launch("volume_resample", 0.0, float(vol.numel() * vol.element_size() + 4 * out.numel()),
            lambda: call("octmae_volume_resample", vol.data_ptr(), _VOL_DTYPES[vol.dtype], D, H, W, _p(box), out.data_ptr(), T, OH, OW,
                         int(bool(flip_d)), int(bool(flip_w)), int(normalize is not None), sub, div, _stream()))
    return out


def image_resample(img: torch.Tensor, size, crop=None, flip: bool = False, lut: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pillow's 8-bit bicubic resize (``Image.resize(..., Image.BICUBIC)``, what torchvision's Resize / resized_crop with
    interpolation=3 call for a PIL image), bit for bit, of uint8 images [H, W], [H, W, 3], [n, H, W] or [n, H, W, 3] (a 3-D input whose
    last axis is 3 is ONE RGB image) to ``size`` = (OH, OW), in one launch: ``crop`` = (top, left, height, width) is taken first (the
    windows clamp at its edges), ``flip`` reverses the result's width axis.  With ``lut`` (float32 [3, 256]: ToTensor -> Normalize of
    every grey level per channel) the result is float32 [n, 3, OH, OW], a grey input replicated (convert("RGB")); without, uint8 in the
    layout of the input.  ``out``: a contiguous tensor of the result's shape, which may be a slice of a batch.  No autograd; integer
    arithmetic, so autocast changes nothing."""
    if img.dtype != torch.uint8 or img.dim() not in (2, 3, 4) or (img.dim() == 4 and img.shape[-1] != 3):
        raise RuntimeError(f"image_resample: expected uint8 [H, W], [H, W, 3], [n, H, W] or [n, H, W, 3], got {tuple(img.shape)} {img.dtype}")
    img = _chk(img.detach(), torch.uint8, "image_resample")
    C = 3 if img.dim() == 4 or (img.dim() == 3 and img.shape[-1] == 3) else 1
    batched = img.dim() - (C == 3) == 3
    n = img.shape[0] if batched else 1
    H, W = img.shape[1:3] if batched else img.shape[:2]
    OH, OW = (int(s) for s in size)
    top, left, ch, cw = (0, 0, 0, 0) if crop is None else (int(v) for v in crop)
    if crop is not None and (ch < 1 or cw < 1):
        raise RuntimeError(f"image_resample: empty crop {tuple(crop)}")
    if lut is not None:
        _chk(lut, F32, "image_resample lut")
        if tuple(lut.shape) != (3, 256) or lut.device != img.device:
            raise RuntimeError("image_resample: lut must be float32 [3, 256] on the image's device")
        shape, dtype = (n, 3, OH, OW), F32
    else:
        shape, dtype = ((n,) if batched else ()) + (OH, OW) + ((3,) if C == 3 else ()), torch.uint8
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=img.device)
    else:
        _chk(out, dtype, "image_resample out")
        if tuple(out.shape) != shape or out.device != img.device:
            raise RuntimeError(f"image_resample: out is {tuple(out.shape)} on {out.device}, expected {shape} on {img.device}")
    # algorithmic HBM bytes: the (cropped) images read once, the output written once
    nbytes = float(n * (ch or H) * (cw or W) * C + out.numel() * out.element_size())
    _launch("image_resample", 0.0, nbytes,
            lambda: call("octmae_image_resample", img.data_ptr(), n, H, W, C, top, left, ch, cw, OH, OW, int(bool(flip)), _p(lut),
                         out.data_ptr(), _stream()))
    return out


# one octmae_aug_desc (include/octmae.h) per image: 72 bytes
AUG_DESC = np.dtype([("kind", "<i4"), ("mode", "<i4"), ("m", "<f8", (6,)), ("factor", "<f4"), ("iarg", "<i4"), ("fill", "u1", (4,)),
                     ("reserved", "<i4")])
AUG_NONE, AUG_TABLE, AUG_COLOR, AUG_SHARPNESS, AUG_AFFINE = range(5)
(AUG_LUT_INVERT, AUG_LUT_POSTERIZE, AUG_LUT_SOLARIZE, AUG_LUT_SOLARIZE_ADD, AUG_LUT_BRIGHTNESS, AUG_LUT_CONTRAST, AUG_LUT_AUTOCONTRAST,
 AUG_LUT_EQUALIZE) = range(8)


def aug_needs_stats(desc: np.ndarray) -> np.ndarray:
    """bool [n]: the descriptors whose op reads the image's histograms (Contrast, AutoContrast, Equalize)."""
    return (desc["kind"] == AUG_TABLE) & (desc["mode"] >= AUG_LUT_CONTRAST)


def _upload(a: np.ndarray, device) -> torch.Tensor:
    # through pinned memory, so that the copy is asynchronous: the chain never waits for the device
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).pin_memory().to(device, non_blocking=True)


def _chk_images(img: torch.Tensor, name: str):
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[-1] != 3:
        raise RuntimeError(f"{name}: expected uint8 [n, H, W, 3], got {tuple(img.shape)} {img.dtype}")
    return _chk(img.detach(), torch.uint8, name)


def image_stats(img: torch.Tensor, needed=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 256-bin histograms of R, G, B and L = convert("L") of uint8 images [n, H, W, 3], in one launch: int32 [n, 4, 256], left on
    the GPU.  ``needed``: n booleans on the host; the images whose flag is unset are skipped and their rows are zero."""
    img = _chk_images(img, "image_stats")
    n, H, W, _ = img.shape
    if out is None:
        out = torch.empty((n, 4, 256), dtype=torch.int32, device=img.device)
    else:
        _chk(out, torch.int32, "image_stats out")
        if tuple(out.shape) != (n, 4, 256) or out.device != img.device:
            raise RuntimeError(f"image_stats: out is {tuple(out.shape)} on {out.device}, expected {(n, 4, 256)} on {img.device}")
    flags = None
    if needed is not None:
        needed = np.asarray(needed, dtype=np.uint8).reshape(-1)
        if needed.shape[0] != n:
            raise RuntimeError(f"image_stats: {needed.shape[0]} flags for {n} images")
        flags = _upload(needed, img.device)
    _launch("image_stats", 0.0, float(img.numel()),
            lambda: call("octmae_image_stats", img.data_ptr(), n, H, W, _p(flags), out.data_ptr(), _stream()))
    return out


def image_augment(img: torch.Tensor, desc: np.ndarray, hist: Optional[torch.Tensor] = None, lut: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One Pillow operation per image, bit for bit, on uint8 images [n, H, W, 3] in one launch.  ``desc``: n ``AUG_DESC`` records on
    the host (octcubem_amd.rand_augment.describe_op writes them); ``hist``: image_stats' output, needed when an op reads the image's
    statistics.  The result is uint8 [n, H, W, 3], or with ``lut`` (float32 [3, 256], ToTensor -> Normalize as in image_resample)
    float32 [n, 3, H, W].  ``out`` must not alias ``img``.  No autograd."""
    img = _chk_images(img, "image_augment")
    n, H, W, _ = img.shape
    if not isinstance(desc, np.ndarray) or desc.dtype != AUG_DESC or desc.shape != (n,):
        raise RuntimeError(f"image_augment: expected {n} AUG_DESC records on the host")
    desc = np.ascontiguousarray(desc)
    if hist is not None:
        _chk(hist, torch.int32, "image_augment hist")
        if tuple(hist.shape) != (n, 4, 256) or hist.device != img.device:
            raise RuntimeError("image_augment: hist must be int32 [n, 4, 256] on the images' device")
    elif bool(aug_needs_stats(desc).any()):
        raise RuntimeError("image_augment: an op reads the image statistics and hist is missing")
    if lut is not None:
        _chk(lut, F32, "image_augment lut")
        if tuple(lut.shape) != (3, 256) or lut.device != img.device:
            raise RuntimeError("image_augment: lut must be float32 [3, 256] on the images' device")
        shape, dtype = (n, 3, H, W), F32
    else:
        shape, dtype = (n, H, W, 3), torch.uint8
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=img.device)
    else:
        _chk(out, dtype, "image_augment out")
        if tuple(out.shape) != shape or out.device != img.device:
            raise RuntimeError(f"image_augment: out is {tuple(out.shape)} on {out.device}, expected {shape} on {img.device}")
        if out.data_ptr() == img.data_ptr():
            raise RuntimeError("image_augment: out aliases img")
    dev = _upload(desc, img.device)
    # algorithmic HBM bytes: the images read once, the output written once
    _launch("image_augment", 0.0, float(img.numel() + out.numel() * out.element_size()),
            lambda: call("octmae_image_augment", img.data_ptr(), n, H, W, dev.data_ptr(), desc.ctypes.data, _p(hist), _p(lut),
                         out.data_ptr(), _stream()))
    return out


def mae_compose(pred: torch.Tensor, imgs: torch.Tensor, mask: torch.Tensor, frame_idx: Optional[torch.Tensor], u: int, p: int,
                denorm: bool = False) -> torch.Tensor:
    """The four reconstruction volumes of the validation pass (custom_util/misc.py:1225-1299 get_visible_images) in one kernel:
    uint8 [B, 4, Tp, H, W] = original frames, masked input, reconstruction, reconstruction pasted with the visible patches, grey levels
    of untransform_image (:727-728), bit-equal to the reference's chain.  ``pred`` f32 [B, L, u*p*p]: contiguous, or any view whose
    samples are contiguous [L, PD] blocks a multiple of 4 floats apart (``pred_full[:, 1:, :]`` of the decoder's output: no copy);
    ``imgs`` f32 [B, 1, T, H, W]; ``mask`` f32 [B, L], 1 = removed; ``frame_idx`` None or Tp int32 source frames.  ``denorm``: map
    pred back from per-patch standardised units first (a norm_pix_loss model).  No autograd."""
    if pred.dim() != 3 or imgs.dim() != 5 or imgs.shape[1] != 1:
        raise RuntimeError(f"mae_compose: expected pred [B, L, PD] and imgs [B, 1, T, H, W], got {tuple(pred.shape)} and {tuple(imgs.shape)}")
    pred, mask = pred.detach(), mask.detach()
    imgs = _chk(imgs.detach(), F32, "mae_compose imgs")
    if not pred.is_cuda or pred.dtype != F32:
        raise RuntimeError(f"mae_compose pred: expected a float32 GPU tensor, got {pred.dtype} on {pred.device}")
    Bn, L, PD = pred.shape
    _, _, T, Hh, Ww = imgs.shape
    if pred.stride(2) != 1 or pred.stride(1) != PD or (Bn > 1 and (pred.stride(0) < L * PD or pred.stride(0) % 4)):
        pred = pred.contiguous()
    bs = pred.stride(0) if Bn > 1 else L * PD
    mask = _chk(mask.reshape(Bn, L), F32, "mae_compose mask")
    if imgs.shape[0] != Bn or PD != u * p * p or Hh % p or Ww % p or L % ((Hh // p) * (Ww // p)):
        raise RuntimeError(f"mae_compose: pred {tuple(pred.shape)} does not tile imgs {tuple(imgs.shape)} with u={u}, p={p}")
    Tp = L // ((Hh // p) * (Ww // p)) * u
    if frame_idx is not None:
        _chk(frame_idx, torch.int32, "mae_compose frame_idx")
        if frame_idx.numel() != Tp:
            raise RuntimeError(f"mae_compose: frame_idx has {frame_idx.numel()} entries, the prediction has {Tp} frames")
    out = torch.empty((Bn, 4, Tp, Hh, Ww), dtype=torch.uint8, device=imgs.device)
    # algorithmic HBM bytes: pred, the gathered frames (twice more with denorm) and the mask read, four uint8 panels written
    nvox = Bn * Tp * Hh * Ww
    _launch("mae_compose", 0.0, float(4 * Bn * L * PD + 4 * nvox * (2 if denorm else 1) + 4 * Bn * L + 4 * nvox),
            lambda: call("octmae_mae_compose", pred.data_ptr(), bs, imgs.data_ptr(), _p(frame_idx), mask.data_ptr(), out.data_ptr(),
                         Bn, T, Hh, Ww, u, p, L, int(bool(denorm)), _stream()))
    return out


def mae_compose_nc(pred: torch.Tensor, imgs: torch.Tensor, mask: torch.Tensor, u: int, p: int, scale=(1.0, 1.0, 1.0),
                   shift=(0.0, 0.0, 0.0), denorm: bool = False) -> torch.Tensor:
    """The four panels of ``mae_compose`` for ``C`` channels and any affine grey scale (get_visible_images_2d, custom_util/misc.py:
    1134-1223): uint8 [B, 4, Tp, H, W, C], channels innermost.  ``pred`` f32 [B, L, u*p*p*C] in the order (a < u, py, px, c < C) --
    models_mae_2d.patchify's for u = 1, models_mae.patchify's for C = 1 -- contiguous or the ``pred_full[:, 1:, :]`` view;
    ``imgs`` f32 [B, C, T, H, W]; ``mask`` f32 [B, L], 1 = removed.  The level of channel c is
    ``(int) clip(((v * scale[c]) + shift[c]) * 255, 0, 255)``, every operation rounded to fp32 on its own: the defaults are the
    reference's untransform_image_no_normalization bit for bit, ``scale = std`` / ``shift = mean`` the inverse of a Normalize
    transform.  A scalar ``scale`` / ``shift`` stands for every channel.  Predicted frame f is frame f of ``imgs``.  Everything the
    entry point refuses is refused here first, before a launch.  No autograd."""
    if pred.dim() != 3 or imgs.dim() != 5:
        raise RuntimeError(f"mae_compose_nc: expected pred [B, L, PD] and imgs [B, C, T, H, W], got {tuple(pred.shape)} and {tuple(imgs.shape)}")
    Bn, L, PD = pred.shape
    _, Cc, T, Hh, Ww = imgs.shape
    u, p = int(u), int(p)
    if Cc not in (1, 3):
        raise RuntimeError(f"mae_compose_nc: 1 or 3 channels, got {Cc}")
    if u > 1 and Cc > 1:
        raise RuntimeError(f"mae_compose_nc: a temporal patch of {u} frames with {Cc} channels has no caller and no stated element order")
    if u < 1 or p < 4 or p % 4 or Ww % 4:
        raise RuntimeError(f"mae_compose_nc: p and W must be multiples of 4 and u positive, got u={u}, p={p}, W={Ww}")

    def three(v, what):
        v = [float(v)] * 3 if isinstance(v, (int, float)) else [float(x) for x in v]
        if len(v) == 1:
            v = v * 3
        if len(v) < Cc or len(v) > 3 or not all(math.isfinite(x) for x in v):
            raise RuntimeError(f"mae_compose_nc: {what} must hold {Cc} finite values, got {v}")
        return v + [v[-1]] * (3 - len(v))
    sc, sh = three(scale, "scale"), three(shift, "shift")
    if imgs.shape[0] != Bn or Bn < 1 or L < 1 or PD != u * p * p * Cc or Hh % p or Ww % p or L % ((Hh // p) * (Ww // p)):
        raise RuntimeError(f"mae_compose_nc: pred {tuple(pred.shape)} does not tile imgs {tuple(imgs.shape)} with u={u}, p={p}")
    Tp = L // ((Hh // p) * (Ww // p)) * u
    if Tp > T:
        raise RuntimeError(f"mae_compose_nc: the prediction has {Tp} frames, the volume {T}")
    pred, mask = pred.detach(), mask.detach()
    imgs = _chk(imgs.detach(), F32, "mae_compose_nc imgs")
    if not pred.is_cuda or pred.dtype != F32:
        raise RuntimeError(f"mae_compose_nc pred: expected a float32 GPU tensor, got {pred.dtype} on {pred.device}")
    if pred.stride(2) != 1 or pred.stride(1) != PD or (Bn > 1 and (pred.stride(0) < L * PD or pred.stride(0) % 4)):
        pred = pred.contiguous()
    bs = pred.stride(0) if Bn > 1 else L * PD
    mask = _chk(mask.reshape(Bn, L), F32, "mae_compose_nc mask")
    out = torch.empty((Bn, 4, Tp, Hh, Ww, Cc), dtype=torch.uint8, device=imgs.device)
    nel = Bn * Tp * Hh * Ww * Cc
    _launch("mae_compose_nc", 0.0, float(4 * Bn * L * PD + 4 * nel * (2 if denorm else 1) + 4 * Bn * L + 4 * nel),
            lambda: call("octmae_mae_compose_nc", pred.data_ptr(), bs, imgs.data_ptr(), mask.data_ptr(), out.data_ptr(), Bn, Cc, T, Hh,
                         Ww, u, p, L, *sc, *sh, int(bool(denorm)), _stream()))
    return out


def _cover_pred(pred: torch.Tensor, what: str):
    """pred f32 [B, L, PD] as the entry points read it: (tensor, batch stride in floats); a view they cannot read in place is copied."""
    if pred.dim() != 3:
        raise RuntimeError(f"{what} pred: expected [B, L, PD], got {tuple(pred.shape)}")
    if not pred.is_cuda or pred.dtype != F32:
        raise RuntimeError(f"{what} pred: expected a float32 GPU tensor, got {pred.dtype} on {pred.device}")
    Bn, L, PD = pred.shape
    if Bn < 1 or L < 1 or PD < 4 or PD % 4:
        raise RuntimeError(f"{what} pred: B and L must be positive and PD a positive multiple of 4, got {tuple(pred.shape)}")
    if Bn * L > 0x7fffffff:
        raise RuntimeError(f"{what} pred: {Bn} x {L} tokens are more than 2^31 - 1")
    if pred.stride(2) != 1 or pred.stride(1) != PD or (Bn > 1 and (pred.stride(0) < L * PD or pred.stride(0) % 4)) or \
            pred.data_ptr() % 16:
        pred = pred.contiguous()
    return pred, (pred.stride(0) if Bn > 1 else L * PD)


def cover_accumulate(pred: torch.Tensor, mask: torch.Tensor, sum: Optional[torch.Tensor] = None, cnt: Optional[torch.Tensor] = None,
                     first: Optional[bool] = None):
    """One pass of the full-coverage reconstruction (csrc/cover.hip): the predictions of the tokens ``mask`` removed are added into the
    per-token sums.  ``pred`` f32 [B, L, PD], contiguous or the ``pred_full[:, 1:, :]`` view ``forward`` returns (read in place);
    ``mask`` f32 [B, L], != 0 = removed.  Without ``sum`` / ``cnt`` this is the first pass: both are allocated here and every row is
    written (a removed token's row is its prediction and its count 1, every other row +0.0 and 0).  With them (f32 [B, L, PD] and int32
    [B, L], updated in place) a removed token gets ``sum += pred`` and ``cnt += 1`` and no other row is touched: pass by pass the
    bits of ``torch.where(mask, sum + pred, sum)``.  ``first=True`` with buffers overwrites them as the first pass does.  Returns
    ``(sum, cnt)``.  Everything the entry point refuses is refused here first, before a launch.  No autograd."""
    pred, bs = _cover_pred(pred.detach(), "cover_accumulate")
    Bn, L, PD = pred.shape
    mask = mask.detach()
    if mask.numel() != Bn * L:
        raise RuntimeError(f"cover_accumulate mask: expected {Bn} x {L} values, got {tuple(mask.shape)}")
    mask = _chk(mask.reshape(Bn, L), F32, "cover_accumulate mask")
    if (sum is None) != (cnt is None):
        raise RuntimeError("cover_accumulate: sum and cnt are given together or not at all")
    if first is None:
        first = sum is None
    if sum is None:
        if not first:
            raise RuntimeError("cover_accumulate: first=False needs the sum and cnt of the earlier passes")
        sum = torch.empty((Bn, L, PD), dtype=F32, device=pred.device)
        cnt = torch.empty((Bn, L), dtype=torch.int32, device=pred.device)
    else:
        _chk(sum, F32, "cover_accumulate sum"); _chk(cnt, torch.int32, "cover_accumulate cnt")
        if tuple(sum.shape) != (Bn, L, PD) or tuple(cnt.shape) != (Bn, L) or sum.device != pred.device or cnt.device != pred.device:
            raise RuntimeError(f"cover_accumulate: sum {tuple(sum.shape)} / cnt {tuple(cnt.shape)} do not match pred {tuple(pred.shape)}")
        if sum.data_ptr() % 16 or sum.data_ptr() == pred.data_ptr():
            raise RuntimeError("cover_accumulate sum: expected a 16-byte aligned buffer of its own")
    # algorithmic HBM bytes: the mask; the first pass writes every row and reads the removed ones; a later pass reads both and writes one
    # on the removed rows only (their number is data: counted as all rows, an upper bound)
    _launch("cover_accumulate", 0.0, float(4 * Bn * L + 4 * Bn * L * PD * (2 if first else 3)),
            lambda: call("octmae_cover_accumulate", pred.data_ptr(), bs, mask.data_ptr(), sum.data_ptr(), cnt.data_ptr(), Bn, L, PD,
                         int(bool(first)), _stream()))
    return sum, cnt


def cover_finish(sum: torch.Tensor, cnt: torch.Tensor, imgs: torch.Tensor, frame_idx: Optional[torch.Tensor], u: int, p: int,
                 denorm: bool = False, error_volume: bool = True, token_score: bool = True):
    """The finishing pass of the full-coverage reconstruction (csrc/cover.hip): ``(recon, err, score)`` from the sums of
    ``cover_accumulate``.  For a token with ``cnt > 0`` the value is ``v = sum / cnt`` (``denorm``: mapped back through the mean and
    unbiased variance of the token's target patch first, as ``mae_compose`` does); ``recon`` uint8 [B, Tp, H, W] holds the grey levels
    of ``v`` un-shuffled to (frame, y, x) -- panel 2 of ``mae_compose`` for ``pred = v``; ``err`` f32 [B, Tp, H, W] (None with
    ``error_volume=False``) holds ``(v - x) ** 2`` against the source frame's voxel; ``score`` f32 [B, L] (None with
    ``token_score=False``) the mean of a token's squared errors.  A token that was never removed draws the input: its grey levels,
    error 0, score 0.  ``imgs`` f32 [B, 1, T, H, W]; ``frame_idx`` None or Tp int32 source frames.  Deterministic; no autograd."""
    u, p = int(u), int(p)
    if sum.dim() != 3 or imgs.dim() != 5 or imgs.shape[1] != 1:
        raise RuntimeError(f"cover_finish: expected sum [B, L, PD] and imgs [B, 1, T, H, W], got {tuple(sum.shape)} and {tuple(imgs.shape)}")
    sum, cnt = _chk(sum.detach(), F32, "cover_finish sum"), _chk(cnt.detach(), torch.int32, "cover_finish cnt")
    imgs = _chk(imgs.detach(), F32, "cover_finish imgs")
    Bn, L, PD = sum.shape
    _, _, T, Hh, Ww = imgs.shape
    if u < 1 or p < 4 or p % 4 or Ww % 4:
        raise RuntimeError(f"cover_finish: p and W must be multiples of 4 and u positive, got u={u}, p={p}, W={Ww}")
    if imgs.shape[0] != Bn or Bn < 1 or L < 1 or PD != u * p * p or Hh % p or Ww % p or L % ((Hh // p) * (Ww // p)):
        raise RuntimeError(f"cover_finish: sum {tuple(sum.shape)} does not tile imgs {tuple(imgs.shape)} with u={u}, p={p}")
    if tuple(cnt.shape) != (Bn, L) or cnt.device != sum.device or imgs.device != sum.device:
        raise RuntimeError(f"cover_finish cnt: expected int32 {(Bn, L)} on {sum.device}, got {tuple(cnt.shape)} on {cnt.device}")
    if Bn * L > 0x7fffffff:
        raise RuntimeError(f"cover_finish sum: {Bn} x {L} tokens are more than 2^31 - 1")
    if sum.data_ptr() % 16 or imgs.data_ptr() % 16:
        raise RuntimeError("cover_finish: sum and imgs must be 16-byte aligned")
    Tp = L // ((Hh // p) * (Ww // p)) * u
    if frame_idx is not None:
        _chk(frame_idx, torch.int32, "cover_finish frame_idx")
        if frame_idx.numel() != Tp:
            raise RuntimeError(f"cover_finish: frame_idx has {frame_idx.numel()} entries, the prediction has {Tp} frames")
    elif Tp > T:
        raise RuntimeError(f"cover_finish: the prediction has {Tp} frames, the volume {T}, and no frame_idx says which")
    recon = torch.empty((Bn, Tp, Hh, Ww), dtype=torch.uint8, device=sum.device)
    err = torch.empty((Bn, Tp, Hh, Ww), dtype=F32, device=sum.device) if error_volume else None
    score = torch.empty((Bn, L), dtype=F32, device=sum.device) if token_score else None
    nvox = Bn * Tp * Hh * Ww
    # algorithmic HBM bytes: the sums, the counts and the gathered frames read (twice more with denorm), recon, err and score written
    _launch("cover_finish", 0.0, float(4 * Bn * L * PD + 4 * Bn * L + 4 * nvox * (3 if denorm else 1) + nvox
                                       + (4 * nvox if error_volume else 0) + (4 * Bn * L if token_score else 0)),
            lambda: call("octmae_cover_finish", sum.data_ptr(), cnt.data_ptr(), imgs.data_ptr(), _p(frame_idx), recon.data_ptr(), _p(err),
                         _p(score), Bn, T, Hh, Ww, u, p, L, int(bool(denorm)), _stream()))
    return recon, err, score


# ------------------------------------------------------------------------------------------------
# low-rank adapters (csrc/lora.hip)
# ------------------------------------------------------------------------------------------------
LORA_MAX_RANK = 64


def lora_rp(r: int) -> int:
    """the rank rounded up to the 16 columns of an MFMA tile: the width of the padded operand copies"""
    return (int(r) + 15) // 16 * 16


def _lora_gpu(name: str, t, dtype, what: str, dims: int = 2):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{name}: {what} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: {what} must be {dtype}, got {t.dtype}")
    if t.dim() != dims:
        raise ValueError(f"{name}: {what} must have {dims} dimensions, got {tuple(t.shape)}")
    return t


def _lora_rows(name: str, t: torch.Tensor, what: str, align: int):
    """unit column stride, a row stride >= the width (a view into a wider buffer), the first element ``align`` bytes aligned"""
    rows, cols = t.shape
    if (cols > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < cols):
        raise ValueError(f"{name}: {what} needs unit column stride and a row stride >= {cols}, got strides {tuple(t.stride())}")
    if t.data_ptr() % align:
        raise ValueError(f"{name}: {what} must be {align}-byte aligned")
    return t.stride(0) if rows > 1 else cols


def _lora_dims(name: str, O: int, I: int, r: int):
    if not 1 <= r <= LORA_MAX_RANK:
        raise ValueError(f"{name}: rank {r} outside 1 .. {LORA_MAX_RANK}")
    if I < 8 or O < 8 or I % 8 or O % 8:
        raise ValueError(f"{name}: in / out features must be positive multiples of 8 (the widths of 16-bit GEMM operands), got {I} / {O}")


def lora_merge(W: torch.Tensor, A: torch.Tensor, B: torch.Tensor, s: float, out: torch.Tensor, A_lp: Optional[torch.Tensor] = None,
               B_lp: Optional[torch.Tensor] = None):
    """``out [O, I] = W + s B A`` for the fp32 master weight ``W [O, I]`` and the adapter ``A [r, I]``, ``B [O, r]`` (csrc/lora.hip):
    ``delta`` by fused multiply-adds in ascending k, then ``v = fma(s, delta, W)``; ``out`` is float32 (``v``) or the 16-bit operand type
    (``v`` rounded once).  ``A_lp [rp, I]`` / ``B_lp [O, rp]`` (optional) receive the adapter rounded to the operand type with zeros in
    the padding, ``rp = lora_rp(r)``: the operands of ``lora_wgrad``.  All contiguous.  No autograd."""
    name = "lora_merge"
    W, A, B = (_lora_gpu(name, t.detach(), F32, nm) for t, nm in ((W, "W"), (A, "A"), (B, "B")))
    O, I = W.shape
    r = A.shape[0]
    _lora_dims(name, O, I, r)
    if tuple(A.shape) != (r, I) or tuple(B.shape) != (O, r):
        raise ValueError(f"{name}: expected A [{r}, {I}] and B [{O}, {r}] for W {tuple(W.shape)}, got {tuple(A.shape)} and {tuple(B.shape)}")
    rp = lora_rp(r)
    if not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype not in (F32, BF16) or tuple(out.shape) != (O, I):
        raise ValueError(f"{name}: out must be a float32 or {BF16} GPU tensor of shape {(O, I)}")
    tensors = [(W, "W"), (A, "A"), (B, "B"), (out, "out")]
    for t, nm, shape in ((A_lp, "A_lp", (rp, I)), (B_lp, "B_lp", (O, rp))):
        if t is not None:
            _lora_gpu(name, t, BF16, nm)
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: {nm} must be {shape}, got {tuple(t.shape)}")
            tensors.append((t, nm))
    for t, nm in tensors:
        if not t.is_contiguous() or t.device != W.device:
            raise ValueError(f"{name}: {nm} must be contiguous and on {W.device}")
        if t.data_ptr() % (4 if nm == "B" else 16):
            raise ValueError(f"{name}: {nm} must be 16-byte aligned")
    esz = 4 if out.dtype == F32 else 2
    _launch("lora_merge", 2.0 * O * I * (r + 1), float(4 * O * I + esz * O * I + 4 * r * (I + O) + 2 * rp * (I + O)),
            lambda: call("octmae_lora_merge", W.data_ptr(), A.data_ptr(), B.data_ptr(), float(s), O, I, r, out.data_ptr(),
                         int(out.dtype == F32), _p(A_lp), _p(B_lp), _stream()))
    return out


def lora_plan(M: int, I: int, O: int, rp: int):
    """(rows per chunk, chunks, 64-column tiles of X, of dY) of ``lora_wgrad``: host-side arithmetic, no GPU is touched"""
    import ctypes
    out = (ctypes.c_int * 4)()
    call("octmae_lora_plan", int(M), int(I), int(O), int(rp), out)
    return tuple(out)


def lora_ws_bytes(M: int, I: int, O: int, rp: int) -> int:
    import ctypes
    n = ctypes.c_longlong()
    call("octmae_lora_ws_bytes", int(M), int(I), int(O), int(rp), ctypes.byref(n))
    return n.value


_lora_ws = {}


def _lora_ws_for(nbytes: int, dev) -> torch.Tensor:
    """one workspace per device and stream, grown on demand: launches on one stream run in order, so consecutive calls may share it"""
    key = (dev.index, _stream())
    ws = _lora_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _lora_ws[key] = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    return ws


def lora_wgrad(x: torch.Tensor, dy: torch.Tensor, A_lp: torch.Tensor, B_lp: torch.Tensor, s: float, r: int,
               gA: Optional[torch.Tensor], gB: Optional[torch.Tensor], ws: Optional[torch.Tensor] = None):
    """The adapter gradients of one Linear without its weight gradient (csrc/lora.hip, the two-pass form): with ``x [M, I]`` and
    ``dy [M, O]`` (16 bit, row views of wider buffers allowed) and the padded operand copies of ``lora_merge``,
    ``gA [r.., I] += s (dy B)^T x`` and ``gB [O, r..] += s dy^T (x A^T)`` in fp32; only the first r rows of ``gA`` and the first r columns
    of ``gB`` are touched (views with their own row strides).  Either gradient may be None.  No atomics: a fixed order of additions."""
    name = "lora_wgrad"
    x, dy = _lora_gpu(name, x, BF16, "x"), _lora_gpu(name, dy, BF16, "dy")
    _lora_gpu(name, A_lp, BF16, "A_lp"); _lora_gpu(name, B_lp, BF16, "B_lp")
    M, I = x.shape
    O = dy.shape[1]
    r = int(r)
    _lora_dims(name, O, I, r)
    rp = lora_rp(r)
    if dy.shape[0] != M or M < 1 or M > 2 ** 31 - 1:
        raise ValueError(f"{name}: x {tuple(x.shape)} and dy {tuple(dy.shape)} must share a positive row count below 2^31")
    if tuple(A_lp.shape) != (rp, I) or tuple(B_lp.shape) != (O, rp) or not A_lp.is_contiguous() or not B_lp.is_contiguous():
        raise ValueError(f"{name}: expected contiguous A_lp {(rp, I)} and B_lp {(O, rp)}, got {tuple(A_lp.shape)} and {tuple(B_lp.shape)}")
    if A_lp.data_ptr() % 16 or B_lp.data_ptr() % 16:
        raise ValueError(f"{name}: A_lp and B_lp must be 16-byte aligned")
    ldx, ldy = _lora_rows(name, x, "x", 16), _lora_rows(name, dy, "dy", 16)
    if ldx % 8 or ldy % 8:
        raise ValueError(f"{name}: the row strides of x and dy must be multiples of 8, got {ldx} and {ldy}")
    if gA is None and gB is None:
        raise ValueError(f"{name}: neither gA nor gB")
    lda = ldb = 0
    if gA is not None:
        _lora_gpu(name, gA, F32, "gA")
        if gA.shape[0] < r or gA.shape[1] != I:
            raise ValueError(f"{name}: gA must be [>= {r}, {I}], got {tuple(gA.shape)}")
        lda = _lora_rows(name, gA, "gA", 4)
    if gB is not None:
        _lora_gpu(name, gB, F32, "gB")
        if gB.shape[0] != O or gB.shape[1] < r:
            raise ValueError(f"{name}: gB must be [{O}, >= {r}], got {tuple(gB.shape)}")
        ldb = _lora_rows(name, gB, "gB", 4)
    for t, nm in ((dy, "dy"), (A_lp, "A_lp"), (B_lp, "B_lp"), (gA, "gA"), (gB, "gB")):
        if t is not None and t.device != x.device:
            raise ValueError(f"{name}: {nm} is on {t.device}, x on {x.device}")
    need = lora_ws_bytes(M, I, O, rp)
    if ws is None:
        ws = _lora_ws_for(need, x.device)
    elif not ws.is_cuda or ws.device != x.device or ws.numel() * ws.element_size() < need or ws.data_ptr() % 16 or not ws.is_contiguous():
        raise ValueError(f"{name}: ws must be a contiguous 16-byte aligned buffer of at least {need} bytes on {x.device}")
    _, nchunks, _, _ = lora_plan(M, I, O, rp)
    both = int(gA is not None) + int(gB is not None)
    # per wanted gradient: one operand read by its projection and the other by its outer product (both gradients: X and dY twice),
    # T or U written and read, its half of the slabs written and read, the gradient read and written
    flops = 2.0 * M * rp * (I + O) * both
    nbytes = 2.0 * M * (I + O) * both + 4.0 * M * rp * both + 4.0 * nchunks * rp * (I + O) * both + 4.0 * r * (I + O) * both
    _launch("lora_wgrad", flops, nbytes,
            lambda: call("octmae_lora_wgrad", x.data_ptr(), ldx, dy.data_ptr(), ldy, A_lp.data_ptr(), B_lp.data_ptr(), float(s), M, I, O, r,
                         _p(gA), lda, _p(gB), ldb, ws.data_ptr(), ws.numel() * ws.element_size(), _stream()))


def white_border_limits(W: int):
    """The four column limits of the reference's border blanking (custom_util/misc.py:1458-1473) as integers, each found with the
    reference's own double expression: the left run is followed iff ``not (f > 0.01 * W)`` i.e. f < limits[0]; it is extended iff its
    end ``e > 0.05 * W`` i.e. e >= limits[1]; the right run is followed iff ``not (l < W - 0.01 * W)`` i.e. l >= limits[2]; its slice
    is assigned iff ``s < W - 0.05 * W`` i.e. s < limits[3].  At W = 512: (6, 26, 507, 487)."""
    W = int(W)
    cols = range(W + 1)
    return (next(i for i in cols if i > 0.01 * W), next(i for i in cols if i > 0.05 * W),
            next(i for i in cols if not (i < W - 0.01 * W)), next(i for i in cols if not (i < W - 0.05 * W)))


def white_border(imgs: torch.Tensor):
    """find_and_convert_large_white_region(image, 'tensor') (custom_util/misc.py:1438-1484) for a batch, IN PLACE: ``imgs`` f32
    [B, T, H, W] (contiguous, W a multiple of 4).  Per image the white pixels of frame 0 are those above max - 15/255 (max - min) over
    all frames; the runs of white columns that touch the left / right edge of a row are set to 0, and every frame becomes a copy of
    the blanked frame 0.  Returns ``(imgs, region)``, ``region`` bool [B, T, H, W] of the marked pixels.  Two launches, no
    synchronisation.  No autograd."""
    if imgs.dim() != 4:
        raise RuntimeError(f"white_border: expected imgs [B, T, H, W], got {tuple(imgs.shape)}")
    _chk(imgs, F32, "white_border imgs")
    Bn, T, Hh, Ww = imgs.shape
    if min(Bn, T, Hh, Ww) < 1 or Ww % 4:
        raise RuntimeError(f"white_border: needs a non-empty batch and a width that is a multiple of 4, got {tuple(imgs.shape)}")
    if imgs.requires_grad:
        raise RuntimeError("white_border: edits its input in place and has no backward")
    n_ws = load().octmae_white_border_ws_floats(Bn, T, Hh, Ww)
    if n_ws <= 0:
        raise RuntimeError(f"white_border: no workspace size for {tuple(imgs.shape)} (rc={n_ws})")
    ws = torch.empty(n_ws, dtype=F32, device=imgs.device)
    region = torch.empty(imgs.shape, dtype=torch.uint8, device=imgs.device)
    lim = white_border_limits(Ww)
    npx = Bn * T * Hh * Ww
    # algorithmic HBM bytes: every frame read once for the extremes, every frame and every mark written (frame 0's rows are re-read from cache)
    _launch("white_border", 0.0, float(4 * npx + 4 * npx + npx),
            lambda: call("octmae_white_border", imgs.data_ptr(), region.data_ptr(), ws.data_ptr(), Bn, T, Hh, Ww, *lim, _stream()))
    return imgs, region.view(torch.bool)


def _rank_counts(name: str, scores: torch.Tensor, labels: torch.Tensor, valid: Optional[torch.Tensor]) -> torch.Tensor:
    """The checks and the launch that ``rank_counts`` (valid None) and ``rank_counts_masked`` share."""
    flags = {"labels": labels} if valid is None else {"labels": labels, "valid": valid}
    n, C, planes = _plane_contract(name, {"scores": scores}, flags)
    ss, ls, *vs = _plane_strides(name, n, C, planes)
    scores, labels, mask = planes["scores"], planes["labels"], planes.get("valid")
    nan = torch.isnan(scores)
    if mask is not None:
        nan = nan & (mask != 0)
    if bool(nan.any()):
        raise ValueError(f"{name}: scores contain NaN" + ("" if valid is None else " at a valid position"))
    counts = torch.empty((n, C, 4), dtype=torch.int32, device=scores.device)
    # algorithmic HBM bytes: scores, labels (and the mask) read once (the re-reads of the j stream hit the caches), the counts written once
    if mask is None:
        _launch(name, 0.0, float(n * C * (4 + 1 + 16)),
                lambda: call("octmae_rank_counts", scores.data_ptr(), ss, labels.data_ptr(), ls, counts.data_ptr(), n, C, _stream()))
    else:
        _launch(name, 0.0, float(n * C * (4 + 1 + 1 + 16)),
                lambda: call("octmae_rank_counts_masked", scores.data_ptr(), ss, labels.data_ptr(), ls, mask.data_ptr(), vs[0],
                             counts.data_ptr(), n, C, _stream()))
    return counts


def rank_counts(scores: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """int32 [n, C, 4] = {gt_all, gt_pos, ge_all, ge_pos} per sample i and class c: the samples j with scores[j, c] > scores[i, c], how
    many of those are positive, and the same for >= (i counts itself).  AUROC, average precision and the precision-recall curve
    follow exactly from them (octcubem_amd/metrics.py).  ``scores`` float32 [n, C], ``labels`` bool or uint8 [n, C] (!= 0 = positive);
    both may be column slices of wider buffers (unit column stride, any row stride >= C).  IEEE comparisons: -0.0 ties with 0.0 and
    +-inf are ordinary values; a NaN raises ValueError before the launch (scikit-learn raises there too, and a NaN would silently count
    as zero).  That check reads one flag back from the device.  No autograd; no 16-bit operand, so autocast changes nothing."""
    return _rank_counts("rank_counts", scores, labels, None)


def rank_counts_masked(scores: torch.Tensor, labels: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
    """``rank_counts`` over a per-column population: column c ranks the samples with ``valid[:, c] != 0`` among themselves, and a
    sample outside the population gets four zeros (the output is fully written).  One launch for all the tasks of the multi-task
    evaluation, whose populations differ per task (OCTCube/engine_finetune.py:130-139 filters by boolean indexing on the CPU).
    ``scores`` float32 [n, C], ``labels`` and ``valid`` bool or uint8 [n, C]; each may be a column slice of a wider buffer (unit column
    stride, any row stride >= C).  Comparisons as in ``rank_counts``; a NaN raises ValueError before the launch only where it is VALID
    (the reference filters first, so a NaN in an excluded row is legal).  No autograd; no 16-bit operand."""
    return _rank_counts("rank_counts_masked", scores, labels, valid)


def bootstrap_rank_metrics(scores: torch.Tensor, labels: torch.Tensor, mult: torch.Tensor, unit: Optional[torch.Tensor] = None,
                           valid: Optional[torch.Tensor] = None) -> dict:
    """The ranking metrics of R bootstrap resamples of one evaluation set, from one sort (csrc/bootstrap.hip).  ``scores`` float32
    [n, C], ``labels`` and ``valid`` bool or uint8 [n, C] (column slices of wider buffers pass, as in ``rank_counts``); ``mult`` int32
    [R, U]: how often resampling unit u is drawn in resample r; ``unit`` int32 or int64 [n]: the unit of every sample (None: the sample
    itself, ``U == n``).  Returns device tensors ``P``, ``N``, ``U2`` (int64 [R, C]: weighted positives, negatives, twice the
    Mann-Whitney statistic) and ``ap_sum``, ``auprc``, ``max_f1`` (float64 [R, C]: average precision times P, the trapezoid area under
    the precision-recall points, the reference's best F1); ``octcubem_amd.metrics.bootstrap_rank_metrics`` divides and marks the pairs
    with ``P == 0`` or ``N == 0`` undefined.

    Every column is sorted once (``torch.sort``, descending, stable) and the unit ids and flag bytes of the kernel are built with ATen
    ops; the kernel then walks every resample over them.  ValueError before the launch, from four device reductions read back
    together: a unit id outside [0, U), a negative multiplicity, largest cluster x largest row sum of ``mult`` >= 2^31 (the running sums
    are 32-bit), a NaN score at a valid position.  +-inf are ordinary scores, -0.0 ties with 0.0.  No autograd, no CPU path."""
    name = "bootstrap_rank_metrics"
    flags = {"labels": labels} if valid is None else {"labels": labels, "valid": valid}
    n, C, planes = _plane_contract(name, {"scores": scores}, flags, _resample_tables(mult, unit))
    R, U, mult, unit, bad_unit, negative = _resample_contract(name, mult, unit, n)
    _plane_strides(name, n, C, planes)
    scores, lab = planes["scores"], planes["labels"] != 0
    val = None if valid is None else planes["valid"] != 0
    nan = torch.isnan(scores)
    if val is not None:
        nan = nan & val
    row_sum = mult.sum(dim=1, dtype=torch.int64).max()
    if unit is None:
        cluster = torch.ones((), dtype=torch.int64, device=scores.device)
    else:
        cluster = torch.bincount(unit.clamp(0, U - 1), minlength=U).max()
    # the four checks as one readback: [bad unit, negative multiplicity, NaN, largest cluster, largest row sum]
    bad_u, neg, has_nan, cl, rs = torch.stack([bad_unit.long(), negative.long(), nan.any().long(), cluster, row_sum]).tolist()
    if bad_u:
        raise ValueError(f"{name}: unit ids must lie in [0, {U})")
    if neg:
        raise ValueError(f"{name}: mult holds a negative multiplicity")
    if has_nan:
        raise ValueError(f"{name}: scores contain NaN" + ("" if valid is None else " at a valid position"))
    if cl * rs >= 2 ** 31:
        raise ValueError(f"{name}: a resample can weigh {cl} x {rs} >= 2^31 (largest cluster x largest row sum of mult): the running "
                         "sums of the kernel are 32-bit")
    vals, order = torch.sort(scores, dim=0, descending=True, stable=True)
    end = torch.ones((n, C), dtype=torch.bool, device=scores.device)
    if n > 1:
        end[:-1] = vals[:-1] != vals[1:]
    fl = torch.gather(lab, 0, order).to(torch.uint8) | (end.to(torch.uint8) << 1)
    fl |= 4 if val is None else torch.gather(val, 0, order).to(torch.uint8) << 2
    flag_bytes = fl.t().contiguous()
    unit_sorted = (order if unit is None else unit[order]).to(torch.int32).t().contiguous()
    dev = scores.device
    out = {k: torch.empty((R, C), dtype=torch.int64, device=dev) for k in ("P", "N", "U2")}
    out.update({k: torch.empty((R, C), dtype=torch.float64, device=dev) for k in ("ap_sum", "auprc", "max_f1")})
    # algorithmic HBM bytes: the unit ids and flag bytes once (every resample re-reads them from the caches), mult once, the outputs
    _launch(name, 0.0, float(C * n * 5 + R * U * 4 + R * C * 48),
            lambda: call("octmae_bootstrap_rank_metrics", unit_sorted.data_ptr(), flag_bytes.data_ptr(), mult.data_ptr(),
                         out["P"].data_ptr(), out["N"].data_ptr(), out["U2"].data_ptr(), out["ap_sum"].data_ptr(),
                         out["auprc"].data_ptr(), out["max_f1"].data_ptr(), n, C, R, U, _stream()))
    return out


def bootstrap_moments(pred: torch.Tensor, target: torch.Tensor, mult: torch.Tensor, unit: Optional[torch.Tensor] = None,
                      valid: Optional[torch.Tensor] = None, centre: Optional[torch.Tensor] = None) -> dict:
    """The eight weighted sums behind the regression metrics of R bootstrap resamples, as one int32 x f64 matrix product on the f64
    MFMA (csrc/bootmoments.hip).  ``pred`` and ``target`` float32 [n, C] and ``valid`` bool or uint8 [n, C] (column slices of wider
    buffers pass: unit column stride, any row stride >= C); ``mult`` int32 [R, U]; ``unit`` int32 or int64 [n] (None: the sample
    itself, ``U == n``); ``centre`` float64 [2, C], the shift of the predictions and of the targets (None: the float64 mean of the
    valid entries of each column, 0 for a column without one; a shift only, any value is mathematically correct).

    Returns device tensors ``moments`` float64 [R, C, 8] (per resample and column: count, sum a, sum b, sum a^2, sum b^2, sum a b,
    sum e^2, sum |e| with a = x - centre[0], b = y - centre[1], e = y - x), ``centre`` float64 [2, C] as used, and ``unit_moments``
    float64 [U, C, 8], the same sums per unit.  ``octcubem_amd.metrics.bootstrap_regression_measures`` finishes them.  Fixed summation
    order: the same bits on every run, and a resample's row does not depend on the other rows.

    ValueError before any launch, from one readback: a unit id outside [0, U), a negative multiplicity, a non-finite prediction or
    target at a valid position, a non-finite ``centre``.  No autograd, no CPU path."""
    name = "bootstrap_moments"
    n, C, planes = _plane_contract(name, {"pred": pred, "target": target}, {} if valid is None else {"valid": valid},
                                   _resample_tables(mult, unit) + ([] if centre is None else [("centre", centre, (torch.float64,))]))
    R, U, mult, unit, bad_unit, negative = _resample_contract(name, mult, unit, n)
    if centre is not None and centre.shape != (2, C):
        raise ValueError(f"{name}: expected centre [2, {C}], got {tuple(centre.shape)}")
    ps, ts, *vs = _plane_strides(name, n, C, planes)
    pred, target, val_bytes = planes["pred"], planes["target"], planes.get("valid")
    dev = pred.device
    val = None if val_bytes is None else val_bytes != 0
    bad_value = ~(torch.isfinite(pred) & torch.isfinite(target))
    if val is not None:
        bad_value = bad_value & val
    bad_centre = torch.zeros((), dtype=torch.bool, device=dev) if centre is None else ~torch.isfinite(centre).all()
    # the four checks as one readback: [bad unit, negative multiplicity, non-finite value, non-finite centre]
    bad_u, neg, bad_v, bad_c = torch.stack([bad_unit, negative, bad_value.any(), bad_centre]).tolist()
    if bad_u:
        raise ValueError(f"{name}: unit ids must lie in [0, {U})")
    if neg:
        raise ValueError(f"{name}: mult holds a negative multiplicity")
    if bad_v:
        raise ValueError(f"{name}: pred or target is not finite" + ("" if valid is None else " at a valid position"))
    if bad_c:
        raise ValueError(f"{name}: centre is not finite")
    if centre is None:
        # float64 sums over dim 0 of a fixed shape: torch reduces them without atomics, the same bits on every run
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        keep = torch.ones_like(pred, dtype=torch.bool) if val is None else val
        cnt = keep.sum(dim=0).clamp(min=1).double()
        centre = torch.stack([torch.where(keep, pred.double(), zero).sum(dim=0) / cnt, torch.where(keep, target.double(), zero).sum(dim=0) / cnt])
    centre = centre.detach().contiguous()
    if unit is None:
        order = torch.arange(n, dtype=torch.int32, device=dev)
        start = torch.arange(U + 1, dtype=torch.int32, device=dev)
    else:
        order = torch.sort(unit, stable=True).indices.to(torch.int32)
        start = torch.zeros(U + 1, dtype=torch.int32, device=dev)
        start[1:] = torch.cumsum(torch.bincount(unit, minlength=U), dim=0)
    cpad8 = (8 * C + 15) // 16 * 16
    F = torch.empty((U, cpad8), dtype=torch.float64, device=dev)
    D = torch.empty((R, cpad8), dtype=torch.float64, device=dev)
    nws = int(load().octmae_bootstrap_moments_ws(R, U, C))
    if nws < 0:
        raise ValueError(f"{name}: R = {R}, U = {U}, C = {C} exceed the kernel's limits (R <= 2^20, U <= 2^24, C <= 4096, R x padded columns < 2^32)")
    ws = torch.empty(max(nws, 1), dtype=torch.float64, device=dev)
    _launch("unit_moments", 0.0, float(n * C * 9 + U * cpad8 * 8),
            lambda: call("octmae_unit_moments", pred.data_ptr(), ps, target.data_ptr(), ts, 0 if val_bytes is None else val_bytes.data_ptr(),
                         vs[0] if vs else C, centre.data_ptr(), order.data_ptr(), start.data_ptr(), F.data_ptr(), n, C, U, _stream()))
    # algorithmic HBM bytes: mult once, F once (every block of resamples re-reads it from the caches), the output
    _launch(name, 2.0 * R * U * cpad8, float(R * U * 4 + U * cpad8 * 8 + R * cpad8 * 8),
            lambda: call("octmae_bootstrap_moments", mult.data_ptr(), F.data_ptr(), D.data_ptr(), ws.data_ptr(), R, U, C, _stream()))
    return {"moments": D[:, :8 * C].reshape(R, C, 8), "centre": centre, "unit_moments": F[:, :8 * C].reshape(U, C, 8)}


def _plane_contract(name: str, values: dict, flags: dict, tables=None):
    """The operand contract of the evaluation ops over [n, C] planes: ``values`` (float32) and ``flags`` (bool or uint8) by name, GPU
    tensors of one shape on one device, not empty.  ``tables``: a list of (name, tensor, dtypes) for the op's further operands, which must be GPU tensors of one of ``dtypes`` on that device; their shapes are the op's business.  Returns
    (n, C, planes): every plane by name, values first, detached, a flag plane as uint8 (a bool is stored as 0 / 1: the same bytes)."""
    operands = [(what, t, (F32,)) for what, t in values.items()] + [(what, t, (torch.bool, torch.uint8)) for what, t in flags.items()]
    operands += tables or []
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for _, t, _ in operands):
        raise RuntimeError(f"{name}: expected GPU tensors (the HIP path has no CPU fallback)")
    for what, t, dtypes in operands:
        if t.dtype not in dtypes:
            raise TypeError(f"{name}: {what} must be {' or '.join(str(d).split('.')[-1] for d in dtypes)}, got {t.dtype}")
    planes = {**values, **flags}
    first = next(iter(planes.values()))
    if first.dim() != 2 or any(t.shape != first.shape for t in planes.values()) or any(t.device != first.device for _, t, _ in operands):
        raise ValueError(f"{name}: expected {' and '.join(planes)} [n, C] on one device, got "
                         f"{' and '.join(str(tuple(t.shape)) for t in planes.values())}")
    n, C = first.shape
    if n < 1 or C < 1:
        raise ValueError(f"{name}: empty input {tuple(first.shape)}")
    return n, C, {what: t.detach().view(torch.uint8) if t.dtype == torch.bool else t.detach() for what, t in planes.items()}


def _plane_strides(name: str, n: int, C: int, planes: dict):
    """The row strides the kernels take for the planes of ``_plane_contract``, in their order: unit column stride, any row stride >= C
    (column slices of wider buffers); a single row has no stride to speak of and passes C.  Apart from ``_plane_contract`` because
    the bootstrap ops refuse a misshapen resampling table between the two."""
    for what, t in planes.items():
        if (C > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) < C):
            raise ValueError(f"{name}: {what} needs unit column stride and a row stride >= {C}, got strides {tuple(t.stride())}")
    return [t.stride(0) if n > 1 else C for t in planes.values()]


def _resample_tables(mult, unit):
    """The resampling operands as ``tables`` of ``_plane_contract``, which refuses a wrong dtype ahead of every shape."""
    return [("mult", mult, (torch.int32,))] + ([] if unit is None else [("unit", unit, (torch.int32, torch.int64))])


def _resample_contract(name: str, mult: torch.Tensor, unit: Optional[torch.Tensor], n: int):
    """The resampling contract of the bootstrap ops, after ``_plane_contract``: ``mult`` [R, U], not empty; ``unit`` [n], or None: every
    sample is its own unit and ``U == n``.  Returns (R, U, mult contiguous, unit as int64 or None) and two DEVICE flags for the
    caller's one readback: a unit id outside [0, U), a negative multiplicity.  Nothing here waits for the device."""
    if mult.dim() != 2 or mult.shape[0] < 1 or mult.shape[1] < 1:
        raise ValueError(f"{name}: expected mult [R, U], got {tuple(mult.shape)}")
    R, U = mult.shape
    if unit is None and U != n:
        raise ValueError(f"{name}: without unit every sample is its own unit: mult must be [R, {n}], got {tuple(mult.shape)}")
    if unit is not None and unit.shape != (n,):
        raise ValueError(f"{name}: expected unit [{n}], got {tuple(unit.shape)}")
    mult = mult.detach().contiguous()
    if unit is None:
        bad_unit = torch.zeros((), dtype=torch.bool, device=mult.device)
    else:
        unit = unit.detach().long()
        bad_unit = ((unit < 0) | (unit >= U)).any()
    return R, U, mult, unit, bad_unit, (mult < 0).any()


def _pair_shapes(name: str, a, b, others, fits: Optional[str] = None, f32_others: bool = False):
    """The operand contract of the ops on the f32 similarity tile (csrc/simtile.hpp): ``a`` float32 [n, d] and ``b`` float32 [m, d]
    on one GPU, none empty, row counts in int32.  ``others``: (tensor or None, name) pairs that must be GPU tensors too, and float32
    with ``f32_others``.  ``fits``: what of the op must fit int32 over the rows of ``b``; None: both row counts index tiles.
    Returns (n, m, d)."""
    operands = ((a, "a"), (b, "b")) + tuple(others)
    for t, nm in operands:
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{name}: {nm} must be a GPU tensor (the HIP path has no CPU fallback)")
    for t, nm in operands if f32_others else operands[:2]:
        if t is not None and t.dtype != F32:
            raise TypeError(f"{name}: {nm} must be float32, got {t.dtype}")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.device != b.device:
        raise ValueError(f"{name}: expected a [n, d] and b [m, d] on one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    n, d = a.shape
    m = b.shape[0]
    if n < 1 or m < 1 or d < 1:
        raise ValueError(f"{name}: empty input {tuple(a.shape)} / {tuple(b.shape)}")
    if fits is not None and m > 2 ** 31 - 1:
        raise ValueError(f"{name}: b has {m} rows, {fits} must fit int32")
    if fits is None and max(n, m) > 2 ** 31 - 1:
        raise ValueError(f"{name}: {max(n, m)} rows, the kernel indexes tiles with int32")
    return n, m, d


def _pair_strides(name: str, a: torch.Tensor, b: torch.Tensor):
    """The row strides the kernels take for the checked ``a`` and ``b``: unit column stride, any row stride >= d (slices of wider
    buffers); a single row has no stride to speak of and passes d.  Apart from ``_pair_shapes`` because ``retrieval_topk`` refuses a
    bad ``k`` between the two."""
    d = a.shape[1]
    for t, nm in ((a, "a"), (b, "b")):
        if (d > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < d):
            raise ValueError(f"{name}: {nm} needs unit column stride and a row stride >= {d}, got strides {tuple(t.stride())}")
    return (a.stride(0) if a.shape[0] > 1 else d), (b.stride(0) if b.shape[0] > 1 else d)


def _pair_tables(name: str, dev, n: int, m: int, target, keep, row_group, col_group):
    """The per-row and per-column tables of the retrieval ops: ``target`` and ``row_group`` int32 [n], ``col_group`` int32 [m] (the
    groups together or not at all), ``keep`` bool / uint8 [m], each optional and on ``dev``.  Returns them detached and contiguous,
    ``keep`` as uint8."""
    if (row_group is None) != (col_group is None):
        raise ValueError(f"{name}: row_group and col_group are given together or not at all")
    for t, nm, rows in ((target, "target", n), (row_group, "row_group", n), (col_group, "col_group", m)):
        if t is None:
            continue
        if t.dtype != torch.int32:
            raise TypeError(f"{name}: {nm} must be int32, got {t.dtype}")
        if tuple(t.shape) != (rows,) or t.device != dev:
            raise ValueError(f"{name}: {nm} must be [{rows}] on {dev}, got {tuple(t.shape)} on {t.device}")
    if keep is not None:
        if keep.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"{name}: keep must be bool or uint8, got {keep.dtype}")
        if tuple(keep.shape) != (m,) or keep.device != dev:
            raise ValueError(f"{name}: keep must be [{m}] on {dev}, got {tuple(keep.shape)} on {keep.device}")
        keep = keep.detach().contiguous()
        if keep.dtype == torch.bool:
            keep = keep.view(torch.uint8)
    target, row_group, col_group = (None if t is None else t.detach().contiguous() for t in (target, row_group, col_group))
    return target, keep, row_group, col_group


def retrieval_ranks(a: torch.Tensor, b: torch.Tensor, target: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                    row_group: Optional[torch.Tensor] = None, col_group: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [n, 4] per row i of ``a`` float32 [n, d] against the rows of ``b`` float32 [m, d], with s(i, j) the f32 fmaf chain over k
    (f32-input MFMA tiles, csrc/retrieval.hip; the [n, m] matrix is never stored) and t_i = s(i, target[i]):

      0  the kept columns j != target[i] with s(i, j) > t_i        1  the kept columns j < target[i] with s(i, j) == t_i
      2  the columns with col_group[j] == row_group[i], s(i, j) >= 0   3  the columns with col_group[j] == row_group[i]

    ``[:, 0] + [:, 1]`` is the target's place under a stable descending sort.  ``target`` int32 [n] (None: the diagonal, needs n == m),
    ``keep`` bool / uint8 [m] (None: every column), ``row_group`` int32 [n] and ``col_group`` int32 [m] (both or neither; without them
    columns 2 and 3 are 0).  ``a`` and ``b`` may be slices of wider buffers (unit column stride, any row stride >= d).  Non-finite
    features raise ValueError before the launch (that check reads one flag back from the device; a target that is not kept is refused
    the same way).  No autograd; no 16-bit operand, so autocast changes nothing."""
    name = "retrieval_ranks"
    n, m, d = _pair_shapes(name, a, b, ((target, "target"), (keep, "keep"), (row_group, "row_group"), (col_group, "col_group")),
                           fits="a count")
    a, b = a.detach(), b.detach()
    sa, sb = _pair_strides(name, a, b)
    if target is None and n != m:
        raise ValueError(f"{name}: without target the partner of row i is column i, which needs n == m; got n={n}, m={m}")
    target, keep, row_group, col_group = _pair_tables(name, a.device, n, m, target, keep, row_group, col_group)
    # one flag for every host-side refusal that needs the data: a single read-back
    bad = torch.stack([(~torch.isfinite(a)).any(), (~torch.isfinite(b)).any(),
                       ((target < 0) | (target >= m)).any() if target is not None else a.new_zeros((), dtype=torch.bool)]).tolist()
    if bad[0] or bad[1]:
        raise ValueError(f"{name}: {'a' if bad[0] else 'b'} contains non-finite values")
    if bad[2]:
        raise ValueError(f"{name}: target must lie in [0, {m})")
    if keep is not None:
        kept = keep[target.long()] if target is not None else keep
        if not bool((kept != 0).all()):
            raise ValueError(f"{name}: every target must be a kept column")
    out = torch.empty((n, 4), dtype=torch.int32, device=a.device)
    # algorithmic HBM bytes: a and b read once (the re-reads per tile hit the caches), the counts written once
    _launch(name, 2.0 * n * m * d, float(4 * (n + m) * d + 16 * n),
            lambda: call("octmae_retrieval_ranks", a.data_ptr(), sa, b.data_ptr(), sb, _p(target), _p(keep), _p(row_group), _p(col_group),
                         out.data_ptr(), n, m, d, _stream()))
    return out


RETRIEVAL_PAIR_MAX = 3      # RP_MAX_PAIRS of csrc/retrieval_pair.hip


def retrieval_pair_ranks(pairs) -> torch.Tensor:
    """int32 [P, 2, N, 2] for ``pairs`` = P (1 .. 3) tuples (a_p, b_p) of float32 [N, D] features, N and D the same for all: one walk
    over the f32 MFMA tiles of each product counts BOTH directions (csrc/retrieval_pair.hip), so

      out[p, 0] == retrieval_ranks(a_p, b_p)[:, :2]      out[p, 1] == retrieval_ranks(b_p, a_p)[:, :2]

    bit for bit (the partner of sample i is sample i; ``[..., 0] + [..., 1]`` is its place under a stable descending sort) at half the
    matrix work of the 2 P launches.  No ``target``, ``keep`` or groups.  Operands may be slices of wider buffers (unit column stride,
    any row stride >= D) and may be shared between pairs.  Non-finite features raise ValueError before the launch (one flag per
    operand, read back together).  No autograd; no 16-bit operand, so autocast changes nothing."""
    name = "retrieval_pair_ranks"
    pairs = [tuple(p) for p in pairs] if isinstance(pairs, (list, tuple)) else None
    if pairs is None or not 1 <= len(pairs) <= RETRIEVAL_PAIR_MAX or any(len(p) != 2 for p in pairs):
        raise ValueError(f"{name}: expected a list of 1 .. {RETRIEVAL_PAIR_MAX} (a, b) pairs")
    n, _, d = _pair_shapes(name, pairs[0][0], pairs[0][1], ())
    checked = []
    for a, b in pairs:
        shape = _pair_shapes(name, a, b, ())
        if shape != (n, n, d) or a.device != pairs[0][0].device:
            raise ValueError(f"{name}: every operand must be [{n}, {d}] on one device, got {tuple(a.shape)} and {tuple(b.shape)} on "
                             f"{a.device}")
        a, b = a.detach(), b.detach()
        checked.append((a, b) + _pair_strides(name, a, b))
    dev = checked[0][0].device
    # one flag per operand, one read-back (max |x| is finite iff every x is: a NaN propagates through the maximum)
    bad = (~torch.isfinite(torch.stack([torch.linalg.vector_norm(t, ord=float("inf")) for a, b, _, _ in checked for t in (a, b)]))).tolist()
    if any(bad):
        k = bad.index(True)
        raise ValueError(f"{name}: {'ab'[k % 2]} of pair {k // 2} contains non-finite values")
    P = len(checked)
    nws = int(load().octmae_retrieval_pair_ws(n, P))
    if nws < 0:
        raise ValueError(f"{name}: n = {n}, {P} pairs is beyond the kernel's workspace query")
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    out = torch.empty((P, 2, n, 2), dtype=torch.int32, device=dev)
    args = []
    for k in range(RETRIEVAL_PAIR_MAX):
        args += [checked[k][0].data_ptr(), checked[k][2], checked[k][1].data_ptr(), checked[k][3]] if k < P else [None, 0, None, 0]
    # algorithmic HBM bytes: every operand read once (the re-reads per tile hit the caches), the counts written once
    _launch(name, 2.0 * P * n * n * d, float(8 * P * n * d + 16 * P * n),
            lambda: call("octmae_retrieval_pair_ranks", *args, P, out.data_ptr(), ws.data_ptr(), nws, n, d, _stream()))
    return out


RETRIEVAL_TOPK_MAX = 32     # RT_KMAX of csrc/retrieval_topk.hip


def retrieval_topk(a: torch.Tensor, b: torch.Tensor, k: int, keep: Optional[torch.Tensor] = None,
                   row_group: Optional[torch.Tensor] = None, col_group: Optional[torch.Tensor] = None):
    """(idx int32 [n, k], score float32 [n, k]): per row i of ``a`` float32 [n, d] the k best rows of ``b`` float32 [m, d] under the
    score s(i, j) of ``retrieval_ranks`` (the same f32 fmaf chain off the same MFMA tiles, the same bits; csrc/retrieval_topk.hip --
    nothing of size [n, m] is stored).  Column j is a candidate of row i iff ``keep[j] != 0`` (``keep`` bool / uint8 [m]; None: every
    column) and ``col_group[j] != row_group[i]`` (int32 [n] and [m], both or neither; ``arange`` as both excludes the query itself).
    Order: higher score first, equal scores by ascending column -- a stable descending sort, IEEE comparisons (-0.0 ties with 0.0);
    the order is strict, so the result does not depend on the launch shape and two calls give the same bits.  A row with c < k
    candidates has ``idx = -1`` and ``score = -inf`` in slots c .. k-1; emptiness is the index.  ``k`` in 1 .. 32.  ``a`` and ``b`` may
    be slices of wider buffers (unit column stride, any row stride >= d).  Non-finite features raise ValueError before the launch
    (that check reads one flag back from the device).  No autograd; no 16-bit operand, so autocast changes nothing."""
    name = "retrieval_topk"
    n, m, d = _pair_shapes(name, a, b, ((keep, "keep"), (row_group, "row_group"), (col_group, "col_group")), fits="a column index")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= RETRIEVAL_TOPK_MAX:
        raise ValueError(f"{name}: k must be an int in [1, {RETRIEVAL_TOPK_MAX}], got {k!r}")
    a, b = a.detach(), b.detach()
    sa, sb = _pair_strides(name, a, b)
    _, keep, row_group, col_group = _pair_tables(name, a.device, n, m, None, keep, row_group, col_group)
    # max |x| is finite iff every x is (a NaN propagates through the maximum): two reductions without an [n, d] temporary, one read-back
    bad = (~torch.isfinite(torch.stack([torch.linalg.vector_norm(t, ord=float("inf")) for t in (a, b)]))).tolist()
    if bad[0] or bad[1]:
        raise ValueError(f"{name}: {'a' if bad[0] else 'b'} contains non-finite values")
    nws = int(load().octmae_retrieval_topk_ws(n, m, k))
    if nws < 0:
        raise ValueError(f"{name}: n = {n}, m = {m}, k = {k} is beyond the kernel's workspace query")
    ws = torch.empty(nws, dtype=torch.uint8, device=a.device) if nws else None
    idx = torch.empty((n, k), dtype=torch.int32, device=a.device)
    score = torch.empty((n, k), dtype=F32, device=a.device)
    # algorithmic HBM bytes: a and b read once (the re-reads per tile hit the caches), the lists written once
    _launch(name, 2.0 * n * m * d, float(4 * (n + m) * d + 8 * n * k),
            lambda: call("octmae_retrieval_topk", a.data_ptr(), sa, b.data_ptr(), sb, _p(keep), _p(row_group), _p(col_group), k,
                         idx.data_ptr(), score.data_ptr(), _p(ws), nws, n, m, d, _stream()))
    return idx, score


from ._autocast import no_autocast as _no_autocast  # noqa: E402


class ClipPairLossFn(torch.autograd.Function):
    """The checked operands of ``clip_pair_loss`` through octmae_clip_loss_fwd / _bwd (csrc/cliploss.hip).  Saved for the backward:
    the operands and the two log-sum-exp vectors -- nothing of size [n, m]."""

    @staticmethod
    def forward(ctx, a, b, scale, wr, wc, offset):
        n, d = a.shape
        m = b.shape[0]
        sa = a.stride(0) if n > 1 else d
        sb = b.stride(0) if m > 1 else d
        dev = a.device
        lse_row = torch.empty(n, dtype=F32, device=dev)
        lse_col = torch.empty(m, dtype=F32, device=dev) if wc is not None else None
        tscore = torch.empty(n, dtype=F32, device=dev)
        loss = torch.empty((), dtype=F32, device=dev)
        nws = load().octmae_clip_loss_ws_floats(n, m)
        if nws < 0:
            raise ValueError(f"clip_pair_loss: n = {n}, m = {m} is beyond the kernel's workspace")
        ws = torch.empty(nws, dtype=F32, device=dev)
        # algorithmic HBM bytes: a and b read once per side that walks them (the re-reads per tile hit the caches)
        _launch("clip_pair_loss", (4.0 if wc is not None else 2.0) * n * m * d, float(4 * (n + m) * d * (2 if wc is not None else 1)),
                lambda: call("octmae_clip_loss_fwd", a.data_ptr(), sa, b.data_ptr(), sb, scale.data_ptr(), wr.data_ptr(), _p(wc), offset,
                             lse_row.data_ptr(), _p(lse_col), tscore.data_ptr(), loss.data_ptr(), ws.data_ptr(), nws, n, m, d, _stream()))
        ctx.save_for_backward(a, b, scale, wr, wc, lse_row, lse_col)
        ctx.offset = offset
        return loss

    @staticmethod
    def backward(ctx, g):
        a, b, scale, wr, wc, lse_row, lse_col = ctx.saved_tensors
        n, d = a.shape
        m = b.shape[0]
        sa = a.stride(0) if n > 1 else d
        sb = b.stride(0) if m > 1 else d
        dev = a.device
        g = g.detach().to(F32).contiguous()
        need_a, need_b, need_s = ctx.needs_input_grad[:3]
        da = torch.empty((n, d), dtype=F32, device=dev) if need_a else None
        db = torch.empty((m, d), dtype=F32, device=dev) if need_b else None
        ds = torch.empty((), dtype=F32, device=dev) if need_s else None
        ws = torch.empty(n, dtype=F32, device=dev) if need_s else None
        if need_a or need_b or need_s:
            sides = (2.0 if need_a or need_s else 0.0) + (2.0 if need_b else 0.0)
            _launch("clip_pair_loss_bwd", sides * 2.0 * n * m * d, float(4 * (n + m) * d * 3),
                    lambda: call("octmae_clip_loss_bwd", a.data_ptr(), sa, b.data_ptr(), sb, scale.data_ptr(), wr.data_ptr(), _p(wc), ctx.offset,
                                 lse_row.data_ptr(), _p(lse_col), g.data_ptr(), _p(da), d, _p(db), d, _p(ds), _p(ws), n if need_s else 0, n, m,
                                 d, _stream()))
        return da, db, (ds.reshape(scale.shape) if need_s else None), None, None, None


@_no_autocast
def clip_pair_loss(a: torch.Tensor, b: torch.Tensor, logit_scale, wr: torch.Tensor, wc: Optional[torch.Tensor] = None,
                   offset: int = 0) -> torch.Tensor:
    """The scalar  L = sum_i wr[i] (lse_j z(i, j) - z(i, t_i)) + sum_i wc[i] (lse_i' z(i', t_i) - z(i, t_i))  with z = logit_scale * a @ b.T
    in the kernel's f32 arithmetic (s(i, j) the fmaf chain over k of csrc/retrieval.hip) and t_i = i + offset the partner column of row i;
    the second sum only when ``wc`` is given.  ``a`` float32 [n, d], ``b`` float32 [m, d] (slices of wider buffers are fine: unit column
    stride, any row stride >= d), ``logit_scale`` a float32 GPU scalar (0-dim or one element; read on the device), ``wr`` / ``wc`` float32
    [n].  n == m, offset 0, wr = wc = 1 / (2 n) is the reference's ClipLoss (open_clip/loss.py:148-230); without ``wc`` it is one
    ``cross_entropy(reduction='sum')`` with per-row weights of the rectangular block (``local_loss``: offset = local batch * rank).
    Gradients for ``a``, ``b`` and ``logit_scale``, none for the weights; the [n, m] logits are never stored, forward or backward, and two
    runs are bit-equal (csrc/cliploss.hip).  A non-finite feature gives a NaN loss and NaN gradients, as the ATen composition does: the
    caller's skip-step logic reads it.  ``offset`` outside 0 <= offset <= m - n raises ValueError before any launch.  No 16-bit operand,
    and an enclosing autocast changes nothing."""
    name = "clip_pair_loss"
    n, m, d = _pair_shapes(name, a, b, ((logit_scale, "logit_scale"), (wr, "wr"), (wc, "wc")), f32_others=True)
    _pair_strides(name, a, b)
    if logit_scale.numel() != 1 or logit_scale.device != a.device:
        raise ValueError(f"{name}: logit_scale must be one element on {a.device}, got {tuple(logit_scale.shape)} on {logit_scale.device}")
    for t, nm in ((wr, "wr"), (wc, "wc")):
        if t is not None and (tuple(t.shape) != (n,) or t.device != a.device):
            raise ValueError(f"{name}: {nm} must be [{n}] on {a.device}, got {tuple(t.shape)} on {t.device}")
    if not isinstance(offset, (int, np.integer)) or isinstance(offset, bool):
        raise TypeError(f"{name}: offset must be an int, got {type(offset).__name__}")
    offset = int(offset)
    if offset < 0 or n + offset > m:
        raise ValueError(f"{name}: the partner of row i is column i + offset, which needs 0 <= offset <= m - n; got offset={offset}, "
                         f"n={n}, m={m}")
    wr = wr.detach().contiguous()
    wc = None if wc is None else wc.detach().contiguous()
    return ClipPairLossFn.apply(a, b, logit_scale, wr, wc, offset)


def mix_tables(kind, lam, oml, box, Bn: int, H: int, W: int):
    """The host tables of ``mix_batch`` checked and brought to their device types: (kind int32 [B], lam f32 [B], oml f32 [B],
    box int32 [B, 4]).  ValueError for a wrong length, a kind outside {0, 1, 2}, or a cutmix box (yl, yh, xl, xh) that does not
    satisfy 0 <= yl <= yh <= H and 0 <= xl <= xh <= W.  Needs no GPU."""
    name = "mix_batch"
    kind = np.ascontiguousarray(kind, dtype=np.int32).reshape(-1)
    lam = np.ascontiguousarray(lam, dtype=np.float32).reshape(-1)
    oml = np.ascontiguousarray(oml, dtype=np.float32).reshape(-1)
    box = np.ascontiguousarray(box, dtype=np.int32)
    if kind.shape != (Bn,) or lam.shape != (Bn,) or oml.shape != (Bn,) or box.shape != (Bn, 4):
        raise ValueError(f"{name}: kind, lam, oml must have {Bn} entries and box [{Bn}, 4], got {kind.shape}, {lam.shape}, {oml.shape}, "
                         f"{box.shape}")
    if ((kind < 0) | (kind > 2)).any():
        raise ValueError(f"{name}: kind must be 0 (untouched), 1 (mixup) or 2 (cutmix)")
    b = box[kind == 2]
    if ((b[:, 0] < 0) | (b[:, 0] > b[:, 1]) | (b[:, 1] > H) | (b[:, 2] < 0) | (b[:, 2] > b[:, 3]) | (b[:, 3] > W)).any():
        raise ValueError(f"{name}: a cutmix box (yl, yh, xl, xh) must satisfy 0 <= yl <= yh <= {H} and 0 <= xl <= xh <= {W}")
    return kind, lam, oml, box


def mix_bytes(kind, box, S: int, H: int, W: int) -> float:
    """The bytes one ``mix_batch`` launch moves: a pair with a mixing side reads both samples and writes each side that mixes (and the
    partner's box where that side cuts); a pair that only cuts reads and writes its boxes, in every plane; kind 0 moves nothing."""
    Bn = len(kind)
    area = np.where(kind == 2, (box[:, 1] - box[:, 0]).astype(np.int64) * (box[:, 3] - box[:, 2]), 0) * (S // (H * W))
    ki, kj = kind[:Bn // 2], kind[::-1][:Bn // 2]
    ai, aj = area[:Bn // 2], area[::-1][:Bn // 2]
    full = (ki == 1) | (kj == 1)
    return 4.0 * float(np.where(full, 2 * S + np.where(ki == 1, S, ai) + np.where(kj == 1, S, aj), 2 * (ai + aj)).sum())


def mix_batch(x: torch.Tensor, kind, lam, oml, box, H: int, W: int) -> torch.Tensor:
    """Mixup / cutmix of the contiguous float32 GPU batch ``x`` [B, ..., H, W] in place, one launch (csrc/mixup.hip); returns ``x``.
    Per sample i, with partner j = B - 1 - i and x0 the batch before the call: ``kind[i]`` 0 leaves it untouched, 1 gives
    ``x[i] = x[i] * lam[i] + x0[j] * oml[i]`` (each product rounded on its own: bit-equal to torch's mul and add), 2 gives
    ``x[i][..., yl:yh, xl:xh] = x0[j][..., yl:yh, xl:xh]`` with ``box[i] = (yl, yh, xl, xh)`` over the last two dimensions.  ``kind``,
    ``lam``, ``oml`` and ``box`` are HOST tables (sequences or numpy arrays of length B; [B, 4] for the boxes): they are checked
    (``mix_tables``), packed and uploaded in one copy from pinned memory, without a device synchronisation.  A wrong table raises
    ValueError before the launch.  No autograd; no 16-bit operand, so autocast changes nothing."""
    name = "mix_batch"
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{name}: x must be a GPU tensor (the HIP path has no CPU fallback)")
    if x.dtype != F32:
        raise TypeError(f"{name}: x must be float32, got {x.dtype}")
    if x.dim() < 2 or not x.is_contiguous():
        raise ValueError(f"{name}: x must be a contiguous [B, ..., H, W] tensor, got {tuple(x.shape)} with strides {tuple(x.stride())}")
    Bn = x.shape[0]
    S = x.numel() // max(Bn, 1)
    H, W = int(H), int(W)
    if Bn < 2 or Bn % 2 or H < 1 or W < 1 or S < 1 or S % (H * W):
        raise ValueError(f"{name}: needs an even batch of samples that are whole [{H}, {W}] planes, got {tuple(x.shape)}")
    kind, lam, oml, box = mix_tables(kind, lam, oml, box, Bn, H, W)
    if not kind.any():
        return x                                        # nothing to do: no upload, no launch
    # one table, one copy: kind | lam | oml | box as 7 B 32-bit words in pinned memory (the caching host allocator keeps the block
    # until the copy has run)
    host = torch.empty(7 * Bn, dtype=torch.int32, pin_memory=True)
    h = host.numpy()
    h[:Bn] = kind
    h[Bn:2 * Bn] = lam.view(np.int32)
    h[2 * Bn:3 * Bn] = oml.view(np.int32)
    h[3 * Bn:] = box.reshape(-1)
    dev = host.to(x.device, non_blocking=True)
    base = dev.data_ptr()
    _launch(name, 0.0, mix_bytes(kind, box, S, H, W),
            lambda: call("octmae_mix_batch", x.data_ptr(), base, base + 4 * Bn, base + 8 * Bn, base + 12 * Bn, Bn, S, H, W, _stream()))
    return x


# optimistic (no running max) forward first, safe kernel as the device-side fallback.  Not in the half build: the un-normalised
# P = exp2(s) of that kernel is an MFMA operand, and half ends at 65 504 = e^11.09 where bfloat16 has fp32's range (the online-max
# kernel keeps P <= 2^8)
ATTN_OPTIMISTIC = not LP_IS_F16


_ATTN_CAPTURE: Optional[list] = None


class capture_attention:
    """``with ops.capture_attention() as seen:`` -- while it is active every ``attn_fwd`` appends ``(qkv, B, N, H, HD, scale)`` to
    ``seen``: the tensor it was given, no copy (the caller decides how long it lives: L * B * N * 3C * 2 bytes for a trunk of L
    blocks).  Off by default, and off it is one ``is None`` test: no launch, no allocation, not a bit of any output.  One hook for
    ``AttentionFn``, ``BlockFn`` and the SLIViT head (``saliency.attention_rollout`` reads it).  Not re-entrant across threads; a nested
    use captures into the inner list and restores the outer one."""

    def __enter__(self) -> list:
        global _ATTN_CAPTURE
        self._outer = _ATTN_CAPTURE
        _ATTN_CAPTURE = seen = []
        return seen

    def __exit__(self, *exc):
        global _ATTN_CAPTURE
        _ATTN_CAPTURE = self._outer
        return False


def attn_fwd(qkv: torch.Tensor, B: int, N: int, H: int, HD: int, scale: float, optimistic: Optional[bool] = None):
    if _ATTN_CAPTURE is not None:
        _ATTN_CAPTURE.append((qkv, B, N, H, HD, scale))
    o = torch.empty((B * N, H * HD), dtype=BF16, device=qkv.device)
    lse = torch.empty((B, H, N), dtype=F32, device=qkv.device)
    opt = ATTN_OPTIMISTIC if optimistic is None else optimistic
    flag = torch.empty((1,), dtype=torch.int32, device=qkv.device) if opt else None
    _launch(f"attn_fwd_hd{HD}", 4.0 * B * H * N * N * HD, 2.0 * 4 * B * N * H * HD,
            lambda: call("octmae_attn_fwd", qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), _p(flag), B, N, H, HD, float(scale), _stream()))
    return o, lse


# Which backward runs per head_dim: the single-pass kernel (csrc/attn_bwd.hip) or the dQ + dK/dV kernel pair (csrc/attn.hip).
# Measured on MI355X (same process, interleaved; docs/HISTORY.md section 4 "Attention"): head_dim 32 (decoder, N = 5121) fused 11 % faster;
# head_dim 64 fused 4 % faster at N = 1281 (encoder) and 2 % at N = 5121 (fine-tune) since its LDS-DMA requests go out between
# the sub-tiles and its sub-tile addressing is hand-placed (before: the pair 10-13 % faster).
ATTN_BWD_FUSED = {32: True, 64: True}


def set_option(key: str, value: int) -> int:
    """octmae_set_option: kernel-selection switch for A/B measurements and tests ("attn_bwd_hd32_form" / "attn_bwd_hd64_form":
    1 = one wave per SIMD (default), 0 = the two-waves-per-SIMD kernel; "gemm_small": 1 (default) = forward / dgrad launches that
    would leave most CUs idle take the small-launch kernel, 0 = never; "wgrad_stagger": length step of the k slices of a
    many-way split-K weight gradient, 0 = equal slices).  Returns the previous value."""
    prev = load().octmae_set_option(key.encode(), int(value))
    if prev < 0:
        raise RuntimeError(f"octmae_set_option: unknown key {key!r}")
    return prev


def set_deterministic(flag: bool) -> bool:
    """Deterministic mode (octmae_set_option("deterministic"), include/octmae.h): no float of a training step is added in the order
    workgroups happen to finish -- k-split weight gradients go through slabs and a fixed-order fold, bias gradients through the
    fixed-order column sums, the gradient norm through per-chunk partials.  Off by default; with it off nothing changes.  Returns
    the previous setting.  The environment variable OCTMAE_DETERMINISTIC wins over this call (is_deterministic() tells)."""
    return bool(set_option("deterministic", 1 if flag else 0))


def is_deterministic() -> bool:
    """Whether the library runs in deterministic mode (the environment variable included)."""
    return bool(load().octmae_deterministic())


_N_CU = {}
# fused backward only if its B * H workgroups fill this share of their rounds of CUs (0: always; OCTMAE_ATTN_BWD_MIN_FILL for A/B runs)
ATTN_BWD_FUSED_MIN_FILL = float(os.environ.get("OCTMAE_ATTN_BWD_MIN_FILL", "0.74"))


def attn_bwd_use_fused(B: int, H: int, HD: int, device=None) -> bool:
    """Which backward a call takes when the caller does not say.  The fused single-pass kernels run ONE workgroup per (batch, head) and CU:
    B * H workgroups, in rounds of the CU count.  Below three quarters of a round -- or of the last of a few rounds -- the idle CUs cost more
    than the dQ + dK/dV pair's two extra matrix products (it parallelises over query and key tiles as well): measured through the whole
    step on MI355X (H = 16; profiles/r04_small_batch.txt), 1 volume 42.2 vs 23.6 volumes/s for the pair, 2: 67.8 vs 43.0, 4: 98.9 vs 74.1,
    8: 126.6 vs 114.8, 12 (192 workgroups): equal, 16 (one full round): 148.3 vs 139.6 for the fused form, 24 (1.5 rounds): equal."""
    if not ATTN_BWD_FUSED[HD]:
        return False
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    ncu = _N_CU.get(idx)
    if ncu is None:
        ncu = _N_CU[idx] = int(torch.cuda.get_device_properties(idx).multi_processor_count)
    wgs = B * H
    rounds = -(-wgs // ncu)
    return wgs >= ATTN_BWD_FUSED_MIN_FILL * rounds * ncu


def attn_bwd(qkv, o, dout, lse, B, N, H, HD, scale, fused: Optional[bool] = None, delta: Optional[torch.Tensor] = None):
    """Gradient of attn_fwd w.r.t. the packed qkv.  Algorithmic work ("x3" in total): 4 matrix products =
    8 B H N^2 HD flop (dP, dV, dK, dQ); the recomputation of S is not counted.  ``delta`` (fp32 [B * N, H], from
    linear_dgrad_delta): the fused form then skips its pass over O and dO."""
    dqkv = torch.empty_like(qkv)
    st = _stream()
    unit = 2.0 * B * H * N * N * HD
    if attn_bwd_use_fused(B, H, HD, qkv.device) if fused is None else fused:
        kib = load().octmae_attn_bwd_fused_ws_kib(B, N, H, HD)
        if kib < 0:
            raise RuntimeError("octmae_attn_bwd_fused_ws_kib: unsupported shape")
        ws = torch.empty((kib * 256,), dtype=F32, device=qkv.device)     # dQ fp32 + padded row constants (contents irrelevant)
        # executes 5 products (S once); plus an fp32 read-modify-write of dQ per key block
        if delta is not None:
            _chk(delta, F32, "delta")
            _launch(f"attn_bwd_fused_hd{HD}", 4 * unit, 2.0 * 6 * B * N * H * HD,
                    lambda: call("octmae_attn_bwd_fused_delta", qkv.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                 ws.data_ptr(), dqkv.data_ptr(), B, N, H, HD, float(scale), st), exec_flops=5 * unit)
            return dqkv
        _launch(f"attn_bwd_fused_hd{HD}", 4 * unit, 2.0 * 6 * B * N * H * HD,
                lambda: call("octmae_attn_bwd_fused", qkv.data_ptr(), o.data_ptr(), dout.data_ptr(), lse.data_ptr(), ws.data_ptr(),
                             dqkv.data_ptr(), B, N, H, HD, float(scale), st), exec_flops=5 * unit)
        return dqkv
    rowc = torch.empty((2, B, H, N), dtype=F32, device=qkv.device)      # -lse*log2e | -rowsum(dO * O)
    # The two-kernel form executes 7 products: dq 3 (S, dP, dQ), dkv 4 (S, dP, dV, dK); the algorithmic 4 are booked
    # 1.6 / 2.4 in proportion.  The dQ kernel also produces the row constants (rowc) that the dK/dV kernel reads.
    _launch(f"attn_bwd_dq_hd{HD}", 1.6 * unit, 2.0 * 6 * B * N * H * HD,
            lambda: call("octmae_attn_bwd_dq_rowconst", qkv.data_ptr(), o.data_ptr(), dout.data_ptr(), lse.data_ptr(), rowc.data_ptr(),
                         dqkv.data_ptr(), B, N, H, HD, float(scale), st), exec_flops=3 * unit)
    _launch(f"attn_bwd_dkv_hd{HD}", 2.4 * unit, 2.0 * 6 * B * N * H * HD,
            lambda: call("octmae_attn_bwd_dkv", qkv.data_ptr(), dout.data_ptr(), rowc.data_ptr(), dqkv.data_ptr(), B, N, H, HD,
                         float(scale), st), exec_flops=4 * unit)
    return dqkv


def random_masking_ids(noise: torch.Tensor, len_keep: int, want_shuffle: bool = False):
    """Index part of random_masking (models_mae_joint_res_flash_attn.py:349-369): stable argsort on the GPU.
    Returns mask f32 [B,L], ids_restore i64 [B,L], ids_keep i64 [B,len_keep] (, ids_shuffle)."""
    _chk(noise, F32, "noise")
    Bn, L = noise.shape
    dev = noise.device
    ids_restore = torch.empty((Bn, L), dtype=torch.int64, device=dev)
    ids_keep = torch.empty((Bn, len_keep), dtype=torch.int64, device=dev)
    ids_shuffle = torch.empty((Bn, L), dtype=torch.int64, device=dev) if want_shuffle else None
    mask = torch.empty((Bn, L), dtype=F32, device=dev)
    call("octmae_random_masking_ids", noise.data_ptr(), ids_restore.data_ptr(), ids_keep.data_ptr() if len_keep > 0 else None, _p(ids_shuffle),
         mask.data_ptr(), Bn, L, len_keep, _stream())
    if want_shuffle:
        return mask, ids_restore, ids_keep, ids_shuffle
    return mask, ids_restore, ids_keep


def patch_gather(imgs: torch.Tensor, ids_keep: Optional[torch.Tensor], tp: int, p: int, nkeep: int) -> torch.Tensor:
    _chk(imgs, F32, "imgs")
    Bn, Cc, T, Hh, Ww = imgs.shape
    out = torch.empty((Bn * nkeep, Cc * tp * p * p), dtype=BF16, device=imgs.device)
    call("octmae_patch_gather", imgs.data_ptr(), _p(ids_keep), 1, out.data_ptr(), Bn, Cc, T, Hh, Ww, tp, p, nkeep, _stream())
    return out


def patch_scatter(dpatch: torch.Tensor, ids_keep: Optional[torch.Tensor], shape, tp: int, p: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The adjoint of ``patch_gather``: 16-bit ``dpatch`` [B*nkeep, C*tp*p*p] -> float32 [B, C, T, H, W] = ``shape``; the voxels of a
    kept token are its row widened exactly, every other voxel is +0.0 (whatever ``out`` held).  ``ids_keep``: int64 or int32
    [B, nkeep] with distinct ids per sample (the masking kernel's; not checked), or None = tokens 0 .. nkeep-1."""
    _chk(dpatch, BF16, "patch_scatter dpatch")
    Bn, Cc, T, Hh, Ww = (int(v) for v in shape)
    kdim = Cc * tp * p * p
    if dpatch.dim() != 2 or dpatch.shape[1] != kdim or dpatch.shape[0] % Bn:
        raise RuntimeError(f"patch_scatter: dpatch {tuple(dpatch.shape)} does not hold whole samples of [nkeep, {kdim}] rows for {Bn} samples")
    nkeep = dpatch.shape[0] // Bn
    is64 = 1
    if ids_keep is not None:
        if ids_keep.dtype not in (torch.int64, torch.int32):
            raise RuntimeError(f"patch_scatter ids_keep: expected int64 or int32, got {ids_keep.dtype}")
        _chk(ids_keep, ids_keep.dtype, "patch_scatter ids_keep")
        if tuple(ids_keep.shape) != (Bn, nkeep) or ids_keep.device != dpatch.device:
            raise RuntimeError(f"patch_scatter: ids_keep is {tuple(ids_keep.shape)} on {ids_keep.device}, expected {(Bn, nkeep)} on {dpatch.device}")
        is64 = int(ids_keep.dtype == torch.int64)
    if out is None:
        out = torch.empty((Bn, Cc, T, Hh, Ww), dtype=F32, device=dpatch.device)
    else:
        _chk(out, F32, "patch_scatter out")
        if tuple(out.shape) != (Bn, Cc, T, Hh, Ww) or out.device != dpatch.device:
            raise RuntimeError(f"patch_scatter: out is {tuple(out.shape)} on {out.device}, expected {(Bn, Cc, T, Hh, Ww)} on {dpatch.device}")
    # algorithmic HBM bytes: the kept rows read once (2 B), the whole volume written once (4 B)
    _launch("patch_scatter", 0.0, 2.0 * dpatch.numel() + 4.0 * out.numel(),
            lambda: call("octmae_patch_scatter", dpatch.data_ptr(), _p(ids_keep), is64, out.data_ptr(), Bn, Cc, T, Hh, Ww, tp, p, nkeep,
                         _stream()))
    return out


def _chk_stream(t: torch.Tensor, n_prefix: int, name: str):
    _chk(t, F32, name)
    if t.dim() != 3 or n_prefix < 0 or t.shape[1] <= n_prefix or t.shape[2] % 4 or t.shape[0] < 1:
        raise RuntimeError(f"{name}: expected float32 [B, {n_prefix} + L, C] with L >= 1 and C % 4 == 0, got {tuple(t.shape)}")
    return t.shape[0], t.shape[1] - n_prefix, t.shape[2]


def cam_weights(G: torch.Tensor, n_prefix: int = 1) -> torch.Tensor:
    """Grad-CAM's channel weights: float32 [B, C] = the mean of ``G`` float32 [B, n_prefix + L, C] over its L patch rows (the
    ``n_prefix`` leading rows -- the cls token -- are not read).  Two deterministic launches; no autograd."""
    G = G.detach()
    Bn, L, C = _chk_stream(G, n_prefix, "cam_weights G")
    n = load().octmae_cam_ws_floats(Bn, L, C)
    if n < 0:
        raise RuntimeError(f"cam_weights: unsupported size {tuple(G.shape)}")
    ws = torch.empty((n,), dtype=F32, device=G.device)
    w = torch.empty((Bn, C), dtype=F32, device=G.device)
    _launch("cam_weights", float(Bn * L * C), 4.0 * Bn * L * C + 4.0 * Bn * C,
            lambda: call("octmae_cam_weights", G.data_ptr(), w.data_ptr(), ws.data_ptr(), Bn, L, n_prefix, C, _stream()))
    return w


def cam_tokens(A: torch.Tensor, w: torch.Tensor, n_prefix: int = 1) -> torch.Tensor:
    """float32 [B, L]: cam[b, l] = max(0, sum_c w[b, c] * A[b, n_prefix + l, c]) for ``A`` float32 [B, n_prefix + L, C] and the
    ``cam_weights`` output ``w`` float32 [B, C].  One launch; no autograd."""
    A, w = A.detach(), w.detach()
    Bn, L, C = _chk_stream(A, n_prefix, "cam_tokens A")
    _chk(w, F32, "cam_tokens w")
    if tuple(w.shape) != (Bn, C) or w.device != A.device:
        raise RuntimeError(f"cam_tokens: w is {tuple(w.shape)} on {w.device}, expected {(Bn, C)} on {A.device}")
    cam = torch.empty((Bn, L), dtype=F32, device=A.device)
    _launch("cam_tokens", 2.0 * Bn * L * C, 4.0 * Bn * L * C + 4.0 * Bn * L,
            lambda: call("octmae_cam_tokens", A.data_ptr(), w.data_ptr(), cam.data_ptr(), Bn, L, n_prefix, C, _stream()))
    return cam


def cam_eigen(A: torch.Tensor, w: torch.Tensor, n_prefix: int = 1, iters: int = 32, relu: bool = True):
    """Eigen-smoothed Grad-CAM (pytorch_grad_cam's ``eigen_smooth``): ``(cam, residual)``, float32 [B, L] and [B].  Per sample the map is
    the projection of the centred weighted activations ``Mc = M - mean_l M``, ``M[l, c] = w[c] A[n_prefix + l, c]``, on their first right
    singular vector, found by ``iters`` power iterations on ``Mc^T Mc`` that never form ``M`` (include/octmae.h: octmae_cam_eigen).
    The sign is fixed so that the map correlates positively with the centred plain CAM; ``relu=False`` returns the signed projection.
    ``residual`` = ||Mc^T Mc v - lambda v|| / lambda: about (sigma2 / sigma1)^(2 iters), NaN for a sample with a non-finite value, 0 with
    an all-zero map where Mc vanishes.  3 iters + 7 deterministic launches; no autograd."""
    A, w = A.detach(), w.detach()
    Bn, L, C = _chk_stream(A, n_prefix, "cam_eigen A")
    _chk(w, F32, "cam_eigen w")
    if tuple(w.shape) != (Bn, C) or w.device != A.device:
        raise RuntimeError(f"cam_eigen: w is {tuple(w.shape)} on {w.device}, expected {(Bn, C)} on {A.device}")
    iters = int(iters)
    if iters < 1:
        raise RuntimeError(f"cam_eigen: iters = {iters}, at least one power iteration is needed")
    n = load().octmae_cam_eigen_ws_floats(Bn, L, C)
    if n < 0 or Bn > 65535:
        raise RuntimeError(f"cam_eigen: unsupported size {tuple(A.shape)}")
    ws = torch.empty((n,), dtype=F32, device=A.device)
    cam = torch.empty((Bn, L), dtype=F32, device=A.device)
    res = torch.empty((Bn,), dtype=F32, device=A.device)
    # per iteration A is read twice (rows, transposed product); once more for the mean, once for the centred plain CAM
    _launch("cam_eigen", 4.0 * (iters + 2) * Bn * L * C, 4.0 * (2 * iters + 4) * Bn * L * C,
            lambda: call("octmae_cam_eigen", A.data_ptr(), w.data_ptr(), cam.data_ptr(), res.data_ptr(), ws.data_ptr(), Bn, L, n_prefix, C,
                         iters, int(bool(relu)), _stream()))
    return cam, res


def cam_accumulate(acc: torch.Tensor, cam: torch.Tensor, width: int, flip: bool, weight: float, first: bool) -> torch.Tensor:
    """One pass of augmentation smoothing folded into ``acc`` in place (and returned): ``cam``, ``acc`` float32 [B, n] with
    ``n % width == 0``; ``acc[b, r, x] (first ? = : +=) weight * (cam[b, r, x'] - min_b) / (1e-7 + max_b - min_b)`` with ``x' = width - 1
    - x`` when ``flip`` (pytorch_grad_cam's scale_cam_image, then the horizontal flip undone).  ``first`` stores, so ``acc`` may be
    uninitialised.  A constant map contributes 0.  Two launches; no autograd."""
    cam = cam.detach()
    _chk(acc, F32, "cam_accumulate acc")
    _chk(cam, F32, "cam_accumulate cam")
    width = int(width)
    if (cam.dim() != 2 or acc.shape != cam.shape or acc.device != cam.device or cam.numel() < 1 or width < 1 or cam.shape[1] % width
            or acc.requires_grad):
        raise RuntimeError(f"cam_accumulate: expected float32 acc and cam [B, n] with n % width == 0 on one device, got {tuple(acc.shape)}, "
                           f"{tuple(cam.shape)} and width {width}")
    if acc.data_ptr() == cam.data_ptr():
        raise RuntimeError("cam_accumulate: acc and cam must not be the same buffer")
    Bn, n = cam.shape
    mnmx = torch.empty((Bn, 2), dtype=F32, device=cam.device)
    _launch("cam_accumulate", 4.0 * Bn * n, 4.0 * Bn * n * (3 if first else 4),
            lambda: call("octmae_cam_accumulate", acc.data_ptr(), cam.data_ptr(), mnmx.data_ptr(), Bn, n, width, int(bool(flip)),
                         float(weight), int(bool(first)), _stream()))
    return acc


def heatmap(m: torch.Tensor, size) -> torch.Tensor:
    """uint8 [B, F, H, W] heat volume of the float32 map ``m`` [B, t, h, w], ``size`` = (F, H, W) with W % 4 == 0: per sample
    v = (m - min) / (1e-7 + (max - min)) on the coarse map, resampled linearly along t and bilinearly over (h, w)
    (``F.interpolate``'s align_corners=False positions), then floor(255 v).  A constant map gives zeros.  Two launches; no autograd."""
    m = m.detach()
    _chk(m, F32, "heatmap map")
    Fo, Ho, Wo = (int(v) for v in size)
    if m.dim() != 4 or min(m.shape) < 1 or min(Fo, Ho, Wo) < 1 or Wo % 4:
        raise RuntimeError(f"heatmap: expected a float32 [B, t, h, w] map and a size (F, H, W) with W % 4 == 0, got {tuple(m.shape)} and "
                           f"{(Fo, Ho, Wo)}")
    Bn, t, h, w = m.shape
    mnmx = torch.empty((Bn, 2), dtype=F32, device=m.device)
    out = torch.empty((Bn, Fo, Ho, Wo), dtype=torch.uint8, device=m.device)
    _launch("heatmap", 0.0, 4.0 * m.numel() + float(out.numel()),
            lambda: call("octmae_heatmap", m.data_ptr(), mnmx.data_ptr(), out.data_ptr(), Bn, t, h, w, Fo, Ho, Wo, _stream()))
    return out


ROLLOUT_FUSIONS = ("mean", "max", "min")    # the `fusion` codes 0, 1, 2 of octmae_rollout_step
ROLLOUT_MAX_HD = 128                        # RO_MAX_HD of csrc/rollout.hip


def rollout_step(q: torch.Tensor, k: torch.Tensor, B: int, N: int, H: int, HD: int, scale: float, r: torch.Tensor,
                 head_fusion: str = "mean", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One block of attention rollout as a vector step (csrc/rollout.hip): float32 [B, N]

        r_out[b, j] = sum_i (r[b, i] / rho[b, i]) * (F[b, i, j] + [i == j])

    with ``P^h = softmax_j(scale * q_i . k_j)`` recomputed on the f32 MFMA tile of csrc/simtile.hpp, ``F = head_fusion_h P^h`` ("mean",
    "max" or "min") and ``rho = 1 + sum_j F`` (2 for "mean").  ``q``, ``k``: float32 [B * N, H * HD] (row b * N + i, head h at columns
    h * HD ..), unit column stride, any row stride >= H * HD -- the two thirds of a widened packed ``qkv`` are such slices.  ``r``:
    float32 [B, N], contiguous; ``out`` (optional): the same, another buffer.  Nothing of size [N, N] is stored; the workspace is
    (H + 1 + split) * B * N floats.  No atomics: two calls give the same bits, and a sample's row does not depend on the batch around
    it.  A non-finite ``q`` or ``k`` comes out as NaN.  No autograd; no 16-bit operand, so autocast changes nothing."""
    name = "rollout_step"
    B, N, H, HD = int(B), int(N), int(H), int(HD)
    if head_fusion not in ROLLOUT_FUSIONS:
        raise ValueError(f"{name}: head_fusion should be one of {ROLLOUT_FUSIONS}, got {head_fusion!r}")
    if min(B, N, H) < 1 or not 1 <= HD <= ROLLOUT_MAX_HD:
        raise ValueError(f"{name}: B, N, H >= 1 and 1 <= HD <= {ROLLOUT_MAX_HD} expected, got B={B}, N={N}, H={H}, HD={HD}")
    operands = ((q, "q"), (k, "k"), (r, "r")) + (((out, "out"),) if out is not None else ())
    for t, nm in operands:
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{name}: {nm} must be a GPU tensor (the HIP path has no CPU fallback)")
        if t.dtype != F32:
            raise TypeError(f"{name}: {nm} must be float32, got {t.dtype}")
        if t.device != q.device:
            raise ValueError(f"{name}: {nm} is on {t.device}, q on {q.device}")
    q, k, r = q.detach(), k.detach(), r.detach()
    W = H * HD
    for t, nm in ((q, "q"), (k, "k")):
        if tuple(t.shape) != (B * N, W):
            raise ValueError(f"{name}: {nm} must be [B * N, H * HD] = [{B * N}, {W}], got {tuple(t.shape)}")
        if (W > 1 and t.stride(1) != 1) or (B * N > 1 and t.stride(0) < W):
            raise ValueError(f"{name}: {nm} needs unit column stride and a row stride >= {W}, got strides {tuple(t.stride())}")
    for t, nm in operands[2:]:
        if tuple(t.shape) != (B, N) or not t.is_contiguous():
            raise ValueError(f"{name}: {nm} must be a contiguous [{B}, {N}] tensor, got {tuple(t.shape)} with strides {tuple(t.stride())}")
    if out is None:
        out = torch.empty((B, N), dtype=F32, device=q.device)
    elif out.requires_grad or out.data_ptr() == r.data_ptr():
        raise ValueError(f"{name}: out must be a buffer of its own that needs no gradient")
    fusion = ROLLOUT_FUSIONS.index(head_fusion)
    nws = int(load().octmae_rollout_ws(B, N, H, fusion))
    if nws < 0:
        raise ValueError(f"{name}: B = {B}, N = {N}, H = {H} is beyond the kernel's workspace query")
    ws = torch.empty(nws, dtype=torch.uint8, device=q.device)
    sq, sk = (q.stride(0) if B * N > 1 else W), (k.stride(0) if B * N > 1 else W)
    walks = 2 if fusion == 0 else 3
    # algorithmic HBM bytes: q and k read once per walk (the re-reads per tile hit the caches), the statistics written and read
    _launch(f"{name}_{head_fusion}", walks * 2.0 * B * H * N * N * HD, float(walks * 8 * B * N * W + 8 * B * H * N + 8 * B * N),
            lambda: call("octmae_rollout_step", q.data_ptr(), sq, k.data_ptr(), sk, B, N, H, HD, float(scale), fusion, r.data_ptr(),
                         out.data_ptr(), ws.data_ptr(), nws, _stream()))
    return out


# ------------------------------------------------------------------------------------------------
# autograd Functions
# ------------------------------------------------------------------------------------------------
def _as2d_bf16(g: torch.Tensor, cols: int) -> torch.Tensor:
    return cast_bf16(g.reshape(-1, cols).contiguous())


class LayerNormFn(torch.autograd.Function):
    """y(bf16) = LayerNorm(x f32) -- nn.LayerNorm(eps=1e-6) at video_vit.py:181-184 / models_mae…:489,:592."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        shp = x.shape
        x2 = _chk(x.reshape(-1, shp[-1]), F32, "layernorm input")
        y, mean, rstd = layernorm_fwd(x2, gamma, beta, eps)
        ctx.save_for_backward(x2, mean, rstd, gamma, beta)
        ctx.shp = shp
        return y.view(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, gamma, beta = ctx.saved_tensors
        D = x2.shape[1]
        dyb = _as2d_bf16(dy, D)
        colsum = torch.zeros(D, dtype=F32, device=x2.device)
        wg = _weight_grads
        dx, dxb = layernorm_bwd(dyb, x2, mean, rstd, gamma, grad_buf(gamma) if wg else None, grad_buf(beta) if wg else None,
                                want_bf16=True, dxsum=colsum)
        if wg:
            notify_grad_ready((gamma, beta))
        dx = dx.view(ctx.shp)
        _sidecar_put(dx, dxb.view(ctx.shp), colsum)      # the producing Block's backward takes these instead of redoing them
        return dx, None, None, None



class SlicePoolFn(torch.autograd.Function):
    """out fp32 [B, D] = mean over the S slices of fc_norm(pooled slice row), pooled = mean of the patch tokens (or the cls token) of
    x fp32 [B*S, T, D] -- the RETFound-all head (OCTCube/models_vit_3dhead_flash_attn.py:47-58 over models_vit_flash_attn.py:143-149);
    S = 1 is the 2-D ViT's own pooling.  The backward writes the dense token gradient together with its 16-bit copy and column sums
    for the producing Block (as LayerNormFn does)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, S, cls):
        x = _chk(x if x.is_contiguous() else x.contiguous(), F32, "slice_pool input")
        out, pooled, mean, rstd = slice_pool_fwd(x, gamma, beta, eps, S, cls)
        ctx.save_for_backward(pooled, mean, rstd, gamma, beta)
        ctx.meta = (x.shape, S, bool(cls))
        return out

    @staticmethod
    def backward(ctx, dout):
        pooled, mean, rstd, gamma, beta = ctx.saved_tensors
        shp, S, cls = ctx.meta
        dout = dout.contiguous().float()
        D = shp[-1]
        want_dx = ctx.needs_input_grad[0]
        colsum = torch.zeros(D, dtype=F32, device=dout.device) if want_dx else None
        dx, dxb = slice_pool_bwd(dout, pooled, mean, rstd, gamma, shp[1], S, cls,
                                 grad_buf(gamma) if ctx.needs_input_grad[1] and _weight_grads else None,
                                 grad_buf(beta) if ctx.needs_input_grad[2] and _weight_grads else None, want_bf16=want_dx, dxsum=colsum)
        if _weight_grads:
            notify_grad_ready((gamma, beta))
        if not want_dx:
            return None, None, None, None, None, None
        _sidecar_put(dx, dxb, colsum)      # the producing Block's backward takes these instead of redoing them
        return dx, None, None, None, None, None


class JoinFn(torch.autograd.Function):
    """(y, n_0, ..., n_{M-1}) = join of M raw tower outputs in front of the COEM classification head (csrc/join.hip): n_k the L2-normalised
    features (zeros where ``present_mask`` has bit k clear; pass None for that input), y = LayerNorm(concat n_k) in the 16-bit operand
    type, ready to be fc1's operand.  The backward routes the gradients arriving at the n_k (a model that also returns them) into the
    same kernel as ``dn_extra``; gamma / beta gradients are accumulated into their buffers as LayerNormFn does."""

    @staticmethod
    def forward(ctx, gamma, beta, eps, present_mask, *feats):
        feats = tuple(None if f is None else (f if f.is_contiguous() else f.contiguous()) for f in feats)
        y, n_out, inv_norm, mean, rstd = join_fwd(feats, present_mask, gamma, beta, eps)
        ctx.save_for_backward(gamma, beta, inv_norm, mean, rstd, *[f for f in feats if f is not None])
        ctx.slots = [f is not None for f in feats]
        ctx.mask = int(present_mask)
        ctx.set_materialize_grads(False)
        return (y,) + n_out.unbind(0)

    @staticmethod
    def backward(ctx, dy, *dn):
        gamma, beta, inv_norm, mean, rstd, *given = ctx.saved_tensors
        it = iter(given)
        feats = tuple(next(it) if s else None for s in ctx.slots)
        M = len(feats)
        ref = given[0]
        B, D = ref.shape
        dy = torch.zeros((B, M * D), dtype=F32, device=ref.device) if dy is None else dy.reshape(B, M * D).to(F32).contiguous()
        extra = None
        if any(d is not None for d in dn):
            zero = None
            parts = []
            for d in dn:
                if d is None:
                    zero = torch.zeros((B, D), dtype=F32, device=ref.device) if zero is None else zero
                    d = zero
                parts.append(d.to(F32))
            extra = torch.stack(parts).contiguous()
        wg = _weight_grads
        df = join_bwd(dy, extra, feats, inv_norm, mean, rstd, gamma, ctx.mask,
                      grad_buf(gamma) if wg and ctx.needs_input_grad[0] else None, grad_buf(beta) if wg and ctx.needs_input_grad[1] else None)
        if wg:
            notify_grad_ready((gamma, beta))
        return (None, None, None, None) + tuple(df[k] if (ctx.mask >> k) & 1 and ctx.needs_input_grad[4 + k] else None for k in range(M))


class SliceEmbedFn(torch.autograd.Function):
    """y fp32 [N, T, dim] = Linear(LayerNorm(C * L)(slice t of x transposed to [C, L] and flattened)) for the token stream
    x fp32 [N, n_prefix + T * L, C]: the Rearrange, LayerNorm and Linear of the SLIViT head's to_patch_embedding (models_slivit_head.py:37-38
    over vit-pytorch) fed by models_vit_st_flash_attn_slivit.py:245-257.  slab_norm_fwd writes the GEMM's 16-bit operand straight from the
    stream; the backward hands the dgrad GEMM's output to slab_norm_bwd.  No fp32 transposed copy exists either way; saved: the
    operand, the row statistics and a reference to x.  ``gamma`` / ``beta`` are the LayerNorm's parameters (their gradients are
    accumulated into their buffers as LayerNormFn does), ``params`` = (weight, bias) of the Linear with ``gw`` / ``gb`` their buffers."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, T, L, n_prefix, w_lp, b32, gw, gb, *params):
        x = x if x.is_contiguous() else x.contiguous()
        A, mean, rstd = slab_norm_fwd(x, gamma, beta, eps, T, L, n_prefix)
        y = linear_fwd(A, w_lp, b32, "f32")
        ctx.save_for_backward(x, A, mean, rstd, gamma, beta, w_lp)
        ctx.meta = (int(T), int(L), int(n_prefix))
        ctx.gw, ctx.gb, ctx.params = gw, gb, params
        return y.view(x.shape[0], T, w_lp.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x, A, mean, rstd, gamma, beta, w_lp = ctx.saved_tensors
        T, L, n_prefix = ctx.meta
        wg = _weight_grads
        want_w = wg and any(ctx.needs_input_grad[11:])
        want_g, want_b = wg and ctx.needs_input_grad[1], wg and ctx.needs_input_grad[2]
        nothing = (None,) * (11 + len(ctx.params))
        if not (ctx.needs_input_grad[0] or want_w or want_g or want_b):
            return nothing
        dyb = _as2d_bf16(dy, w_lp.shape[0])
        if want_w:
            linear_wgrad_accum(dyb, A, ctx.gw(), ctx.gb())
        dx = None
        if ctx.needs_input_grad[0] or want_g or want_b:
            dx = slab_norm_bwd(linear_dgrad(dyb, w_lp), x, mean, rstd, gamma, T, L, n_prefix,
                               grad_buf(gamma) if want_g else None, grad_buf(beta) if want_b else None)
        if wg:
            notify_grad_ready(((gamma, beta) if want_g or want_b else ()) + (tuple(ctx.params) if want_w else ()))
        return (dx if ctx.needs_input_grad[0] else None,) + nothing[1:]


class LinearFn(torch.autograd.Function):
    """y = x W^T + b on bf16 operands.  ``w_lp`` / ``b32`` are the (possibly fused q|k|v) bf16 weight and fp32 bias
    views; ``params`` = (weight params..., bias params...) whose .grad buffers are adjacent views of the arena."""

    @staticmethod
    def forward(ctx, x, w_lp, b32, gw, gb, out_f32, *params):
        shp = x.shape
        x2 = cast_bf16(x.reshape(-1, shp[-1]))
        y = linear_fwd(x2, w_lp, b32, "f32" if out_f32 else "bf16")
        ctx.save_for_backward(x2, w_lp)
        ctx.gw, ctx.gb, ctx.params, ctx.shp = gw, gb, params, shp
        return y.view(*shp[:-1], w_lp.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w_lp = ctx.saved_tensors
        N = w_lp.shape[0]
        dyb = _as2d_bf16(dy, N)
        if _weight_grads:
            gw, gb = ctx.gw(), ctx.gb()
            linear_wgrad_accum(dyb, x2, gw, gb)
            notify_grad_ready(ctx.params)
        dx = linear_dgrad(dyb, w_lp).view(ctx.shp) if ctx.needs_input_grad[0] else None
        return (dx, None, None, None, None, None) + (None,) * len(ctx.params)


class PatchEmbedFn(torch.autograd.Function):
    """PatchEmbed (Conv3d k=s=(tp,p,p) as a GEMM, video_vit.py:74-83) restricted to the kept tokens."""

    @staticmethod
    def forward(ctx, imgs, ids_keep, w_lp, b32, gw, gb, tp, p, nkeep, weight, bias):
        patches = patch_gather(imgs, ids_keep, tp, p, nkeep)
        tok = linear_fwd(patches, w_lp, b32, "bf16")
        if ctx.needs_input_grad[0]:      # the image gradient is wanted (saliency): its dgrad needs the weight and the kept ids as well
            ctx.save_for_backward(patches, w_lp, ids_keep)
            ctx.geom = (tuple(imgs.shape), tp, p)
        else:
            ctx.save_for_backward(patches)
        ctx.gw, ctx.gb, ctx.params = gw, gb, (weight, bias)
        return tok

    @staticmethod
    def backward(ctx, dtok):
        patches = ctx.saved_tensors[0]
        dyb = _as2d_bf16(dtok, dtok.shape[-1])
        if _weight_grads:
            gw = ctx.gw()
            linear_wgrad_accum(dyb, patches, gw.view(gw.shape[0], -1), ctx.gb())
            notify_grad_ready(ctx.params)
        dimgs = None
        if ctx.needs_input_grad[0]:      # adjoint of the gather applied to the GEMM's 16-bit activation gradient
            _, w_lp, ids_keep = ctx.saved_tensors
            shape, tp, p = ctx.geom
            dimgs = patch_scatter(linear_dgrad(dyb, w_lp), ids_keep, shape, tp, p)
        return (dimgs,) + (None,) * 10


class AttentionFn(torch.autograd.Function):
    """Attention (video_vit.py:112-138): fused q|k|v projection, flash attention core, output projection, and
    (inside a Block, video_vit.py:182) the residual add fused into the projection epilogue."""

    @staticmethod
    def forward(ctx, y, res, wqkv_lp, bqkv32, wproj_lp, bproj32, grads, H, *params):
        shp = y.shape
        Bn, N, Cc = shp
        HD = Cc // H
        scale = HD ** -0.5
        y2 = cast_bf16(y.reshape(-1, Cc))
        qkv = linear_fwd(y2, wqkv_lp, bqkv32, "bf16")
        o, lse = attn_fwd(qkv, Bn, N, H, HD, scale)
        if res is not None:
            out = linear_fwd(o, wproj_lp, bproj32, "resid", res=_chk(res.reshape(-1, Cc), F32, "residual"))
        else:
            out = linear_fwd(o, wproj_lp, bproj32, "bf16")
        ctx.save_for_backward(y2, qkv, o, lse, wqkv_lp, wproj_lp)
        ctx.meta = (Bn, N, H, HD, scale, res is not None)
        ctx.grads, ctx.params, ctx.shp = grads, params, shp
        return out.view(shp)

    @staticmethod
    def backward(ctx, dout):
        y2, qkv, o, lse, wqkv_lp, wproj_lp = ctx.saved_tensors
        Bn, N, H, HD, scale, has_res = ctx.meta
        Cc = H * HD
        wg = _weight_grads
        gwqkv, gbqkv, gwproj, gbproj = ctx.grads() if wg else (None,) * 4
        d2 = dout.reshape(-1, Cc)
        if not d2.is_contiguous():
            d2 = d2.contiguous()
        dob = cast_bf16(d2)
        if gbproj is not None:
            colsum_accum(d2 if d2.dtype in (F32, BF16) else dob, gbproj)
        if wg:
            linear_wgrad_accum(dob, o, gwproj)
        fused_bwd = attn_bwd_use_fused(Bn, H, HD, qkv.device)
        do, delta = linear_dgrad_delta(dob, wproj_lp, o, H, HD) if fused_bwd else (linear_dgrad(dob, wproj_lp), None)
        dqkv = attn_bwd(qkv, o, do, lse, Bn, N, H, HD, scale, fused=fused_bwd, delta=delta)
        if wg:
            linear_wgrad_accum(dqkv, y2, gwqkv, gbqkv)
            notify_grad_ready(ctx.params)
        dy = linear_dgrad(dqkv, wqkv_lp).view(ctx.shp)
        dres = dout if has_res else None
        return (dy, dres, None, None, None, None, None, None) + (None,) * len(ctx.params)


class MlpFn(torch.autograd.Function):
    """timm Mlp (fc1 -> exact GELU -> fc2) with the Block's residual add (video_vit.py:183) fused into fc2."""

    @staticmethod
    def forward(ctx, y, res, w1_lp, b1_32, w2_lp, b2_32, grads, *params):
        shp = y.shape
        Cc = shp[-1]
        y2 = cast_bf16(y.reshape(-1, Cc))
        ctx.pre_is_dgelu, ctx.fc1_bias = GELU_PRIME_FWD, b1_32 is not None
        pre, act = linear_fwd(y2, w1_lp, b1_32, "gelu", store_dgelu=ctx.pre_is_dgelu)
        if res is not None:
            out = linear_fwd(act, w2_lp, b2_32, "resid", res=_chk(res.reshape(-1, Cc), F32, "residual"))
        else:
            out = linear_fwd(act, w2_lp, b2_32, "bf16")
        ctx.save_for_backward(y2, pre, act, w1_lp, w2_lp)
        ctx.grads, ctx.params, ctx.shp, ctx.has_res = grads, params, shp, res is not None
        return out.view(*shp[:-1], w2_lp.shape[0])      # a head whose fc2 is not as wide as its input (models_vit_2mod); a Block's is

    @staticmethod
    def backward(ctx, dout):
        y2, pre, act, w1_lp, w2_lp = ctx.saved_tensors
        wg = _weight_grads
        gw1, gb1, gw2, gb2 = ctx.grads() if wg else (None,) * 4
        d2 = dout.reshape(-1, w2_lp.shape[0])
        if not d2.is_contiguous():
            d2 = d2.contiguous()
        dob = cast_bf16(d2)
        if gb2 is not None:
            colsum_accum(d2, gb2)
        if wg:
            linear_wgrad_accum(dob, act, gw2)
        dpre = linear_dgrad(dob, w2_lp, pre=pre, colsum=gb1, pre_is_dgelu=ctx.pre_is_dgelu, fold_entry=ctx.fc1_bias and not wg)
        if wg:
            linear_wgrad_accum(dpre, y2, gw1)
            notify_grad_ready(ctx.params)
        dy = linear_dgrad(dpre, w1_lp).view(ctx.shp)
        return (dy, dout if ctx.has_res else None, None, None, None, None, None) + (None,) * len(ctx.params)


class ConvNextLayerFn(torch.autograd.Function):
    """HF ConvNextLayer on a channels-last fp32 map [B, H, W, C]: depthwise 7x7 convolution (fp32) -> LayerNorm over C (eps 1e-6, 16-bit
    output) -> pwconv1 with the GELU epilogue -> pwconv2 (fp32 output) -> x + layer_scale * branch.  ``views`` = (dw weight [C, 7, 7], dw
    bias, LayerNorm weight, LayerNorm bias, layer scale) as fp32 arena views, (w1, w2) the 16-bit operand views and (b1, b2) the fp32
    biases of the two Linears; ``grads()`` returns the gradient views (gdw, gdwb, gln_w, gln_b, gw1, gb1, gw2, gb2, ggamma)."""

    @staticmethod
    def forward(ctx, x, views, w1_lp, b1_32, w2_lp, b2_32, grads, eps, *params):
        dw_w, dw_b, ln_w, ln_b, gamma = views
        B, H, W, C = x.shape
        x = _chk(x, F32, "ConvNextLayerFn input")
        z = dwconv7_fwd(x, dw_w, dw_b)
        z2 = z.view(-1, C)
        y, mean, rstd = layernorm_fwd(z2, ln_w, ln_b, eps)
        pre, act = linear_fwd(y, w1_lp, b1_32, "gelu")
        branch = linear_fwd(act, w2_lp, b2_32, "f32")
        out = layer_scale_fwd(x.view(-1, C), branch, gamma)
        ctx.save_for_backward(x, z2, mean, rstd, y, pre, act, branch, dw_w, ln_w, gamma, w1_lp, w2_lp)
        ctx.grads, ctx.params = grads, params
        return out.view(B, H, W, C)

    @staticmethod
    def backward(ctx, dout):
        x, z2, mean, rstd, y, pre, act, branch, dw_w, ln_w, gamma, w1_lp, w2_lp = ctx.saved_tensors
        B, H, W, C = x.shape
        wg = _weight_grads
        gdw, gdwb, gln_w, gln_b, gw1, gb1, gw2, gb2, ggamma = ctx.grads() if wg else (None,) * 9
        dout = dout if dout.is_contiguous() else dout.contiguous()
        d2 = _chk(dout.view(-1, C), F32, "ConvNextLayerFn gradient")
        dbr = layer_scale_bwd(d2, branch, gamma, ggamma)
        dpre = linear_dgrad(dbr, w2_lp, pre=pre, colsum=gb1, fold_entry=not wg)
        if wg:
            linear_wgrad_accum_pair((dbr, act, gw2, gb2), (dpre, y, gw1, None))
        dy = linear_dgrad(dpre, w1_lp)
        dz, _ = layernorm_bwd(dy, z2, mean, rstd, ln_w, gln_w, gln_b)
        dz = dz.view(B, H, W, C)
        if wg:
            dwconv7_bwd_weight(dz, x, gdw, gdwb)
            notify_grad_ready(ctx.params)
        dx = dwconv7_bwd_input(dz, dw_w, dres=dout) if ctx.needs_input_grad[0] else None
        return (dx,) + (None,) * (7 + len(ctx.params))


class MlpPairFn(torch.autograd.Function):
    """fc1 -> exact GELU ONCE over 2 B rows, then one fc2 per half: rows [0, B) through (w2a, b2a), rows [B, 2 B) through (w2b, b2b) --
    the two modality heads of models_vit_2mod behind one shared trunk pass.  The same launches as MlpFn without a residual, the fc2
    side once per half; the fc1 bias gradient is accumulated by both halves' dgrad epilogues."""

    @staticmethod
    def forward(ctx, y, w1_lp, b1_32, w2a_lp, b2a_32, w2b_lp, b2b_32, grads, *params):
        y2 = cast_bf16(y.reshape(-1, y.shape[-1]))
        if y2.shape[0] % 2:
            raise ValueError(f"MlpPairFn: {y2.shape[0]} rows are not two halves")
        B = y2.shape[0] // 2
        ctx.pre_is_dgelu = GELU_PRIME_FWD
        pre, act = linear_fwd(y2, w1_lp, b1_32, "gelu", store_dgelu=ctx.pre_is_dgelu)
        out_a = linear_fwd(act[:B], w2a_lp, b2a_32, "bf16")
        out_b = linear_fwd(act[B:], w2b_lp, b2b_32, "bf16")
        ctx.save_for_backward(y2, pre, act, w1_lp, w2a_lp, w2b_lp)
        ctx.grads, ctx.params, ctx.shp = grads, params, y.shape
        ctx.set_materialize_grads(False)
        return out_a, out_b

    @staticmethod
    def backward(ctx, da, db):
        y2, pre, act, w1_lp, w2a_lp, w2b_lp = ctx.saved_tensors
        B = y2.shape[0] // 2
        wg = _weight_grads
        gw1, gb1, gw2a, gb2a, gw2b, gb2b = ctx.grads() if wg else (None,) * 6
        halves = []
        for d, w2, gw2, gb2, rows in ((da, w2a_lp, gw2a, gb2a, slice(0, B)), (db, w2b_lp, gw2b, gb2b, slice(B, 2 * B))):
            if d is None:      # this head's output took no part in the loss
                halves.append(torch.zeros((B, w1_lp.shape[0]), dtype=BF16, device=y2.device))
                continue
            d2 = d.reshape(B, w2.shape[0])
            if not d2.is_contiguous():
                d2 = d2.contiguous()
            dob = cast_bf16(d2)
            if gb2 is not None:
                colsum_accum(d2, gb2)
            if wg:
                linear_wgrad_accum(dob, act[rows], gw2)
            halves.append(linear_dgrad(dob, w2, pre=pre[rows], colsum=gb1, pre_is_dgelu=ctx.pre_is_dgelu, fold_entry=not wg))
        dpre = torch.cat(halves)
        if wg:
            linear_wgrad_accum(dpre, y2, gw1)
            notify_grad_ready(ctx.params)
        dy = linear_dgrad(dpre, w1_lp).view(ctx.shp)
        return (dy,) + (None,) * 7 + (None,) * len(ctx.params)


# Gradients handed from one fused op to the one upstream of it, keyed by the fp32 gradient tensor they describe:
#   data_ptr -> (weakref to that tensor, bf16 copy, column sums)
# The consumer (the Block whose OUTPUT gradient this is) uses the pair only if the tensor autograd hands it is that very
# tensor; if autograd summed other contributions into a new tensor the entry is ignored (and the work redone locally).
import weakref

_grad_sidecar = {}


def _sidecar_purge():
    # entries whose fp32 gradient is gone can never be claimed: the first Block of a stack hands its gradient to a consumer that is
    # not a Block (sequence assembly), and its bf16 copy -- 0.34 / 0.67 GB at 128 volumes -- would otherwise stay pinned here
    # (the allocator hands out the same addresses step after step, so in practice two to four stale entries: 1.9 of the 252 GiB
    # a 128-volume micro-batch allocated)
    for k in [k for k, ent in _grad_sidecar.items() if ent[0]() is None]:
        del _grad_sidecar[k]


def _sidecar_put(dx: torch.Tensor, dxb: torch.Tensor, colsum: torch.Tensor):
    _sidecar_purge()
    if len(_grad_sidecar) > 64:
        _grad_sidecar.clear()
    _grad_sidecar[dx.data_ptr()] = (weakref.ref(dx), dxb, colsum)


def _sidecar_take(d: torch.Tensor):
    ent = _grad_sidecar.pop(d.data_ptr(), None)
    if ent is None:
        return None
    ref, dxb, colsum = ent
    if ref() is not d or dxb.shape != d.shape:
        return None
    return dxb, colsum


RECOMPUTE_NONE, RECOMPUTE_LIGHT, RECOMPUTE_FULL = 0, 1, 2


def _block_chain(x2d, Bn, N, H, HD, scale, eps1, eps2, lp, ln, s1, store_dgelu):
    """A Block's forward up to and including fc1 + GELU: every intermediate BlockFn's backward reads.  The forward runs it, and the
    backward of a Block at recompute level "full" runs it again on the saved input -- the same launches on the same operands, so
    (every launch being deterministic) the same bits."""
    wqkv, bqkv, wproj, bproj, w1, b1 = lp[:6]
    g1, be1, g2, be2 = ln
    y1, mean1, rstd1 = layernorm_fwd(x2d, g1, be1, eps1)
    qkv = linear_fwd(y1, wqkv, bqkv, "bf16")
    o, lse = attn_fwd(qkv, Bn, N, H, HD, scale)
    x2 = linear_fwd(o, wproj, bproj, "resid", res=x2d, rowscale=s1, rows_per_scale=N)
    y2, mean2, rstd2 = layernorm_fwd(x2, g2, be2, eps2)
    pre, act = linear_fwd(y2, w1, b1, "gelu", store_dgelu=store_dgelu)
    return mean1, rstd1, y1, qkv, o, lse, x2, mean2, rstd2, y2, pre, act


class BlockFn(torch.autograd.Function):
    """One pre-norm transformer Block (video_vit.py:181-184) as a single autograd node.

    forward : x -> LN1 -> Wqkv -> attention -> proj (+x) -> LN2 -> fc1 + GELU -> fc2 (+x2)          (7 launches)
    backward: the same chain in reverse with everything that only existed to please per-op autograd fused away:
              both residual gradient adds and the bf16 gradient copy happen inside the LayerNorm backward kernels, which also
              produce the proj / fc2 bias gradients (column sums of what they write); GELU' is the fc2-dgrad epilogue.

    ``recompute`` -- what the node keeps for its backward, per token and block at width C, hidden 4 C and 16-bit operands:
      0 none   36 C bytes: x, y1, qkv, o, x2, y2, pre, act (+ the row statistics and lse); nothing is rebuilt.
      1 light  24 C bytes: y1, y2 and act are dropped.  The backward rebuilds the LayerNorm outputs from the saved row statistics
               (ln_apply) and the GELU output from the stored pre-activation (gelu_apply): three memory-bound passes, launched only
               when weight gradients are wanted (nothing else reads the three).  With OCTMAE_GELU_PRIME_FWD=1 ``pre`` holds GELU'
               and the GELU output cannot be rebuilt from it: ``act`` then stays saved (28 C bytes).
      2 full    4 C bytes: x only (with the weights and the stochastic-depth factors).  The backward runs the forward chain again up
               to fc1 + GELU -- not the fc2 GEMM, whose output nothing reads -- and then proceeds as at level 0.
    The rebuilt tensors are bit-equal to the dropped ones, so the backward of every level runs the same launches on the same operands:
    outputs and input gradients are bit-identical, and so are the parameter gradients wherever level 0 repeats itself (everywhere but
    in split-K weight gradients that add fp32 atomically, at large sizes).  The stochastic-depth factors are the saved ones, never redrawn."""

    @staticmethod
    def forward(ctx, x, H, eps1, eps2, lp, grads, s1, s2, final_residual, recompute, lora, *params):
        """lora: None, or the adapter bundle of an adapted Block (octcubem_amd.lora.LoraBundle): its ``lp`` -- the merged operands
        W + s B A of the adapted Linears, written by ops.lora_merge -- replaces ``lp``, and the backward produces the adapter gradients
        (ops.lora_wgrad) and NO gradient of a base parameter of this Block (class docstring of LoraBundle).
        s1 / s2: None, or fp32 [B] per-sample stochastic-depth factors (0 or 1/keep_prob) of the attention / MLP branch.
        final_residual=False returns the MLP branch alone (flash_compat: what flash-attn's prenorm Block hands back as
        ``hidden_states`` and the reference's flash models feed to the final norm, models_mae_joint_res_flash_attn.py:480-489)."""
        if recompute not in (RECOMPUTE_NONE, RECOMPUTE_LIGHT, RECOMPUTE_FULL):
            raise ValueError(f"BlockFn: recompute level {recompute!r} (0 none, 1 light, 2 full)")
        shp = x.shape
        C = shp[-1]
        Bn, N = shp[0], shp[1]
        HD = C // H
        scale = HD ** -0.5
        if _grad_sidecar:
            _sidecar_purge()
        if lora is not None:
            lp = lora.lp
        ctx.lora = lora
        wqkv, bqkv, wproj, bproj, w1, b1, w2, b2 = lp
        g1, be1, g2, be2 = params[0], params[1], params[2], params[3]
        x2d = _chk(x.reshape(-1, C), F32, "block input")
        ctx.pre_is_dgelu, ctx.fc1_bias = GELU_PRIME_FWD, b1 is not None
        mean1, rstd1, y1, qkv, o, lse, x2, mean2, rstd2, y2, pre, act = _block_chain(
            x2d, Bn, N, H, HD, scale, eps1, eps2, lp, (g1, be1, g2, be2), s1, ctx.pre_is_dgelu)
        if final_residual:
            x3 = linear_fwd(act, w2, b2, "resid", res=x2, rowscale=s2, rows_per_scale=N)
        else:
            x3, s2 = linear_fwd(act, w2, b2, "f32"), None
        ctx.final_residual = final_residual
        ctx.recompute = recompute
        if recompute == RECOMPUTE_NONE:
            ctx.save_for_backward(x2d, mean1, rstd1, y1, qkv, o, lse, x2, mean2, rstd2, y2, pre, act, wqkv, wproj, w1, w2, g1, g2)
        elif recompute == RECOMPUTE_LIGHT:
            ctx.save_for_backward(x2d, mean1, rstd1, None, qkv, o, lse, x2, mean2, rstd2, None, pre, act if ctx.pre_is_dgelu else None,
                                  wqkv, wproj, w1, w2, g1, g2, be1, be2)
        else:
            ctx.save_for_backward(x2d, wqkv, wproj, w1, w2, g1, g2, be1, be2, bqkv, bproj, b1)
            ctx.eps = (eps1, eps2)
        ctx.scales = (s1, s2)
        ctx.meta = (Bn, N, H, HD, scale, shp)
        ctx.grads, ctx.params = grads, params
        if not final_residual:      # (MLP branch, stream before it): the pair flash-attn's prenorm Block returns
            return x3.view(shp), x2.view(shp)
        return x3.view(shp)

    @staticmethod
    def backward(ctx, dx3, dx2_in=None):
        Bn, N, H, HD, scale, shp = ctx.meta
        C = H * HD
        s1, s2 = ctx.scales
        if ctx.recompute == RECOMPUTE_FULL:
            x2d, wqkv, wproj, w1, w2, g1, g2, be1, be2, bqkv, bproj, b1 = ctx.saved_tensors
            with torch.no_grad():
                mean1, rstd1, y1, qkv, o, lse, x2, mean2, rstd2, y2, pre, act = _block_chain(
                    x2d, Bn, N, H, HD, scale, *ctx.eps, (wqkv, bqkv, wproj, bproj, w1, b1), (g1, be1, g2, be2), s1, ctx.pre_is_dgelu)
        else:
            x2d, mean1, rstd1, y1, qkv, o, lse, x2, mean2, rstd2, y2, pre, act, wqkv, wproj, w1, w2, g1, g2, *betas = ctx.saved_tensors
        lora = ctx.lora
        awg = _weight_grads and lora is not None      # adapter gradients at the two weight-gradient sites
        # off: every parameter-gradient side output below is a null pointer, the launches are the same.  An adapted Block never
        # produces a gradient of a base parameter: its side outputs are the null pointers of the switched-off path.
        wg = _weight_grads and lora is None
        (gg1, gb1n, gg2, gb2n, gwqkv, gbqkv, gwproj, gbproj, gw1, gb1, gw2, gb2) = ctx.grads() if wg else (None,) * 12
        if dx3.dtype != F32 or not dx3.is_contiguous():
            dx3 = dx3.contiguous().float()
        s1, s2 = ctx.scales
        side = _sidecar_take(dx3)
        d3 = dx3.view(-1, C)
        if s2 is not None:                       # stochastic depth: the MLP branch sees s2[b] * dx3 (the hand-off is unscaled)
            d3b = cast_bf16_rowscale(d3, s2, N)
            if gb2 is not None:
                colsum_accum(d3b, gb2)
        elif side is not None:                   # produced by the LayerNorm backward of the next Block
            d3b, colsum3 = side
            d3b = d3b.view(-1, C)
            if gb2 is not None:
                gb2.add_(colsum3)
        else:
            d3b = cast_bf16(d3)
            if gb2 is not None:
                colsum_accum(d3, gb2)
        # ---- MLP
        dpre = linear_dgrad(d3b, w2, pre=pre, colsum=gb1, pre_is_dgelu=ctx.pre_is_dgelu, fold_entry=ctx.fc1_bias and not wg)   # GELU' and fc1's bias gradient in the epilogue
        if wg:
            if ctx.recompute == RECOMPUTE_LIGHT:      # only the weight gradients read the two
                act = gelu_apply(pre) if act is None else act
                y2 = ln_apply(x2, mean2, rstd2, g2, betas[1])
            linear_wgrad_accum_pair((d3b, act, gw2, None), (dpre, y2, gw1, None))
        elif awg and (lora.has("fc1") or lora.has("fc2")):
            if ctx.recompute == RECOMPUTE_LIGHT:      # rebuilt only for the adapters that read them
                if lora.has("fc2"):
                    act = gelu_apply(pre) if act is None else act
                if lora.has("fc1"):
                    y2 = ln_apply(x2, mean2, rstd2, g2, betas[1])
            lora.wgrad("fc2", act, d3b)
            lora.wgrad("fc1", y2, dpre)
        if wg or awg:
            act = y2 = None
        dy2 = linear_dgrad(dpre, w1)
        # ---- LN2 backward + residual add + bf16 copy + proj bias gradient
        if ctx.final_residual:
            dres2 = d3
        else:                       # gradient arriving through the returned stream (None when only the branch was used)
            dres2 = None if dx2_in is None else dx2_in.contiguous().float().view(-1, C)
        if s1 is None:
            dx2, dx2b = layernorm_bwd(dy2, x2, mean2, rstd2, g2, gg2, gb2n, dres=dres2, want_bf16=True, dxsum=gbproj)
        else:
            dx2, _ = layernorm_bwd(dy2, x2, mean2, rstd2, g2, gg2, gb2n, dres=dres2, want_bf16=False, dxsum=None)
            dx2b = cast_bf16_rowscale(dx2, s1, N)
            if gbproj is not None:
                colsum_accum(dx2b, gbproj)
        # ---- attention
        fused_bwd = attn_bwd_use_fused(Bn, H, HD, qkv.device)
        do, delta = linear_dgrad_delta(dx2b, wproj, o, H, HD) if fused_bwd else (linear_dgrad(dx2b, wproj), None)
        dqkv = attn_bwd(qkv, o, do, lse, Bn, N, H, HD, scale, fused=fused_bwd, delta=delta)
        # the qkv bias gradient rides in the weight-gradient GEMM (column sums of its dY operand); fusing it into the attention
        # backward kernels had been measured and dropped (+10..25 % on their main loops for a 2 % pass)
        if wg:
            if ctx.recompute == RECOMPUTE_LIGHT:
                y1 = ln_apply(x2d, mean1, rstd1, g1, betas[0])
            linear_wgrad_accum_pair((dx2b, o, gwproj, None), (dqkv, y1, gwqkv, gbqkv))
        elif awg and (lora.has("proj") or lora.has("qkv")):
            if ctx.recompute == RECOMPUTE_LIGHT and lora.has("qkv"):
                y1 = ln_apply(x2d, mean1, rstd1, g1, betas[0])
            lora.wgrad("proj", o, dx2b)
            lora.wgrad("qkv", y1, dqkv)
        dy1 = linear_dgrad(dqkv, wqkv)
        # ---- LN1 backward + residual add; its bf16 copy / column sums are what the previous Block's backward needs
        colsum = torch.zeros(C, dtype=F32, device=dx3.device)
        dx, dxb = layernorm_bwd(dy1, x2d, mean1, rstd1, g1, gg1, gb1n, dres=dx2, want_bf16=True, dxsum=colsum)
        if wg:
            notify_grad_ready(ctx.params)
        elif awg:
            notify_grad_ready(lora.params)
        dx = dx.view(shp)
        _sidecar_put(dx, dxb.view(shp), colsum)
        return (dx, None, None, None, None, None, None, None, None, None, None) + (None,) * len(ctx.params)


class EncAssembleFn(torch.autograd.Function):
    """cls concat + gathered positional embedding (models_mae_joint_res_flash_attn.py:409-478).
    ``ids_restore`` (the masking's inverse permutation, [B, L]) lets the backward build the positional table's gradient as a
    deterministic gather (octmae_scatter_add_rows) instead of ATen's atomic index_add_; without it (the ViT models, where every
    token is kept in order) the ATen path is used."""

    @staticmethod
    def forward(ctx, tok, pos, cls, pos_cls, ids_keep, ids_restore=None):
        Bn, nkeep = ids_keep.shape
        D = tok.shape[-1]
        _chk(tok, BF16, "tokens"); _chk(ids_keep, torch.int64, "ids_keep")
        pos2 = _chk(pos.reshape(-1, D), F32, "pos table")
        x = torch.empty((Bn, nkeep + 1, D), dtype=F32, device=tok.device)
        call("octmae_enc_assemble", tok.data_ptr(), pos2.data_ptr(), cls.data_ptr(), pos_cls.data_ptr(), ids_keep.data_ptr(),
             x.data_ptr(), Bn, nkeep, D, _stream())
        if ids_restore is not None and (ids_restore.shape[0] != Bn or ids_restore.shape[1] != pos2.shape[0] or Bn > 1024 or D % 4):
            ids_restore = None
        if ids_restore is not None:
            # contract of octmae_scatter_add_rows: ids_restore is the inverse of the shuffle whose first nkeep entries are ids_keep
            # (source row of table row l = its rank ids_restore[b, l], when < nkeep); type / layout are checked here, the
            # permutation property by tests/test_gpu_kernels.py (and by OCTMAE_CHECK_IDS=1 on every call)
            _chk(ids_restore, torch.int64, "ids_restore")
            if _CHECK_IDS and not torch.equal(ids_restore.gather(1, ids_keep),
                                              torch.arange(nkeep, device=tok.device).expand(Bn, -1)):
                raise RuntimeError("EncAssembleFn: ids_restore is not the inverse permutation of ids_keep")
        ctx.save_for_backward(ids_keep, ids_restore if ids_restore is not None else ids_keep.new_empty(0))
        ctx.has_restore = ids_restore is not None
        ctx.pos_shape, ctx.cls_shape, ctx.pc_shape = pos.shape, cls.shape, pos_cls.shape
        return x

    @staticmethod
    def backward(ctx, dx):
        ids_keep, ids_restore = ctx.saved_tensors
        dx = dx.contiguous()
        Bn, n1, D = dx.shape
        nkeep = n1 - 1
        dtok = torch.empty((Bn * nkeep, D), dtype=BF16, device=dx.device)
        call("octmae_gather_rows_cast", dx.data_ptr(), None, dtok.data_ptr(), Bn, nkeep, n1, D, _stream())
        if not _weight_grads:        # no positional / cls table gradient
            return dtok, None, None, None, None, None
        if ctx.has_restore:
            L = ids_restore.shape[1]
            dpos = torch.empty(ctx.pos_shape, dtype=F32, device=dx.device)
            call("octmae_scatter_add_rows", dx.data_ptr(), ids_restore.data_ptr(), dpos.data_ptr(), Bn, nkeep, L, D, n1, 1, 0, _stream())
        else:
            dpos = torch.zeros(ctx.pos_shape, dtype=F32, device=dx.device)
            dpos.view(-1, D).index_add_(0, ids_keep.reshape(-1), dx[:, 1:, :].reshape(-1, D))
        dc = dx[:, 0, :].sum(0)
        return dtok, dpos, dc.view(ctx.cls_shape), dc.view(ctx.pc_shape).clone(), None, None


class DecAssembleFn(torch.autograd.Function):
    """mask-token append, un-shuffle, cls concat, positional embedding (models_mae_joint_res_flash_attn.py:515-573).
    ``dcls is None``: the 2-D MAE form (OCTCube/models_mae.py:175-178) -- emb carries 1 + nkeep rows per sample and its
    row 0 is the cls row."""

    @staticmethod
    def forward(ctx, emb, mask_token, dpos, dcls, dpos_cls, ids_restore, ids_keep):
        Bn, L = ids_restore.shape
        nkeep = ids_keep.shape[1]
        D = emb.shape[-1]
        _chk(emb, BF16, "decoder tokens"); _chk(ids_restore, torch.int64, "ids_restore"); _chk(ids_keep, torch.int64, "ids_keep")
        if _CHECK_IDS and not torch.equal(ids_restore.gather(1, ids_keep), torch.arange(nkeep, device=emb.device).expand(Bn, -1)):
            raise RuntimeError("DecAssembleFn: ids_restore is not the inverse permutation of ids_keep")
        dpos2 = _chk(dpos.reshape(-1, D), F32, "decoder pos table")
        x = torch.empty((Bn, L + 1, D), dtype=F32, device=emb.device)
        call("octmae_dec_assemble", emb.data_ptr(), mask_token.data_ptr(), dpos2.data_ptr(), _p(dcls), dpos_cls.data_ptr(),
             ids_restore.data_ptr(), x.data_ptr(), Bn, nkeep, L, D, 1 if dcls is None else 0, _stream())
        ctx.save_for_backward(ids_restore, ids_keep)
        ctx.shapes = (mask_token.shape, dpos.shape, None if dcls is None else dcls.shape, dpos_cls.shape)
        return x

    @staticmethod
    def backward(ctx, dx):
        ids_restore, ids_keep = ctx.saved_tensors
        dx = dx.contiguous()
        Bn, L1, D = dx.shape
        nkeep = ids_keep.shape[1]
        ms, ps, cs, pcs = ctx.shapes
        if cs is None:      # cls row travels with the tokens: ids = [-1, ids_keep]  (source row = 1 + id)
            ids = torch.cat([ids_keep.new_full((Bn, 1), -1), ids_keep], dim=1).contiguous()
            demb = torch.empty((Bn * (nkeep + 1), D), dtype=BF16, device=dx.device)
            call("octmae_gather_rows_cast", dx.data_ptr(), ids.data_ptr(), demb.data_ptr(), Bn, nkeep + 1, L1, D, _stream())
        else:
            demb = torch.empty((Bn * nkeep, D), dtype=BF16, device=dx.device)
            call("octmae_gather_rows_cast", dx.data_ptr(), ids_keep.data_ptr(), demb.data_ptr(), Bn, nkeep, L1, D, _stream())
        if not _weight_grads:        # no mask-token, positional / cls table gradient
            return demb, None, None, None, None, None, None
        if Bn <= 1024 and D % 4 == 0:
            # one pass over dx: positional-table gradient and, per table row, the sum over the samples that masked it
            L = L1 - 1
            ddpos = torch.empty((L, D), dtype=F32, device=dx.device)
            part = torch.empty((L, D), dtype=F32, device=dx.device)
            call("octmae_dec_assemble_bwd", dx.data_ptr(), ids_restore.data_ptr(), ddpos.data_ptr(), part.data_ptr(), Bn, nkeep, L, D,
                 _stream())
            dmask = torch.zeros(D, dtype=F32, device=dx.device)
            colsum_accum(part, dmask)
        else:
            body = dx[:, 1:, :]
            masked = (ids_restore >= nkeep).to(F32).unsqueeze(-1)
            dmask = (body * masked).sum((0, 1))
            ddpos = body.sum(0)
        dc = dx[:, 0, :].sum(0)
        return (demb, dmask.view(ms), ddpos.view(ps), None if cs is None else dc.view(cs), dc.view(pcs).clone(), None, None)


class PatchMSEFn(torch.autograd.Function):
    """Fused patchify + per-token MSE (models_mae_joint_res_flash_attn.py:289-314, :649-650).
    pred_full f32 [B, L+1, PD] (row 0 = cls) -> loss_tok f32 [B, L]."""

    @staticmethod
    def forward(ctx, pred_full, imgs, frame_idx, u_sz, p, norm_pix):
        Bn, L1, PD = pred_full.shape
        L = L1 - 1
        _, Cc, T, Hh, Ww = imgs.shape
        _chk(pred_full, F32, "pred"); _chk(imgs, F32, "imgs")
        loss_tok = torch.empty((Bn, L), dtype=F32, device=imgs.device)
        call("octmae_mse_fwd", pred_full.data_ptr(), imgs.data_ptr(), _p(frame_idx), loss_tok.data_ptr(), Bn, Cc, T, Hh, Ww, u_sz, p, L,
             int(norm_pix), _stream())
        ctx.save_for_backward(pred_full, imgs, frame_idx if frame_idx is not None else torch.empty(0, device=imgs.device))
        ctx.meta = (u_sz, p, int(norm_pix), frame_idx is not None)
        return loss_tok

    @staticmethod
    def backward(ctx, dl):
        if ctx.needs_input_grad[1]:
            # the reference's loss is differentiable through its target patchify(imgs) as well; that term is not built, and the
            # encoder-side gradient alone would be a partial one
            raise RuntimeError("PatchMSEFn: the gradient of the reconstruction loss with respect to imgs was requested, but the "
                               "term through the loss target patchify(imgs) is not implemented; detach imgs (the pre-training step "
                               "never needs this gradient)")
        pred_full, imgs, frame_idx = ctx.saved_tensors
        u_sz, p, norm_pix, has_fi = ctx.meta
        Bn, L1, PD = pred_full.shape
        _, Cc, T, Hh, Ww = imgs.shape
        dl = dl.contiguous().to(F32)
        coef = torch.full((1,), 2.0 / PD, dtype=F32, device=imgs.device)
        dpred = torch.empty((Bn, L1, PD), dtype=BF16, device=imgs.device)
        call("octmae_mse_bwd", pred_full.data_ptr(), imgs.data_ptr(), frame_idx.data_ptr() if has_fi else None, dl.data_ptr(),
             coef.data_ptr(), dpred.data_ptr(), Bn, Cc, T, Hh, Ww, u_sz, p, L1 - 1, norm_pix, _stream())
        return dpred, None, None, None, None, None
