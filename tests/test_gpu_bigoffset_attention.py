"""The attention kernels with qkv, dqkv, o, dout and the fused backward's workspace past 2^31 and 2^32 bytes -- `pytest -m gpu` on an
MI355X.

Many short samples make the tensors large while the N^2 work stays trivial (tests/bigoffset_ref.py::ATTN_CASES): (H, HD, N) =
(16, 64, 257) and (8, 32, 513), one key past the first full key block of the fused backward, so its main kernel and its tail both
run; B such that qkv passes 2^31 and 2^32 bytes, and once such that o and dout (a third of qkv) pass 2^31 too -- there the fp32 dQ
workspace is itself past 2^32 bytes.  The tile loaders address one SAMPLE through 32-bit descriptor offsets (csrc/attn_tile.hpp);
what reaches past 2^31 here is everything that spans samples: the sample's base pointer, the row index of the stores, lse, the row
constants and the workspace.

Every form of tests/test_gpu_attention_rows.py::_Case.every_form is a case of its own, and the fused backward with `delta`
supplied: both forwards; the dQ + dK/dV pair; the fused backward in both main-kernel forms; its tail in a launch of its own.  The
backward forms are handed the o and lse of the default forward KERNEL.

Reference: float64 softmax attention and its gradients in closed form, per chunk of CS samples on the device.  Bound: the rule of
tests/rowwise.py / tests/test_gpu_attention_rows.py -- the rounding model of the kernels (oracle/bf16_points.py, float64 with a rounding
where the kernels round, fed what the kernel under test is fed) has a worst row of its own against float64 over the whole tensor,
and the kernel may have 2 x that.  The model runs on the device here, chunk by chunk beside the reference.  The worst row is kept
per band of byte offsets of the tensor it belongs to (o, lse by o's offsets; dQ, dK, dV by qkv's) and goes to the parity ledger."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import ops
    from octcubem_amd._lib import load
    LP = ops.BF16
else:
    LP = torch.bfloat16
from tests import bigoffset_ref as BR
from tests.conftest import parity

DEV = "cuda"
FACTOR = 2.0
CS = 16                       # samples per chunk of the reference
F64 = torch.float64
FORMS = ("fwd_optimistic", "fwd_online_max", "bwd_pair", "bwd_fused_form1", "bwd_fused_form0", "bwd_fused_tail_unfused", "bwd_fused_delta")


def _draw(B, N, H, HD, seed):
    """qkv [B*N, 3*H*HD] and do [B*N, H*HD] as tests/rowwise.py::draw_inputs makes them (value rows with an offset that ramps along the
    sequence, dO rows with a scale that cycles), drawn on the device in chunks of samples; random across samples, never periodic"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = torch.empty((B * N, 3 * H * HD), dtype=LP, device=DEV)
    do = torch.empty((B * N, H * HD), dtype=LP, device=DEV)
    n = torch.arange(N, dtype=torch.float32, device=DEV)
    ramp = (3.0 * (n + 0.5) / N - 1.5).view(1, N, 1, 1)
    cyc = (2.0 ** (2.0 * ((n * 0.381966) % 1.0) - 1.0)).view(1, N, 1, 1)
    for b0 in range(0, B, 64):
        b1 = min(b0 + 64, B)
        x = torch.randn((b1 - b0, N, 3, H, HD), generator=g, device=DEV)
        x[:, :, 2] += ramp
        qkv[b0 * N:b1 * N] = x.reshape(-1, 3 * H * HD).to(LP)
        d = torch.randn((b1 - b0, N, H, HD), generator=g, device=DEV) * cyc
        do[b0 * N:b1 * N] = d.reshape(-1, H * HD).to(LP)
    return qkv, do


def _heads(t, n, N, H, HD):
    return t.view(n, N, H, HD).transpose(1, 2)


def _split(t, n, N, H, HD):
    return t.view(n, N, 3, H, HD).permute(2, 0, 3, 1, 4)


def _reference(q, k, v, do, scale):
    """float64 softmax attention and its gradients for one chunk [n, H, N, HD]"""
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse.unsqueeze(-1))
    del s
    o = P @ v
    dV = P.transpose(-1, -2) @ do
    dS = P * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    del P
    return {"o": o, "lse": lse, "dq": scale * (dS @ k), "dk": scale * (dS.transpose(-1, -2) @ q), "dv": dV}


class _Meter:
    """kernel and model errors of one tensor, per band"""

    def __init__(self, sample_bytes):
        self.kern, self.model = BR.Worst(sample_bytes, DEV), BR.Worst(sample_bytes, DEV)
        self.ref_max = torch.zeros((), dtype=F64, device=DEV)

    def rows(self, b0, got, mod, ref):
        self.kern.add(b0, BR.attn_row_err_rows(got, ref).flatten(1).amax(1))
        self.model.add(b0, BR.attn_row_err_rows(mod, ref).flatten(1).amax(1))

    def lse(self, b0, got, mod, ref):
        """tests/rowwise.py::lse_err: |lse - ref| / (1 + max |ref|), the maximum taken over the whole tensor at the end"""
        for w, t in ((self.kern, got), (self.model, mod)):
            e = (t.to(F64) - ref).abs()
            w.add(b0, torch.where(torch.isfinite(e), e, torch.full_like(e, math.inf)).flatten(1).amax(1))
        self.ref_max = torch.maximum(self.ref_max, ref.abs().max())

    def report(self, label, fails, lse=False):
        div = 1.0 + float(self.ref_max) if lse else 1.0
        own = max(v for v in self.model.result() if v is not None) / div
        bound = FACTOR * own
        for name, v in zip(BR.BANDS, self.kern.result()):
            if v is None:
                continue
            print(f"{label}/{name}: worst row {v / div:.3e}, model {own:.3e}, bound {bound:.3e}")
            try:
                parity(f"{label}/{name}", v / div, bound)
            except AssertionError as e:
                fails.append(str(e))


def _fused_ws(B, N, H, HD):
    kib = load().octmae_attn_bwd_fused_ws_kib(B, N, H, HD)
    assert kib > 0
    return torch.empty((kib * 256,), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(BR.ATTN_CASES))
def test_attention_rows_past_2g_and_4g(case, form):
    from oracle import bf16_points as R
    H, HD, N, B, _ = BR.ATTN_CASES[case]
    BR.require(BR.attn_need(H, HD, N, B, CS))
    scale = HD ** -0.5
    C = H * HD
    st = ops._stream()
    key = f"attn_bwd_hd{HD}_form"
    prev = {k: ops.set_option(k, 1) for k in (key, "attn_bwd_tail_fused")}
    label = f"bigoffset_attn/{str(LP).split('.')[-1]}/{case}/{form}"
    try:
        qkv, do = _draw(B, N, H, HD, seed=17 * B + HD)
        bufs = {}
        fwd = form.startswith("fwd")
        if fwd:
            bufs["o"] = BR.guarded((B * N, C), LP, DEV)
            bufs["lse"] = BR.guarded((B, H, N), torch.float32, DEV)
            o, lse = bufs["o"][1], bufs["lse"][1]
            flag = torch.empty((1,), dtype=torch.int32, device=DEV) if form == "fwd_optimistic" else None
            ops.call("octmae_attn_fwd", qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), ops._p(flag), B, N, H, HD, float(scale), st)
        else:
            o, lse = ops.attn_fwd(qkv, B, N, H, HD, scale)                   # the default forward's: what every backward form is handed
            bufs["dqkv"] = BR.guarded((B * N, 3 * C), LP, DEV)
            dqkv = bufs["dqkv"][1]
            if form == "bwd_pair":
                rowc = torch.empty((2, B, H, N), dtype=torch.float32, device=DEV)
                ops.call("octmae_attn_bwd_dq_rowconst", qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), rowc.data_ptr(),
                         dqkv.data_ptr(), B, N, H, HD, float(scale), st)
                ops.call("octmae_attn_bwd_dkv", qkv.data_ptr(), do.data_ptr(), rowc.data_ptr(), dqkv.data_ptr(), B, N, H, HD, float(scale), st)
            else:
                ws = _fused_ws(B, N, H, HD)
                if form == "bwd_fused_form0":
                    ops.set_option(key, 0)
                if form == "bwd_fused_tail_unfused":
                    ops.set_option("attn_bwd_tail_fused", 0)
                if form == "bwd_fused_delta":
                    # delta fp32 [B * N, H] = -rowsum over each head of dO * O, as octmae_linear_dgrad_delta's epilogue leaves it
                    delta = torch.empty((B * N, H), dtype=torch.float32, device=DEV)
                    for r0, r1 in BR.chunks(B * N):
                        delta[r0:r1] = -(do[r0:r1].double() * o[r0:r1].double()).view(r1 - r0, H, HD).sum(-1).float()
                    ops.call("octmae_attn_bwd_fused_delta", qkv.data_ptr(), do.data_ptr(), lse.data_ptr(), delta.data_ptr(), ws.data_ptr(),
                             dqkv.data_ptr(), B, N, H, HD, float(scale), st)
                else:
                    ops.call("octmae_attn_bwd_fused", qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), ws.data_ptr(),
                             dqkv.data_ptr(), B, N, H, HD, float(scale), st)
        torch.cuda.synchronize()
        for name, (buf, out) in bufs.items():
            assert BR.guards_intact(buf, out), f"{label}: a store outside {name} (guard band overwritten)"

        o_bytes, qkv_bytes = N * C * 2, N * 3 * C * 2
        meters = {n: _Meter(o_bytes) for n in ("o", "lse")} if fwd else {n: _Meter(qkv_bytes) for n in ("dq", "dk", "dv")}
        sc2 = R.scale_log2e(scale).to(DEV)
        with R.operand_type(LP):
            for b0 in range(0, B, CS):
                b1 = min(b0 + CS, B)
                n = b1 - b0
                q, k, v = _split(qkv[b0 * N:b1 * N].double(), n, N, H, HD)
                dod = _heads(do[b0 * N:b1 * N].double(), n, N, H, HD)
                ref = _reference(q, k, v, dod, scale)
                o_m, lse_m, qs = R.attention_forward(q, k, v, sc2)
                if fwd:
                    meters["o"].rows(b0, _heads(o[b0 * N:b1 * N], n, N, H, HD), o_m, ref["o"])
                    meters["lse"].lse(b0, lse[b0:b1], lse_m, ref["lse"])
                    continue
                o_k = _heads(o[b0 * N:b1 * N].double(), n, N, H, HD)
                dQf, dQp, dK, dV = R.attention_backward(q, k, v, qs, o_k, lse[b0:b1].double(), dod, scale, sc2, both_dq=form == "bwd_pair")
                gq, gk, gv = _split(dqkv[b0 * N:b1 * N], n, N, H, HD)
                meters["dq"].rows(b0, gq, R.bf(dQp if form == "bwd_pair" else dQf), ref["dq"])
                meters["dk"].rows(b0, gk, R.bf(dK), ref["dk"])
                meters["dv"].rows(b0, gv, R.bf(dV), ref["dv"])
        fails = []
        for name, m in meters.items():
            m.report(f"{label}/{name}", fails, lse=name == "lse")
        assert not fails, f"{len(fails)} row-wise checks failed:\n" + "\n".join(fails)
    finally:
        for k_, v_ in prev.items():
            ops.set_option(k_, v_)
        qkv = do = o = lse = dqkv = ws = rowc = delta = bufs = meters = ref = q = k = v = dod = o_m = lse_m = qs = o_k = None
        dQf = dQp = dK = dV = gq = gk = gv = None
        BR.release()


def test_attention_entry_points_decline_ranges_they_cannot_address():
    """-1 before any launch, outputs untouched (as check_argument_checks of tests/test_gpu_slivit_kernels.py): one sample's qkv rows (with
    the tiles the rings fetch past the end) beyond the 32-bit descriptor range, B or H beyond the grid's z / y in the forward and the
    pair, B * N beyond the int row walk of the row-constant pre-pass; in the fused backward the same per-sample range, B * H beyond the 2^32 threads
    of one launch and B * (N / 64 + 2) beyond the int block count of its row-constant pre-pass."""
    lib, st = load(), ops._stream()
    H, HD, N = 2, 32, 8
    C = H * HD
    qkv = torch.randn((N, 3 * C), device=DEV).to(LP)
    full = lambda shape, dt: torch.full(shape, BR.SENTINEL, dtype=dt, device=DEV)      # noqa: E731
    o, do, dqkv = full((N, C), LP), torch.randn((N, C), device=DEV).to(LP), full((N, 3 * C), LP)
    lse, rowc, ws = full((1, H, N), torch.float32), full((2, 1, H, N), torch.float32), full((1 << 16,), torch.float32)
    delta = torch.zeros((N, H), device=DEV)
    p = lambda t: t.data_ptr()                                                          # noqa: E731
    # (B, N, H, HD) no entry point of csrc/attn.hip may launch with
    bad = [(1, 1, 65535, 64),            # (1 + 512) rows of 3 * 65535 * 64 elements: 1.3e10 bytes from the sample's first row
           (1, 698600, 16, 64),          # the fine-tune width at a length whose rows, with the tiles fetched past them, pass 2^32 bytes
           (1, 8, 65536, 32),            # H beyond the grid's y
           (65536, 8, 2, 32)]            # B beyond the grid's z
    calls = []
    for B, n, h, hd in bad:
        calls += [lib.octmae_attn_fwd(p(qkv), p(o), p(lse), None, B, n, h, hd, 0.125, st),
                  lib.octmae_attn_bwd_dq(p(qkv), p(do), p(rowc), p(dqkv), B, n, h, hd, 0.125, st),
                  lib.octmae_attn_bwd_dq_rowconst(p(qkv), p(o), p(do), p(lse), p(rowc), p(dqkv), B, n, h, hd, 0.125, st),
                  lib.octmae_attn_bwd_dkv(p(qkv), p(do), p(rowc), p(dqkv), B, n, h, hd, 0.125, st),
                  lib.octmae_attn_bwd(p(qkv), p(o), p(do), p(lse), p(rowc), p(dqkv), B, n, h, hd, 0.125, st)]
    calls += [lib.octmae_attn_bwd_rowconst(p(o), p(do), p(lse), p(rowc), 65536, 32768, H, HD, st),                  # B * N = 2^31
              lib.octmae_attn_bwd_fused(p(qkv), p(o), p(do), p(lse), p(ws), p(dqkv), 1 << 20, 1, 4096, 32, 0.125, st),      # B * H = 2^32
              lib.octmae_attn_bwd_fused_delta(p(qkv), p(do), p(lse), p(delta), p(ws), p(dqkv), 1 << 26, 1, 64, 32, 0.125, st)]
    # the fused forms: B * H = 2^23 workgroups of 512 threads are the first launch the runtime refuses; B * (N / 64 + 2) = 2^22 * 1026
    # blocks of the row-constant pre-pass pass 2^31 - 1 with B * H = 2^22 still inside; (N + 512) rows of 6 KiB pass 2^32 bytes where
    # N rows alone do not
    for B, n, h, hd in [(1 << 17, 8, 64, 32), (1 << 22, 65536, 1, 32), (1, 698600, 16, 64)]:
        calls += [lib.octmae_attn_bwd_fused(p(qkv), p(o), p(do), p(lse), p(ws), p(dqkv), B, n, h, hd, 0.125, st),
                  lib.octmae_attn_bwd_fused_delta(p(qkv), p(do), p(lse), p(delta), p(ws), p(dqkv), B, n, h, hd, 0.125, st)]
    torch.cuda.synchronize()
    assert calls == [-1] * len(calls), calls
    for t in (o, dqkv, lse, rowc, ws):
        assert bool((t == BR.SENTINEL).all()), "a declined call wrote to an output"
    # the same buffers at their real shape are accepted
    assert lib.octmae_attn_fwd(p(qkv), p(o), p(lse), None, 1, N, H, HD, HD ** -0.5, st) == 0
    torch.cuda.synchronize()
    assert not bool((o == BR.SENTINEL).any())
