"""Row-wise error metric for the attention tests (a helper, not a conftest; tests/test_cpu_rowwise.py proves on the CPU that it
sees what a whole-tensor L2 norm cannot).

A relative L2 norm over a whole [B, H, N, hd] tensor dilutes a fault confined to one row by sqrt(B H N): a key row whose dK is
dropped entirely moves it by 1e-2 at N = 1281, a row of o that is 10 % off by 3e-3 -- both inside the bounds of
tests/test_gpu_kernels.py.  row_err() takes the worst ROW instead; a correct 16-bit kernel stays below 1e-2 there, a one-row fault
of 10 % is at 8e-2 or more."""
import torch

NAMES = ("o", "dq", "dk", "dv")


def row_err(got: torch.Tensor, ref: torch.Tensor, with_index: bool = False):
    """max over rows of ||got_row - ref_row|| / max(||ref_row||, rms_n ||ref_row||) for tensors [B, H, N, hd]; the RMS is over the N
    rows of the same (b, h).  The floor keeps near-zero reference rows (dQ / dK rows whose dS cancels) from dominating.
    with_index: also the (b, h, n) of the worst row."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape and ref.dim() == 4, (got.shape, ref.shape)
    rn = ref.norm(dim=-1)                                               # [B, H, N]
    floor = rn.pow(2).mean(-1, keepdim=True).sqrt()
    e = (got - ref).norm(dim=-1) / torch.maximum(rn, floor).clamp_min(1e-300)
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))     # a NaN row is the worst row, not an ignored one
    worst = int(e.argmax())
    N, H = ref.shape[2], ref.shape[1]
    val = float(e.flatten()[worst])
    return (val, (worst // (H * N), (worst // N) % H, worst % N)) if with_index else val


def lse_err(got: torch.Tensor, ref: torch.Tensor, with_index: bool = False):
    """max over rows of |lse - lse_ref| / (1 + max |lse_ref|) for [B, H, N]."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape and ref.dim() == 3, (got.shape, ref.shape)
    e = (got - ref).abs() / (1.0 + float(ref.abs().max()))
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    worst = int(e.argmax())
    N, H = ref.shape[2], ref.shape[1]
    val = float(e.flatten()[worst])
    return (val, (worst // (H * N), (worst // N) % H, worst % N)) if with_index else val


def rel_l2(got, ref):
    """The whole-tensor metric of tests/test_gpu_kernels.py."""
    got = got.detach().double().flatten().cpu()
    ref = ref.detach().double().flatten().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def draw_inputs(B, H, N, HD, seed, dtype=torch.bfloat16, plain=False):
    """qkv [B*N, 3*H*HD] and do [B*N, H*HD] in `dtype`, packed as the kernels take them, with rows that are NOT exchangeable: the
    value rows carry a per-position offset that ramps from -1.5 to +1.5 along the sequence (zero mean, so o keeps its size; the size
    of dK row m follows |v_m|) and the rows of dO a per-position scale that cycles through [0.5, 2] (the size of dQ row n follows
    it).  A kernel that writes row n's result to row n +- 1 is then wrong by the size of the row, not by a statistical accident.
    plain: no offset and no scale -- the exchangeable randn rows of tests/test_gpu_kernels.py."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, 3, H, HD, generator=g)
    do = torch.randn(B, N, H, HD, generator=g)
    if plain:
        return x.reshape(B * N, 3 * H * HD).to(dtype), do.reshape(B * N, H * HD).to(dtype)
    n = torch.arange(N, dtype=torch.float32)
    x[:, :, 2] += (3.0 * (n + 0.5) / N - 1.5).view(1, N, 1, 1)
    do *= (2.0 ** (2.0 * ((n * 0.381966) % 1.0) - 1.0)).view(1, N, 1, 1)
    return x.reshape(B * N, 3 * H * HD).to(dtype), do.reshape(B * N, H * HD).to(dtype)


def split_heads(qkv, B, N, H, HD):
    """packed [B*N, 3*H*HD] -> q, k, v [B, H, N, HD] (views)."""
    return qkv.view(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)


def heads(t, B, N, H, HD):
    """[B*N, H*HD] -> [B, H, N, HD]."""
    return t.view(B, N, H, HD).transpose(1, 2)


def reference(qkv, do, B, N, H, HD):
    """float64 softmax attention and its autograd gradients on the given 16-bit operands (attn_ref of tests/test_gpu_kernels.py),
    on the device of `qkv`.  Returns o, dq, dk, dv [B, H, N, HD] and lse [B, H, N], float64, on the CPU."""
    qd = qkv.double().requires_grad_(True)
    q, k, v = split_heads(qd, B, N, H, HD)
    s = (q @ k.transpose(-2, -1)) * HD ** -0.5
    o = s.softmax(-1) @ v
    lse = torch.logsumexp(s, -1)
    o.backward(heads(do.double(), B, N, H, HD))
    dq, dk, dv = split_heads(qd.grad, B, N, H, HD)
    return {"o": o.detach().cpu(), "dq": dq.cpu(), "dk": dk.cpu(), "dv": dv.cpu(), "lse": lse.detach().cpu()}


def model(qkv, do, B, N, H, HD, dtype=torch.bfloat16, o=None, lse=None):
    """The attention part of oracle/bf16_points.py (float64 with a rounding to `dtype` where the kernels round) on the CPU.
    o [B*N, H*HD], lse [B, H, N]: the forward results a backward kernel under test was handed -- the model's backward then starts from
    them as well (same inputs on both sides); without them it starts from the model's own forward."""
    from oracle import bf16_points as R
    q, k, v = split_heads(qkv.cpu().double(), B, N, H, HD)
    fed = {} if o is None else {"o": heads(o.cpu().double(), B, N, H, HD), "lse": lse.cpu().double()}
    with R.operand_type(dtype):
        return R.attention_forward_backward(q, k, v, heads(do.cpu().double(), B, N, H, HD), HD ** -0.5, **fed)
