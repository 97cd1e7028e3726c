"""Torch restatements of the kernels of csrc/saliency.hip (a helper, not a conftest): the patch gather and its adjoint, Grad-CAM's two
reductions in float64 with the any-order summation bound, and the heat volume in float64 and in float32.  tests/test_cpu_saliency.py
checks the restatements against themselves and against F.interpolate; tests/test_gpu_saliency.py holds the kernels to them."""
import torch
import torch.nn.functional as F

F64 = torch.float64
U32 = 2.0 ** -24          # unit roundoff of fp32


# ---- patch gather / scatter ---------------------------------------------------------------------------------------------------------
def _token_index(ids, B, C, T, H, W, tp, p, nkeep):
    """flat voxel index [B, nkeep, C*tp*p*p] of every element of every kept token's patch, in conv-weight order (c, u, py, px)"""
    gh, gw = H // p, W // p
    if ids is None:
        ids = torch.arange(nkeep).expand(B, nkeep)
    ids = ids.to(torch.int64).cpu()
    t, hy, wx = ids // (gh * gw), (ids // gw) % gh, ids % gw                                  # [B, nkeep]
    c = torch.arange(C).view(C, 1, 1, 1)
    u = torch.arange(tp).view(1, tp, 1, 1)
    py = torch.arange(p).view(1, 1, p, 1)
    px = torch.arange(p).view(1, 1, 1, p)
    fr = t.view(B, nkeep, 1, 1, 1, 1) * tp + u
    y = hy.view(B, nkeep, 1, 1, 1, 1) * p + py
    x = wx.view(B, nkeep, 1, 1, 1, 1) * p + px
    b = torch.arange(B).view(B, 1, 1, 1, 1, 1)
    idx = (((b * C + c) * T + fr) * H + y) * W + x
    return idx.reshape(B, nkeep, C * tp * p * p)


def gather_ref(x, ids, tp, p, nkeep):
    """octmae_patch_gather without the rounding: [B*nkeep, C*tp*p*p] in the dtype of x"""
    B, C, T, H, W = x.shape
    idx = _token_index(ids, B, C, T, H, W, tp, p, nkeep)
    return x.detach().cpu().reshape(-1)[idx.reshape(-1)].reshape(B * nkeep, -1)


def scatter_ref(dpatch, ids, shape, tp, p):
    """octmae_patch_scatter: the dtype of dpatch widened is the caller's business; +0.0 wherever no kept token lies.  ids distinct."""
    B, C, T, H, W = shape
    nkeep = dpatch.shape[0] // B
    idx = _token_index(ids, B, C, T, H, W, tp, p, nkeep)
    out = torch.zeros(B * C * T * H * W, dtype=dpatch.dtype)
    out[idx.reshape(-1)] = dpatch.detach().cpu().reshape(-1)
    return out.view(B, C, T, H, W)


# ---- Grad-CAM -----------------------------------------------------------------------------------------------------------------------
def gamma(n):
    return n * U32 / (1.0 - n * U32)


def cam_ref64(A, G, n_prefix):
    """(w, w_bound, cam, cam_bound) in float64 for float32 A, G [B, n_prefix + L, C].

    The kernels compute, in fp32 and in an unspecified order,  w^ = fl(sum_l G_lc) / L  and  cam^ = max(0, fl(sum_c w^_c A_lc)).
      * a sum of L numbers in any order is within gamma_{L-1} sum|G| of the exact sum, the division adds one rounding:
            |w^_c - w_c| <= gamma_{L+1} Wabs_c,   Wabs_c = (1/L) sum_l |G_lc|     (Wabs, not |w|: the sum may cancel)
        and |w^_c| <= (1 + gamma_{L+1}) Wabs_c;
      * a dot product of C terms in any order, fused or not, is within gamma_C sum_c |w^_c| |A_lc| of the exact dot of w^ with A;
      * the exact dot of w^ with A differs from the one of w by at most sum_c |w^_c - w_c| |A_lc|;
      * max(0, .) is 1-Lipschitz.
    Together  |cam^ - cam| <= (gamma_C (1 + gamma_{L+1}) + gamma_{L+1}) sum_c Wabs_c |A_lc|   (<= gamma_{C+L+2} ... for these sizes),
    plus 1e-40 so that an all-zero row has a positive bound (fp32 underflow of a product is below that for the test inputs)."""
    A, G = A.detach().cpu().to(F64), G.detach().cpu().to(F64)
    L, C = A.shape[1] - n_prefix, A.shape[2]
    Ap, Gp = A[:, n_prefix:], G[:, n_prefix:]
    w = Gp.sum(1) / L
    wabs = Gp.abs().sum(1) / L
    w_bound = gamma(L + 1) * wabs + 1e-40
    cam = torch.einsum("bc,blc->bl", w, Ap).clamp_min(0.0)
    cam_bound = (gamma(C) * (1.0 + gamma(L + 1)) + gamma(L + 1)) * torch.einsum("bc,blc->bl", wabs, Ap.abs()) + 1e-40
    return w, w_bound, cam, cam_bound


# ---- heat volume --------------------------------------------------------------------------------------------------------------------
def _lin_matrix(n_in, n_out, dtype=F64):
    """[n_out, n_in] weights of F.interpolate's linear resampling with align_corners=False: src = (dst + 0.5) in / out - 0.5, a negative
    src becomes 0, the upper neighbour is clamped.  n_in == n_out is the identity."""
    dst = torch.arange(n_out, dtype=dtype)
    src = ((dst + 0.5) * n_in / n_out - 0.5).clamp_min(0.0)
    i0 = src.floor().to(torch.int64).clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    l1 = src - i0.to(dtype)
    M = torch.zeros(n_out, n_in, dtype=dtype)
    M.scatter_add_(1, i0[:, None], (1.0 - l1)[:, None])
    M.scatter_add_(1, i1[:, None], l1[:, None])
    return M


def heat_value64(m, size):
    """float64 [B, F, H, W]: 255 v before the floor, v the normalised coarse map resampled separably (t, then h and w)."""
    m32 = m.detach().cpu().float()
    B, t, h, w = m32.shape
    Fo, Ho, Wo = size
    mn = m32.reshape(B, -1).min(1).values.to(F64).view(B, 1, 1, 1)
    mx = m32.reshape(B, -1).max(1).values.to(F64).view(B, 1, 1, 1)
    eps = float(torch.tensor(1e-7, dtype=torch.float32))
    v = (m32.to(F64) - mn) / (eps + (mx - mn))
    v = torch.einsum("ft,btyx->bfyx", _lin_matrix(t, Fo), v)
    v = torch.einsum("Yy,bfyx->bfYx", _lin_matrix(h, Ho), v)
    v = torch.einsum("Xx,bfyx->bfyX", _lin_matrix(w, Wo), v)
    return 255.0 * v


def heat_ref64(m, size):
    return heat_value64(m, size).floor().clamp(0, 255).to(torch.uint8)


def heat_interpolate(m, size, dtype):
    """The same map through F.interpolate in `dtype`: normalise, `linear` along t, `bilinear` over (h, w); 255 v before the floor."""
    m = m.detach().cpu().float()
    B, t, h, w = m.shape
    Fo, Ho, Wo = size
    mn = m.reshape(B, -1).min(1).values.view(B, 1, 1, 1)
    mx = m.reshape(B, -1).max(1).values.view(B, 1, 1, 1)
    if dtype == torch.float32:
        v = (m - mn) / (torch.tensor(1e-7, dtype=torch.float32) + (mx - mn))
    else:
        v = (m.to(dtype) - mn.to(dtype)) / (float(torch.tensor(1e-7, dtype=torch.float32)) + (mx.to(dtype) - mn.to(dtype)))
    if Fo != t:
        v = F.interpolate(v.permute(0, 2, 3, 1).reshape(B, h * w, t), size=Fo, mode="linear", align_corners=False)
        v = v.reshape(B, h, w, Fo).permute(0, 3, 1, 2)
    if (Ho, Wo) != (h, w):
        v = F.interpolate(v.contiguous(), size=(Ho, Wo), mode="bilinear", align_corners=False)
    return 255.0 * v


def heat_ref32(m, size):
    return heat_interpolate(m, size, torch.float32).floor().clamp(0, 255).to(torch.uint8)


HEAT_CASES = {      # name: (B, (t, h, w), (F, H, W), where the largest voxel of every sample is put)
    "identity": (1, (3, 8, 12), (3, 8, 12), None),
    "up_t2_hw": (1, (2, 2, 3), (6, 32, 48), (0, 0, 1)),
    "flat_2d": (2, (1, 4, 4), (1, 32, 32), (0, 1, 1)),
    "even_t": (1, (3, 4, 4), (12, 16, 16), (1, 1, 1)),
    "ranges": (2, (2, 3, 4), (4, 12, 16), (0, 1, 1)),
}


def heat_input(name):
    """The largest voxel maps to 255 (1 - 1e-7 / range): a hair below 255 in float64, exactly 255 once v is rounded to fp32 -- which is
    why the maximum of a heat volume is "254 or 255".  An upsampled border voxel is repeated over a whole plateau of output voxels
    (negative source positions become 0), so a maximum on the border would put that one undecidable value on 1-2 % of the bytes.  The
    maximum of every sample is therefore moved (swapped) to a voxel that is interior along one upsampled axis, where no output
    position coincides with it; every other voxel keeps the generic "a byte differs only across a floor" behaviour."""
    B, coarse, size, peak = HEAT_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    m = torch.randn(B, *coarse, generator=g)
    if peak is not None:
        for b in range(B):
            flat = m[b].reshape(-1)
            i, j = int(flat.argmax()), (peak[0] * coarse[1] + peak[1]) * coarse[2] + peak[2]
            vi, vj = float(flat[i]), float(flat[j])
            flat[i], flat[j] = vj, vi
    if name == "ranges":        # very different ranges per sample: normalisation must be per sample
        m[0] = m[0] * 1e-3 + 5.0
        m[1] = m[1] * 1e3 - 40.0
    return m.float().contiguous(), size
