"""Where did the model look: input gradients and Grad-CAM volumes for the fine-tuned models.

The reference ships a Grad-CAM base class over ``pytorch_grad_cam`` (retinal-COEM/src/oph_vis_util/base_cam_retclip_3mod.py, with
``compute_input_gradient=True`` for the plain gradient).  Here:

    input_gradient(model, x, target=None, *, times_input=False) -> dict(logits, target, grad, map)
    grad_cam(model, x, target=None, *, layer=-1)               -> dict(logits, target, cam)
                                                                  (return_streams=True: also activations, gradients)
    heatmap(map, size)                                         -> uint8 [B, F, H, W]   ([B, H, W] for 2-D maps)

Both passes run the model in ``eval()`` mode under ``torch.enable_grad()`` and ``ops.weight_grads(False)``: the backward launches the
activation-gradient kernels only, so no ``p.grad``, no gradient arena and no registered reducer is touched -- a saliency pass may sit
between two accumulation micro-steps.  The score is ``sum_b logits[b, target[b]]``; ``target=None`` takes the arg-max class of every
sample (pytorch_grad_cam's ClassifierOutputTarget default), a one-column head (regression, one-logit binary) column 0.

Departures from the reference's stack: the heat volume is normalised BEFORE it is upsampled, the resize is
bilinear (``F.interpolate`` positions) and not ``cv2.resize``, Grad-CAM is the plain form (no eigen-smoothing, no test-time
augmentation smoothing), and the MAE loss has no gradient through its target.
"""
from __future__ import annotations

import torch

from . import ops
from ._autocast import no_autocast

__all__ = ["input_gradient", "grad_cam", "heatmap"]


def _logits_of(out):
    if isinstance(out, (tuple, list)):
        out = out[0]
    if not isinstance(out, torch.Tensor) or out.dim() not in (1, 2):
        raise RuntimeError("saliency: the model must return logits [B, classes] (or [B]) as its (first) output")
    return out if out.dim() == 2 else out[:, None]


def _score(logits: torch.Tensor, target):
    Bn, K = logits.shape
    if K == 1:
        tgt = torch.zeros(Bn, dtype=torch.int64, device=logits.device)
    elif target is None:
        tgt = logits.detach().argmax(dim=1)
    else:
        tgt = torch.as_tensor(target, device=logits.device).to(torch.int64).reshape(-1)
        if tgt.numel() == 1:
            tgt = tgt.expand(Bn)
        if tgt.shape != (Bn,):
            raise ValueError(f"saliency: target must hold one class per sample ({Bn}), got {tuple(tgt.shape)}")
        if bool(((tgt < 0) | (tgt >= K)).any()):
            raise ValueError(f"saliency: target must lie in [0, {K})")
    return logits.gather(1, tgt[:, None]).sum(), tgt


class _Quiet:
    """eval() for the call, every module's own training flag and every ``p.grad`` OBJECT restored afterwards (a forward under
    enable_grad re-attaches a ``p.grad`` that is None to the gradient arena; a saliency pass must not leave that behind)."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.modes = [(m, m.training) for m in self.model.modules()]
        self.grads = [(p, p.grad) for p in self.model.parameters()]
        self.model.eval()
        self.ctx = (torch.enable_grad(), ops.weight_grads(False))
        for c in self.ctx:
            c.__enter__()
        return self

    def __exit__(self, *exc):
        for c in reversed(self.ctx):
            c.__exit__(*exc)
        for m, flag in self.modes:
            m.training = flag
        for p, g in self.grads:
            if p.grad is not g:
                p.grad = g
        return False


def _leaf(x: torch.Tensor) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("saliency: x must be a GPU tensor (the HIP path has no CPU fallback)")
    # a detached copy: the caller's tensor gets no .grad, and a model whose parameters are all frozen still builds a graph
    return x.detach().float().contiguous().clone().requires_grad_(True)


@no_autocast
def input_gradient(model, x, target=None, *, times_input: bool = False) -> dict:
    """The gradient of the class score with respect to the input, for every model whose images enter through the patch-embedding
    kernels (models_vit_st, models_vit, models_vit_flash_attn, the 3-D-head models, the COEM towers).  ``grad`` has the shape of ``x``;
    ``map`` = max over the channel axis of |grad| (``times_input``: of |grad * x|), [B, T, H, W] for 5-D and [B, H, W] for 4-D input."""
    xi = _leaf(x)
    with _Quiet(model):
        logits = _logits_of(model(xi))
        score, tgt = _score(logits, target)
        (grad,) = torch.autograd.grad(score, xi)
    g = grad * xi.detach() if times_input else grad
    return {"logits": logits.detach(), "target": tgt, "grad": grad.view(x.shape), "map": g.abs().amax(dim=1)}


def _cam_grid(model, x):
    """(blocks, token grid) of the classes Grad-CAM is built for."""
    from . import models_vit, models_vit_flash_attn, models_vit_st
    if isinstance(model, models_vit_st.VisionTransformer):
        return model.blocks, tuple(int(v) for v in model.input_size)
    if type(model) in (models_vit.VisionTransformer, models_vit_flash_attn.VisionTransformer):
        pe = model.patch_embed
        return model.blocks, (int(pe.img_size[0] // pe.patch_size[0]), int(pe.img_size[1] // pe.patch_size[1]))
    raise NotImplementedError(f"grad_cam: no token grid is known for {type(model).__module__}.{type(model).__qualname__}; built for "
                              "models_vit_st.VisionTransformer, models_vit.VisionTransformer and models_vit_flash_attn.VisionTransformer")


@no_autocast
def grad_cam(model, x, target=None, *, layer: int = -1, return_streams: bool = False) -> dict:
    """Grad-CAM (Selvaraju et al. 2017, as pytorch_grad_cam's GradCAM computes it for a token stream) at the output of block ``layer``:
    A = what the block hands on (the first element of a FlashBlock's pair), G = d score / d A, cam[b, l] = max(0, sum_c mean_l'(G)[b, c]
    A[b, l, c]) over the patch tokens, as float32 [B, t, h, w] (models_vit_st) or [B, h, w] (the 2-D ViT classes).  The two reductions
    are the kernels of csrc/saliency.hip; the [B, L, C] products of the ATen form never exist.  ``return_streams`` adds A and G themselves
    (``activations``, ``gradients``: two float32 [B, n_prefix + L, C] tensors, 84 MB each for ViT-L at batch 4) to the result."""
    blocks, grid = _cam_grid(model, x)
    blk = blocks[layer]
    seen = []

    def hook(_m, _inp, out):
        seen.append(out[0] if isinstance(out, (tuple, list)) else out)

    xi = _leaf(x)
    with _Quiet(model):
        h = blk.register_forward_hook(hook)
        try:
            logits = _logits_of(model(xi))
        finally:
            h.remove()
        if len(seen) != 1:
            raise RuntimeError(f"grad_cam: block {layer} ran {len(seen)} times in one forward")
        A = seen[0]
        score, tgt = _score(logits, target)
        (G,) = torch.autograd.grad(score, A)
    A = A.detach().float().contiguous()
    G = G.float().contiguous()
    L = 1
    for v in grid:
        L *= v
    n_prefix = A.shape[1] - L
    if n_prefix < 0:
        raise RuntimeError(f"grad_cam: the block's output has {A.shape[1]} rows, the token grid {grid} needs {L}")
    cam = ops.cam_tokens(A, ops.cam_weights(G, n_prefix), n_prefix)
    res = {"logits": logits.detach(), "target": tgt, "cam": cam.view(A.shape[0], *grid)}
    if return_streams:
        res.update(activations=A, gradients=G)
    return res


@no_autocast
def heatmap(map: torch.Tensor, size) -> torch.Tensor:
    """uint8 heat volume of a saliency map: [B, t, h, w] -> [B, F, H, W] with ``size`` = (F, H, W), or [B, h, w] -> [B, H, W] with
    ``size`` = (H, W); W % 4 == 0.  Per sample min-max normalisation ON THE COARSE MAP, then linear (t) x bilinear (h, w) resampling at
    ``F.interpolate``'s align_corners=False positions, then floor(255 v) (``ops.heatmap``)."""
    m = map.detach().float().contiguous()
    if m.dim() == 3:
        if len(size) != 2:
            raise ValueError("heatmap: a [B, h, w] map takes size = (H, W)")
        return ops.heatmap(m[:, None], (1, int(size[0]), int(size[1])))[:, 0]
    if m.dim() != 4 or len(size) != 3:
        raise ValueError("heatmap: expected a [B, t, h, w] map with size = (F, H, W), or a [B, h, w] map with size = (H, W)")
    return ops.heatmap(m, size)
