"""Where did the model look: input gradients and Grad-CAM volumes for the fine-tuned models.

The reference ships a Grad-CAM base class over ``pytorch_grad_cam`` (retinal-COEM/src/oph_vis_util/base_cam_retclip_3mod.py, with
``compute_input_gradient=True`` for the plain gradient).  Here:

    input_gradient(model, x, target=None, *, times_input=False) -> dict(logits, target, grad, map)
    grad_cam(model, x, target=None, *, layer=-1)               -> dict(logits, target, cam)
                                                                  (return_streams=True: also activations, gradients;
                                                                   eigen_smooth=True: also residual; aug_smooth=True: cam in [0, 1])
    grad_cam_multimodal(model, inputs, target=None, *, layers=-1, single_modality=None)
                                                               -> dict(logits, target, cam = {modality: map or None})
                                                                  for the COEM classifiers; the same three switches, dicts per modality
    attention_rollout(model, x, *, head_fusion="mean", start=None, first_layer=0)
                                                               -> dict(logits, tokens, rollout): class-free, no backward pass; the
                                                                  reference has no counterpart (csrc/rollout.hip)
    heatmap(map, size)                                         -> uint8 [B, F, H, W]   ([B, H, W] for 2-D maps)

The gradient passes run the model in ``eval()`` mode under ``torch.enable_grad()`` and ``ops.weight_grads(False)``: the backward launches the
activation-gradient kernels only, so no ``p.grad``, no gradient arena and no registered reducer is touched -- a saliency pass may sit
between two accumulation micro-steps.  The score is ``sum_b logits[b, target[b]]``; ``target=None`` takes the arg-max class of every
sample (pytorch_grad_cam's ClassifierOutputTarget default), a one-column head (regression, one-logit binary) column 0.

Departures from the reference's stack: the heat volume is normalised BEFORE it is upsampled, the resize is
bilinear (``F.interpolate`` positions) and not ``cv2.resize``, and the MAE loss has no gradient through its target.  Eigen-smoothing is
a fixed number of power iterations (``ops.cam_eigen``) with a stated sign -- the projection correlates positively with the centred plain
CAM, where the reference keeps whatever sign LAPACK's SVD returns -- and a ``residual`` that tells an unconverged map.  Augmentation
smoothing runs the reference's six default passes one after the other, normalises each COARSE map, mirrors it back along W and averages
(``ops.cam_accumulate``); the flip takes the last axis of volumes too (ttach's ``flip(3)`` is H there).  Still out: several target layers
per tower averaged (``aggregate_multi_layers``), ``cv2.resize`` and the matplotlib side; for ``attention_rollout`` a ``discard_ratio``, a
gradient-weighted rollout and both COEM towers in one call.
"""
from __future__ import annotations

import torch

from . import ops
from ._autocast import no_autocast

__all__ = ["input_gradient", "grad_cam", "grad_cam_multimodal", "attention_rollout", "heatmap"]


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


def _cam_grid(model, x=None):
    """(blocks, token grid) of the classes Grad-CAM is built for."""
    from . import models_vit, models_vit_2mod, models_vit_flash_attn, models_vit_st
    if isinstance(model, models_vit_st.VisionTransformer):
        return model.blocks, tuple(int(v) for v in model.input_size)
    if type(model) in (models_vit.VisionTransformer, models_vit_flash_attn.VisionTransformer, models_vit_2mod.VisionTransformer):
        pe = model.patch_embed
        return model.blocks, (int(pe.img_size[0] // pe.patch_size[0]), int(pe.img_size[1] // pe.patch_size[1]))
    raise NotImplementedError(f"grad_cam: no token grid is known for {type(model).__module__}.{type(model).__qualname__}; built for "
                              "models_vit_st.VisionTransformer, models_vit.VisionTransformer, models_vit_flash_attn.VisionTransformer and "
                              "models_vit_2mod.VisionTransformer")


# pytorch_grad_cam's aug_smooth: tta.Compose([HorizontalFlip(), Multiply([0.9, 1, 1.1])]) -- the product of the two lists, in this order
_AUGMENTATIONS = tuple((flip, factor) for flip in (False, True) for factor in (0.9, 1.0, 1.1))
_IDENTITY = _AUGMENTATIONS.index((False, 1.0))


def _augment(x: torch.Tensor, flip: bool, factor: float) -> torch.Tensor:
    """one test-time augmentation of an input: the last (W) axis mirrored or not, then every value times ``factor``"""
    xa = x.detach().float()
    if flip:
        xa = xa.flip(-1)
    return xa if factor == 1.0 else xa * factor


def _cam_of(A, G, grid, eigen_smooth, eigen_iters, what="grad_cam"):
    """(cam float32 [B, *grid], residual or None) from the float32 streams of one hooked block"""
    L = 1
    for v in grid:
        L *= v
    n_prefix = A.shape[1] - L
    if n_prefix < 0:
        raise RuntimeError(f"{what}: the block's output has {A.shape[1]} rows, the token grid {grid} needs {L}")
    w = ops.cam_weights(G, n_prefix)
    if eigen_smooth:
        cam, residual = ops.cam_eigen(A, w, n_prefix, eigen_iters)
    else:
        cam, residual = ops.cam_tokens(A, w, n_prefix), None
    return cam.view(A.shape[0], *grid), residual


def _fold(acc, cam, flip, first):
    """one augmented pass into the mean of the six: normalised per sample, the mirrored W axis put back, weight 1/6"""
    if acc is None:
        acc = torch.empty_like(cam)
    ops.cam_accumulate(acc.view(cam.shape[0], -1), cam.reshape(cam.shape[0], -1), cam.shape[-1], flip, 1.0 / len(_AUGMENTATIONS), first)
    return acc


def _worst(a, b):
    """element-wise maximum of two residual vectors; a NaN in either stays"""
    return b if a is None else torch.maximum(a, b)


def _grad_cam_pass(model, blk, layer, x, target):
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
    return logits.detach(), tgt, A.detach().float().contiguous(), G.float().contiguous()


@no_autocast
def grad_cam(model, x, target=None, *, layer: int = -1, return_streams: bool = False, eigen_smooth: bool = False, eigen_iters: int = 32,
             aug_smooth: bool = False) -> dict:
    """Grad-CAM (Selvaraju et al. 2017, as pytorch_grad_cam's GradCAM computes it for a token stream) at the output of block ``layer``:
    A = what the block hands on (the first element of a FlashBlock's pair), G = d score / d A, cam[b, l] = max(0, sum_c mean_l'(G)[b, c]
    A[b, l, c]) over the patch tokens, as float32 [B, t, h, w] (models_vit_st) or [B, h, w] (the 2-D ViT classes).  The two reductions
    are the kernels of csrc/saliency.hip; the [B, L, C] products of the ATen form never exist.  ``return_streams`` adds A and G themselves
    (``activations``, ``gradients``: two float32 [B, n_prefix + L, C] tensors, 84 MB each for ViT-L at batch 4) to the result.

    ``eigen_smooth``: the map is the projection of the centred weighted activations on their first principal direction
    (``ops.cam_eigen``: ``eigen_iters`` power iterations, the sign that correlates positively with the plain CAM, then the ReLU) and the
    result gains ``residual`` [B], which tells an unconverged map (about (sigma2 / sigma1)^(2 eigen_iters); NaN: a non-finite stream).
    ``aug_smooth``: the reference's default test-time augmentation -- six passes, (no flip | flip of the W axis) x (0.9 | 1 | 1.1) --
    each map min-max normalised per sample ON THE COARSE GRID, un-flipped and averaged by ``ops.cam_accumulate``; ``cam`` then lies in
    [0, 1].  ``target=None`` takes the arg-max class of every pass, as the reference does; ``logits``, ``target`` and the streams are those
    of the unaugmented pass, ``residual`` the worst of the six.  ttach's hflip is ``flip(3)``, the W axis of a 4-D input only (H of a
    volume); here it is the last axis for volumes too."""
    blocks, grid = _cam_grid(model, x)
    blk = blocks[layer]
    if not aug_smooth:
        logits, tgt, A, G = _grad_cam_pass(model, blk, layer, x, target)
        cam, residual = _cam_of(A, G, grid, eigen_smooth, eigen_iters)
        res = {"logits": logits, "target": tgt, "cam": cam}
    else:
        acc = residual = res = None
        for k, (flip, factor) in enumerate(_AUGMENTATIONS):
            logits, tgt, Ak, Gk = _grad_cam_pass(model, blk, layer, _augment(x, flip, factor), target)
            cam, r = _cam_of(Ak, Gk, grid, eigen_smooth, eigen_iters)
            acc = _fold(acc, cam, flip, k == 0)
            if eigen_smooth:
                residual = _worst(residual, r)
            if k == _IDENTITY:
                res = {"logits": logits, "target": tgt}
                if return_streams:
                    A, G = Ak, Gk
            del Ak, Gk, cam                              # one pass's streams at a time
        res["cam"] = acc
    if eigen_smooth:
        res["residual"] = residual
    if return_streams:
        res.update(activations=A, gradients=G)
    return res


def _multimodal_names(model):
    from . import coem
    if isinstance(model, coem.CustomTextCLIP3ModClassification):
        return ("image", "text1", "text2")
    if isinstance(model, coem.CustomTextCLIPClassification):
        return ("image", "text")
    raise NotImplementedError(f"grad_cam_multimodal: built for coem.CustomTextCLIPClassification and "
                              f"coem.CustomTextCLIP3ModClassification, not for {type(model).__module__}.{type(model).__qualname__}")


def _multimodal_pass(model, names, present, blks, layers, inputs, target, single_modality):
    """one forward, one autograd.grad with respect to the hooked streams of both towers -> logits, target, {name: (A, G)}"""
    seen = {"visual": [], "text": []}

    def hook_into(key):
        def hook(_m, _inp, out):
            seen[key].append(out[0] if isinstance(out, (tuple, list)) else out)
        return hook

    args = [_leaf(inputs[n]) if n in present else inputs.get(n) for n in names]
    with _Quiet(model):
        hs = [blks[k].register_forward_hook(hook_into(k)) for k in ("visual", "text")]
        try:
            logits = _logits_of(model(*args, single_modality=single_modality))
        finally:
            for h in hs:
                h.remove()
        # which rows of which run of the hooked block belong to which modality
        Bn = logits.shape[0]
        where = {}
        if "image" in present:
            where["image"] = ("visual", 0, slice(None))
        texts = [n for n in names[1:] if n in present]
        if len(texts) == 2 and len(seen["text"]) == 1:      # forward_pair: one trunk pass over cat(text1, text2)
            where[texts[0]], where[texts[1]] = ("text", 0, slice(0, Bn)), ("text", 0, slice(Bn, 2 * Bn))
        else:                                              # one pass per en-face image, in the order of the names
            for i, n in enumerate(texts):
                where[n] = ("text", i, slice(None))
        want = {"visual": int("image" in present), "text": len({w[1] for w in where.values() if w[0] == "text"})}
        for k in ("visual", "text"):
            if len(seen[k]) != want[k]:
                raise RuntimeError(f"grad_cam_multimodal: block {layers[k]} of the {k} tower ran {len(seen[k])} times in one forward, "
                                   f"{want[k]} expected")
        for n, (k, i, rows) in where.items():
            if seen[k][i].shape[0] != (Bn if rows == slice(None) else 2 * Bn):
                raise RuntimeError(f"grad_cam_multimodal: the {k} tower's block ran at {seen[k][i].shape[0]} rows for a batch of {Bn}")
        score, tgt = _score(logits, target)
        flat = [a for k in ("visual", "text") for a in seen[k]]
        grads = torch.autograd.grad(score, flat)
    G = {"visual": grads[:len(seen["visual"])], "text": grads[len(seen["visual"]):]}
    streams = {n: (seen[k][i].detach()[rows].float().contiguous(), G[k][i][rows].float().contiguous()) for n, (k, i, rows) in where.items()}
    return logits.detach(), tgt, streams


@no_autocast
def grad_cam_multimodal(model, inputs, target=None, *, layers=-1, single_modality=None, eigen_smooth: bool = False, eigen_iters: int = 32,
                        aug_smooth: bool = False, return_streams: bool = False) -> dict:
    """Grad-CAM for the COEM classifiers (the reference's base_cam_retclip_3mod.py: one target layer per tower, one backward, one map per
    modality): ``coem.CustomTextCLIPClassification`` with ``inputs = {"image", "text"}`` and ``coem.CustomTextCLIP3ModClassification`` with
    ``{"image", "text1", "text2"}``.  ``layers``: the hooked block of both towers, or a pair (visual block, en-face block).  One forward,
    one ``autograd.grad`` of the class score with respect to the hooked streams of both towers, under the same conditions as ``grad_cam``
    (eval mode, no weight gradients, nothing of the model left changed).  With ``pair=True`` the en-face block runs once over
    ``cat(text1, text2)``: rows [0, B) are text1, rows [B, 2B) text2; with ``pair=False`` it runs twice, in that order.

    Returns ``logits``, ``target`` and ``cam`` = {"image": [B, t, h, w], "text1": [B, h, w], "text2": [B, h, w]} ("text" for the
    two-modality model), with None for a modality ``single_modality`` leaves out (its input may be missing).  ``eigen_smooth`` /
    ``aug_smooth`` as in ``grad_cam`` (every input is flipped along its last axis and scaled in every augmented pass); ``residual`` is then a
    dict too, and ``return_streams`` adds ``activations`` / ``gradients`` as dicts of float32 [B, n_prefix + L, C] tensors.  ``heatmap``
    turns each map into its overlay.  Not built: several target layers per tower averaged (``aggregate_multi_layers``), ``cv2.resize``
    and the matplotlib side; the ``*_gradcam`` model classes are not needed, the hooks take their place."""
    names = _multimodal_names(model)
    if single_modality is not None and single_modality not in names:
        raise ValueError(f"grad_cam_multimodal: single_modality should be one of {names} or None, got {single_modality!r}")
    present = names if single_modality is None else (single_modality,)
    missing = [n for n in present if not isinstance(inputs.get(n), torch.Tensor)]
    if missing:
        raise ValueError(f"grad_cam_multimodal: inputs lacks {missing}")
    lv, lt = (layers, layers) if isinstance(layers, int) else (int(v) for v in layers)
    (bv, gv), (bt, gt) = _cam_grid(model.visual), _cam_grid(model.text)
    blks, lay = {"visual": bv[lv], "text": bt[lt]}, {"visual": lv, "text": lt}
    grids = {n: (gv if n == "image" else gt) for n in names}
    passes = _AUGMENTATIONS if aug_smooth else ((False, 1.0),)
    identity = _IDENTITY if aug_smooth else 0
    cams, residual, res, streams = dict.fromkeys(names), dict.fromkeys(names), None, None
    for k, (flip, factor) in enumerate(passes):
        xs = {n: (_augment(inputs[n], flip, factor) if aug_smooth else inputs[n]) for n in present}
        for n in names:
            xs.setdefault(n, inputs.get(n))
        logits, tgt, st = _multimodal_pass(model, names, present, blks, lay, xs, target, single_modality)
        for n in present:
            cam, r = _cam_of(*st[n], grids[n], eigen_smooth, eigen_iters, "grad_cam_multimodal")
            cams[n] = _fold(cams[n], cam, flip, k == 0) if aug_smooth else cam
            if eigen_smooth:
                residual[n] = _worst(residual[n], r)
        if k == identity:
            res, streams = {"logits": logits, "target": tgt}, (st if return_streams else None)
        del st                                           # one pass's streams at a time
    res["cam"] = cams
    if eigen_smooth:
        res["residual"] = residual
    if return_streams:
        res["activations"] = {n: (streams[n][0] if n in present else None) for n in names}
        res["gradients"] = {n: (streams[n][1] if n in present else None) for n in names}
    return res


def _rollout_start(model, start, Bn, N, n_prefix, dev):
    """the start row w float32 [B, N]: given, or the row the model's own pooling reads"""
    if start is None:
        w = torch.zeros((Bn, N), dtype=torch.float32, device=dev)
        if getattr(model, "global_pool", False):
            w[:, n_prefix:] = 1.0 / (N - n_prefix)          # the head reads the mean of the patch tokens
        else:
            w[:, 0] = 1.0                                   # the head reads the class token
        return w
    if not isinstance(start, torch.Tensor) or tuple(start.shape) != (Bn, N):
        raise ValueError(f"attention_rollout: start must be a tensor [{Bn}, {N}] (one weight per token, prefix first)")
    w = start.detach().to(dev, torch.float32).contiguous()
    if not bool((torch.isfinite(w) & (w >= 0)).all()):
        raise ValueError("attention_rollout: start must be finite and non-negative")
    return w.clone() if w.data_ptr() == start.data_ptr() else w


@no_autocast
def attention_rollout(model, x, *, head_fusion: str = "mean", start=None, first_layer: int = 0) -> dict:
    """Attention rollout (Abnar & Zuidema 2020) for the classes ``grad_cam`` knows: how much of the start row's attention reaches
    every input token when the attention matrices of the blocks are multiplied through, the residual connection counted as an
    identity.  Per block l: P_l^h = softmax(scale q k^T) from the 16-bit q, k that the model's own attention consumed in this forward,
    F_l = ``head_fusion`` over the heads ("mean", "max", "min"), Ahat_l = (F_l + I) / rowsum, R = Ahat_L ... Ahat_{first_layer + 1};
    the map is ``start^T R``.  Only that row is computed: L vector steps of ``ops.rollout_step``, each a weighted column sum of a
    softmax that is recomputed on f32 MFMA tiles and never stored -- no [B, H, N, N] array exists, no atomics, two calls give the same
    bits.

    What it is not: it uses no class score and no gradient, so it says where attention flows, not what moved a logit (``grad_cam``
    does that, and needs a head); it ignores the MLPs, the LayerNorms and the value vectors.  That is also why it works for an encoder
    without a head -- an MAE-pre-trained trunk, a COEM tower, any checkpoint in between -- as long as ``model(x)`` runs.

    ``start=None`` follows the model's pooling: the class-token row where the head reads the class token, uniform over the patch tokens
    where ``global_pool`` averages them.  A float tensor [B, N] (prefix first) is used as given; a negative or non-finite entry raises.
    ``first_layer``: the blocks below it are left out of the product.  One forward under ``no_grad`` in eval mode inside
    ``ops.capture_attention()``; the captured ``qkv`` stay alive until the chain is done: L * B * N * 3C * 2 bytes (755 MB per ViT-L
    volume of 5121 tokens), plus one block's widened q | k (42 MB per volume) at a time.

    Returns ``logits`` (whatever ``model(x)`` returns first), ``tokens`` float32 [B, N] (sums to sum(start) per sample) and ``rollout``
    float32 [B, *grid]: the patch tokens of ``tokens``, prefix dropped, as ``heatmap`` takes a CAM."""
    blocks, grid = _cam_grid(model, x)
    if head_fusion not in ops.ROLLOUT_FUSIONS:
        raise ValueError(f"attention_rollout: head_fusion should be one of {ops.ROLLOUT_FUSIONS}, got {head_fusion!r}")
    depth = len(blocks)
    first_layer = int(first_layer)
    if not 0 <= first_layer < depth:
        raise ValueError(f"attention_rollout: first_layer must lie in [0, {depth}), got {first_layer}")
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("saliency: x must be a GPU tensor (the HIP path has no CPU fallback)")
    with _Quiet(model), torch.no_grad(), ops.capture_attention() as seen:
        logits = _logits_of(model(x.detach().float().contiguous()))
    if len(seen) != depth or len({e[1:5] for e in seen}) != 1:
        raise RuntimeError(f"attention_rollout: the forward ran {len(seen)} attention launches of shapes "
                           f"{sorted({e[1:5] for e in seen})}; one per block ({depth}) of one (B, N, H, HD) expected")
    _, Bn, N, H, HD, _ = seen[0]
    L = 1
    for v in grid:
        L *= v
    n_prefix = N - L
    if n_prefix < 0 or Bn != x.shape[0]:
        raise RuntimeError(f"attention_rollout: the blocks ran at {Bn} x {N} tokens, the token grid {grid} of {x.shape[0]} samples needs {L}")
    r = _rollout_start(model, start, Bn, N, n_prefix, x.device)
    C = H * HD
    for layer in range(depth - 1, first_layer - 1, -1):
        qkv, _, _, _, _, scale = seen[layer]
        qk = qkv.detach().view(Bn * N, 3 * C)[:, :2 * C].float()          # widening 16 bits to f32 is exact
        r = ops.rollout_step(qk[:, :C], qk[:, C:], Bn, N, H, HD, scale, r, head_fusion)
        seen[layer] = None                                               # one block's qkv less to hold
        del qkv, qk
    return {"logits": logits.detach(), "tokens": r, "rollout": r[:, n_prefix:].reshape(Bn, *grid)}


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
