"""float64 torch restatement of the three-modality validation loss (coem.three_way_val_loss / coem.evaluate_3modalities;
train_retclip_3modalities.py:407-467) for tests/test_cpu_eval3mod.py and tests/test_gpu_eval3mod.py.

``batch_loss``   one batch: six cross entropies with reduction 'none' on the three logit matrices and their transposes; image / text1
                 weighted by w1 over sum(w1), image / text2 by w2 over sum(w2), text1 / text2 by ``text_pair_weight``: 'w1' (the
                 reference's, w1 alone over sum(w1)) or 'w1w2' (what ThreeModalityClipLoss would suggest -- kept to show the difference);
                 a zero weight sum gives 0 for its two terms; the sum over 6
``val_loss``     sum over the batches of batch_loss * batch size, over the number of samples"""
import numpy as np
import torch
import torch.nn.functional as F


def _t(x):
    return torch.from_numpy(np.array(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64))


def same_feature_targets(f, t=1e-8):
    d = torch.sqrt(((f.unsqueeze(1) - f.unsqueeze(0)) ** 2).sum(dim=-1))
    return (d <= t).to(torch.float64)


def batch_loss(image, text1, text2, scale, scale1, scale2, w1, w2, correct_label=False, text_pair_weight="w1") -> float:
    image, text1, text2, w1, w2 = (_t(x) for x in (image, text1, text2, w1, w2))
    if correct_label:
        # the duplicates are found on the features as given (float32 arithmetic in the code under test: bit copies are at distance 0
        # either way, and no other two rows of the test problems come within 1e-8)
        targets = same_feature_targets(text1)
    else:
        targets = torch.arange(image.shape[0])
    wp = {"w1": w1, "w1w2": w1 * w2}[text_pair_weight]
    total = 0.0
    for logits, w in ((float(scale) * image @ text1.T, w1), (float(scale1) * image @ text2.T, w2), (float(scale2) * text1 @ text2.T, wp)):
        for m in (logits, logits.T):
            rows = F.cross_entropy(m, targets, reduction="none")
            total += float((rows * w).sum() / w.sum()) if float(w.sum()) != 0 else 0.0
    return total / 6


def val_loss(batches, correct_label=False, text_pair_weight="w1") -> float:
    """batches: iterable of (image, text1, text2, scale, scale1, scale2, w1, w2)"""
    num, den = 0.0, 0
    for b in batches:
        n = len(b[0])
        num += batch_loss(*b, correct_label=correct_label, text_pair_weight=text_pair_weight) * n
        den += n
    return num / den
