"""octcubem_amd -- MI355X-native (gfx950) 3-D MAE hot path of OCTCubeM.

Only what the path needs: HIP kernels + C ABI (csrc/, liboctmae.so), and the host-side mirror of the
reference's Python interface for this path (video_vit, models_mae, misc, lr_sched, engine_pretrain).
"""
from . import _lib  # noqa: F401  (does not load the shared library until first use)
from .mixup import Mixup  # noqa: F401  (the fine-tune loop's mixup_fn; host decisions + one launch of csrc/mixup.hip)

from . import saliency  # noqa: F401  (input gradients, Grad-CAM and heat volumes; csrc/saliency.hip)
from . import lora  # noqa: F401  (low-rank adapters on the fused Block: parameter-efficient fine-tuning; csrc/lora.hip)
from .ops import set_deterministic  # noqa: F401  (deterministic mode: bit-reproducible weight gradients and gradient norm)

__all__ = ["models_mae", "video_vit", "misc", "lr_sched", "engine_pretrain", "optim", "parallel", "ops", "Mixup", "saliency",
           "lora", "set_deterministic"]
