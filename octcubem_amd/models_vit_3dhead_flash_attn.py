"""Module-name alias for the reference's ``OCTCube/models_vit_3dhead_flash_attn.py``: its fine-tune drivers select the model with
``models_vit_3dhead_flash_attn.__dict__[args.model]`` (patient_dataset_type ``3D_flash_attn``).  The model lives in models_vit_3dhead."""
from .models_vit_3dhead import (VisionTransformerWith3DPoolingHead, flash_attn_vit_large_patch16_3DSliceHead,  # noqa: F401
                                vit_large_patch16_3DSliceHead)
