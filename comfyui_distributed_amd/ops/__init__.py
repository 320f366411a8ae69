from .dispatch import (
    attention,
    attention_packed,
    act_mul,
    blend_tile,
    extract_resize,
    gated_residual,
    group_norm_silu,
    layer_norm,
    hip_available,
    norm_modulate,
    qk_norm_rope,
    rms_norm,
)

__all__ = [
    "attention",
    "act_mul",
    "blend_tile",
    "extract_resize",
    "gated_residual",
    "group_norm_silu",
    "layer_norm",
    "hip_available",
    "norm_modulate",
    "qk_norm_rope",
    "rms_norm",
]
