"""FP8 (e4m3fn) weights for the WAN / Flux transformer blocks.

``quantize_linears`` swaps the block projections and MLP Linears of a model
for :class:`Fp8Linear`, which holds the weight as ``float8_e4m3fn`` with one
fp32 scale per output channel (half the bytes of bf16) and runs
``ops.linear_fp8``: per-row activation quantisation + the block-scaled-MFMA
GEMM of ``ops/hip/gemm_fp8.hip`` on GPU, the same quantised math in torch on
CPU. It is opt-in (``create_diffusion_stack(..., linear_dtype="fp8")``); the
default stays bf16.

What converts: WAN ``q k v o cq ck cv co ffn1 ffn2``; Flux ``*_qkv *_proj
*_mlp.{0,2} linear1 linear2``, each only if ``in_features`` is a multiple of
128 and at most 16384 (the kernel's K contract) and ``out_features`` is at
least 128 (under half of the kernel's 256-wide N-tile a layer is mostly
padding). Embedders, modulation Linears, ``time_*``, ``txt_in`` / ``img_in``
and the output heads stay as they are: they see M = batch rows, are
quality-sensitive and are not on the hot path.

Activations are fused where that is free: WAN ``ffn1`` + SiLU, Flux
``*_mlp.0`` + GELU-tanh. Flux ``linear1`` feeds q, k, v and the MLP from one
output, so its activation stays separate.

Where a norm feeds FP8 Linears directly, the norm quantises: the blocks call
:func:`norm_rows`, which returns ``ops.Fp8Rows`` (``ops.norm_modulate_fp8``,
one kernel from activations to e4m3 rows and row scales) when every consumer
of that norm is an :class:`Fp8Linear`, and the bf16 tensor otherwise. One
``Fp8Rows`` serves all consumers: WAN ``norm1`` -> ``q k v``, ``norm2`` ->
``cq``, ``norm3`` -> ``ffn1``; Flux ``*_norm1`` -> ``*_qkv``, ``*_norm2`` ->
``*_mlp.0``, ``norm`` -> ``linear1``. ``WanModel`` quantises the text context
once for the ``ck`` / ``cv`` of all blocks. ``norm_modulate_fp8`` is defined
as the quantiser applied to the norm's bf16 output, so the model computes bit
for bit what it computes with a quantiser in front of every GEMM;
``DISTGPU_FP8_FUSED_NORM=0`` restores that routing for A/B. Linears fed by
attention or an activation (``o co ffn2 *_proj *_mlp.2 linear2``) keep their
own quantiser.
"""

from __future__ import annotations

import os
from typing import Callable, Sequence

import torch
from torch import nn

from ..ops import dispatch as ops

LINEAR_DTYPES = (None, "fp8")
MIN_OUT_FEATURES = 128

WAN_BLOCK_LINEARS = ("q", "k", "v", "o", "cq", "ck", "cv", "co", "ffn1", "ffn2")
FLUX_DOUBLE_LINEARS = tuple(
    f"{p}_{n}" for p in ("img", "txt") for n in ("qkv", "proj", "mlp.0", "mlp.2"))
FLUX_SINGLE_LINEARS = ("linear1", "linear2")

# norms hand e4m3 rows to the FP8 Linears they feed (norm_rows); off = every
# Fp8Linear quantises its own input
FP8_FUSED_NORM = os.environ.get("DISTGPU_FP8_FUSED_NORM", "1") == "1"


class Fp8Linear(nn.Module):
    """``nn.Linear`` with an e4m3 weight. Buffers: ``qweight`` [N, K]
    float8_e4m3fn, ``wscale`` [N] fp32, ``bias`` [N] fp32 or None. The bf16
    weight is not kept. ``act`` (None, "silu", "gelu_tanh") is applied after
    the bias inside the GEMM epilogue. ``forward`` takes the activation, or
    an ``ops.Fp8Rows`` holding its rows already quantised."""

    def __init__(self, linear: nn.Linear, act: str | None = None):
        super().__init__()
        if not isinstance(linear, nn.Linear):
            raise TypeError(f"expected nn.Linear, got {type(linear).__name__}")
        if not ops.fp8_shape_supported(linear.in_features):
            raise ValueError(
                f"in_features {linear.in_features} unsupported (multiple of "
                f"128, <= {ops.FP8_MAX_K})")
        if act not in (None, "silu", "gelu_tanh"):
            raise ValueError(f"act {act!r} is not None, 'silu' or 'gelu_tanh'")
        self.in_features = linear.in_features
        self.out_features = linear.out_features
        self.act = act
        qw, sw = ops.quantize_weight_fp8(linear.weight)
        self.register_buffer("qweight", qw)
        self.register_buffer("wscale", sw)
        self.register_buffer(
            "bias", None if linear.bias is None
            else linear.bias.detach().float().contiguous())

    def _apply(self, fn, recurse=True):
        # .to(device) moves the buffers; .to(dtype) / .half() / .bfloat16()
        # must not turn the e4m3 weight or the fp32 scales into something else
        def keep_dtype(t):
            out = fn(t)
            return out if out.dtype == t.dtype else t.to(out.device)

        return super()._apply(keep_dtype, recurse)

    def forward(self, x):
        return ops.linear_fp8(x, self.qweight, self.wscale, self.bias, self.act)

    def extra_repr(self):
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, "
                f"bias={self.bias is not None}, act={self.act}")


def norm_rows(norm: nn.Module, x: torch.Tensor,
              scale: torch.Tensor | None, shift: torch.Tensor | None,
              consumers: Sequence[nn.Module]):
    """``norm(x) * (1 + scale) + shift`` (both None: the plain norm) for the
    modules in ``consumers``. ``norm`` is an affine-free ``nn.LayerNorm`` or
    an RMSNorm (``weight``, ``eps``). Returns ``ops.Fp8Rows`` when
    ``FP8_FUSED_NORM`` is on and every consumer is an :class:`Fp8Linear`, so
    a layer that ``quantize_linears``' predicate vetoed keeps its call site
    on bf16; otherwise the tensor ``ops.norm_modulate`` gives."""
    if isinstance(norm, nn.LayerNorm):
        mode, weight = "layer", None
    else:
        mode, weight = "rms", norm.weight
    fn = ops.norm_modulate
    if FP8_FUSED_NORM and consumers and all(
            isinstance(m, Fp8Linear) for m in consumers):
        fn = ops.norm_modulate_fp8
    return fn(x, mode, weight, scale, shift, norm.eps)


def linear_eligible(linear: nn.Module) -> bool:
    return (isinstance(linear, nn.Linear)
            and ops.fp8_shape_supported(linear.in_features)
            and linear.out_features >= MIN_OUT_FEATURES)


def _get(block: nn.Module, path: str) -> nn.Module:
    for part in path.split("."):
        block = getattr(block, part)
    return block


def _set(block: nn.Module, path: str, new: nn.Module) -> None:
    *parents, leaf = path.split(".")
    for part in parents:
        block = getattr(block, part)
    setattr(block, leaf, new)


def _block_plan(block: nn.Module):
    """(paths, {path: fused act}) of the hot-path Linears of one block."""
    from .flux import DoubleStreamBlock, SingleStreamBlock
    from .wan import WanBlock

    if isinstance(block, WanBlock):
        return WAN_BLOCK_LINEARS, {"ffn1": "silu"}
    if isinstance(block, DoubleStreamBlock):
        return FLUX_DOUBLE_LINEARS, {"img_mlp.0": "gelu_tanh",
                                     "txt_mlp.0": "gelu_tanh"}
    if isinstance(block, SingleStreamBlock):
        return FLUX_SINGLE_LINEARS, {}
    return None


def quantize_linears(
        module: nn.Module,
        predicate: Callable[[str, nn.Linear], bool] | None = None) -> int:
    """Swap the eligible block Linears under ``module`` (a model or a single
    block) for :class:`Fp8Linear`, in place; returns how many were swapped.
    ``predicate(qualified_name, linear)`` can veto layers. Ineligible layers
    and modules without WAN / Flux blocks are left alone without error."""
    count = 0
    for bname, block in list(module.named_modules()):
        plan = _block_plan(block)
        if plan is None:
            continue
        paths, fused = plan
        for path in paths:
            lin = _get(block, path)
            qual = f"{bname}.{path}" if bname else path
            if not linear_eligible(lin):
                continue
            if predicate is not None and not predicate(qual, lin):
                continue
            act = fused.get(path)
            _set(block, path, Fp8Linear(lin, act=act))
            if act == "gelu_tanh":
                # Flux *_mlp is Sequential(Linear, GELU, Linear): the GELU
                # now runs in the GEMM epilogue
                seq, idx = path.split(".")
                getattr(block, seq)[int(idx) + 1] = nn.Identity()
            count += 1
    return count


def weight_bytes(*modules: nn.Module) -> int:
    """Bytes of every parameter and buffer (Fp8Linear keeps its weight in
    buffers, so parameters alone would miss it)."""
    total = 0
    for m in modules:
        for t in list(m.parameters()) + list(m.buffers()):
            total += t.numel() * t.element_size()
    return total


def resolve_linear_dtype(linear_dtype: str | None) -> tuple[str | None, bool]:
    """(value, explicit). ``None`` reads env ``DISTGPU_LINEAR_DTYPE``
    (unset / empty / "bf16" = the bf16 default)."""
    import os

    explicit = linear_dtype is not None
    if not explicit:
        linear_dtype = os.environ.get("DISTGPU_LINEAR_DTYPE", "") or None
    if linear_dtype in ("bf16", "default"):
        linear_dtype = None
    if linear_dtype not in LINEAR_DTYPES:
        raise ValueError(
            f"linear_dtype {linear_dtype!r} is not one of None, 'fp8'")
    return linear_dtype, explicit
