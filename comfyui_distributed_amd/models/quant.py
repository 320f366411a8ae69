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

``DISTGPU_FP8_MX=1`` takes the quantiser out of the feed-forward pairs (WAN
``ffn1 -> ffn2``, Flux ``*_mlp.0 -> *_mlp.2``) where both members convert:
the first Linear gets ``emit="mx"`` and hands the second its activation as
``ops.MxRows`` (MXFP8: e4m3 codes with one power-of-two scale per 32
elements, made in the GEMM epilogue and applied by the second GEMM's matrix
instruction), so ``ffn2`` / ``*_mlp.2`` run no quantiser launch. The MX GEMM
has no per-row scale, so an emitting Linear does not take the norm's
``Fp8Rows``: ``norm3`` / ``*_norm2`` give it bf16 and it quantises its
narrower input itself (``ops.quantize_rows_mx``). Off by default; ``o co
*_proj linear2`` keep their quantiser either way.

For the widths of the SD1.5 / SDXL UNet transformer blocks the same modules
take ``pad_k``: ``in_features`` that are a multiple of 64 but not of 128 (320,
960) run on rows and weights padded to the next multiple of 128, and
:class:`Fp8GegluLinear` is the GEGLU ``proj_in`` with the gate in the GEMM
epilogue. The affine LayerNorm hands such a module e4m3 rows through
``ops.layer_norm_fp8``. Converting a UNet with them is not wired up yet.

``quantize_unet_convs`` is the conv counterpart for the UNet families
(``create_diffusion_stack(..., conv_dtype="fp8")``, opt-in): it leaves the
modules in place and attaches an e4m3 copy of each 3x3 conv's weight, and
``ops.conv2d_mfma`` then runs ``ops.quant_nhwc_fp8`` (one activation scale per
image) and ``ops.conv_fp8`` for those modules.
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
# quantize_linears routes the feed-forward pairs through MXFP8 rows
FP8_MX = os.environ.get("DISTGPU_FP8_MX", "0") == "1"


class Fp8Linear(nn.Module):
    """``nn.Linear`` with an e4m3 weight. Buffers: ``qweight`` [N, K]
    float8_e4m3fn, ``wscale`` [N] fp32, ``bias`` [N] fp32 or None. The bf16
    weight is not kept. ``act`` (None, "silu", "gelu_tanh") is applied after
    the bias inside the GEMM epilogue. ``forward`` takes the activation, or
    an ``ops.Fp8Rows`` / ``ops.MxRows`` holding its rows already quantised.
    ``emit="mx"``: ``forward`` returns ``ops.MxRows`` for another Fp8Linear
    (``out_features`` % 32 == 0) and takes a tensor or ``MxRows`` only.

    ``pad_k=True`` also takes ``in_features`` that are a multiple of 64 only:
    ``qweight`` is then [N, Kp], Kp = K rounded up to 128, with zero columns
    behind K, and the activation rows are quantised at the same pitch
    (``ops.quantize_rows(x, pad_k=True)``), so the GEMM runs unchanged over
    Kp."""

    def __init__(self, linear: nn.Linear, act: str | None = None,
                 pad_k: bool = False, emit: str | None = None):
        super().__init__()
        if not isinstance(linear, nn.Linear):
            raise TypeError(f"expected nn.Linear, got {type(linear).__name__}")
        if pad_k and not ops.fp8_pad_shape_supported(linear.in_features):
            raise ValueError(
                f"in_features {linear.in_features} unsupported (multiple of "
                f"64, <= {ops.FP8_MAX_K})")
        if not pad_k and not ops.fp8_shape_supported(linear.in_features):
            raise ValueError(
                f"in_features {linear.in_features} unsupported (multiple of "
                f"128, <= {ops.FP8_MAX_K})")
        if act not in (None, "silu", "gelu_tanh"):
            raise ValueError(f"act {act!r} is not None, 'silu' or 'gelu_tanh'")
        self.in_features = linear.in_features
        self.out_features = linear.out_features
        self.act = act
        self.pad_k = pad_k and linear.in_features % 128 != 0
        self.set_emit(emit)
        qw, sw, bias = self._quantize(linear)
        self.register_buffer("qweight", qw)
        self.register_buffer("wscale", sw)
        self.register_buffer("bias", bias)

    def set_emit(self, emit: str | None) -> None:
        if emit not in (None, "mx"):
            raise ValueError(f"emit {emit!r} is not None or 'mx'")
        if emit == "mx" and (self.pad_k or self.out_features % 32):
            raise ValueError(
                "emit='mx' needs in_features % 128 == 0 and out_features % 32 "
                f"== 0, got {self.in_features} -> {self.out_features}")
        self.emit = emit

    def _quantize(self, linear):
        """(qweight, wscale, bias or None) of the Linear."""
        qw, sw = ops.quantize_weight_fp8(linear.weight, self.pad_k)
        return qw, sw, (None if linear.bias is None
                        else linear.bias.detach().float().contiguous())

    def _apply(self, fn, recurse=True):
        # .to(device) moves the buffers; .to(dtype) / .half() / .bfloat16()
        # must not turn the e4m3 weight or the fp32 scales into something else
        def keep_dtype(t):
            out = fn(t)
            return out if out.dtype == t.dtype else t.to(out.device)

        return super()._apply(keep_dtype, recurse)

    def forward(self, x):
        if self.pad_k and not isinstance(x, ops.Fp8Rows):
            x = ops.quantize_rows(x, pad_k=True)
        return ops.linear_fp8(x, self.qweight, self.wscale, self.bias, self.act,
                              emit=self.emit)

    def extra_repr(self):
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, "
                f"bias={self.bias is not None}, act={self.act}"
                + (f", emit={self.emit}" if self.emit else ""))


class Fp8GegluLinear(Fp8Linear):
    """The GEGLU projection ``a, gate = linear(x).chunk(2, -1); a *
    gelu_tanh(gate)`` with an e4m3 weight, one ``ops.linear_geglu_fp8`` call:
    x [..., K] (or its ``ops.Fp8Rows``) -> [..., inner]. ``qweight``
    [2*inner, Kp], ``wscale`` and ``bias`` [2*inner] hold value and gate rows
    in ``ops.pack_geglu_weight``'s pairing; inner % 16 == 0."""

    def __init__(self, linear: nn.Linear, pad_k: bool = False):
        if linear.out_features % 32:
            raise ValueError(
                f"out_features {linear.out_features} is not 2 * inner with "
                "inner % 16 == 0")
        super().__init__(linear, pad_k=pad_k)
        self.out_features = linear.out_features // 2

    def _quantize(self, linear):
        qw, sw, bias = ops.pack_geglu_weight_fp8(
            linear.weight, linear.bias, self.pad_k)
        return qw, sw, (bias if linear.bias is not None else None)

    def forward(self, x):
        return ops.linear_geglu_fp8(x, self.qweight, self.wscale, self.bias)


def norm_rows(norm: nn.Module, x: torch.Tensor,
              scale: torch.Tensor | None, shift: torch.Tensor | None,
              consumers: Sequence[nn.Module]):
    """``norm(x) * (1 + scale) + shift`` (both None: the plain norm) for the
    modules in ``consumers``. ``norm`` is an affine-free ``nn.LayerNorm`` or
    an RMSNorm (``weight``, ``eps``). Returns ``ops.Fp8Rows`` when
    ``FP8_FUSED_NORM`` is on and every consumer is an :class:`Fp8Linear`, so
    a layer that ``quantize_linears``' predicate vetoed keeps its call site
    on bf16; otherwise the tensor ``ops.norm_modulate`` gives. A consumer
    that emits MX rows takes no per-row scale and gets the tensor too."""
    if isinstance(norm, nn.LayerNorm):
        mode, weight = "layer", None
    else:
        mode, weight = "rms", norm.weight
    fn = ops.norm_modulate
    if FP8_FUSED_NORM and consumers and all(
            isinstance(m, Fp8Linear) and m.emit is None for m in consumers):
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
    """(paths, {path: fused act}, feed-forward (producer, consumer) pairs) of
    the hot-path Linears of one block."""
    from .flux import DoubleStreamBlock, SingleStreamBlock
    from .wan import WanBlock

    if isinstance(block, WanBlock):
        return WAN_BLOCK_LINEARS, {"ffn1": "silu"}, (("ffn1", "ffn2"),)
    if isinstance(block, DoubleStreamBlock):
        return FLUX_DOUBLE_LINEARS, {"img_mlp.0": "gelu_tanh",
                                     "txt_mlp.0": "gelu_tanh"}, (
            ("img_mlp.0", "img_mlp.2"), ("txt_mlp.0", "txt_mlp.2"))
    if isinstance(block, SingleStreamBlock):
        return FLUX_SINGLE_LINEARS, {}, ()
    return None


def quantize_linears(
        module: nn.Module,
        predicate: Callable[[str, nn.Linear], bool] | None = None) -> int:
    """Swap the eligible block Linears under ``module`` (a model or a single
    block) for :class:`Fp8Linear`, in place; returns how many were swapped.
    ``predicate(qualified_name, linear)`` can veto layers. Ineligible layers
    and modules without WAN / Flux blocks are left alone without error. With
    ``FP8_MX`` the first Linear of each feed-forward pair emits ``ops.MxRows``
    for the second, if both converted."""
    count = 0
    for bname, block in list(module.named_modules()):
        plan = _block_plan(block)
        if plan is None:
            continue
        paths, fused, pairs = plan
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
        for first, second in pairs if FP8_MX else ():
            a, b = _get(block, first), _get(block, second)
            if (type(a) is Fp8Linear and type(b) is Fp8Linear
                    and not b.pad_k and a.out_features % 32 == 0):
                a.set_emit("mx")
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


# ---------------------------------------------------------------------------
# FP8 convs (ops.conv_fp8) for the 3x3 convs of the UNet
# ---------------------------------------------------------------------------

CONV_DTYPES = (None, "fp8")


def conv_eligible(conv: nn.Module, include_1x1: bool = False) -> bool:
    """An ``MfmaConv2d`` the FP8 conv kernel covers: 3x3 pad 1 (stride 1 or
    2) with ``in_channels`` a multiple of 64; the 1x1 skips only on request,
    because their quantiser pass costs more than K = C saves."""
    from .unet import MfmaConv2d

    if not (isinstance(conv, MfmaConv2d) and ops.conv_supported(conv)
            and conv.in_channels % 64 == 0):
        return False
    return conv.kernel_size == (3, 3) or include_1x1


def quantize_unet_convs(model: nn.Module, include_1x1: bool = False) -> int:
    """Mark the eligible convs under ``model`` for the FP8 route: each gets
    ``ops.quantize_conv_weight_fp8``'s cached e4m3 pack beside its bf16
    weight, which is what ``ops.conv2d_mfma`` looks for. The weight stays, so
    shapes outside the kernel's cover (small batches, the upsample convs) and
    measured losses keep running on bf16. Returns how many were marked."""
    count = 0
    for m in model.modules():
        if conv_eligible(m, include_1x1):
            ops.quantize_conv_weight_fp8(m)
            count += 1
    return count


def resolve_conv_dtype(conv_dtype: str | None) -> tuple[str | None, bool]:
    """(value, explicit). ``None`` reads env ``DISTGPU_CONV_DTYPE`` (unset /
    empty / "bf16" = the bf16 default)."""
    explicit = conv_dtype is not None
    if not explicit:
        conv_dtype = os.environ.get("DISTGPU_CONV_DTYPE", "") or None
    if conv_dtype in ("bf16", "default"):
        conv_dtype = None
    if conv_dtype not in CONV_DTYPES:
        raise ValueError(
            f"conv_dtype {conv_dtype!r} is not one of None, 'fp8'")
    return conv_dtype, explicit


# ---------------------------------------------------------------------------
# FP8 attention (ops.attention_fp8) for the self-attention of the blocks
# ---------------------------------------------------------------------------

ATTN_DTYPES = (None, "fp8")


def resolve_attn_dtype(attn_dtype: str | None) -> tuple[str | None, bool]:
    """(value, explicit). ``None`` reads env ``DISTGPU_ATTN_DTYPE`` (unset /
    empty / "bf16" = the bf16 default)."""
    explicit = attn_dtype is not None
    if not explicit:
        attn_dtype = os.environ.get("DISTGPU_ATTN_DTYPE", "") or None
    if attn_dtype in ("bf16", "default"):
        attn_dtype = None
    if attn_dtype not in ATTN_DTYPES:
        raise ValueError(
            f"attn_dtype {attn_dtype!r} is not one of None, 'fp8'")
    return attn_dtype, explicit


def set_attn_dtype(module: nn.Module, attn_dtype: str | None,
                   strict: bool = True) -> int:
    """Route the self-attention of every WAN / Flux block under ``module``
    through ``ops.attention_fp8`` ("fp8") or back to ``ops.attention_packed``
    (None); returns the number of blocks now on ``attn_dtype``. Cross-attention
    is not touched. The kernel is built for head dim 128: a block with any
    other is an error here, not at the first forward, or, with
    ``strict=False`` (a value that came from the environment), stays on
    bf16. Going back to bf16 also removes a window set by
    ``set_attn_window``, which only the FP8 kernel can run."""
    if attn_dtype not in ATTN_DTYPES:
        raise ValueError(
            f"attn_dtype {attn_dtype!r} is not one of None, 'fp8'")
    count = 0
    for blk in module.modules():
        if _block_plan(blk) is None:
            continue
        if attn_dtype == "fp8" and blk.head_dim != ops.ATTN_FP8_D:
            if strict:
                raise ValueError(
                    f"attn_dtype='fp8' needs head dim {ops.ATTN_FP8_D}, "
                    f"{type(blk).__name__} has {blk.head_dim}")
            continue
        blk.attn_dtype = attn_dtype
        count += 1
    if attn_dtype != "fp8":
        # a sliding-tile window (set_attn_window) needs the FP8 kernel
        for m in module.modules():
            if getattr(m, "attn_window", None) is not None:
                m.attn_window = None
    return count


def self_attention(block: nn.Module, q: torch.Tensor, k: torch.Tensor,
                   v: torch.Tensor, blocks=None) -> torch.Tensor:
    """The block's self-attention on packed [B, N, H*D] q, k, v:
    ``ops.attention_packed``, or ``ops.attention_fp8`` after
    ``set_attn_dtype(..., "fp8")``. ``blocks`` (an ``ops.AttnBlocks``) needs
    the latter."""
    if getattr(block, "attn_dtype", None) == "fp8":
        return ops.attention_fp8(q, k, v, heads=block.heads, blocks=blocks)
    if blocks is not None:
        raise ValueError("block-sparse self-attention needs attn_dtype='fp8'")
    return ops.attention_packed(q, k, v, heads=block.heads)


# ---------------------------------------------------------------------------
# sliding-tile window (ops.attn_window) for the WAN self-attention
# ---------------------------------------------------------------------------


def _check_attn_window(window):
    """(tile, radius), each three ints, or None."""
    if window is None:
        return None
    try:
        tile, radius = (tuple(int(x) for x in t) for t in window)
    except (TypeError, ValueError):
        tile = radius = ()
    if len(tile) != 3 or len(radius) != 3 or min(tile) < 1 or min(radius) < 0:
        raise ValueError(
            f"attn_window {window!r} is not ((tt, th, tw), (rt, rh, rw)) "
            f"with tile sizes >= 1 and radii >= 0")
    return tile, radius


def resolve_attn_window(window):
    """(value, explicit). ``None`` reads env ``DISTGPU_ATTN_WINDOW``
    ("tt,th,tw:rt,rh,rw"; unset / empty = no window)."""
    explicit = window is not None
    if not explicit:
        text = os.environ.get("DISTGPU_ATTN_WINDOW", "")
        if text:
            window = tuple(tuple(p.split(",")) for p in text.split(":"))
            if len(window) != 2:
                raise ValueError(
                    f"DISTGPU_ATTN_WINDOW {text!r} is not 'tt,th,tw:rt,rh,rw'")
    return _check_attn_window(window), explicit


def set_attn_window(model: nn.Module, tile=None, radius=None,
                    strict: bool = True) -> bool:
    """Restrict the self-attention of a ``WanModel`` to a sliding window of
    token tiles (``ops.attn_window`` over its (T, H, W) token grid), or, with
    ``tile`` None, remove the window; returns whether one is set. The
    block-sparse kernel is the FP8 one: every block must be on
    ``attn_dtype == "fp8"``. A model that cannot take the window is an error,
    or, with ``strict=False`` (a value from the environment), is left
    without."""
    from .wan import WanModel

    window = None if tile is None else _check_attn_window((tile, radius))
    if window is not None:
        ok = isinstance(model, WanModel) and len(model.blocks) and all(
            getattr(b, "attn_dtype", None) == "fp8" for b in model.blocks)
        if not ok:
            if strict:
                raise ValueError(
                    "attn_window applies to a WAN model whose blocks run "
                    f"attn_dtype='fp8'; got {type(model).__name__}")
            window = None
    if isinstance(model, WanModel):
        model.attn_window = window
    return window is not None
