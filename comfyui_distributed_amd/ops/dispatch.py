"""Op dispatch: HIP kernels on GPU, reference Python implementations on CPU.

On a GPU host the HIP extension is mandatory — a missing extension raises
``KernelUnavailableError`` instead of silently running eager PyTorch. The
CPU implementations exist for CPU-only test runs and for the reference
numerics the GPU tests compare against; they implement *the same math* as
the kernels (documented per-op).
"""

from __future__ import annotations

import math
import os
from dataclasses import dataclass
from functools import lru_cache

import torch
import torch.nn.functional as F

from . import ext

LANCZOS_A = 3
ATTN_DPADS = (48, 64, 96, 128, 160, 256, 512)


def hip_available() -> bool:
    return ext.get_ext(required=False) is not None


def _versions(*tensors: torch.Tensor) -> tuple:
    """The in-place update counters of the tensors (``load_state_dict``,
    ``copy_``, ``mul_`` ... each bump one): what a cache derived from them
    remembers, a host integer per tensor. Inference tensors keep no counter
    (and cannot be updated in place outside inference mode): None."""
    return tuple(None if t.is_inference() else t._version for t in tensors)


def _f32(t: torch.Tensor | None):
    """fp32 view of a (usually bf16) parameter, cached ON the tensor object
    — the GN/conv launchers used to re-cast weight+bias on every call:
    ~27k bf16->f32 copy kernels per flagship canvas (rocprof r02).

    The cache remembers ``t._version`` and is refreshed, into the same fp32
    tensor, after an in-place update of ``t``; an unchanged parameter returns
    the identical tensor with no launch. A HIP graph captured before the
    update replays the copy it captured, so it sees new values only through
    this same tensor and only after an eager call has refreshed it."""
    if t is None or t.numel() == 0 or t.dtype == torch.float32:
        return t
    c = getattr(t, "_distgpu_f32", None)
    ver = _versions(t)
    if c is not None and c.device == t.device and c.shape == t.shape:
        if getattr(t, "_distgpu_f32_ver", None) != ver:
            c.copy_(t.detach())
            t._distgpu_f32_ver = ver
        return c
    c = t.detach().float().contiguous()
    try:
        t._distgpu_f32 = c
        t._distgpu_f32_ver = ver
    except Exception:  # non-writable tensor subclass: fall back
        pass
    return c


def _on_gpu(*tensors: torch.Tensor) -> bool:
    return any(t.is_cuda for t in tensors if isinstance(t, torch.Tensor))


# ---------------------------------------------------------------------------
# norms / elementwise
# ---------------------------------------------------------------------------


def group_norm_silu(
    x: torch.Tensor,
    groups: int,
    weight: torch.Tensor,
    bias: torch.Tensor,
    eps: float = 1e-6,
    silu: bool = True,
    addend: torch.Tensor | None = None,
) -> torch.Tensor:
    """GroupNorm(+SiLU) of x [B, C, ...]. ``addend`` [B, C] is a per-sample,
    per-channel term added to x first: the result is that of
    ``group_norm_silu(x + addend[:, :, None, None], ...)``. The GPU
    channels_last kernel adds it while it reads (no summed tensor is
    written); every other path adds it in x.dtype here."""
    if _on_gpu(x):
        if (
            x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last)
            and not x.is_contiguous()
        ):
            return group_norm_silu_cl(x, groups, weight, bias, eps, silu,
                                      addend)
        if addend is not None:
            x = x + addend[:, :, None, None]
        return ext.get_ext(True).group_norm_fused(
            x.to(torch.bfloat16), groups, _f32(weight), _f32(bias), eps, silu
        )
    if addend is not None:
        x = x + addend[:, :, None, None]
    # manual GN (F.group_norm rejects 1-value-per-group shapes, e.g. a
    # batch-1 tensor at 1x1 spatial in deep tiny-config levels)
    b, c = x.shape[0], x.shape[1]
    xf = x.float().reshape(b, groups, -1)
    mean = xf.mean(-1, keepdim=True)
    var = xf.var(-1, unbiased=False, keepdim=True)
    y = ((xf - mean) / (var + eps).sqrt()).reshape(x.shape)
    shape = [1, c] + [1] * (x.dim() - 2)
    y = y * weight.float().view(shape) + bias.float().view(shape)
    if silu:
        y = F.silu(y)
    return y.to(x.dtype)


def group_norm_silu_cl(x: torch.Tensor, groups: int, weight, bias,
                       eps: float = 1e-5, silu: bool = True,
                       addend: torch.Tensor | None = None) -> torch.Tensor:
    """GroupNorm(+SiLU) for channels_last NCHW tensors on GPU. A bf16
    ``addend`` [B, C] beside a bf16 x goes to the kernel, which works on
    bf16(x + addend) without writing it; other dtypes are added here."""
    assert x.is_cuda
    if addend is not None and not (
            x.dtype == torch.bfloat16 and addend.dtype == torch.bfloat16
            and addend.shape == (x.shape[0], x.shape[1])):
        x = x + addend[:, :, None, None]
        addend = None
    y = ext.get_ext(True).group_norm_nhwc(
        _nhwc_bf16(x), groups, _f32(weight), _f32(bias), eps, silu, addend
    )
    return y.permute(0, 3, 1, 2)


def layer_norm(
    x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5
) -> torch.Tensor:
    if _on_gpu(x):
        # fp32 parameters, cast once and cached: the launcher's own cast is
        # then a no-op (it was two copy kernels per call)
        return ext.get_ext(True).layer_norm(
            x.to(torch.bfloat16), _f32(weight), _f32(bias), eps)
    y = F.layer_norm(x.float(), (x.shape[-1],), weight.float(), bias.float(), eps)
    return y.to(x.dtype)


def act_mul(a: torch.Tensor, b: torch.Tensor, gelu: bool = False) -> torch.Tensor:
    """a * act(b): SiLU-mul / GEGLU gate."""
    if _on_gpu(a):
        return ext.get_ext(True).act_mul(a.to(torch.bfloat16), b.to(torch.bfloat16), gelu)
    bf = b.float()
    act = F.gelu(bf, approximate="tanh") if gelu else F.silu(bf)
    return (a.float() * act).to(a.dtype)


# ---------------------------------------------------------------------------
# channels-last conv path (hand-written implicit-GEMM MFMA kernels)
# ---------------------------------------------------------------------------


def conv_supported(conv) -> bool:
    """True when the MFMA conv kernel covers this nn.Conv2d."""
    k = conv.kernel_size
    stride_ok = conv.stride == (1, 1) or (
        # stride-2 3x3 (UNet/VAE Downsample) runs on the 256-tile kernel;
        # keeping it off MIOpen also kills its exhaustive-find warmup
        conv.stride == (2, 2) and k == (3, 3) and conv.in_channels % 64 == 0
    )
    # the 256-tile kernel bounds-masks any K_out (the UNet's K=4 out_conv
    # and the VAE's K=3/K=8 edge convs included — MIOpen's heuristic picks
    # for those are pathological); the direct kernel needs K % 16
    kout_ok = (conv.out_channels % 16 == 0
               or (_CONV256 and conv.in_channels % 64 == 0))
    return (
        stride_ok
        and conv.in_channels % 32 == 0
        and kout_ok
        and ((k == (3, 3) and conv.padding == (1, 1))
             or (k == (1, 1) and conv.padding == (0, 0)))
        and conv.dilation == (1, 1)
        and conv.groups == 1
    )


def _repacked_weight(conv) -> torch.Tensor:
    """[K, R*S*C] bf16, (r,s,c) with c innermost — cached on the module.
    The cache remembers ``conv.weight._version`` and is repacked, into the
    same tensor, after an in-place update of the weight (a HIP graph captured
    earlier replays the copy it captured: it reads this same tensor)."""
    weight = conv.weight  # [K, C, R, S]
    wt = getattr(conv, "_distgpu_wt", None)
    ver = _versions(weight)
    k, c, r, s = weight.shape
    if (wt is not None and wt.device == weight.device
            and wt.shape == (k, r * s * c)):
        if getattr(conv, "_distgpu_wt_ver", None) != ver:
            wt.view(k, r, s, c).copy_(weight.detach().permute(0, 2, 3, 1))
            conv._distgpu_wt_ver = ver
        return wt
    wt = weight.detach().permute(0, 2, 3, 1).reshape(k, -1).contiguous()
    wt = wt.to(torch.bfloat16)
    conv._distgpu_wt = wt
    conv._distgpu_wt_ver = ver
    return wt


def _nhwc_bf16(x: torch.Tensor) -> torch.Tensor:
    """Contiguous bf16 [B, H, W, C] of an NCHW tensor: a view when x is
    channels_last bf16, a copy otherwise."""
    nhwc = x.permute(0, 2, 3, 1)
    if not nhwc.is_contiguous():
        nhwc = nhwc.contiguous()
    return nhwc.to(torch.bfloat16)


def _conv_params(conv, device):
    """(repacked weight, taps, fp32 bias or an empty tensor) of a 3x3 / 1x1
    nn.Conv2d, as the conv launchers take them."""
    rs = 9 if conv.kernel_size == (3, 3) else 1
    bias = (_f32(conv.bias) if conv.bias is not None
            else torch.empty(0, device=device))
    return _repacked_weight(conv), rs, bias


_CONV256 = os.environ.get("DISTGPU_CONV256", "1") == "1"
# nn.Linear routing. hipBLASLt keeps every shape except the rows of
# _LINEAR_ROUTES, which measured ahead on gemm256_linear (gemm.hip: N-tile
# width per call, residual operand) in profiles/r23_linear_route.md,
# `tools/kernel_bench.py --op linear_route`.
# A row is (K, N, M_lo, M_hi, fuse): x [M, K] with M_lo <= M <= M_hi and a
# weight [N, K] go to the kernel; `fuse` says whether a residual goes into its
# epilogue there or stays a separate add after it (per site: the fused call
# against product + add). The rows are the measured M (SD1.5 at tile batch 16,
# 24 and 32, SDXL at 32), points and not bands, because the ratio follows how
# the tile count fills rounds of the 256 CUs and not M: 320 -> 320 is 1.01 at
# M = 73984, 0.78 at 110976, 0.92 at 147968, and 320 -> 960 is 0.91, 1.05,
# 0.76 at the same three. Only 640 -> 640 was ahead at every M from 27744 up.
# Left on hipBLASLt: 1280 -> 320 at 68x68 (1.00) and SDXL's 2560 -> 640
# (0.97), ties; 2560 -> 640 below M = 36992 (1.04, 1.23); the 34x34 fused QKV
# (1.24); every 17x17 / SDXL 32x32 Linear (1.3-1.6, with K split 2 or 3:
# 1.4-3.0); the context KV projections (1.6-1.8 at 256 wide, 1.4-1.8 with a K
# split, 1.0 at 128 wide with 3 slices: a tie). DISTGPU_GEMM256=0 sends
# everything to hipBLASLt.
_GEMM256 = os.environ.get("DISTGPU_GEMM256", "1") == "1"
_LINEAR_ROUTES: tuple = (
    # 68x68 tokens, 320 -> 320. Tile batch 32: 0.92; the fused residual was
    # 1.02 and 0.94 of product + add in two sessions, so the add stays.
    # Tile batch 24: 0.78, fused 0.73
    (320, 320, 147968, 147968, False),
    (320, 320, 110976, 110976, True),
    # fused QKV (no residual at this site): 0.76 and 0.91
    (320, 960, 147968, 147968, False),
    (320, 960, 73984, 73984, False),
    # 34x34 tokens at tile batch 24 and 32 (hipBLASLt's slow pick at M =
    # 36992) and SDXL's 64x64: 0.91 / 0.68 / 0.88, fused residual 0.80 / 0.89
    # / 0.75 of product + add
    (640, 640, 27744, 36992, True),
    (2560, 640, 36992, 36992, True),     # 0.83, fused 0.96
    (640, 1920, 32768, 32768, False),    # SDXL fused QKV: 0.81
)
# epilogue residual fusion (ResBlock skip add): measured 1.5% SLOWER than
# the separate eager add on the flagship (same-box A/B, gpurun_out/call17:
# 7.915 vs 8.032 tiles/s — the dependent per-element load makes the
# store-issue-bound epilogue longer than the well-overlapped add pass).
# Kept available for shapes where it may win; off by default. With the
# 8-byte epilogue stores the same A/B is a tie (11.088-11.126 fused against
# 11.064-11.083 tiles/s, profiles/r07_conv_tiles.md), so the default stays.
_FUSE_RES = os.environ.get("DISTGPU_FUSE_RESIDUAL", "0") == "1"
# fused DiT glue kernels (dit_ops.hip): off = the eager torch sequences the
# CPU path runs, on GPU tensors too, for same-box A/B
_DIT_FUSED = os.environ.get("DISTGPU_DIT_FUSED", "1") == "1"


def conv2d_mfma(x: torch.Tensor, conv, fuse_silu: bool = False,
                up2: bool = False,
                residual: torch.Tensor | None = None) -> torch.Tensor:
    """x: NCHW tensor in channels_last memory format (bf16, on GPU) ->
    same layout. Dispatches to the implicit-GEMM NHWC kernel: the 256-tile
    glds template (gemm.hip) when shapes allow, else the direct kernel
    (conv.hip, 64x64 or 128x128 tile).
    The 256-tile launcher picks its N-tile width (128/256/320) and a K
    split per call from (M, K_out, Kdim); ``ext.conv256_plan`` reports the
    choice and ``ext.conv256_nhwc_ex`` pins it.
    ``up2`` fuses a nearest-2x upsample into the conv's tap addressing
    (the upsampled tensor never materializes). ``residual`` (a
    channels_last NCHW tensor of the OUTPUT shape) is added in the
    epilogue — the ResBlock skip connection without its own kernel.
    A module that carries ``quantize_conv_weight_fp8``'s pack
    (``quant.quantize_unet_convs``) runs ``quant_nhwc_fp8`` + ``conv_fp8``
    instead, where C % 64 == 0, B*H*W >= 256, not ``up2`` and
    ``conv_fp8_route`` does not list the shape as a loss."""
    assert x.is_cuda
    if residual is not None and not _FUSE_RES:
        return conv2d_mfma(x, conv, fuse_silu, up2) + residual
    b, c, h, w = x.shape
    nhwc = _nhwc_bf16(x)
    wt, rs, bias = _conv_params(conv, x.device)
    stride = conv.stride[0]
    if (getattr(conv, "_distgpu_fp8", None) is not None and not up2
            and c % 64 == 0 and b * h * w >= 256
            and conv_fp8_route(c, conv.out_channels, h, w, stride)):
        # a conv marked by quant.quantize_unet_convs, inside the FP8 kernel's
        # cover and not a measured loss: image quantiser + conv_fp8_kernel
        qw, sw = quantize_conv_weight_fp8(conv)
        q, sa = quant_nhwc_fp8(nhwc)
        y = conv_fp8(q, sa, qw, sw, bias if bias.numel() else None, rs=rs,
                     stride=stride, fuse_silu=fuse_silu,
                     residual=None if residual is None
                     else _nhwc_bf16(residual))
        return y.permute(0, 3, 1, 2)
    if _CONV256 and c % 64 == 0 and (b * h * w >= 256 or up2):
        if residual is not None:
            res = _nhwc_bf16(residual)
        else:
            res = torch.empty(0, device=x.device, dtype=torch.bfloat16)
        y = ext.get_ext(True).conv256_nhwc(
            nhwc, wt, bias, res, b, h, w, c,
            conv.out_channels, rs, stride, up2, fuse_silu,
        )
        return y.permute(0, 3, 1, 2)
    assert stride == 1 and not up2, "strided/up2 conv needs the conv256 path"
    if residual is not None:
        return conv2d_mfma(x, conv, fuse_silu) + residual
    y = ext.get_ext(True).conv_nhwc(
        nhwc, wt, bias, b, h, w, c, conv.out_channels, rs, fuse_silu,
    )
    return y.permute(0, 3, 1, 2)  # NCHW semantic, channels_last storage


def linear_route(M: int, N: int, K: int) -> tuple[bool, bool]:
    """(routed, fuse): whether a bf16 Linear of x [M, K] by a weight [N, K]
    on the GPU goes to ``gemm256_linear``, and whether a residual is added in
    its epilogue there. Table lookup, no launch."""
    if _GEMM256:
        for k, n, m_lo, m_hi, fuse in _LINEAR_ROUTES:
            if K == k and N == n and m_lo <= M <= m_hi:
                return True, fuse
    return False, False


def _bf16(t: torch.Tensor) -> torch.Tensor:
    """bf16 copy of a parameter, cached on the tensor like ``_f32``; a bf16
    parameter (the flagship's) is returned as it is, with no launch."""
    if t.dtype == torch.bfloat16:
        return t
    c = getattr(t, "_distgpu_bf16", None)
    ver = _versions(t)
    if c is not None and c.device == t.device and c.shape == t.shape:
        if getattr(t, "_distgpu_bf16_ver", None) != ver:
            c.copy_(t.detach())
            t._distgpu_bf16_ver = ver
        return c
    c = t.detach().to(torch.bfloat16).contiguous()
    t._distgpu_bf16 = c
    t._distgpu_bf16_ver = ver
    return c


def linear_mfma(x: torch.Tensor, weight: torch.Tensor,
                bias: torch.Tensor | None = None,
                fuse_silu: bool = False,
                residual: torch.Tensor | None = None) -> torch.Tensor:
    """torch-Linear, x [..., K], plus ``residual`` (the output's shape) when
    given. A bf16 x on the GPU whose (M, N, K) is a row of ``_LINEAR_ROUTES``
    runs on the 256-tile MFMA GEMM (``gemm256_linear``): fp32 accumulation,
    bias, SiLU and, where the row fuses it, the residual in fp32 before the
    one rounding. Everything else is hipBLASLt's ``F.linear`` and a separate
    add."""
    K = x.shape[-1]
    M = x.numel() // K
    N = weight.shape[0]
    routed, fuse = (linear_route(M, N, K)
                    if _on_gpu(x) and x.dtype == torch.bfloat16
                    else (False, False))
    if routed:
        x2 = x.reshape(M, K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        w = _bf16(weight)
        if not w.is_contiguous():
            w = w.contiguous()
        b = (_f32(bias) if bias is not None
             else torch.empty(0, device=x.device))
        res = torch.empty(0, device=x.device, dtype=torch.bfloat16)
        # any other residual (dtype, a broadcast shape) is added afterwards,
        # as on the hipBLASLt path
        if (residual is not None and fuse
                and residual.dtype == torch.bfloat16
                and residual.shape == (*x.shape[:-1], N)):
            res = residual.reshape(M, N)
            if not res.is_contiguous():
                res = res.contiguous()
            residual = None
        y = ext.get_ext(True).gemm256_linear(x2, w, b, res, fuse_silu)
        y = y.reshape(*x.shape[:-1], N)
        return y if residual is None else y + residual
    y = F.linear(x, weight, bias)
    if fuse_silu:
        y = F.silu(y)
    return y if residual is None else y + residual


# GEGLU-fused feed-forward projection (gemm.hip, gemm_geglu): the
# [M, 2*inner] projection is never written. Not bit-identical to the pair it
# replaces (which rounds the projection to bf16 before the gate); opt-in.
# What the fusion saves (the act_mul pass) and what the kernel loses to
# hipBLASLt on the product both scale with M * inner, the loss also with K:
# at the UNet levels the fused call takes 0.83x of the pair's time at K = 320,
# 1.02x at K = 640 and 1.18x at K = 1280 (profiles/r16_geglu_gemm.md), so the
# route stops at the largest K that measured ahead.
_GEGLU_GEMM = os.environ.get("DISTGPU_GEGLU_GEMM", "0") == "1"
_GEGLU_MAX_K = 320


def _geglu_paired(t: torch.Tensor) -> torch.Tensor:
    """View of t [2*inner, ...] (value half, then gate half) as
    [inner/16, 2, 16, ...]: flattened over its first three dims, value row j
    is row 32*(j//16) + j%16 and gate row j is row 32*(j//16) + 16 + j%16,
    so that both land in the same lane of the same wave of the kernel."""
    inner = t.shape[0] // 2
    return t.reshape(2, inner // 16, 16, *t.shape[1:]).transpose(0, 1)


def pack_geglu_weight(weight: torch.Tensor, bias: torch.Tensor | None = None
                      ) -> tuple[torch.Tensor, torch.Tensor]:
    """weight [2*inner, K], bias [2*inner] or None of a GEGLU projection
    (rows [0, inner): value, [inner, 2*inner): gate) -> (w_packed
    [2*inner, K] in weight's dtype, bias_packed fp32 [2*inner], empty without
    a bias) in the pairing ``gemm_geglu`` reads. Plain torch, run once per
    layer; inner % 16 == 0."""
    if weight.dim() != 2 or weight.shape[0] % 32:
        raise ValueError(
            f"weight must be [2*inner, K] with inner % 16 == 0, got "
            f"{tuple(weight.shape)}")
    if bias is not None and bias.shape != weight.shape[:1]:
        raise ValueError(
            f"bias {tuple(bias.shape)} does not match weight "
            f"{tuple(weight.shape)}")
    def packed(t):  # always a copy: with inner = 16 the pairing is a view
        return _geglu_paired(t.detach()).clone(
            memory_format=torch.contiguous_format).reshape(t.shape)

    if bias is None:
        return packed(weight), torch.empty(0, device=weight.device)
    return packed(weight), packed(bias).float()


def _geglu_packed(weight: torch.Tensor, bias: torch.Tensor | None):
    """pack_geglu_weight in bf16, cached on the weight (for a module's
    ``proj_in.weight`` that is the module's lifetime). The cache remembers
    ``_versions(weight, bias)`` and which bias it was made with; after an
    in-place update of either, both packed tensors are refreshed in place,
    so a HIP graph captured earlier, which reads these same tensors, sees
    the new values once an eager call has refreshed them."""
    ver = _versions(*(t for t in (weight, bias) if t is not None))
    c = getattr(weight, "_distgpu_geglu", None)
    if (c is not None and c[2] is bias and c[0].device == weight.device
            and c[0].shape == weight.shape):
        if getattr(weight, "_distgpu_geglu_ver", None) != ver:
            for dst, src in ((c[0], weight), (c[1], bias)):
                if src is not None:
                    paired = _geglu_paired(src.detach())
                    dst.view(paired.shape).copy_(paired)
            weight._distgpu_geglu_ver = ver
        return c[0], c[1]
    wp, bp = pack_geglu_weight(weight.to(torch.bfloat16), bias)
    weight._distgpu_geglu = (wp, bp, bias)
    weight._distgpu_geglu_ver = ver
    return wp, bp


def linear_geglu(x: torch.Tensor, weight: torch.Tensor,
                 bias: torch.Tensor | None = None) -> torch.Tensor:
    """GEGLU projection: with ``a, gate = F.linear(x, weight, bias).chunk(2,
    -1)``, returns ``a * gelu_tanh(gate)``. x [..., K] -> [..., inner] in
    x.dtype.

    GPU with ``DISTGPU_GEGLU_GEMM=1``: one ``gemm_geglu`` launch for bf16 x
    with tokens >= 1024, K % 64 == 0, K <= 320
    (where it measured ahead of the pair) and inner % 16 == 0; accumulation, bias, GELU and the product in fp32, one
    rounding. Everything else (CPU, the flag off, other shapes and dtypes)
    runs the Linear, ``chunk`` and ``act_mul(gelu=True)``."""
    K = x.shape[-1]
    M = x.numel() // K
    if (
        _GEGLU_GEMM
        and _on_gpu(x)
        and x.dtype == torch.bfloat16
        and M >= 1024
        and K % 64 == 0
        and K <= _GEGLU_MAX_K
        and weight.shape[0] % 32 == 0
    ):
        x2 = x.reshape(M, K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        y = ext.get_ext(True).gemm_geglu(x2, *_geglu_packed(weight, bias))
        return y.reshape(*x.shape[:-1], weight.shape[0] // 2)
    a, gate = linear_mfma(x, weight, bias).chunk(2, dim=-1)
    return act_mul(a, gate, gelu=True)


def conv2d_smallc(x: torch.Tensor, conv, fuse_silu: bool = False) -> torch.Tensor:
    """Stem conv (in_channels <= 8) on the dedicated HIP kernel — MIOpen/CK
    fall back to very slow paths for NHWC C=4. x: channels_last NCHW."""
    assert x.is_cuda and conv.in_channels <= 8
    b, c, h, w = x.shape
    wt, rs, bias = _conv_params(conv, x.device)
    y = ext.get_ext(True).conv_smallc(
        _nhwc_bf16(x), wt, bias, b, h, w, c, conv.out_channels, rs, fuse_silu,
    )
    return y.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------
# dense-block conv (conv_dense.hip): the RRDBNet upscale model's convolution
# ---------------------------------------------------------------------------

# off = the torch sequence of the CPU path, on device tensors too, and the
# textbook torch.cat forward in models/upscaler.py, for same-box A/B
_RRDB_HIP = os.environ.get("DISTGPU_RRDB_HIP", "1") == "1"


def _dense_pitch(t: torch.Tensor, name: str, shape: tuple) -> int:
    """Pixel pitch of a [B, H, W, C] channel-slice view, after checking the
    layout conv_dense.hip addresses: channels contiguous, pixels ``pitch``
    elements apart, rows and images packed at that pitch, pitch and start
    multiples of 8 elements."""
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got "
                         f"{tuple(t.shape)}")
    b, h, w, c = shape
    pitch = (t.stride(2) if w > 1 else t.stride(1) if h > 1
             else t.stride(0) if b > 1 else (c + 7) // 8 * 8)  # one pixel
    if c > 1 and t.stride(3) != 1:
        raise ValueError(f"{name}: channels are not contiguous")
    if pitch < c or pitch % 8 or t.storage_offset() % 8:
        raise ValueError(f"{name}: pixel pitch {pitch} / start "
                         f"{t.storage_offset()} must be multiples of 8 "
                         f"elements, the pitch at least C = {c}")
    if (h > 1 and t.stride(1) != w * pitch) or (
            b > 1 and t.stride(0) != h * w * pitch):
        raise ValueError(f"{name}: rows / images are not packed at the pixel "
                         f"pitch {pitch}")
    return pitch


def _dense_span(t: torch.Tensor, pitch: int) -> tuple[int, int]:
    """[first, last) element of the view in its storage."""
    b, h, w, c = t.shape
    return t.storage_offset(), t.storage_offset() + (b * h * w - 1) * pitch + c


def _dense_channels_overlap(a: torch.Tensor, pa: int, b: torch.Tensor,
                            pb: int) -> bool:
    """Do two channel-slice views touch a common element? Views of one
    storage at one pitch are compared by channel range inside the pitch;
    anything else by extent."""
    if (a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr()
            or a.dtype != b.dtype):
        return False
    a0, a1 = _dense_span(a, pa)
    b0, b1 = _dense_span(b, pb)
    if a1 <= b0 or b1 <= a0:
        return False
    if pa != pb:
        return True
    ca, cb = a0 % pa, b0 % pb
    if ca + a.shape[3] > pa or cb + b.shape[3] > pb:   # a slice across pixels
        return True
    return ca < cb + b.shape[3] and cb < ca + a.shape[3]


def _dense_same_elements(a: torch.Tensor, b: torch.Tensor) -> bool:
    return (a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and a.storage_offset() == b.storage_offset()
            and a.stride() == b.stride() and a.dtype == b.dtype)


def conv3x3_dense(x: torch.Tensor, conv, out: torch.Tensor, *,
                  lrelu: float | None = None, alpha: float = 1.0,
                  res1: torch.Tensor | None = None, beta1: float = 1.0,
                  res2: torch.Tensor | None = None,
                  up2: bool = False) -> torch.Tensor:
    """3x3 / stride 1 / pad 1 convolution with K_out <= 64 on NHWC channel
    slices, written into ``out``::

        t   = conv(x) + bias                       fp32
        t   = leaky_relu(t, lrelu)                 if lrelu is not None
        out = alpha * t + beta1 * res1 + res2      one rounding

    ``x`` [B, H, W, C_in], ``out`` / ``res1`` / ``res2`` [B, Ho, Wo, K_out]
    are views with a contiguous last dim, each with its own pixel pitch and
    start (multiples of 8 elements), rows and images packed at that pitch:
    ``buf[..., :C_in]`` and ``buf[..., C_in:C_in + 32]`` of one wide buffer
    are the typical pair, which is how a dense block's concat disappears.
    ``up2`` convolves the nearest-2x upsample of x (Ho = 2H) without writing
    it. C_in % 32 == 0 in 32..512, K_out in 1..64.

    ``out`` may be elementwise identical to ``res1`` / ``res2``, and may share
    a buffer with ``x`` when it touches none of the channels x reads;
    overlap raises ValueError. On the GPU (bf16) this is conv_dense.hip; on
    the CPU, and with ``DISTGPU_RRDB_HIP=0``, the same formula in fp32 torch."""
    k, c = conv.out_channels, conv.in_channels
    if (conv.kernel_size != (3, 3) or conv.stride != (1, 1)
            or conv.padding != (1, 1) or conv.dilation != (1, 1)
            or conv.groups != 1):
        raise ValueError("conv3x3_dense: a 3x3, stride 1, pad 1 conv expected")
    if c % 32 or not 32 <= c <= 512:
        raise ValueError(f"conv3x3_dense: C_in = {c} must be a multiple of 32 "
                         f"in 32..512")
    if not 1 <= k <= 64:
        raise ValueError(f"conv3x3_dense: K_out = {k} must be in 1..64")
    if x.dim() != 4 or x.shape[3] != c:
        raise ValueError(f"conv3x3_dense: x must be [B, H, W, {c}], got "
                         f"{tuple(x.shape)}")
    b, h, w, _ = x.shape
    oshape = (b, 2 * h, 2 * w, k) if up2 else (b, h, w, k)
    px = _dense_pitch(x, "x", (b, h, w, c))
    po = _dense_pitch(out, "out", oshape)
    if _dense_channels_overlap(x, px, out, po):
        raise ValueError("conv3x3_dense: out overlaps the channels x reads")
    for name, r in (("res1", res1), ("res2", res2)):
        if r is None:
            continue
        pr = _dense_pitch(r, name, oshape)
        if (not _dense_same_elements(r, out)
                and _dense_channels_overlap(r, pr, out, po)):
            raise ValueError(f"conv3x3_dense: out overlaps {name} without "
                             f"being identical to it")
    if _on_gpu(x) and _RRDB_HIP:
        bias = (_f32(conv.bias) if conv.bias is not None
                else torch.empty(0, device=x.device))
        ext.get_ext(True).conv_dense(
            x, _repacked_weight(conv), bias, out, res1, res2,
            lrelu is not None, 0.0 if lrelu is None else float(lrelu),
            float(alpha), float(beta1), bool(up2))
        return out
    xf = x.float().permute(0, 3, 1, 2)
    if up2:
        xf = F.interpolate(xf, scale_factor=2, mode="nearest")
    t = F.conv2d(xf, conv.weight.float(),
                 None if conv.bias is None else conv.bias.float(), padding=1)
    if lrelu is not None:
        t = F.leaky_relu(t, float(lrelu))
    v = (alpha * t).permute(0, 2, 3, 1)
    if res1 is not None:
        v = v + beta1 * res1.float()
    if res2 is not None:
        v = v + res2.float()
    out.copy_(v)   # v is complete before the (possibly aliased) write
    return out


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------


def _dpad_for(d: int) -> int:
    for p in ATTN_DPADS:
        if d <= p:
            return p
    raise ValueError(f"head dim {d} unsupported (max {ATTN_DPADS[-1]})")


def attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    heads: int,
    kv_heads: int | None = None,
    scale: float | None = None,
) -> torch.Tensor:
    """Multi-head attention over packed heads.

    q: [B*H, Nq, D], k/v: [B*Hkv, Nk, D]; returns [B*H, Nq, D].
    GPU path: the MFMA flash kernels (bf16, fp32 accumulation) for head
    dims that are multiples of 8 up to 512: attn_fwd_kernel up to 160,
    attn_wide_kernel above. The kernels pad D to their compute width and
    mask the key tail themselves; nothing is padded or copied here.
    """
    kv_heads = kv_heads or heads
    d = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    if _on_gpu(q):
        _dpad_for(d)  # validates the supported range
        o = ext.get_ext(True).attn_fwd(
            q.to(torch.bfloat16).contiguous(),
            k.to(torch.bfloat16).contiguous(),
            v.to(torch.bfloat16).contiguous(),
            heads, kv_heads, k.shape[1], scale,
        )
        return o
    # CPU reference: fp32 math, GQA by repeating kv heads.
    qf, kf, vf = q.float(), k.float(), v.float()
    if kv_heads != heads:
        rep = heads // kv_heads
        b = q.shape[0] // heads
        kf = kf.reshape(b, kv_heads, 1, *kf.shape[1:]).expand(-1, -1, rep, -1, -1)
        kf = kf.reshape(b * heads, *k.shape[1:])
        vf = vf.reshape(b, kv_heads, 1, *vf.shape[1:]).expand(-1, -1, rep, -1, -1)
        vf = vf.reshape(b * heads, *v.shape[1:])
    s = torch.bmm(qf, kf.transpose(1, 2)) * scale
    p = torch.softmax(s, dim=-1)
    return torch.bmm(p, vf).to(q.dtype)


def attention_packed(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    heads: int,
    kv_heads: int | None = None,
    scale: float | None = None,
) -> torch.Tensor:
    """Attention on the packed projection layout: q [B, Nq, H*D],
    k/v [B, Nk, Hkv*D] -> [B, Nq, H*D]. On GPU this feeds the strided
    kernel directly (zero reshapes/copies), D % 8 == 0 up to 512; on CPU
    it unpacks and reuses the reference path."""
    kv_heads = kv_heads or heads
    d = q.shape[-1] // heads
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    if _on_gpu(q):
        _dpad_for(d)
        return ext.get_ext(True).attn_fwd_packed(
            q.to(torch.bfloat16).contiguous(),
            k.to(torch.bfloat16).contiguous(),
            v.to(torch.bfloat16).contiguous(),
            heads, kv_heads, scale,
        )
    b, nq, _ = q.shape
    nk = k.shape[1]

    def split(u, h):
        return (u.reshape(b, -1, h, d).permute(0, 2, 1, 3)
                .reshape(b * h, -1, d))

    o = attention(split(q, heads), split(k, kv_heads), split(v, kv_heads),
                  heads=heads, kv_heads=kv_heads, scale=scale)
    return (o.reshape(b, heads, nq, d).permute(0, 2, 1, 3)
            .reshape(b, nq, heads * d))


def attention_qkv(qkv: torch.Tensor, heads: int,
                  scale: float | None = None) -> torch.Tensor:
    """Self-attention straight off a fused projection [B, N, 3*H*D];
    D % 8 == 0 up to 512 on the GPU."""
    hd = qkv.shape[-1] // 3
    d = hd // heads
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    if _on_gpu(qkv):
        _dpad_for(d)
        return ext.get_ext(True).attn_fwd_qkv(
            qkv.to(torch.bfloat16).contiguous(), heads, scale)
    q, k, v = qkv.split(hd, dim=-1)
    return attention_packed(q.contiguous(), k.contiguous(), v.contiguous(),
                            heads=heads, scale=scale)


def attention_q_kv(q: torch.Tensor, kv: torch.Tensor, heads: int,
                   scale: float | None = None) -> torch.Tensor:
    """Cross-attention: q [B,Nq,H*D] + fused kv [B,Nk,2*H*D]; D % 8 == 0
    up to 512 on the GPU."""
    hd = q.shape[-1]
    d = hd // heads
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    if _on_gpu(q):
        _dpad_for(d)
        return ext.get_ext(True).attn_fwd_q_kv(
            q.to(torch.bfloat16).contiguous(),
            kv.to(torch.bfloat16).contiguous(), heads, scale)
    k, v = kv.split(hd, dim=-1)
    return attention_packed(q, k.contiguous(), v.contiguous(), heads=heads,
                            scale=scale)


# ---------------------------------------------------------------------------
# DiT glue (WAN / Flux): QK-norm + RoPE, norm + adaLN modulation, gated adds
# ---------------------------------------------------------------------------


def _dit_fused(*acts: torch.Tensor | None) -> bool:
    """The dit_ops.hip kernels cover bf16 device activations. Everything
    else (CPU, ``_DIT_FUSED`` off, fp32 on device, an fp32 operand beside a
    bf16 one, where torch promotes the result) runs the torch sequences, as
    the models did before the kernels existed."""
    return _DIT_FUSED and all(
        t.is_cuda and t.dtype == torch.bfloat16 for t in acts if t is not None)


def _vec8_view(t: torch.Tensor) -> torch.Tensor:
    """bf16 view the kernels can read in place with 16-byte loads: last dim
    contiguous, every other stride and the start offset a multiple of 8
    elements. Anything else is copied."""
    ok = (t.stride(-1) == 1 and t.storage_offset() % 8 == 0
          and all(s % 8 == 0 for s in t.stride()[:-1]))
    return t if ok else t.contiguous()


def _norm_rope_torch(x, weight, cos, sin, heads, eps, token_offset):
    """Per-head RMSNorm (fp32, cast back to x.dtype) then rotation of the
    (even, odd) channel pairs in x.dtype. x [B, N, H*D] -> same shape."""
    b, n, hd = x.shape
    xv = x.reshape(b, n, heads, hd // heads)
    xf = xv.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    y = (y * weight.float()).to(x.dtype)
    x1, x2 = y[..., 0::2], y[..., 1::2]
    c = cos[None, token_offset:token_offset + n, None, :].to(x.dtype)
    s = sin[None, token_offset:token_offset + n, None, :].to(x.dtype)
    out = torch.empty_like(y)
    out[..., 0::2] = x1 * c - x2 * s
    out[..., 1::2] = x1 * s + x2 * c
    return out.reshape(b, n, hd)


def qk_norm_rope(
    q: torch.Tensor,
    k: torch.Tensor,
    q_weight: torch.Tensor,
    k_weight: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    heads: int,
    eps: float = 1e-6,
    token_offset: int = 0,
    out: tuple[torch.Tensor, torch.Tensor] | None = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-head RMSNorm + rotary embedding of q and k.

    q, k: [B, N, H*D] (views of a fused projection are read in place);
    q_weight, k_weight: [D]; cos, sin: [Npos, D/2]. Input row n lands in row
    ``token_offset + n`` of ``out = (out_q, out_k)`` ([B, Ntot, H*D],
    contiguous) and is rotated by table row ``token_offset + n``; other
    rows of ``out`` are left alone. Without ``out`` ([B, N, H*D] buffers
    are allocated) ``token_offset`` must be 0. Returns (out_q, out_k).

    GPU: one dit_ops.hip launch, fp32 throughout, one bf16 rounding on
    store. CPU / eager: norm in fp32, cast to x.dtype, rotation in x.dtype.
    """
    b, n, hd = q.shape
    if k.shape != q.shape:
        raise ValueError(f"q {tuple(q.shape)} and k {tuple(k.shape)} differ")
    if hd % heads:
        raise ValueError(f"last dim {hd} is not a multiple of heads {heads}")
    d = hd // heads
    if d % 8 or not 16 <= d <= 256:
        raise ValueError(
            f"head dim {d} unsupported (multiple of 8 in [16, 256])")
    if cos.shape != sin.shape or cos.shape[-1] != d // 2 \
            or cos.shape[0] < token_offset + n:
        raise ValueError(
            f"cos/sin {tuple(cos.shape)}/{tuple(sin.shape)} do not cover "
            f"[{token_offset + n}, {d // 2}]")
    if out is None:
        if token_offset:
            raise ValueError("token_offset needs explicit out buffers")
        out = (torch.empty(b, n, hd, dtype=q.dtype, device=q.device),
               torch.empty(b, n, hd, dtype=q.dtype, device=q.device))
    out_q, out_k = out
    for o in out:
        if (o.dim() != 3 or o.shape[0] != b or o.shape[2] != hd
                or token_offset < 0 or o.shape[1] < token_offset + n):
            raise ValueError(
                f"out {tuple(o.shape)} does not hold rows "
                f"[{token_offset}, {token_offset + n}) of [{b}, *, {hd}]")
    if _dit_fused(q, k, out_q, out_k):
        ext.get_ext(True).qk_norm_rope(
            _vec8_view(q), _vec8_view(k), _f32(q_weight), _f32(k_weight),
            cos.float().contiguous(), sin.float().contiguous(),
            out_q, out_k, heads, eps, token_offset)
        return out_q, out_k
    out_q[:, token_offset:token_offset + n] = _norm_rope_torch(
        q, q_weight, cos, sin, heads, eps, token_offset)
    out_k[:, token_offset:token_offset + n] = _norm_rope_torch(
        k, k_weight, cos, sin, heads, eps, token_offset)
    return out_q, out_k


def _norm_modulate_eps(mode, weight, scale, shift, eps) -> float:
    """Argument validation of norm_modulate / norm_modulate_fp8; returns the
    eps to use."""
    if mode not in ("rms", "layer"):
        raise ValueError(f"mode {mode!r} is not 'rms' or 'layer'")
    if (mode == "rms") != (weight is not None):
        raise ValueError("mode 'rms' takes a weight, mode 'layer' none")
    if (scale is None) != (shift is None):
        raise ValueError("scale and shift come together")
    if eps is None:
        eps = 1e-6 if mode == "rms" else 1e-5
    return eps


def _norm_modulate_operands(x, weight, scale, shift):
    """(x, weight, scale, shift) as the dit_ops.hip launchers take them: an
    empty tensor stands for an absent operand."""
    empty = torch.empty(0, device=x.device, dtype=torch.bfloat16)
    return (x.contiguous(),
            _f32(weight) if weight is not None else empty,
            _vec8_view(scale) if scale is not None else empty,
            _vec8_view(shift) if shift is not None else empty)


def norm_modulate(
    x: torch.Tensor,
    mode: str,
    weight: torch.Tensor | None = None,
    scale: torch.Tensor | None = None,
    shift: torch.Tensor | None = None,
    eps: float | None = None,
) -> torch.Tensor:
    """``norm(x) * (1 + scale[b]) + shift[b]`` over the last dim of
    x [B, N, C]. ``mode="rms"``: RMSNorm with ``weight`` [C] (eps 1e-6);
    ``mode="layer"``: mean/variance LayerNorm without affine (eps 1e-5).
    scale/shift: [B, C] (strided views are fine), or both None for the
    plain norm.

    GPU: one dit_ops.hip launch for bf16 x [B, N, C] with C % 8 == 0,
    C <= 8192 and scale/shift of exactly [B, C]; other shapes and dtypes take
    the torch sequence. CPU / eager: the norm is rounded to x.dtype before
    the modulation, as the models did.
    """
    eps = _norm_modulate_eps(mode, weight, scale, shift, eps)
    c = x.shape[-1]
    covered = (
        x.dim() == 3 and c % 8 == 0 and c <= 8192
        and all(m is None or m.shape == (x.shape[0], c)
                for m in (scale, shift)))
    if covered and _dit_fused(x, scale, shift):
        return ext.get_ext(True).norm_modulate(
            *_norm_modulate_operands(x, weight, scale, shift), eps)
    if mode == "rms":
        xf = x.float()
        y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        y = (y * weight.float()).to(x.dtype)
    else:
        y = F.layer_norm(x, (c,), None, None, eps)
    if scale is not None:
        y = y * (1 + scale[:, None]) + shift[:, None]
    return y


def rms_norm(x: torch.Tensor, weight: torch.Tensor,
             eps: float = 1e-6) -> torch.Tensor:
    """RMSNorm over the last dim of x [..., C]."""
    if x.dim() != 3 and _dit_fused(x):  # the kernel wants [B, N, C] rows
        y = norm_modulate(x.reshape(1, -1, x.shape[-1]), "rms", weight,
                          eps=eps)
        return y.reshape(x.shape)
    return norm_modulate(x, "rms", weight, eps=eps)


def gated_residual(x: torch.Tensor, gate: torch.Tensor,
                   y: torch.Tensor) -> torch.Tensor:
    """``x + gate[:, None] * y``. x, y: [B, N, C]; gate: [B, C] (strided
    views are fine). GPU: one dit_ops.hip launch, fp32 multiply-add, one
    rounding, for bf16 operands of exactly these shapes with C % 8 == 0;
    other shapes and dtypes take the torch expression."""
    covered = (
        x.dim() == 3 and x.shape[-1] % 8 == 0 and y.shape == x.shape
        and gate.shape == (x.shape[0], x.shape[-1]))
    if covered and _dit_fused(x, gate, y):
        return ext.get_ext(True).gated_residual(
            x.contiguous(), _vec8_view(gate), y.contiguous())
    return x + gate[:, None] * y


# ---------------------------------------------------------------------------
# FP8 (e4m3fn) Linear: per-channel weights, per-row activations
# ---------------------------------------------------------------------------

E4M3_MAX = 448.0
FP8_MAX_K = 16384
_FP8_ACTS = {None: 0, "none": 0, "silu": 1, "gelu_tanh": 2}
# smallest absmax the scale is taken from: keeps an all-zero row's scale > 0
_FP8_AMAX_FLOOR = 2.0 ** -126 * E4M3_MAX


def _fp8_scale(amax: torch.Tensor) -> torch.Tensor:
    """fp32 scale = max(amax, 2^-126 * 448) * (1/448): one fp32 multiply, the
    same operation the kernel does, so both give the same bits."""
    inv_max = torch.tensor(1.0 / E4M3_MAX, dtype=torch.float32,
                           device=amax.device)
    return amax.float().clamp_min(_FP8_AMAX_FLOOR) * inv_max


def _fp8_quant(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return (x.float() / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(
        torch.float8_e4m3fn)


def fp8_shape_supported(k: int) -> bool:
    """Reduction dims the FP8 path takes: K % 128 == 0, K <= 16384."""
    return k > 0 and k % 128 == 0 and k <= FP8_MAX_K


def fp8_padded_k(k: int) -> int:
    """The pitch of quantised rows under ``pad_k``: K rounded up to the GEMM's
    128-byte K-tile."""
    return (k + 127) // 128 * 128


def fp8_pad_shape_supported(k: int) -> bool:
    """Reduction dims the padded operands take: K % 64 == 0, K <= 16384."""
    return k > 0 and k % 64 == 0 and k <= FP8_MAX_K


def _fp8_pad_cols(q: torch.Tensor) -> torch.Tensor:
    """q [M, K] float8 -> [M, fp8_padded_k(K)] with zero bytes behind K."""
    m, k = q.shape
    out = torch.zeros(m, fp8_padded_k(k), dtype=torch.uint8, device=q.device)
    out[:, :k] = q.view(torch.uint8)
    return out.view(torch.float8_e4m3fn)


def quantize_weight_fp8(w: torch.Tensor, pad_k: bool = False
                        ) -> tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] -> (qw [N, K] float8_e4m3fn, sw [N] fp32): per-output-channel
    absmax / 448. Plain torch, run once per layer. ``pad_k``: qw is
    [N, fp8_padded_k(K)] with zero columns behind K, the operand that goes
    with ``quantize_rows(x, pad_k=True)``."""
    if w.dim() != 2:
        raise ValueError(f"weight must be [N, K], got {tuple(w.shape)}")
    w = w.detach()
    sw = _fp8_scale(w.float().abs().amax(dim=1))
    qw = _fp8_quant(w, sw)
    if pad_k:
        qw = _fp8_pad_cols(qw)
    return qw.contiguous(), sw.contiguous()


def quant_rows_fp8(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """x [M, K] -> (q [M, K] float8_e4m3fn, scale [M] fp32), per-row
    absmax / 448. GPU: the gemm_fp8.hip quantiser (bf16 input). CPU: the same
    definition in torch."""
    if x.dim() != 2:
        raise ValueError(f"x must be [M, K], got {tuple(x.shape)}")
    if not fp8_shape_supported(x.shape[1]):
        raise ValueError(
            f"K = {x.shape[1]} unsupported (multiple of 128, <= {FP8_MAX_K})")
    if _on_gpu(x):
        if x.dtype != torch.bfloat16:
            raise ValueError(f"the FP8 quantiser takes bf16, got {x.dtype}")
        return ext.get_ext(True).quant_rows_fp8(x.contiguous())
    scale = _fp8_scale(x.float().abs().amax(dim=1))
    return _fp8_quant(x, scale), scale


def quant_rows_fp8_pad(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``quant_rows_fp8`` for K % 64 == 0: q is [M, fp8_padded_k(K)] with zero
    bytes in [K, Kp); the scale is taken over the K real elements. GPU: the
    padded quantiser of gemm_fp8.hip (one launch, the pad is stored by the
    loop that stores the codes)."""
    if x.dim() != 2:
        raise ValueError(f"x must be [M, K], got {tuple(x.shape)}")
    if not fp8_pad_shape_supported(x.shape[1]):
        raise ValueError(
            f"K = {x.shape[1]} unsupported (multiple of 64, <= {FP8_MAX_K})")
    if _on_gpu(x):
        if x.dtype != torch.bfloat16:
            raise ValueError(f"the FP8 quantiser takes bf16, got {x.dtype}")
        return ext.get_ext(True).quant_rows_fp8_pad(x.contiguous())
    scale = _fp8_scale(x.float().abs().amax(dim=1))
    return _fp8_pad_cols(_fp8_quant(x, scale)), scale


@dataclass(frozen=True, eq=False)
class Fp8Rows:
    """Activation rows that are already quantised, on their way from a
    producer to one or several FP8 Linears. ``q``: [..., K] float8_e4m3fn,
    contiguous; ``scale``: [...] fp32, one per row; ``dtype``: what the
    consuming Linear returns, the dtype of the activation the rows were
    taken from. ``linear_fp8`` takes one in place of ``x``."""

    q: torch.Tensor
    scale: torch.Tensor
    dtype: torch.dtype


def quantize_rows(x: torch.Tensor, pad_k: bool = False) -> Fp8Rows:
    """``quant_rows_fp8`` over the rows of any x [..., K] (same errors).
    ``pad_k``: ``quant_rows_fp8_pad`` instead, K % 64 == 0; the rows' ``q`` is
    [..., fp8_padded_k(K)] and goes with a weight padded alike."""
    if x.dim() < 1:
        raise ValueError("x must be [..., K]")
    quant = quant_rows_fp8_pad if pad_k else quant_rows_fp8
    q, scale = quant(x.reshape(-1, x.shape[-1]))
    return Fp8Rows(q.reshape(*x.shape[:-1], q.shape[-1]),
                   scale.reshape(x.shape[:-1]), x.dtype)


def layer_norm_fp8(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                   eps: float = 1e-5) -> Fp8Rows:
    """``quantize_rows(layer_norm(x, weight, bias, eps), pad_k=True)``, by
    definition: the rows an FP8 Linear makes of the affine LayerNorm's output,
    made by the norm. C % 64 == 0 (the padded quantiser's contract).

    GPU: one norms.hip launch for bf16 x with C <= 2048. The kernel rounds the
    affine result to bf16 in registers and quantises that, so the bytes and
    the scales are those of the two launches. Everything else runs the two
    steps."""
    c = x.shape[-1]
    if not fp8_pad_shape_supported(c):
        raise ValueError(
            f"C = {c} unsupported (multiple of 64, <= {FP8_MAX_K})")
    if _on_gpu(x) and x.dtype == torch.bfloat16 and c <= 2048:
        q, s = ext.get_ext(True).layer_norm_fp8(
            x.contiguous(), _f32(weight), _f32(bias), eps)
        return Fp8Rows(q, s, x.dtype)
    return quantize_rows(layer_norm(x, weight, bias, eps), pad_k=True)


def norm_modulate_fp8(
    x: torch.Tensor,
    mode: str,
    weight: torch.Tensor | None = None,
    scale: torch.Tensor | None = None,
    shift: torch.Tensor | None = None,
    eps: float | None = None,
) -> Fp8Rows:
    """``quantize_rows(norm_modulate(x, ...))``, by definition: the rows an
    FP8 Linear makes of the norm's output, made by the norm. Arguments as
    ``norm_modulate``; C must be in the FP8 contract (``fp8_shape_supported``).

    GPU: one dit_ops.hip launch for bf16 x [B, N, C] with C <= 8192 and
    scale/shift of exactly [B, C]. The kernel rounds the modulated value to
    bf16 in registers and quantises that, so the bytes and the scales are
    those of the two launches. Everything else (CPU, ``DISTGPU_DIT_FUSED=0``,
    C up to 16384, other ranks) runs the two steps."""
    eps = _norm_modulate_eps(mode, weight, scale, shift, eps)
    c = x.shape[-1]
    if not fp8_shape_supported(c):
        raise ValueError(
            f"C = {c} unsupported (multiple of 128, <= {FP8_MAX_K})")
    covered = (
        x.dim() == 3 and c <= 8192
        and all(m is None or m.shape == (x.shape[0], c)
                for m in (scale, shift)))
    if covered and _dit_fused(x, scale, shift):
        q, s = ext.get_ext(True).norm_modulate_fp8(
            *_norm_modulate_operands(x, weight, scale, shift), eps)
        return Fp8Rows(q, s, x.dtype)
    return quantize_rows(norm_modulate(x, mode, weight, scale, shift, eps))


def gemm_fp8(qa: torch.Tensor, sa: torch.Tensor, qw: torch.Tensor,
             sw: torch.Tensor, bias: torch.Tensor | None = None,
             act: str | None = None) -> torch.Tensor:
    """act((qa . qw^T) * sa[:, None] * sw[None] + bias). qa [M, K], qw [N, K]
    float8_e4m3fn; sa [M], sw [N] fp32. GPU: the block-scaled-MFMA kernel,
    bf16 out. CPU: fp32 matmul of the dequantised operands, fp32 out."""
    if act not in _FP8_ACTS:
        raise ValueError(f"act {act!r} is not one of {list(_FP8_ACTS)}")
    if qa.shape[-1] != qw.shape[-1] or qa.shape[-1] % 128:
        raise ValueError(
            f"qa {tuple(qa.shape)} / qw {tuple(qw.shape)}: K must agree and "
            "be a multiple of 128")
    if _on_gpu(qa):
        # no cached fp32 copy of the bias (a cache could go stale): Fp8Linear
        # keeps its bias in fp32, anything else is cast per call
        b = (bias.float() if bias is not None
             else torch.empty(0, device=qa.device))
        return ext.get_ext(True).gemm_fp8(
            qa.contiguous(), sa.contiguous(), qw.contiguous(),
            sw.contiguous(), b, _FP8_ACTS[act])
    y = (qa.float() @ qw.float().t()) * sa[:, None] * sw[None, :]
    if bias is not None:
        y = y + bias.float()
    if _FP8_ACTS[act] == 1:
        y = F.silu(y)
    elif _FP8_ACTS[act] == 2:
        y = F.gelu(y, approximate="tanh")
    return y


def linear_fp8(x: "torch.Tensor | Fp8Rows | MxRows", qw: torch.Tensor,
               sw: torch.Tensor, bias: torch.Tensor | None = None,
               act: str | None = None, emit: str | None = None):
    """Linear with an FP8 weight: x [..., K] -> [..., N] in x.dtype. The rows
    of x are quantised per call (absmax / 448), the product runs on e4m3
    operands with fp32 accumulation, and ``act`` (None, "silu", "gelu_tanh")
    is fused after the bias. An :class:`Fp8Rows` in place of x holds rows
    that are quantised already: no quantiser runs, only the GEMM.

    An :class:`MxRows` in place of x runs ``gemm_mxfp8`` on its block-scaled
    rows. ``emit="mx"`` returns the result as ``MxRows`` (N % 32 == 0), by
    definition ``quantize_rows_mx`` of the bf16 result, made by the GEMM
    epilogue; its input is an ``MxRows`` or a tensor, which is then quantised
    with ``quant_rows_mxfp8`` (the MX GEMM has no per-row scale, so an
    ``Fp8Rows`` cannot feed it).

    GPU: quant_rows_fp8 + gemm_fp8 (gemm_fp8.hip), bf16 x only. CPU: the same
    quantised operands, dequantised fp32 matmul. K % 128 != 0, K > 16384 or
    a non-bf16 input on GPU raise ValueError: the fallback for such layers is
    decided at module conversion (models/quant.py), not here."""
    if emit not in (None, "mx"):
        raise ValueError(f"emit {emit!r} is not None or 'mx'")
    rows = x if isinstance(x, (Fp8Rows, MxRows)) else None
    k = (rows.q if rows is not None else x).shape[-1]
    if qw.dim() != 2 or qw.shape[1] != k:
        raise ValueError(
            f"x [..., {k}] does not match qw {tuple(qw.shape)}")
    if not fp8_shape_supported(k):
        raise ValueError(
            f"K = {k} unsupported (multiple of 128, <= {FP8_MAX_K})")
    if rows is None and _on_gpu(x) and x.dtype != torch.bfloat16:
        raise ValueError(f"linear_fp8 on GPU takes bf16, got {x.dtype}")
    if emit == "mx" or isinstance(rows, MxRows):
        if isinstance(rows, Fp8Rows):
            raise ValueError(
                "emit='mx' takes a tensor or MxRows: rows with a per-row "
                "scale do not go through the MX GEMM")
        if rows is None:
            rows = quantize_rows_mx(x)
        lead, n = rows.q.shape[:-1], qw.shape[0]
        out = gemm_mxfp8(rows.q.reshape(-1, k), rows.e.reshape(-1, k // 32),
                         qw, sw, bias, act, emit=emit == "mx")
        if emit == "mx":
            return MxRows(out[0].reshape(*lead, n),
                          out[1].reshape(*lead, n // 32), rows.dtype)
        return out.to(rows.dtype).reshape(*lead, n)
    if rows is not None:
        y = gemm_fp8(rows.q.reshape(-1, k), rows.scale.reshape(-1), qw, sw,
                     bias, act)
        return y.to(rows.dtype).reshape(*rows.q.shape[:-1], qw.shape[0])
    x2 = x.reshape(-1, k)
    qa, sa = quant_rows_fp8(x2)
    y = gemm_fp8(qa, sa, qw, sw, bias, act)
    return y.to(x.dtype).reshape(*x.shape[:-1], qw.shape[0])


def pack_geglu_weight_fp8(weight: torch.Tensor, bias: torch.Tensor | None,
                          pad_k: bool = False
                          ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """weight [2*inner, K], bias [2*inner] or None of a GEGLU projection ->
    (qw, sw, bias) as ``gemm_geglu_fp8`` reads them: quantised per output
    channel (``quantize_weight_fp8``), then rows, scales and bias paired by
    ``pack_geglu_weight``. bias comes back fp32, empty without one."""
    qw, sw = quantize_weight_fp8(weight, pad_k)
    packed, bias_p = pack_geglu_weight(qw.view(torch.uint8), bias)
    sw_p, _ = pack_geglu_weight(sw[:, None])
    return packed.view(torch.float8_e4m3fn), sw_p.reshape(-1), bias_p


def gemm_geglu_fp8(qa: torch.Tensor, sa: torch.Tensor, qw: torch.Tensor,
                   sw: torch.Tensor, bias: torch.Tensor | None = None
                   ) -> torch.Tensor:
    """``(a * sa * sw_a + b_a) * gelu_tanh(g * sa * sw_g + b_g)`` with a, g
    the value and gate products ``qa . qw^T`` of one output column. qa [M, K],
    qw [2*inner, K] float8_e4m3fn, sw and bias [2*inner] fp32, all three in
    ``pack_geglu_weight_fp8``'s pairing; inner % 16 == 0 -> [M, inner]. GPU:
    one launch of the FP8 GEMM with the GEGLU epilogue (gemm_fp8.hip), fp32
    throughout, one rounding, bf16 out; the [M, 2*inner] projection is never
    written. CPU: fp32 matmul of the dequantised operands, fp32 out."""
    if qw.dim() != 2 or qw.shape[0] % 32:
        raise ValueError(
            f"qw must be [2*inner, K] with inner % 16 == 0, got "
            f"{tuple(qw.shape)}")
    if qa.shape[-1] != qw.shape[-1] or qa.shape[-1] % 128:
        raise ValueError(
            f"qa {tuple(qa.shape)} / qw {tuple(qw.shape)}: K must agree and "
            "be a multiple of 128")
    if bias is not None and bias.numel() == 0:
        bias = None
    if _on_gpu(qa):
        b = (bias.float() if bias is not None
             else torch.empty(0, device=qa.device))
        return ext.get_ext(True).gemm_geglu_fp8(
            qa.contiguous(), sa.contiguous(), qw.contiguous(),
            sw.contiguous(), b)
    y = (qa.float() @ qw.float().t()) * sa[:, None] * sw[None, :]
    if bias is not None:
        y = y + bias.float()
    y = y.reshape(y.shape[0], -1, 2, 16)  # [M, inner/16, value | gate, 16]
    out = y[:, :, 0] * F.gelu(y[:, :, 1], approximate="tanh")
    return out.reshape(out.shape[0], -1)


def linear_geglu_fp8(x: torch.Tensor | Fp8Rows, qw: torch.Tensor,
                     sw: torch.Tensor, bias: torch.Tensor | None = None
                     ) -> torch.Tensor:
    """GEGLU projection with an FP8 weight: x [..., K] -> [..., inner] in
    x.dtype, ``gemm_geglu_fp8`` over the rows of x. qw [2*inner, Kp], sw and
    bias from ``pack_geglu_weight_fp8``. A tensor x is quantised here, with
    the padded quantiser when Kp != K; an :class:`Fp8Rows` is used as it is."""
    rows = x if isinstance(x, Fp8Rows) else None
    if rows is None:
        k = x.shape[-1]
        if qw.dim() != 2 or qw.shape[1] != fp8_padded_k(k):
            raise ValueError(
                f"x [..., {k}] does not match qw {tuple(qw.shape)}")
        if _on_gpu(x) and x.dtype != torch.bfloat16:
            raise ValueError(
                f"linear_geglu_fp8 on GPU takes bf16, got {x.dtype}")
        rows = quantize_rows(x, pad_k=k % 128 != 0)
    kp = rows.q.shape[-1]
    y = gemm_geglu_fp8(rows.q.reshape(-1, kp), rows.scale.reshape(-1), qw, sw,
                       bias)
    return y.to(rows.dtype).reshape(*rows.q.shape[:-1], qw.shape[0] // 2)


# ---------------------------------------------------------------------------
# FP8 (e4m3fn) conv: per-channel weights, one activation scale per image
# ---------------------------------------------------------------------------

# Shapes that stay on the bf16 kernel under the FP8 route because quantiser +
# conv_fp8 did not measure ahead of conv256_nhwc there
# (profiles/r25_conv_fp8.md, `tools/kernel_bench.py --op conv_fp8`, tile batch
# 32). A row is (C, K_out, H, W, stride), with quantiser + conv over the bf16
# time. The kernel has no K split, so the levels whose grid is a fraction of a
# round of the 256 CUs lose to the bf16 kernel's split; at the stride-2 convs
# the quantiser reads four times the pixels the conv writes.
_CONV_FP8_LOSSES: tuple = (
    (320, 4, 68, 68, 1),        # out conv, one masked N-block: 1.07
    (1280, 1280, 9, 9, 1),      # 9x9 level and mid block: 1.85
    (2560, 1280, 9, 9, 1),      # 1.94
    (320, 320, 68, 68, 2),      # 68 -> 34 downsample: 1.03
    (640, 640, 34, 34, 2),      # 34 -> 17: 1.32
    (1280, 1280, 17, 17, 2),    # 17 -> 9: 1.84
)


def conv_fp8_route(c: int, k_out: int, h: int, w: int, stride: int) -> bool:
    """Whether a marked conv of this shape takes the FP8 kernel. Table lookup,
    no launch."""
    return (c, k_out, h, w, stride) not in _CONV_FP8_LOSSES


def quant_nhwc_fp8(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """x [B, H, W, C] -> (q [B, H, W, C] float8_e4m3fn, scale [B] fp32): one
    scale per image, ``max(amax, 2^-126 * 448) * (1/448)`` over the image, and
    q = rne_e4m3(clamp(x * (1 / max(scale, 2^-126)), +-448)), each step one
    fp32 operation. GPU: the conv_fp8.hip quantiser (bf16 input, C % 8 == 0).
    CPU: the same operations in torch, so both give the same bytes."""
    if x.dim() != 4:
        raise ValueError(f"x must be [B, H, W, C], got {tuple(x.shape)}")
    if _on_gpu(x):
        if x.dtype != torch.bfloat16:
            raise ValueError(f"the FP8 quantiser takes bf16, got {x.dtype}")
        if x.shape[3] % 8:
            raise ValueError(f"C = {x.shape[3]} is not a multiple of 8")
        return ext.get_ext(True).quant_nhwc_fp8(x.contiguous())
    scale = _fp8_scale(x.float().abs().amax(dim=(1, 2, 3)))
    inv = 1.0 / scale.clamp_min(2.0 ** -126)
    q = (x.float() * inv[:, None, None, None]).clamp(-E4M3_MAX, E4M3_MAX)
    return q.to(torch.float8_e4m3fn), scale


def quantize_conv_weight_fp8(conv) -> tuple[torch.Tensor, torch.Tensor]:
    """(qw [K_out, Kp] float8_e4m3fn, sw [K_out] fp32) of a 3x3 / 1x1
    nn.Conv2d: ``_repacked_weight``'s [K_out, RS*C] matrix (c innermost)
    through ``quantize_weight_fp8``, rows zero-padded to Kp = RS*C rounded up
    to 128. Cached on the module with the weight's ``_version`` and refreshed
    into the same tensors after an in-place update, like ``_repacked_weight``.
    A module that carries this pack is one ``conv2d_mfma`` routes to the FP8
    kernel."""
    ver = _versions(conv.weight)
    pack = getattr(conv, "_distgpu_fp8", None)
    live = pack is not None and pack[0].device == conv.weight.device
    if live and getattr(conv, "_distgpu_fp8_ver", None) == ver:
        return pack
    qw, sw = quantize_weight_fp8(_repacked_weight(conv), pad_k=True)
    if live and pack[0].shape == qw.shape:
        pack[0].view(torch.uint8).copy_(qw.view(torch.uint8))
        pack[1].copy_(sw)
    else:
        pack = (qw, sw)
        conv._distgpu_fp8 = pack
    conv._distgpu_fp8_ver = ver
    return pack


def conv_fp8(q: torch.Tensor, scale: torch.Tensor, qw: torch.Tensor,
             sw: torch.Tensor, bias: torch.Tensor | None = None, *,
             rs: int = 9, stride: int = 1, fuse_silu: bool = False,
             residual: torch.Tensor | None = None, bn: int = 0
             ) -> torch.Tensor:
    """act(conv(q, qw) * scale[b] * sw[n] + bias[n]) + residual -> bf16
    [B, Ho, Wo, K_out], NHWC throughout. q [B, H, W, C] float8_e4m3fn with
    C % 64 == 0 and scale [B] from ``quant_nhwc_fp8``; qw [K_out, Kp], sw
    [K_out] from ``quantize_conv_weight_fp8`` (k = tap * C + c, Kp = rs * C
    rounded up to 128); ``rs`` 9 (3x3, pad 1, stride 1 or 2) or 1 (1x1); act
    is SiLU or none; ``residual`` is bf16 of the output's shape. ``bn`` pins
    the kernel's N-tile width (256 / 320) on the GPU.

    GPU: conv_fp8_kernel (conv_fp8.hip). CPU: ``F.conv2d`` in fp32 on the
    dequantised operands, then the scales, bias, act and residual in fp32 and
    one rounding to bf16."""
    if q.dim() != 4 or qw.dim() != 2:
        raise ValueError(
            f"q {tuple(q.shape)} / qw {tuple(qw.shape)}: want [B, H, W, C] "
            "and [K_out, Kp]")
    b, h, w, c = q.shape
    k_out = qw.shape[0]
    if rs not in (9, 1) or stride not in (1, 2) or (stride == 2 and rs == 1):
        raise ValueError(f"rs {rs} / stride {stride}: 3x3 stride 1 or 2, or 1x1")
    if c % 64 or qw.shape[1] != fp8_padded_k(rs * c):
        raise ValueError(
            f"C = {c} must be a multiple of 64 and qw [K_out, "
            f"{fp8_padded_k(rs * c)}], got {tuple(qw.shape)}")
    if _on_gpu(q):
        e = ext.get_ext(True)
        bias_t = (bias.float() if bias is not None
                  else torch.empty(0, device=q.device))
        res = (residual.contiguous() if residual is not None
               else torch.empty(0, device=q.device, dtype=torch.bfloat16))
        return e.conv_fp8_nhwc_ex(
            q.contiguous(), scale.contiguous(), qw.contiguous(),
            sw.contiguous(), bias_t, res, b, h, w, c, k_out, rs, stride,
            fuse_silu, bn)
    r = 3 if rs == 9 else 1
    wt = qw[:, :rs * c].float().reshape(k_out, r, r, c).permute(0, 3, 1, 2)
    y = F.conv2d(q.float().permute(0, 3, 1, 2), wt, stride=stride,
                 padding=r // 2)
    y = y * scale.float()[:, None, None, None] * sw.float()[None, :, None, None]
    if bias is not None:
        y = y + bias.float()[None, :, None, None]
    if fuse_silu:
        y = F.silu(y)
    y = y.permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual.float()
    return y.to(torch.bfloat16).contiguous()


# ---------------------------------------------------------------------------
# MXFP8 activation rows: e4m3 codes, one E8M0 scale per 32 adjacent elements
# ---------------------------------------------------------------------------

@dataclass(frozen=True, eq=False)
class MxRows:
    """Activation rows in the OCP MXFP8 format, on their way from a producer
    to an FP8 Linear. ``q``: [..., K] float8_e4m3fn, contiguous, K % 128 == 0;
    ``e``: [..., K/32] uint8, the E8M0 byte ``exp + 127`` of each block of 32
    adjacent elements (block value = code * 2^exp); ``dtype``: what the
    consuming Linear returns. ``linear_fp8`` takes one in place of ``x``."""

    q: torch.Tensor
    e: torch.Tensor
    dtype: torch.dtype


def _mx_quant(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The format's definition, x [M, K]. Block exponent from the fp32 bits
    of the block absmax ``m * 2^E``: exp = E - 8 for m <= 1.75, else E - 7,
    the smallest power of two with absmax * 2^-exp <= 448; as a byte,
    clamp(biased exponent - 8 + (mantissa > 0.75), 0, 254). Codes:
    e4m3(clamp(x * 2^-exp, +-448)), where 2^-exp = 2^(127 - byte) is built
    from its bits. The kernels do the same integer steps."""
    m, k = x.shape
    xb = x.float().reshape(m, k // 32, 32)
    bits = xb.abs().amax(dim=-1).view(torch.int32)
    byte = ((bits >> 23) - 8 + ((bits & 0x7FFFFF) > 0x600000).int()).clamp(0, 254)
    inv = ((254 - byte) << 23).view(torch.float32)
    q = (xb * inv[..., None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q.reshape(m, k), byte.to(torch.uint8)


def mx_dequant(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """fp32 values of MX rows: code * 2^(e - 127) per block of 32."""
    v = q.float().reshape(*e.shape, 32)
    return torch.ldexp(v, (e.int() - 127)[..., None]).reshape(q.shape)


def quant_rows_mxfp8(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """x [M, K] -> (q [M, K] float8_e4m3fn, e [M, K/32] uint8), one
    power-of-two scale per 32 adjacent elements (``_mx_quant``). GPU: the
    one-pass gemm_mxfp8.hip quantiser (bf16 input). CPU: the definition."""
    if x.dim() != 2:
        raise ValueError(f"x must be [M, K], got {tuple(x.shape)}")
    if not fp8_shape_supported(x.shape[1]):
        raise ValueError(
            f"K = {x.shape[1]} unsupported (multiple of 128, <= {FP8_MAX_K})")
    if _on_gpu(x):
        if x.dtype != torch.bfloat16:
            raise ValueError(f"the FP8 quantiser takes bf16, got {x.dtype}")
        return ext.get_ext(True).quant_rows_mxfp8(x.contiguous())
    return _mx_quant(x)


def quantize_rows_mx(x: torch.Tensor) -> MxRows:
    """``quant_rows_mxfp8`` over the rows of any x [..., K] (same errors)."""
    if x.dim() < 1:
        raise ValueError("x must be [..., K]")
    q, e = quant_rows_mxfp8(x.reshape(-1, x.shape[-1]))
    return MxRows(q.reshape(x.shape), e.reshape(*x.shape[:-1], -1), x.dtype)


def gemm_mxfp8(qa: torch.Tensor, ea: torch.Tensor, qw: torch.Tensor,
               sw: torch.Tensor, bias: torch.Tensor | None = None,
               act: str | None = None, emit: bool = False):
    """act((sum_kb 2^exp[m][kb] * dot32(qa[m][kb], qw[n][kb])) * sw[n] +
    bias[n]). qa [M, K], qw [N, K] float8_e4m3fn; ea [M, K/32] uint8 E8M0;
    sw [N] fp32. ``emit``: return (q [M, N], e [M, N/32]), the MX rows of the
    result rounded to bf16 (N % 32 == 0), instead of the result. GPU: the
    block-scaled-MFMA kernel of gemm_mxfp8.hip, the scales applied by the
    matrix unit and, with ``emit``, the quantiser in the epilogue; bf16 out.
    CPU: fp32 matmul of the dequantised operands, fp32 out."""
    if act not in _FP8_ACTS:
        raise ValueError(f"act {act!r} is not one of {list(_FP8_ACTS)}")
    k = qa.shape[-1]
    if k != qw.shape[-1] or k % 128 or ea.shape != (qa.shape[0], k // 32):
        raise ValueError(
            f"qa {tuple(qa.shape)} / ea {tuple(ea.shape)} / qw "
            f"{tuple(qw.shape)}: K must agree, be a multiple of 128, and ea "
            "be [M, K/32]")
    if emit and qw.shape[0] % 32:
        raise ValueError(f"emit: N = {qw.shape[0]} is not a multiple of 32")
    if _on_gpu(qa):
        b = (bias.float() if bias is not None
             else torch.empty(0, device=qa.device))
        fn = (ext.get_ext(True).gemm_mxfp8_emit if emit
              else ext.get_ext(True).gemm_mxfp8)
        return fn(qa.contiguous(), ea.contiguous(), qw.contiguous(),
                  sw.contiguous(), b, _FP8_ACTS[act])
    y = (mx_dequant(qa, ea) @ qw.float().t()) * sw[None, :]
    if bias is not None:
        y = y + bias.float()
    if _FP8_ACTS[act] == 1:
        y = F.silu(y)
    elif _FP8_ACTS[act] == 2:
        y = F.gelu(y, approximate="tanh")
    return _mx_quant(y.to(torch.bfloat16)) if emit else y


# ---------------------------------------------------------------------------
# FP8 (e4m3fn) attention for head dim 128: quantised QK^T and PV
# ---------------------------------------------------------------------------

ATTN_FP8_D = 128
ATTN_FP8_KT = 128      # keys per tile of the kernel, and per K scale
ATTN_FP8_QROWS = 256   # q rows per workgroup: the q-block of an AttnBlocks
ATTN_FP8_CHUNK = 64    # keys per partial of the quantiser's column pass
# attn_fp8_kernel's power-of-two P scale: p' = e4m3(2^SP * p). With its
# defer-max threshold of 2 (log2 units) p' stays <= 256 < 448.
ATTN_FP8_SP = 6


def _attn_fp8_quant(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """rne_e4m3(clamp(x * (1 / scale), +-448)), scale broadcast against x: the
    kernels' operations, in their order (a reciprocal, then a multiply)."""
    inv = 1.0 / scale.clamp_min(2.0 ** -126)
    return (x * inv).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)


def _attn_tile_perm(device) -> torch.Tensor:
    """Position -> key inside a 128-key V^T tile (its own inverse): position
    64a + 16g + 4f + r holds key 64a + 16f + 4g + r."""
    i = torch.arange(ATTN_FP8_KT, device=device)
    return (i & 0x43) | ((i & 0x30) >> 2) | ((i & 0x0c) << 2)


def _attn_col_sum(k: torch.Tensor) -> torch.Tensor:
    """fp32 sum over the keys of k [B, N, C] in the order of the quantiser's
    column pass: the keys of a 64-key chunk one after the other, then the
    chunk sums one after the other."""
    b, n, c = k.shape
    nch = -(-n // ATTN_FP8_CHUNK)
    kp = F.pad(k, (0, 0, 0, nch * ATTN_FP8_CHUNK - n)).reshape(
        b, nch, ATTN_FP8_CHUNK, c)
    acc = torch.zeros(b, nch, c, dtype=torch.float32, device=k.device)
    for i in range(ATTN_FP8_CHUNK):
        acc = acc + kp[:, :, i]
    tot = torch.zeros(b, c, dtype=torch.float32, device=k.device)
    for j in range(nch):
        tot = tot + acc[:, j]
    return tot


@dataclass
class AttnFp8:
    """Quantised operands of ``attention_fp8`` (``quantize_attn_qkv``), D = 128,
    Np = Nk rounded up to 128 with zero codes behind Nk.

    ``q`` [B, Nq, H*D] e4m3, ``q_scale`` [B, Nq, H]; ``k`` [B, H, Np, D] e4m3 of
    K minus ``k_mean`` [B, H*D], ``k_scale`` [B, H, Np/128]; ``v`` [B, H, D, Np]
    e4m3, transposed, position 64a + 16g + 4f + r of each 128-key tile holding
    key 64a + 16f + 4g + r (the order of the kernel's P operand), ``v_scale``
    [B, H, D]. ``dtype`` is the dtype ``attention_fp8`` returns."""
    q: torch.Tensor
    q_scale: torch.Tensor
    k: torch.Tensor
    k_scale: torch.Tensor
    v: torch.Tensor
    v_scale: torch.Tensor
    k_mean: torch.Tensor
    nk: int
    dtype: torch.dtype

    @property
    def heads(self) -> int:
        return self.k.shape[1]

    def v_codes(self) -> torch.Tensor:
        """fp32 V codes in key order, [B, H, Nk, D]."""
        b, h, d, np_ = self.v.shape
        v = self.v.float().reshape(b, h, d, np_ // ATTN_FP8_KT, ATTN_FP8_KT)
        v = v[..., _attn_tile_perm(v.device)].reshape(b, h, d, np_)
        return v[..., :self.nk].transpose(2, 3)

    def dequant(self) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """fp32 (q [B, Nq, H*D], k, v [B, Nk, H*D]) the codes stand for; k is
        K with its per-(batch, head, channel) mean over the keys removed."""
        b, nq, hd = self.q.shape
        h, d = self.heads, ATTN_FP8_D
        q = (self.q.float().reshape(b, nq, h, d)
             * self.q_scale[..., None]).reshape(b, nq, hd)
        ks = self.k_scale.repeat_interleave(ATTN_FP8_KT, dim=2)[..., None]
        k = (self.k.float() * ks)[:, :, :self.nk]
        v = self.v_codes() * self.v_scale[:, :, None, :]

        def pack(u):
            return u.permute(0, 2, 1, 3).reshape(b, self.nk, hd)

        return q, pack(k), pack(v)


def _attn_fp8_check(q, k, v, heads: int) -> None:
    if q.dim() != 3 or k.dim() != 3 or k.shape != v.shape \
            or q.shape[0] != k.shape[0]:
        raise ValueError(
            f"attention_fp8 takes q [B, Nq, H*D] and k, v [B, Nk, H*D], got "
            f"{tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    if q.shape[1] < 1 or k.shape[1] < 1:
        raise ValueError("attention_fp8 needs at least one query and one key")
    if q.shape[2] != heads * ATTN_FP8_D:
        raise ValueError(
            f"attention_fp8 is built for head dim {ATTN_FP8_D}: q has "
            f"{q.shape[2]} channels for {heads} heads")
    if k.shape[2] != q.shape[2]:
        raise ValueError(
            f"attention_fp8 needs kv_heads == heads: k has {k.shape[2]} "
            f"channels, q {q.shape[2]}")


def quantize_attn_qkv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                      heads: int) -> AttnFp8:
    """q [B, Nq, H*128], k, v [B, Nk, H*128] -> :class:`AttnFp8`.

    Q: one scale per (batch, token, head), absmax over D. K: the fp32 mean
    over the keys of every (batch, head, channel) is subtracted first (softmax
    does not change; channel offsets no longer use up e4m3's range), then one
    scale per (batch, head, block of 128 keys). V: one scale per (batch,
    head, channel), absmax over the keys. All scales through ``_fp8_scale``;
    code = e4m3(clamp(x * (1 / scale), +-448)).

    The mean is sum * fp32(1 / Nk), the sum taken in fp32 in the order of
    ``_attn_col_sum``, which is the GPU quantiser's, so both give the same
    bits. GPU: the quantiser kernels of attention_fp8.hip (bf16 inputs)."""
    _attn_fp8_check(q, k, v, heads)
    b, nq, hd = q.shape
    nk, d = k.shape[1], ATTN_FP8_D
    if _on_gpu(q, k, v):
        if not all(t.dtype == torch.bfloat16 for t in (q, k, v)):
            raise ValueError(
                f"the FP8 attention quantiser takes bf16 on GPU, got "
                f"{q.dtype}, {k.dtype}, {v.dtype}")
        qq, qs, kc, ks, vc, vs, km = ext.get_ext(True).attn_quant_fp8(
            q.contiguous(), k.contiguous(), v.contiguous(), heads)
        return AttnFp8(qq, qs, kc, ks, vc, vs, km, nk, q.dtype)
    np_ = -(-nk // ATTN_FP8_KT) * ATTN_FP8_KT
    qf = q.float().reshape(b, nq, heads, d)
    q_scale = _fp8_scale(qf.abs().amax(dim=-1))
    q_codes = _attn_fp8_quant(qf, q_scale[..., None]).reshape(b, nq, hd)

    kf = k.float()
    k_mean = _attn_col_sum(kf) * torch.tensor(1.0 / nk, dtype=torch.float32)
    kc = (kf - k_mean[:, None]).reshape(b, nk, heads, d).permute(0, 2, 1, 3)
    kc = F.pad(kc, (0, 0, 0, np_ - nk))                   # [B, H, Np, D]
    k_scale = _fp8_scale(
        kc.reshape(b, heads, np_ // ATTN_FP8_KT, -1).abs().amax(dim=-1))
    k_codes = _attn_fp8_quant(
        kc, k_scale.repeat_interleave(ATTN_FP8_KT, dim=2)[..., None])

    vf = v.float().reshape(b, nk, heads, d).permute(0, 2, 3, 1)  # [B, H, D, Nk]
    v_scale = _fp8_scale(vf.abs().amax(dim=-1))
    vc = _attn_fp8_quant(F.pad(vf, (0, np_ - nk)), v_scale[..., None])
    vc = vc.view(torch.uint8).reshape(b, heads, d, -1, ATTN_FP8_KT)
    v_codes = vc[..., _attn_tile_perm(vc.device)].reshape(
        b, heads, d, np_).contiguous().view(torch.float8_e4m3fn)
    return AttnFp8(q_codes, q_scale, k_codes.contiguous(), k_scale, v_codes,
                   v_scale, k_mean, nk, q.dtype)


@dataclass
class AttnBlocks:
    """Block lists of ``attention_fp8(blocks=)`` for one geometry: which
    128-key tiles each q-block of 256 query rows attends to, shared by every
    batch and head. ``mask`` CPU bool [nqb, nkt]; ``idx`` int32 [nqb, maxc] on
    the device, row i the ascending allowed tiles of q-block i, padded with
    its last entry; ``cnt`` int32 [nqb] their number; ``density`` = allowed
    blocks / all blocks. Built by ``attn_blocks``."""
    mask: torch.Tensor
    idx: torch.Tensor
    cnt: torch.Tensor
    density: float


def attn_blocks(mask: torch.Tensor, device="cpu") -> AttnBlocks:
    """bool ``mask`` [nqb, nkt] -> :class:`AttnBlocks` with its lists on
    ``device``. Every q-block must be allowed at least one tile (a softmax
    over no keys is not defined). The kernel does not see the values of the
    lists: this is where they are made valid."""
    if mask.dim() != 2 or mask.dtype != torch.bool or 0 in mask.shape:
        raise ValueError(
            f"attn_blocks takes a bool mask [q-blocks, key tiles], got "
            f"{mask.dtype} {tuple(mask.shape)}")
    mask = mask.cpu()
    cnt = mask.sum(dim=1)
    if int(cnt.min()) < 1:
        raise ValueError(
            f"q-block {int(cnt.argmin())} of the mask has no allowed key tile")
    nkt = mask.shape[1]
    # allowed tiles first, in ascending order (a stable sort of "not allowed")
    order = torch.sort((~mask).to(torch.uint8), dim=1, stable=True).indices
    order = order[:, :int(cnt.max())]
    last = order.gather(1, (cnt - 1)[:, None])
    pos = torch.arange(order.shape[1])[None]
    idx = torch.where(pos < cnt[:, None], order, last)
    assert int(idx.min()) >= 0 and int(idx.max()) < nkt
    return AttnBlocks(mask, idx.to(torch.int32).contiguous().to(device),
                      cnt.to(torch.int32).to(device),
                      float(mask.sum()) / mask.numel())


@lru_cache(maxsize=16)
def _attn_window(grid, tile, radius, device):
    n_tok = grid[0] * grid[1] * grid[2]
    coords = torch.meshgrid(*(torch.arange(n) // t for n, t in zip(grid, tile)),
                            indexing="ij")
    ntile = [-(-n // t) for n, t in zip(grid, tile)]
    tile_of = ((coords[0] * ntile[1] + coords[1]) * ntile[2]
               + coords[2]).reshape(n_tok)
    perm = torch.sort(tile_of, stable=True).indices
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n_tok)

    def axis(n, r):   # [n, n]: tile c sees tile c' along one axis
        c = torch.arange(n)
        if n <= 2 * r + 1:
            return torch.ones(n, n, dtype=torch.bool)
        return (c.clamp(r, n - 1 - r)[:, None] - c[None]).abs() <= r

    vt, vh, vw = (axis(n, r) for n, r in zip(ntile, radius))
    nt = ntile[0] * ntile[1] * ntile[2]
    sees = (vt[:, None, None, :, None, None] & vh[None, :, None, None, :, None]
            & vw[None, None, :, None, None, :]).reshape(nt, nt)

    def members(rows):   # [blocks of `rows` permuted tokens, tiles] 0 / 1
        blk = torch.arange(n_tok) // rows
        m = torch.zeros(int(blk[-1]) + 1, nt)
        m[blk, tile_of[perm]] = 1.0
        return m

    mask = members(ATTN_FP8_QROWS) @ sees.float() \
        @ members(ATTN_FP8_KT).T > 0
    return perm.to(device), inv.to(device), attn_blocks(mask, device)


def attn_window(grid, tile, radius, device="cpu"):
    """Sliding-tile window for self-attention over a ``grid`` = (T, H, W) of
    tokens in raster order -> (perm, inv, :class:`AttnBlocks`).

    Tokens are grouped into tiles of ``tile`` = (tt, th, tw) tokens, ragged at
    the far edges. ``perm`` lists the raster indices in tile-major order
    (tiles in raster order, raster order inside a tile): ``x[:, perm]`` is
    the sequence the block lists are for, and ``y[:, inv]`` brings a result
    back. Query tile c sees key tile c' iff along every axis
    ``|clamp(c, r, n - 1 - r) - c'| <= r`` with ``radius`` = (rt, rh, rw): the
    centre is clamped, so edge tiles keep a full-size window, and an axis of
    n <= 2r + 1 tiles sees everything. A block (256 permuted queries, 128
    permuted keys) is allowed iff some query and some key of it see each
    other: the mask is block-granular, and allowed blocks count whole. Pure
    torch on the CPU, cached per argument tuple."""
    grid, tile, radius = (tuple(int(x) for x in t) for t in (grid, tile, radius))
    if not (len(grid) == len(tile) == len(radius) == 3) or min(grid) < 1 \
            or min(tile) < 1 or min(radius) < 0:
        raise ValueError(
            f"attn_window takes a grid and a tile of three sizes >= 1 and "
            f"three radii >= 0, got {grid}, {tile}, {radius}")
    return _attn_window(grid, tile, radius, str(device))


def attention_fp8(q: "torch.Tensor | AttnFp8", k: torch.Tensor | None = None,
                  v: torch.Tensor | None = None, heads: int | None = None,
                  scale: float | None = None,
                  blocks: AttnBlocks | None = None) -> torch.Tensor:
    """Softmax attention with e4m3 QK^T and PV products, head dim 128: q
    [B, Nq, H*D], k, v [B, Nk, H*D] -> [B, Nq, H*D] in q.dtype. The tensors
    are quantised by ``quantize_attn_qkv``; an :class:`AttnFp8` in place of q
    (k, v and heads left out) is used as it is.

    GPU: attn_fp8_kernel (attention_fp8.hip), bf16 tensors only. CPU, the
    definition: fp32 logits s over ``dequant()``, p = exp(s - rowmax),
    p' = e4m3(2^ATTN_FP8_SP * p), out = (p' @ V codes) / sum(2^SP * p) *
    V scale, the sum over the unrounded weights. The kernel rounds the same
    quantities, but against its running maximum, which may be up to 2 (in
    log2 units) under the row's final one while a tile is processed, so single
    weights can round differently (never by more than e4m3's half ulp).

    ``blocks`` (an :class:`AttnBlocks` whose mask is [ceil(Nq / 256), Np / 128])
    restricts every q-block of 256 rows to its allowed 128-key tiles. GPU:
    attn_fp8_sparse_kernel, which visits only those tiles. Definition: the
    logits of the keys in the other tiles are -inf before the row maximum.
    The operands are quantised as without it (K mean and V scales over all
    keys: a constant vector removed from every key shifts the logits of a row
    equally for any subset of the keys)."""
    if isinstance(q, AttnFp8):
        if k is not None or v is not None:
            raise ValueError("an AttnFp8 already holds k and v")
        a = q
        if heads is not None and heads != a.heads:
            raise ValueError(f"heads {heads} != {a.heads} of the AttnFp8")
    else:
        if k is None or v is None or heads is None:
            raise ValueError("attention_fp8 needs q, k, v and heads")
        _attn_fp8_check(q, k, v, heads)
        a = None
    scale = scale if scale is not None else 1.0 / math.sqrt(ATTN_FP8_D)
    if not scale > 0:
        raise ValueError(f"attention scale must be positive, got {scale}")
    if a is None:
        a = quantize_attn_qkv(q, k, v, heads)
    b, nq, hd = a.q.shape
    if blocks is not None:
        want = (-(-nq // ATTN_FP8_QROWS), a.k.shape[2] // ATTN_FP8_KT)
        if tuple(blocks.mask.shape) != want:
            raise ValueError(
                f"blocks are for {tuple(blocks.mask.shape)} (q-blocks, key "
                f"tiles), the operands have {want}")
    if _on_gpu(a.q):
        if blocks is None:
            o = ext.get_ext(True).attn_fwd_fp8(
                a.q, a.q_scale, a.k, a.k_scale, a.v, a.v_scale, a.nk, scale)
        else:
            o = ext.get_ext(True).attn_fwd_fp8_sparse(
                a.q, a.q_scale, a.k, a.k_scale, a.v, a.v_scale, a.nk, scale,
                blocks.idx, blocks.cnt)
        return o.to(a.dtype)
    h, d = a.heads, ATTN_FP8_D
    qf, kf, _ = a.dequant()
    qh = qf.reshape(b, nq, h, d).permute(0, 2, 1, 3)
    kh = kf.reshape(b, a.nk, h, d).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(2, 3)) * scale
    if blocks is not None:
        allowed = blocks.mask.repeat_interleave(ATTN_FP8_QROWS, dim=0)[:nq] \
            .repeat_interleave(ATTN_FP8_KT, dim=1)[:, :a.nk]
        s = s.masked_fill(~allowed, float("-inf"))
    p = torch.exp(s - s.amax(dim=-1, keepdim=True)) * 2.0 ** ATTN_FP8_SP
    pq = p.to(torch.float8_e4m3fn).float()
    o = (pq @ a.v_codes()) / p.sum(dim=-1, keepdim=True)
    o = o * a.v_scale[:, :, None, :]
    return o.permute(0, 2, 1, 3).reshape(b, nq, hd).to(a.dtype)


# ---------------------------------------------------------------------------
# tile pipeline (Lanczos-3 resample + erf-mask blend)
# ---------------------------------------------------------------------------


def _lanczos3(x: torch.Tensor) -> torch.Tensor:
    ax = x.abs()
    out = torch.where(
        ax < 1e-6,
        torch.ones_like(x),
        torch.sinc(x) * torch.sinc(x / LANCZOS_A),
    )
    return torch.where(ax >= LANCZOS_A, torch.zeros_like(x), out)


def _lanczos_weight_matrix(
    n_out: int, src_lo: float, scale: float, src_size: int
) -> torch.Tensor:
    """Dense [n_out, src_size] weight matrix matching the kernel's per-pixel
    tap enumeration (inclusive [floor(c-s+.5), floor(c+s+.5)], max 16 taps,
    edge clamp, renormalized)."""
    centers = src_lo + (torch.arange(n_out, dtype=torch.float64) + 0.5) * scale - 0.5
    # clamp like the HIP kernel: the full window must fit in 16 taps, or
    # truncation can leave a near-zero weight sum and the renormalization
    # explodes (downscales > 2.5x)
    fscale = min(max(scale, 1.0), (16 - 1) / (2.0 * LANCZOS_A))
    support = LANCZOS_A * fscale
    x0 = torch.floor(centers - support + 0.5)
    x1 = torch.floor(centers + support + 0.5)
    max_taps = min(int((x1 - x0).max().item()) + 1, 16)
    taps = x0[:, None] + torch.arange(max_taps, dtype=torch.float64)[None, :]
    w = _lanczos3(((taps - centers[:, None]) / fscale).float()).double()
    w = torch.where(taps <= x1[:, None], w, torch.zeros_like(w))
    w = w / w.sum(dim=1, keepdim=True).clamp_min(1e-12)
    idx = taps.long().clamp(0, src_size - 1)
    dense = torch.zeros(n_out, src_size, dtype=torch.float64)
    dense.scatter_add_(1, idx, w)
    return dense.float()


def _lanczos_resample_cpu(
    src: torch.Tensor, x1: int, y1: int, x2: int, y2: int, ow: int, oh: int
) -> torch.Tensor:
    """[B,H,W,C] f32 -> [B,oh,ow,C]: separable Lanczos-3 of region."""
    B, H, W, C = src.shape
    wx = _lanczos_weight_matrix(ow, float(x1), (x2 - x1) / ow, W)  # [ow, W]
    wy = _lanczos_weight_matrix(oh, float(y1), (y2 - y1) / oh, H)  # [oh, H]
    t = src.permute(0, 3, 1, 2).reshape(B * C, H, W).float()
    t = torch.einsum("oh,bhw->bow", wy, t)
    t = torch.einsum("pw,bow->bop", wx, t)
    return t.reshape(B, C, oh, ow).permute(0, 2, 3, 1).contiguous()


def extract_resize(
    src: torch.Tensor, region: tuple[int, int, int, int], ow: int, oh: int
) -> torch.Tensor:
    """Crop ``region`` of [B,H,W,C] f32 and Lanczos-3 resample to (ow, oh)."""
    x1, y1, x2, y2 = (int(r) for r in region)
    if _on_gpu(src):
        return ext.get_ext(True).extract_resize(src.float(), x1, y1, x2, y2, ow, oh)
    return _lanczos_resample_cpu(src.float(), x1, y1, x2, y2, ow, oh)


def rect_mask_cpu(
    h: int,
    w: int,
    rect: tuple[int, int, int, int],
    sigma: float,
    device=None,
) -> torch.Tensor:
    """Analytic Gaussian-blurred white-rect mask [h, w] (erf-product form)."""
    rx1, ry1, rx2, ry2 = (float(r) for r in rect)
    xs = torch.arange(w, dtype=torch.float32, device=device)
    ys = torch.arange(h, dtype=torch.float32, device=device)
    if sigma <= 0:
        gx = ((xs >= rx1) & (xs < rx2)).float()
        gy = ((ys >= ry1) & (ys < ry2)).float()
    else:
        inv_s = 1.0 / (sigma * math.sqrt(2.0))
        gx = 0.5 * (torch.erf((xs + 0.5 - rx1) * inv_s) - torch.erf((xs + 0.5 - rx2) * inv_s))
        gy = 0.5 * (torch.erf((ys + 0.5 - ry1) * inv_s) - torch.erf((ys + 0.5 - ry2) * inv_s))
    return gy[:, None] * gx[None, :]


def blend_tile(
    canvas: torch.Tensor,
    tile: torch.Tensor,
    region: tuple[int, int, int, int],
    mask_rect: tuple[int, int, int, int],
    sigma: float,
) -> None:
    """In-place: resample ``tile`` to ``region`` size and composite into
    ``canvas`` under the analytic blurred-rect mask."""
    x1, y1, x2, y2 = (int(r) for r in region)
    if _on_gpu(canvas):
        ext.get_ext(True).blend_tile(
            canvas, tile.float(), x1, y1, x2, y2,
            int(mask_rect[0]), int(mask_rect[1]), int(mask_rect[2]),
            int(mask_rect[3]), float(sigma),
        )
        return
    rw, rh = x2 - x1, y2 - y1
    t = _lanczos_resample_cpu(tile.float(), 0, 0, tile.shape[2], tile.shape[1], rw, rh)
    m_full = rect_mask_cpu(canvas.shape[1], canvas.shape[2], mask_rect, sigma)
    m = m_full[y1:y2, x1:x2][None, :, :, None]
    patch = canvas[:, y1:y2, x1:x2, :]
    canvas[:, y1:y2, x1:x2, :] = patch * (1 - m) + t * m
