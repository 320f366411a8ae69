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

import torch
import torch.nn.functional as F

from . import ext

LANCZOS_A = 3
ATTN_DPADS = (48, 64, 96, 128, 160)


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
# hipBLASLt wins the plain-Linear shapes (measured gpurun_out/call3: 368-1614
# TF vs our 205-1009) — the 256-tile GEMM stays available for fused uses and
# future skinny-N tiles but is opt-in for nn.Linear routing
_GEMM256 = os.environ.get("DISTGPU_GEMM256", "0") == "1"
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
    epilogue — the ResBlock skip connection without its own kernel."""
    assert x.is_cuda
    if residual is not None and not _FUSE_RES:
        return conv2d_mfma(x, conv, fuse_silu, up2) + residual
    b, c, h, w = x.shape
    nhwc = _nhwc_bf16(x)
    wt, rs, bias = _conv_params(conv, x.device)
    stride = conv.stride[0]
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


def linear_mfma(x: torch.Tensor, weight: torch.Tensor,
                bias: torch.Tensor | None = None,
                fuse_silu: bool = False) -> torch.Tensor:
    """torch-Linear on the 256-tile MFMA GEMM when the shape fills it
    (tokens >= 1024, K % 64 == 0); hipBLASLt otherwise. x [..., K]."""
    K = x.shape[-1]
    M = x.numel() // K
    if (
        _GEMM256
        and _on_gpu(x)
        and M >= 1024
        and K % 64 == 0
        and weight.shape[0] >= 64
    ):
        x2 = x.reshape(M, K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        b = bias if bias is not None else torch.empty(0, device=x.device)
        y = ext.get_ext(True).gemm256_bf16(
            x2.to(torch.bfloat16), weight.to(torch.bfloat16), b, fuse_silu)
        return y.reshape(*x.shape[:-1], weight.shape[0])
    y = F.linear(x, weight, bias)
    return F.silu(y) if fuse_silu else y


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
    GPU path: the MFMA flash kernel (bf16, fp32 accumulation); dims are
    zero-padded to the kernel contract (D -> D_PAD, Nq -> 64k, Nk -> 32k)
    here, the kernel masks padded keys.
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
    kernel directly (zero reshapes/copies); on CPU it unpacks and reuses
    the reference path."""
    kv_heads = kv_heads or heads
    d = q.shape[-1] // heads
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    if _on_gpu(q):
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
    """Self-attention straight off a fused projection [B, N, 3*H*D]."""
    hd = qkv.shape[-1] // 3
    d = hd // heads
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    if _on_gpu(qkv):
        return ext.get_ext(True).attn_fwd_qkv(
            qkv.to(torch.bfloat16).contiguous(), heads, scale)
    q, k, v = qkv.split(hd, dim=-1)
    return attention_packed(q.contiguous(), k.contiguous(), v.contiguous(),
                            heads=heads, scale=scale)


def attention_q_kv(q: torch.Tensor, kv: torch.Tensor, heads: int,
                   scale: float | None = None) -> torch.Tensor:
    """Cross-attention: q [B,Nq,H*D] + fused kv [B,Nk,2*H*D]."""
    hd = q.shape[-1]
    d = hd // heads
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    if _on_gpu(q):
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


def quantize_weight_fp8(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] -> (qw [N, K] float8_e4m3fn, sw [N] fp32): per-output-channel
    absmax / 448. Plain torch, run once per layer."""
    if w.dim() != 2:
        raise ValueError(f"weight must be [N, K], got {tuple(w.shape)}")
    w = w.detach()
    sw = _fp8_scale(w.float().abs().amax(dim=1))
    return _fp8_quant(w, sw).contiguous(), sw.contiguous()


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


def quantize_rows(x: torch.Tensor) -> Fp8Rows:
    """``quant_rows_fp8`` over the rows of any x [..., K] (same errors)."""
    if x.dim() < 1:
        raise ValueError("x must be [..., K]")
    q, scale = quant_rows_fp8(x.reshape(-1, x.shape[-1]))
    return Fp8Rows(q.reshape(x.shape), scale.reshape(x.shape[:-1]), x.dtype)


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


def linear_fp8(x: torch.Tensor | Fp8Rows, qw: torch.Tensor, sw: torch.Tensor,
               bias: torch.Tensor | None = None,
               act: str | None = None) -> torch.Tensor:
    """Linear with an FP8 weight: x [..., K] -> [..., N] in x.dtype. The rows
    of x are quantised per call (absmax / 448), the product runs on e4m3
    operands with fp32 accumulation, and ``act`` (None, "silu", "gelu_tanh")
    is fused after the bias. An :class:`Fp8Rows` in place of x holds rows
    that are quantised already: no quantiser runs, only the GEMM.

    GPU: quant_rows_fp8 + gemm_fp8 (gemm_fp8.hip), bf16 x only. CPU: the same
    quantised operands, dequantised fp32 matmul. K % 128 != 0, K > 16384 or
    a non-bf16 input on GPU raise ValueError: the fallback for such layers is
    decided at module conversion (models/quant.py), not here."""
    rows = x if isinstance(x, Fp8Rows) else None
    k = (rows.q if rows is not None else x).shape[-1]
    if qw.dim() != 2 or qw.shape[1] != k:
        raise ValueError(
            f"x [..., {k}] does not match qw {tuple(qw.shape)}")
    if not fp8_shape_supported(k):
        raise ValueError(
            f"K = {k} unsupported (multiple of 128, <= {FP8_MAX_K})")
    if rows is not None:
        y = gemm_fp8(rows.q.reshape(-1, k), rows.scale.reshape(-1), qw, sw,
                     bias, act)
        return y.to(rows.dtype).reshape(*rows.q.shape[:-1], qw.shape[0])
    if _on_gpu(x) and x.dtype != torch.bfloat16:
        raise ValueError(f"linear_fp8 on GPU takes bf16, got {x.dtype}")
    x2 = x.reshape(-1, k)
    qa, sa = quant_rows_fp8(x2)
    y = gemm_fp8(qa, sa, qw, sw, bias, act)
    return y.to(x.dtype).reshape(*x.shape[:-1], qw.shape[0])


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
