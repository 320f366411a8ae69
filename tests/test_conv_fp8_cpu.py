"""The FP8 conv path without a GPU: ``dispatch``'s torch definitions of the
per-image quantiser and of ``conv_fp8``, the cached weight pack, and the
``conv_dtype`` switch of ``create_diffusion_stack``."""

import pytest
import torch
import torch.nn.functional as F

import fp8_bounds as fb
from comfyui_distributed_amd.models import create_diffusion_stack
from comfyui_distributed_amd.models.quant import conv_eligible
from comfyui_distributed_amd.models.unet import MfmaConv2d
from comfyui_distributed_amd.ops import dispatch


def test_quantiser_definition():
    x = torch.randn(3, 5, 7, 64, generator=torch.Generator().manual_seed(0))
    x = x.bfloat16()
    x[1] = 0
    q, scale = dispatch.quant_nhwc_fp8(x)
    assert q.shape == x.shape and q.dtype == fb.FP8 and scale.shape == (3,)
    assert torch.equal(scale, fb.scale_ref(x.float().abs().amax(dim=(1, 2, 3))))
    flat = x.float().reshape(3, -1)
    assert fb.quant_ratio(q.reshape(3, -1), flat, scale) <= 1.0
    assert not q[1].view(torch.uint8).any()


@pytest.mark.parametrize("rs,stride", [(9, 1), (9, 2), (1, 1)])
def test_conv_definition(rs, stride):
    """``conv_fp8`` on the CPU against ``F.conv2d`` on the dequantised
    operands in fp64, within the fp32 dot-product bound and one bf16
    rounding."""
    b, h, w, c, k_out = 2, 6, 6, 64, 24
    r = 3 if rs == 9 else 1
    g = torch.Generator().manual_seed(rs + stride)
    q, sa = dispatch.quant_nhwc_fp8(torch.randn(b, h, w, c, generator=g))
    w4 = torch.randn(k_out, r, r, c, generator=g)
    qw, sw = dispatch.quantize_weight_fp8(w4.reshape(k_out, -1), pad_k=True)
    assert qw.shape == (k_out, (rs * c + 127) // 128 * 128)
    bias = torch.randn(k_out, generator=g)
    dq = (q.float().double() * sa.double()[:, None, None, None]).permute(0, 3, 1, 2)
    dw = (qw[:, :rs * c].float().double() * sw.double()[:, None]).reshape(
        k_out, r, r, c).permute(0, 3, 1, 2)
    pre = F.conv2d(dq, dw, bias.double(), stride=stride, padding=r // 2)
    mag = F.conv2d(dq.abs(), dw.abs(), bias.double().abs(), stride=stride,
                   padding=r // 2).permute(0, 2, 3, 1)
    res = torch.randn(pre.permute(0, 2, 3, 1).shape, generator=g).bfloat16()
    ref = F.silu(pre).permute(0, 2, 3, 1) + res.double()
    y = dispatch.conv_fp8(q, sa, qw, sw, bias, rs=rs, stride=stride,
                          fuse_silu=True, residual=res)
    assert y.dtype == torch.bfloat16
    fb.check(y, ref, fb.bound_from(ref, mag + res.double().abs(), rs * c, "silu"),
             f"conv_fp8 cpu rs={rs} stride={stride}")


def test_weight_pack():
    """Rows are [tap][c] with c innermost, zero-padded to a multiple of 128,
    cached on the module and refreshed in place after an in-place update."""
    conv = MfmaConv2d(64, 8, 3, padding=1)
    qw, sw = dispatch.quantize_conv_weight_fp8(conv)
    assert qw.shape == (8, 640) and qw.dtype == fb.FP8 and sw.shape == (8,)
    assert not qw.view(torch.uint8)[:, 576:].any()
    wt = conv.weight.detach().permute(0, 2, 3, 1).reshape(8, -1).bfloat16()
    q_ref, s_ref = fb.quant_ref(wt)
    assert torch.equal(sw, s_ref)
    assert torch.equal(qw.view(torch.uint8)[:, :576], q_ref.view(torch.uint8))
    again = dispatch.quantize_conv_weight_fp8(conv)
    assert again[0] is qw and again[1] is sw
    with torch.no_grad():
        conv.weight.mul_(-2.0)
    qw2, sw2 = dispatch.quantize_conv_weight_fp8(conv)
    assert qw2 is qw and sw2 is sw
    assert torch.equal(sw, 2 * s_ref)
    assert torch.equal(qw.float()[:, :576], -q_ref.float())


def test_stack_conv_dtype():
    plain = create_diffusion_stack("tiny")
    assert plain.conv_dtype is None and plain.fp8_convs == 0
    assert not any(hasattr(m, "_distgpu_fp8") for m in plain.unet.modules())
    stack = create_diffusion_stack("tiny", conv_dtype="fp8")
    marked = [m for m in stack.unet.modules() if hasattr(m, "_distgpu_fp8")]
    want = [m for m in stack.unet.modules() if conv_eligible(m)]
    assert stack.conv_dtype == "fp8" and stack.fp8_convs == len(want) > 0
    assert marked == want
    assert all(m.kernel_size == (3, 3) and m.in_channels % 64 == 0
               for m in marked)
    assert not any(hasattr(m, "_distgpu_fp8") for m in stack.vae.modules())
    with pytest.raises(ValueError):
        create_diffusion_stack("wan_tiny", conv_dtype="fp8")


def test_stack_conv_dtype_env(monkeypatch):
    monkeypatch.setenv("DISTGPU_CONV_DTYPE", "fp8")
    assert create_diffusion_stack("tiny").fp8_convs > 0
    create_diffusion_stack("wan_tiny")  # ignored there
