"""The FP8 conv path on the GPU (ops/hip/conv_fp8.hip): the per-image
quantiser, conv_fp8_kernel at both N-tile widths, and the route through
``conv2d_mfma``. References are fp64 convs on the CPU from the exact codes the
kernel receives; bounds are fp8_bounds'. Every conv case is B = 2, H = W = 12:
M = 288 (144 at stride 2) is an M tail, and the first tile straddles the two
images. Measured times are in profiles/r25_conv_fp8.md."""

import pytest
import torch
import torch.nn.functional as F

import fp8_bounds as fb
from comfyui_distributed_amd.models.quant import quantize_unet_convs
from comfyui_distributed_amd.models.unet import MfmaConv2d
from comfyui_distributed_amd.ops import dispatch, ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
B, H, W = 2, 12, 12
# C = 64: two taps per K-tile and a half-empty last tile; 128: tap-aligned;
# 192: a tap boundary in the middle of a tile and an odd half count
CS = [64, 128, 192]
GEOS = [(9, 1), (9, 2), (1, 1)]
# K_out = 48: one masked N-block; 320 pinned to each built width
WIDTHS = [(48, 0), (320, 256), (320, 320)]


def _pack(w):
    """w [K_out, R, S, C], values exact in e4m3 -> qw [K_out, Kp]."""
    q = w.reshape(w.shape[0], -1).to(fb.FP8).view(torch.uint8)
    return F.pad(q, (0, -q.shape[1] % 128)).view(fb.FP8)


def _conv64(x, w, stride):
    """fp64 conv of x [B, H, W, C] by w [K_out, R, S, C], pad R // 2 ->
    [B, Ho, Wo, K_out]."""
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2),
                 stride=stride, padding=w.shape[1] // 2)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("k_out,bn", WIDTHS)
@pytest.mark.parametrize("rs,stride", GEOS)
@pytest.mark.parametrize("c", CS)
def test_conv_integer_exact(c, rs, stride, k_out, bn):
    """test_gemm_integer_exact's operands: values from {-1, 0, 1, 2} x
    {1, 0.5}, all scales 1, so every product is a multiple of 1/4, the fp32
    sums are exact in any order and |result| < 64 is exact in bf16: the output
    must EQUAL the conv. The density keeps about 24 products per output
    non-zero at every K = rs * C. The half-row tap choice, the k map, the
    borders, the zero page and the transposed store are in this equality."""
    r = 3 if rs == 9 else 1
    g = torch.Generator().manual_seed(c + rs + stride + k_out)
    keep_p = min(0.25, (24.0 / (rs * c)) ** 0.5)

    def operand(*shape):
        vals = torch.tensor([-1.0, 1.0, 2.0])[
            torch.randint(0, 3, shape, generator=g)]
        keep = torch.rand(shape, generator=g) < keep_p
        half = torch.where(torch.rand(shape, generator=g) < 0.5, 0.5, 1.0)
        return vals * keep * half

    x, w = operand(B, H, W, c), operand(k_out, r, r, c)
    ref = _conv64(x, w, stride)
    assert 0 < ref.abs().max() < 64
    y = dispatch.conv_fp8(
        x.to(fb.FP8).to(DEV), torch.ones(B, device=DEV), _pack(w).to(DEV),
        torch.ones(k_out, device=DEV), rs=rs, stride=stride, bn=bn)
    assert y.dtype == BF and y.shape == ref.shape
    bad = (y.cpu().double() != ref).sum().item()
    assert bad == 0, f"{bad} of {ref.numel()} elements differ from the conv"


@pytest.mark.parametrize("k_out", [48, 320])
@pytest.mark.parametrize("rs,stride", GEOS)
@pytest.mark.parametrize("c", [64, 192])
def test_conv_scale_placement(c, rs, stride, k_out):
    """Random codes, image scales 8x apart, channel scales over 0.02 .. 0.5,
    bias, SiLU and a residual: a scale taken from the other image or a
    neighbouring channel, or an epilogue step out of order, leaves the
    bound."""
    r = 3 if rs == 9 else 1
    g = torch.Generator().manual_seed(c + rs + stride + k_out)
    q = (torch.randn(B, H, W, c, generator=g) * 4).to(fb.FP8)
    qw4 = (torch.randn(k_out, r, r, c, generator=g) * 4).to(fb.FP8)
    sa = torch.tensor([0.01, 0.08])
    sw = 0.02 * 25.0 ** torch.rand(k_out, generator=g)
    bias = torch.randn(k_out, generator=g)
    s = sa.double()[:, None, None, None] * sw.double()
    pre = _conv64(q.float(), qw4.float(), stride) * s + bias.double()
    res = torch.randn(pre.shape, generator=g).to(BF)
    mag = (_conv64(q.float().abs(), qw4.float().abs(), stride) * s
           + bias.double().abs() + res.double().abs())
    ref = F.silu(pre) + res.double()
    y = dispatch.conv_fp8(q.to(DEV), sa.to(DEV), _pack(qw4.float()).to(DEV),
                          sw.to(DEV), bias.to(DEV), rs=rs, stride=stride,
                          fuse_silu=True, residual=res.to(DEV))
    fb.check(y, ref, fb.bound_from(ref, mag, 9 * c, "silu"),
             f"conv_fp8 C={c} rs={rs} stride={stride} K_out={k_out}")


@pytest.mark.parametrize("shape", [(3, 5, 7, 64), (2, 20, 20, 320)])
def test_quantiser(shape):
    """One block per image and eight. Image 0's absmax is negative and sits in
    its last 8 elements; image 1 is all zero (the floor scale, codes 0)."""
    g = torch.Generator().manual_seed(shape[3])
    x = torch.randn(shape, generator=g).to(BF)
    x[0, -1, -1, -3] = -9.0
    x[1] = 0
    q, scale = dispatch.quant_nhwc_fp8(x.to(DEV))
    assert q.dtype == fb.FP8 and q.shape == x.shape
    amax = x.float().abs().amax(dim=(1, 2, 3))
    assert amax[0] == 9.0
    assert torch.equal(scale.cpu(), fb.scale_ref(amax))
    q_ref, scale_ref = dispatch.quant_nhwc_fp8(x)
    assert torch.equal(scale_ref, scale.cpu())
    assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))
    assert not q[1].cpu().view(torch.uint8).any()


def test_route():
    """``conv2d_mfma`` on a ResBlock-sized conv: unmarked it returns the bf16
    kernel's bits; marked it runs quantiser + conv_fp8 and matches
    ``dispatch``'s CPU definition on the same codes within the conv bound."""
    c = 320
    torch.manual_seed(0)
    conv = MfmaConv2d(c, c, 3, padding=1).to(DEV, BF)
    x = torch.randn(B, c, H, W, device=DEV, dtype=BF).contiguous(
        memory_format=torch.channels_last)
    nhwc = x.permute(0, 2, 3, 1)
    wt, rs, bias = dispatch._conv_params(conv, x.device)
    parent = ext.get_ext(True).conv256_nhwc(
        nhwc, wt, bias, torch.empty(0, device=DEV, dtype=BF), B, H, W, c, c,
        rs, 1, False, False)
    assert torch.equal(dispatch.conv2d_mfma(x, conv).permute(0, 2, 3, 1), parent)
    assert quantize_unet_convs(conv) == 1
    y = dispatch.conv2d_mfma(x, conv).permute(0, 2, 3, 1)
    assert not torch.equal(y, parent)
    q, sa = dispatch.quant_nhwc_fp8(nhwc)
    qw, sw = dispatch.quantize_conv_weight_fp8(conv)
    q, sa, qw, sw, bias = (t.cpu() for t in (q, sa, qw, sw, bias))
    ref = dispatch.conv_fp8(q, sa, qw, sw, bias).double()
    w4 = qw[:, :9 * c].float().reshape(c, 3, 3, c)
    mag = (_conv64(q.float().abs(), w4.abs(), 1)
           * sa.double()[:, None, None, None] * sw.double()
           + bias.double().abs())
    fb.check(y, ref, fb.bound_from(ref, mag, 9 * c, None), "conv2d_mfma fp8")
