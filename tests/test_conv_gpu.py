"""GPU numerics for the implicit-GEMM NHWC conv + NHWC GroupNorm kernels."""

import pytest
import torch
import torch.nn.functional as F

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

# The dot-product bound of kernel_bounds.py is applied where RS*C <= 1152.
# Above that its accumulation term n*2^-23*mag dominates (15x the rounding
# term at C=1280 3x3 by CPU emulation) and a lost fragment is worth 2.6
# bounds, not 150+; those shapes keep the relative-max assert alone.


def _nores():
    return torch.empty(0, device="cuda", dtype=torch.bfloat16)


def _module_conv_bound(y, xcl, conv, what, silu=False):
    """Bound check for a dispatch.conv2d_mfma result (NCHW semantic)."""
    c = conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1]
    if c > kb.DOT_BOUND_MAX_RSC:
        return
    ref, bound = kb.conv_ref(xcl.permute(0, 2, 3, 1).float().cpu(),
                             conv.weight.float().cpu(),
                             conv.bias.float().cpu(), silu=silu)
    kb.check(y.permute(0, 2, 3, 1), ref, bound, what)


def _raw_conv_bound(y, x, wkern, b, what, rs_c, **kw):
    """Bound check for an ext.conv256_nhwc / gemm-style result (NHWC)."""
    if rs_c > kb.DOT_BOUND_MAX_RSC:
        return
    ref, bound = kb.conv_ref(x.float().cpu(), wkern.float().cpu(),
                             b.float().cpu(), **kw)
    kb.check(y, ref, bound, what)


@pytest.fixture(scope="module")
def extmod():
    from comfyui_distributed_amd.ops import ext

    return ext.get_ext(required=True)


@pytest.mark.parametrize("shape,k", [
    ((2, 64, 17, 19), 32),     # odd spatial, C=64
    ((1, 128, 32, 32), 128),
    ((1, 512, 16, 16), 256),   # channel change
])
def test_conv3x3_matches_torch(extmod, shape, k):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(shape[1])
    b, c, h, w = shape
    conv = torch.nn.Conv2d(c, k, 3, padding=1).cuda().to(torch.bfloat16)
    x = (torch.randn(b, c, h, w) / 4).cuda().to(torch.bfloat16)
    xcl = x.contiguous(memory_format=torch.channels_last)
    y = dispatch.conv2d_mfma(xcl, conv).float()
    ref = F.conv2d(x.float(), conv.weight.float(), conv.bias.float(), padding=1)
    err = (y - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err / scale < 0.05, f"rel err {err/scale}"
    _module_conv_bound(y, xcl, conv, f"conv2d_mfma 3x3 {shape}->{k}")


def test_conv1x1_matches_torch(extmod):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(0)
    conv = torch.nn.Conv2d(128, 256, 1).cuda().to(torch.bfloat16)
    x = (torch.randn(2, 128, 24, 24) / 4).cuda().to(torch.bfloat16)
    xcl = x.contiguous(memory_format=torch.channels_last)
    y = dispatch.conv2d_mfma(xcl, conv).float()
    ref = F.conv2d(x.float(), conv.weight.float(), conv.bias.float())
    err = (y - ref).abs().max().item()
    assert err / ref.abs().max().item() < 0.05
    _module_conv_bound(y, xcl, conv, "conv2d_mfma 1x1 (2,128,24,24)->256")


def test_conv_fused_silu(extmod):
    from comfyui_distributed_amd.ops import dispatch

    conv = torch.nn.Conv2d(64, 64, 3, padding=1).cuda().to(torch.bfloat16)
    x = (torch.randn(1, 64, 16, 16) / 4).cuda().to(torch.bfloat16)
    xcl = x.contiguous(memory_format=torch.channels_last)
    y = dispatch.conv2d_mfma(xcl, conv, fuse_silu=True).float()
    ref = F.silu(F.conv2d(x.float(), conv.weight.float(), conv.bias.float(), padding=1))
    assert (y - ref).abs().max().item() / (ref.abs().max().item() + 1e-6) < 0.05
    _module_conv_bound(y, xcl, conv, "conv2d_mfma 3x3 + SiLU", silu=True)


def test_groupnorm_nhwc_matches_torch(extmod):
    torch.manual_seed(1)
    x = torch.randn(2, 128, 20, 20)
    w, b = torch.randn(128), torch.randn(128)
    nhwc = x.permute(0, 2, 3, 1).contiguous().cuda().to(torch.bfloat16)
    y = extmod.group_norm_nhwc(nhwc, 32, w.cuda(), b.cuda(), 1e-5, True)
    ref = F.silu(F.group_norm(x, 32, w, b, 1e-5)).permute(0, 2, 3, 1)
    err = (y.float().cpu() - ref).abs()
    assert (err <= 0.02 + 0.01 * ref.abs()).all(), err.max().item()
    ref64, bound = kb.group_norm_ref(kb.bf16_exact(x), 32, w, b, 1e-5, True)
    kb.check(y.permute(0, 3, 1, 2), ref64, bound,
             "group_norm_nhwc (2,128,20,20) G=32 silu")


def test_vae_decode_nhwc_path_consistent(extmod):
    """GPU VAE decode (MFMA conv path) vs CPU fp32 decode: bf16-level
    agreement proves the hand-written conv path computes the same model."""
    from comfyui_distributed_amd.models import create_diffusion_stack

    gpu = create_diffusion_stack("sd15", device="cuda:0", dtype=torch.bfloat16, seed=3)
    cpu = create_diffusion_stack("sd15", device="cpu", dtype=torch.float32, seed=3)
    z = torch.randn(1, 4, 16, 16)
    with torch.no_grad():
        img_gpu = gpu.vae.decode(z.cuda()).cpu()
        img_cpu = cpu.vae.decode(z)
    err = (img_gpu - img_cpu).abs().max().item()
    assert err < 0.12, f"decode mismatch {err}"  # bf16 conv chain tolerance
    assert torch.isfinite(img_gpu).all()


def test_gemm256_matches_fp32_linear():
    """256-tile glds GEMM vs fp32 torch reference, incl. partial M/N tiles
    and the SiLU fusion."""
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    torch.manual_seed(0)
    for (M, N, K) in [(4624, 320, 320), (4624, 2560, 320), (1156, 640, 768),
                      (300, 77, 128), (256, 256, 64)]:
        x = (torch.randn(M, K, device="cuda") / 4).to(torch.bfloat16)
        w = (torch.randn(N, K, device="cuda") / 4).to(torch.bfloat16)
        b = torch.randn(N, device="cuda").to(torch.bfloat16)
        y = mod.gemm256_bf16(x, w, b, False)
        ref = torch.nn.functional.linear(x.float(), w.float(), b.float())
        err = (y.float() - ref).abs().max().item()
        scale = ref.abs().max().item()
        assert err / scale < 0.02, f"gemm {M}x{N}x{K}: rel err {err/scale}"
        # SiLU fusion
        y2 = mod.gemm256_bf16(x, w, b, True)
        ref2 = torch.nn.functional.silu(ref)
        err2 = (y2.float() - ref2).abs().max().item()
        assert err2 / max(scale, 1e-6) < 0.02
        for silu, out in ((False, y), (True, y2)):
            ref64, bound = kb.linear_ref(x.float().cpu(), w.float().cpu(),
                                         b.float().cpu(), silu)
            kb.check(out, ref64, bound, f"gemm256 {M}x{N}x{K} silu={silu}")


@pytest.mark.parametrize("m,n,k", [
    (256, 256, 64),    # one K-tile: the prologue stage alone
    (256, 256, 192),   # three K-tiles: both buffer parities, an odd count
    (300, 77, 128),    # M tail; N % 4 != 0, so the column-by-column store
])
def test_gemm256_integer_exact(m, n, k):
    """Operands from {-1, 1, 2} x {1, 0.5}, 25 % dense and seeded with K
    (as test_gemm_integer_exact of test_fp8_linear_gpu.py), no bias. Every
    product is a multiple of 1/4 and every partial sum stays far below 2^24,
    so the fp32 accumulation is exact in any order, and |result| < 64 keeps
    the multiples of 1/4 exact in bf16: the output must EQUAL the fp64
    matmul. The staging order, the chunk map, the fragment pairing and the
    epilogue's lane-to-(m, n0) walk are all in this one equality."""
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    g = torch.Generator().manual_seed(k)

    def operand(rows):
        vals = torch.tensor([-1.0, 1.0, 2.0])[
            torch.randint(0, 3, (rows, k), generator=g)]
        keep = torch.rand(rows, k, generator=g) < 0.25
        half = torch.where(torch.rand(rows, k, generator=g) < 0.5, 0.5, 1.0)
        return vals * keep * half

    a, w = operand(m), operand(n)
    for t in (a, w):
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    ref = a.double() @ w.double().t()
    assert ref.abs().max() < 64
    assert torch.equal(ref.to(torch.bfloat16).double(), ref)
    if m == n:
        assert not torch.equal(ref, ref.t())
    y = mod.gemm256_bf16(a.to(torch.bfloat16).cuda(),
                         w.to(torch.bfloat16).cuda(), _nores(), False)
    assert y.dtype == torch.bfloat16 and y.shape == (m, n)
    bad = (y.cpu().double() != ref).sum().item()
    assert bad == 0, f"{bad} of {m * n} elements differ from the exact matmul"


def test_conv256_matches_fp32_conv():
    """Implicit-GEMM 256-tile conv (3x3 pad1 + 1x1) vs fp32 reference —
    exercises the zero-page OOB tap redirect at image borders."""
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    torch.manual_seed(1)
    for (B, C, H, W, K, rs) in [(2, 64, 17, 19, 96, 9), (1, 128, 34, 34, 320, 9),
                                (2, 320, 20, 20, 320, 9), (2, 64, 32, 32, 48, 1),
                                # H,W % 16 == 0 -> the 16x16 tile2d mode
                                (1, 128, 32, 48, 64, 9), (2, 64, 16, 16, 96, 9)]:
        x = (torch.randn(B, H, W, C, device="cuda") / 4).to(torch.bfloat16)
        wkern = (torch.randn(K, C, 3, 3, device="cuda") / 8).to(torch.bfloat16)
        if rs == 1:
            wkern = wkern[:, :, :1, :1].contiguous()
        wt = wkern.permute(0, 2, 3, 1).reshape(K, -1).contiguous()
        b = torch.randn(K, device="cuda").to(torch.bfloat16)
        y = mod.conv256_nhwc(x, wt, b, _nores(), B, H, W, C, K, rs, 1, False, False)
        xf = x.permute(0, 3, 1, 2).float()
        ref = torch.nn.functional.conv2d(
            xf, wkern.float(), b.float(), padding=1 if rs == 9 else 0)
        ref = ref.permute(0, 2, 3, 1)
        err = (y.float() - ref).abs().max().item()
        scale = ref.abs().max().item()
        assert err / scale < 0.02, f"conv {B}x{C}x{H}x{W}->{K} rs{rs}: {err/scale}"
        _raw_conv_bound(y, x, wkern, b, f"conv256 {B}x{C}x{H}x{W}->{K} rs{rs}",
                        rs * C)


def test_conv256_stride2_matches_fp32_conv():
    """Stride-2 3x3 (the UNet/VAE Downsample convs) on the 256-tile
    kernel vs the fp32 torch reference."""
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    torch.manual_seed(3)
    for (B, C, H, W, K) in [(2, 64, 32, 32, 96), (1, 128, 34, 34, 128),
                            (2, 320, 20, 24, 320), (1, 64, 17, 19, 64)]:
        x = (torch.randn(B, H, W, C, device="cuda") / 4).to(torch.bfloat16)
        wkern = (torch.randn(K, C, 3, 3, device="cuda") / 8).to(torch.bfloat16)
        wt = wkern.permute(0, 2, 3, 1).reshape(K, -1).contiguous()
        b = torch.randn(K, device="cuda").to(torch.bfloat16)
        y = mod.conv256_nhwc(x, wt, b, _nores(), B, H, W, C, K, 9, 2, False, False)
        xf = x.permute(0, 3, 1, 2).float()
        ref = torch.nn.functional.conv2d(xf, wkern.float(), b.float(),
                                         stride=2, padding=1)
        ref = ref.permute(0, 2, 3, 1)
        assert y.shape == ref.shape, (y.shape, ref.shape)
        err = (y.float() - ref).abs().max().item()
        scale = ref.abs().max().item()
        assert err / scale < 0.02, f"stride2 {B}x{C}x{H}x{W}->{K}: {err/scale}"
        _raw_conv_bound(y, x, wkern, b, f"conv256 stride2 {B}x{C}x{H}x{W}->{K}",
                        9 * C, stride=2)


def test_conv256_fused_upsample_matches_interpolate_conv():
    """up2 mode: conv of a VIRTUAL nearest-2x upsample vs
    F.interpolate + conv fp32 reference (VAE decoder upsample fusion)."""
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    torch.manual_seed(5)
    for (B, C, H, W, K) in [(2, 64, 16, 16, 96), (1, 128, 17, 19, 128),
                            (2, 128, 24, 24, 64)]:
        x = (torch.randn(B, H, W, C, device="cuda") / 4).to(torch.bfloat16)
        wkern = (torch.randn(K, C, 3, 3, device="cuda") / 8).to(torch.bfloat16)
        wt = wkern.permute(0, 2, 3, 1).reshape(K, -1).contiguous()
        b = torch.randn(K, device="cuda").to(torch.bfloat16)
        y = mod.conv256_nhwc(x, wt, b, _nores(), B, H, W, C, K, 9, 1, True, False)
        xf = x.permute(0, 3, 1, 2).float()
        up = torch.nn.functional.interpolate(xf, scale_factor=2,
                                             mode="nearest")
        ref = torch.nn.functional.conv2d(up, wkern.float(), b.float(),
                                         padding=1).permute(0, 2, 3, 1)
        assert y.shape == ref.shape
        err = (y.float() - ref).abs().max().item()
        scale = ref.abs().max().item()
        assert err / scale < 0.02, f"up2 {B}x{C}x{H}x{W}->{K}: {err/scale}"
        _raw_conv_bound(y, x, wkern, b, f"conv256 up2 {B}x{C}x{H}x{W}->{K}",
                        9 * C, up2=True)


def test_conv256_fused_residual_add():
    """Epilogue residual fusion (the ResBlock skip add) vs conv + add."""
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    torch.manual_seed(9)
    B, C, H, W, K = 2, 64, 20, 20, 96
    x = (torch.randn(B, H, W, C, device="cuda") / 4).to(torch.bfloat16)
    wkern = (torch.randn(K, C, 3, 3, device="cuda") / 8).to(torch.bfloat16)
    wt = wkern.permute(0, 2, 3, 1).reshape(K, -1).contiguous()
    b = torch.randn(K, device="cuda").to(torch.bfloat16)
    res = torch.randn(B, H, W, K, device="cuda").to(torch.bfloat16)
    y = mod.conv256_nhwc(x, wt, b, res.contiguous(), B, H, W, C, K, 9, 1,
                         False, False)
    ref = torch.nn.functional.conv2d(
        x.permute(0, 3, 1, 2).float(), wkern.float(), b.float(), padding=1
    ).permute(0, 2, 3, 1) + res.float()
    err = (y.float() - ref).abs().max().item()
    assert err / ref.abs().max().item() < 0.03, err
    _raw_conv_bound(y, x, wkern, b, "conv256 + residual", 9 * C,
                    residual=res.float().cpu())


# ---------------------------------------------------------------------------
# kernel variants no test above launches, called through ext directly so the
# variant is certain; bounds from tests/kernel_bounds.py
# ---------------------------------------------------------------------------


def _dev_bf16(t):
    return t.to(torch.bfloat16).cuda()


def _conv_nhwc_case(extmod, case, variant):
    b, c, h, w, k, rs, silu = case
    x, wk, bias = kb.conv_inputs(c * 100 + k + rs, b, c, h, w, k, rs)
    ref, bound = kb.conv_ref(x, wk, bias, silu=silu)
    y = extmod.conv_nhwc(_dev_bf16(x), _dev_bf16(kb.repack_weight(wk)),
                         bias.cuda(), b, h, w, c, k, rs, silu)
    kb.check(y, ref, bound,
             f"conv_nhwc {variant} {(b, c, h, w)}->{k} rs{rs} silu={silu}")


@pytest.mark.parametrize("case", kb.CONV_V1_CASES, ids=str)
def test_conv_nhwc_v1(extmod, case):
    """conv_direct_kernel<RS, 2, 2, false> (64x64 tile, B fragments from
    global): the launcher takes it whenever K % 128 != 0 or M = B*H*W < 128,
    as at the 8x8 level of the UNet. The cases (kernel_bounds.CONV_V1_CASES)
    have an M tail, a K tail inside the 64-column tile, M below one tile,
    the SiLU epilogue, and three column blocks with a partial last one."""
    b, c, h, w, k, rs, silu = case
    assert k % 128 != 0 or b * h * w < 128   # v1 by the launcher's rule
    _conv_nhwc_case(extmod, case, "v1")


@pytest.mark.parametrize("case", kb.CONV_V2_CASES, ids=str)
def test_conv_nhwc_v2(extmod, case):
    """conv_direct_kernel<RS, 4, 4, true> (128x128 tile, LDS-staged
    weights): taken when K % 128 == 0 and M >= 128. A partial second M tile,
    two column blocks, the 1x1 template with SiLU, and two images meeting
    inside one row tile."""
    b, c, h, w, k, rs, silu = case
    assert k % 128 == 0 and b * h * w >= 128   # v2 by the launcher's rule
    _conv_nhwc_case(extmod, case, "v2")


@pytest.mark.parametrize("case", kb.CONV256_SMALLK_CASES, ids=str)
def test_conv256_small_k_out(extmod, case):
    """conv256_nhwc with K_out of 3, 4 and 8 (the VAE and UNet out convs,
    which conv_supported routes here): all but one 16-column fragment of the
    256-column tile is masked. H, W multiples of 16 select the 16x16 pixel
    tiling, anything else the linear one; plus stride 2 and the fused
    nearest-2x upsample."""
    b, c, h, w, k, rs, stride, up2 = case
    x, wk, bias = kb.conv_inputs(c * 100 + k + rs, b, c, h, w, k, rs)
    ref, bound = kb.conv_ref(x, wk, bias, stride=stride, up2=up2)
    y = extmod.conv256_nhwc(_dev_bf16(x), _dev_bf16(kb.repack_weight(wk)),
                            bias.cuda(), _nores(), b, h, w, c, k, rs, stride,
                            up2, False)
    kb.check(y, ref, bound, f"conv256 {(b, c, h, w)}->{k} s{stride} up2={up2}")


@pytest.mark.parametrize("shape,groups", kb.GN_NHWC_CASES, ids=str)
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_nhwc_paths(extmod, shape, groups, silu):
    """group_norm_nhwc at the SD1.5 UNet widths (Cg = 10/20/40: 16-byte
    vectors straddle two groups), Cg = 8, the G = 64 limit, several images
    with one stats block each, and the per-(n,g) kernel (Cg = 2, G > 64,
    C % 8 != 0 with the 1024-thread block); see kernel_bounds.GN_NHWC_CASES."""
    x, w, b = kb.norm_inputs(shape[1] + groups, shape)
    ref, bound = kb.group_norm_ref(x, groups, w, b, 1e-5, silu)
    y = extmod.group_norm_nhwc(_dev_bf16(x.permute(0, 2, 3, 1).contiguous()),
                               groups, w.cuda(), b.cuda(), 1e-5, silu)
    kb.check(y.permute(0, 3, 1, 2), ref, bound,
             f"group_norm_nhwc {shape} G={groups} silu={silu}")


def test_groupnorm_nhwc_offset_input(extmod):
    """Input of mean 16, std 1 through the two-pass kernels. They take
    var = E[x^2] - mean^2 in fp32, which loses ~2^-23 * (mean/std)^2 of the
    variance: 2^-15 here. By CPU emulation (test_kernel_bounds_cpu.py) the
    bound holds at mean/std = 16, is left from ~32 on at elements where
    xhat*w + b cancels, and the typical element is a whole bf16 ulp off only
    near mean/std 256-512."""
    shape, groups = kb.GN_OFFSET_CASE
    x, w, b = kb.norm_inputs(shape[1] + groups, shape, **kb.NORM_OFFSET)
    ref, bound = kb.group_norm_ref(x, groups, w, b, 1e-5, True)
    y = extmod.group_norm_nhwc(_dev_bf16(x.permute(0, 2, 3, 1).contiguous()),
                               groups, w.cuda(), b.cuda(), 1e-5, True)
    kb.check(y.permute(0, 3, 1, 2), ref, bound,
             f"group_norm_nhwc {shape} G={groups} mean 16")
