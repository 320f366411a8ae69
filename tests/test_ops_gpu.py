"""GPU numerics: HIP kernels vs plain fp32 PyTorch references.

All tests are gpu-marked; they fail loudly (KernelUnavailableError) if the
extension is missing on a GPU box — the HIP path must be the one that runs.
"""


import pytest
import torch
import torch.nn.functional as F

import kernel_bounds as kb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def extmod():
    from comfyui_distributed_amd.ops import ext

    return ext.get_ext(required=True)


def test_mfma_fragment_layout(extmod):
    """C = A @ B with ASYMMETRIC operands (transpose-detecting)."""
    torch.manual_seed(0)
    a = torch.randn(16, 32).to(torch.bfloat16)
    b = torch.randn(32, 16).to(torch.bfloat16)
    bt = b.t().contiguous()  # kernel takes B^T storage
    c = extmod.mfma_selftest(a.cuda(), bt.cuda()).cpu()
    ref = a.float() @ b.float()
    assert torch.allclose(c, ref, atol=0.05, rtol=0.02), (
        (c - ref).abs().max().item()
    )


@pytest.mark.parametrize("d", [40, 64, 80, 128, 160])
@pytest.mark.parametrize("nq,nk", [(64, 64), (77, 77), (1156, 77), (1024, 1024)])
def test_attention_numerics(extmod, d, nq, nk):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(d * 1000 + nq)
    bh = 4
    q = torch.randn(bh, nq, d) / 2
    k = torch.randn(bh, nk, d) / 2
    v = torch.randn(bh, nk, d)
    out_gpu = dispatch.attention(
        q.cuda().to(torch.bfloat16), k.cuda().to(torch.bfloat16),
        v.cuda().to(torch.bfloat16), heads=2,
    ).float().cpu()
    ref = dispatch.attention(q, k, v, heads=2)  # CPU fp32 reference
    err = (out_gpu - ref).abs().max().item()
    assert err < 0.03, f"max err {err} at d={d} nq={nq} nk={nk}"
    ref64, bound = kb.attention_ref(kb.bf16_exact(q), kb.bf16_exact(k),
                                    kb.bf16_exact(v), heads=2)
    kb.check(out_gpu, ref64, bound, f"attention d={d} nq={nq} nk={nk}")


def test_attention_gqa_gpu(extmod):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(3)
    b, h, hkv, n, dh = 2, 8, 2, 128, 64
    q = torch.randn(b * h, n, dh) / 2
    k = torch.randn(b * hkv, n, dh) / 2
    v = torch.randn(b * hkv, n, dh)
    out = dispatch.attention(
        q.cuda().to(torch.bfloat16), k.cuda().to(torch.bfloat16),
        v.cuda().to(torch.bfloat16), heads=h, kv_heads=hkv,
    ).float().cpu()
    ref = dispatch.attention(q, k, v, heads=h, kv_heads=hkv)
    assert (out - ref).abs().max().item() < 0.03
    ref64, bound = kb.attention_ref(kb.bf16_exact(q), kb.bf16_exact(k),
                                    kb.bf16_exact(v), heads=h, kv_heads=hkv)
    kb.check(out, ref64, bound, "attention gqa")


@pytest.mark.parametrize("b,h,n,nk,d", [(2, 8, 640, 640, 40), (1, 4, 100, 77, 64),
                                        (2, 2, 256, 256, 80)])
def test_attention_packed_matches_reference(extmod, b, h, n, nk, d):
    """Packed [B,N,H*D] strided path vs CPU reference."""
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(b * 100 + d)
    q = torch.randn(b, n, h * d) / 2
    k = torch.randn(b, nk, h * d) / 2
    v = torch.randn(b, nk, h * d)
    out = dispatch.attention_packed(
        q.cuda().to(torch.bfloat16), k.cuda().to(torch.bfloat16),
        v.cuda().to(torch.bfloat16), heads=h,
    ).float().cpu()
    ref = dispatch.attention_packed(q, k, v, heads=h)
    err = (out - ref).abs().max().item()
    assert err < 0.03, f"packed err {err} b={b} h={h} n={n} d={d}"
    ref64, bound = kb.attention_packed_ref(
        kb.bf16_exact(q), kb.bf16_exact(k), kb.bf16_exact(v), heads=h)
    kb.check(out, ref64, bound, f"attention packed b={b} h={h} n={n} d={d}")


def test_attention_fused_qkv_matches_reference(extmod):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(11)
    b, h, n, d = 2, 8, 200, 40
    qkv = torch.randn(b, n, 3 * h * d) / 2
    out = dispatch.attention_qkv(qkv.cuda().to(torch.bfloat16), heads=h)
    ref = dispatch.attention_qkv(qkv, heads=h)
    assert (out.float().cpu() - ref).abs().max().item() < 0.03
    ref64, bound = kb.attention_qkv_ref(kb.bf16_exact(qkv), heads=h)
    kb.check(out, ref64, bound, "attention fused qkv")


def test_attention_fused_q_kv_matches_reference(extmod):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(12)
    b, h, nq, nk, d = 2, 4, 150, 77, 64
    q = torch.randn(b, nq, h * d) / 2
    kv = torch.randn(b, nk, 2 * h * d) / 2
    out = dispatch.attention_q_kv(q.cuda().to(torch.bfloat16),
                                  kv.cuda().to(torch.bfloat16), heads=h)
    ref = dispatch.attention_q_kv(q, kv, heads=h)
    assert (out.float().cpu() - ref).abs().max().item() < 0.03
    ref64, bound = kb.attention_q_kv_ref(kb.bf16_exact(q), kb.bf16_exact(kv),
                                         heads=h)
    kb.check(out, ref64, bound, "attention fused q+kv")


def test_conv_smallc_matches_torch(extmod):
    import torch.nn.functional as F

    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(2)
    conv = torch.nn.Conv2d(4, 320, 3, padding=1).cuda().to(torch.bfloat16)
    x = (torch.randn(2, 4, 17, 19) / 2).cuda().to(torch.bfloat16)
    xcl = x.contiguous(memory_format=torch.channels_last)
    y = dispatch.conv2d_smallc(xcl, conv).float()
    ref = F.conv2d(x.float(), conv.weight.float(), conv.bias.float(), padding=1)
    err = (y - ref).abs().max().item()
    assert err / ref.abs().max().item() < 0.05
    ref64, bound = kb.conv_ref(xcl.permute(0, 2, 3, 1).float().cpu(),
                               conv.weight.float().cpu(),
                               conv.bias.float().cpu())
    kb.check(y.permute(0, 2, 3, 1), ref64, bound, "conv_smallc 4->320 3x3")


def test_attention_defer_max_rescale_branch(extmod):
    """Force the defer-max rescale branch (guide T13 hazard): a spiked K row
    in a LATER tile makes the running max jump past the threshold. Results
    must still match the exact CPU softmax."""
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(9)
    bh, n, d = 2, 256, 64
    q = torch.randn(bh, n, d) / 4
    k = torch.randn(bh, n, d) / 4
    v = torch.randn(bh, n, d)
    # tile size is 64: spike keys in tiles 2 and 3 so m jumps mid-stream
    k[:, 140] = q[:, 17] * 40.0  # huge dot for row 17 at tile 2
    k[:, 200] = q[:, 33] * 60.0  # even bigger at tile 3
    out = dispatch.attention(
        q.cuda().to(torch.bfloat16), k.cuda().to(torch.bfloat16),
        v.cuda().to(torch.bfloat16), heads=1,
    ).float().cpu()
    ref = dispatch.attention(q, k, v, heads=1)
    err = (out - ref).abs().max().item()
    assert err < 0.05, f"defer-max branch mismatch {err}"
    ref64, bound = kb.attention_ref(kb.bf16_exact(q), kb.bf16_exact(k),
                                    kb.bf16_exact(v))
    kb.check(out, ref64, bound, "attention defer-max spikes")


def test_attention_softmax_rows_sum(extmod):
    """Uniform V exposes softmax normalization errors: out must equal V."""
    from comfyui_distributed_amd.ops import dispatch

    q = torch.randn(2, 100, 64).cuda().to(torch.bfloat16)
    k = torch.randn(2, 100, 64).cuda().to(torch.bfloat16)
    v = torch.ones(2, 100, 64).cuda().to(torch.bfloat16)
    out = dispatch.attention(q, k, v, heads=1).float()
    assert (out - 1.0).abs().max().item() < 0.01
    ref64, bound = kb.attention_ref(q.float().cpu(), k.float().cpu(),
                                    v.float().cpu())
    kb.check(out, ref64, bound, "attention uniform V")


@pytest.mark.parametrize("shape,groups", [((2, 320, 68, 68), 32), ((1, 512, 64, 64), 32), ((2, 33, 7, 7), 3)])
def test_groupnorm_silu_numerics(extmod, shape, groups):
    torch.manual_seed(1)
    x = torch.randn(*shape)
    w = torch.randn(shape[1])
    b = torch.randn(shape[1])
    y = extmod.group_norm_fused(
        x.cuda().to(torch.bfloat16), groups, w.cuda(), b.cuda(), 1e-5, True
    ).float().cpu()
    ref = F.silu(F.group_norm(x, groups, w, b, 1e-5))
    # bf16 output quantization: |err| <= atol + bf16-relative term
    bound = 0.02 + 0.01 * ref.abs()
    assert ((y - ref).abs() <= bound).all(), (y - ref).abs().max().item()
    ref64, bound = kb.group_norm_ref(kb.bf16_exact(x), groups, w, b, 1e-5, True)
    kb.check(y, ref64, bound, f"group_norm_fused {shape} G={groups} silu")


def test_groupnorm_no_silu(extmod):
    x = torch.randn(2, 64, 32, 32)
    w, b = torch.ones(64), torch.zeros(64)
    y = extmod.group_norm_fused(
        x.cuda().to(torch.bfloat16), 32, w.cuda(), b.cuda(), 1e-5, False
    ).float().cpu()
    ref = F.group_norm(x, 32, w, b, 1e-5)
    assert (y - ref).abs().max().item() < 0.05
    ref64, bound = kb.group_norm_ref(kb.bf16_exact(x), 32, w, b, 1e-5, False)
    kb.check(y, ref64, bound, "group_norm_fused (2,64,32,32) G=32")


@pytest.mark.parametrize("t,c", [(4624, 320), (77, 768), (100, 1280), (3, 2048)])
def test_layernorm_numerics(extmod, t, c):
    torch.manual_seed(2)
    x = torch.randn(t, c)
    w, b = torch.randn(c), torch.randn(c)
    y = extmod.layer_norm(x.cuda().to(torch.bfloat16), w.cuda(), b.cuda(), 1e-5)
    ref = F.layer_norm(x, (c,), w, b, 1e-5)
    assert (y.float().cpu() - ref).abs().max().item() < 0.08
    ref64, bound = kb.layer_norm_ref(kb.bf16_exact(x), w, b, 1e-5)
    kb.check(y, ref64, bound, f"layer_norm ({t},{c})")


def test_act_mul_numerics(extmod):
    a = torch.randn(1000)
    b = torch.randn(1000)
    y = extmod.act_mul(a.cuda().to(torch.bfloat16), b.cuda().to(torch.bfloat16), False)
    assert (y.float().cpu() - a * F.silu(b)).abs().max().item() < 0.05
    y = extmod.act_mul(a.cuda().to(torch.bfloat16), b.cuda().to(torch.bfloat16), True)
    assert (y.float().cpu() - a * F.gelu(b, approximate="tanh")).abs().max().item() < 0.05
    for gelu in (False, True):
        y = extmod.act_mul(a.cuda().to(torch.bfloat16),
                           b.cuda().to(torch.bfloat16), gelu)
        ref64, bound = kb.act_mul_ref(kb.bf16_exact(a), kb.bf16_exact(b), gelu)
        kb.check(y, ref64, bound, f"act_mul n=1000 gelu={gelu}")


def test_extract_resize_matches_cpu(extmod):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(4)
    src = torch.rand(2, 128, 128, 3)
    for region, ow, oh in [((16, 16, 80, 80), 96, 96), ((0, 0, 128, 128), 64, 64),
                           ((100, 100, 128, 128), 40, 40)]:
        gpu = dispatch.extract_resize(src.cuda(), region, ow, oh).cpu()
        cpu = dispatch.extract_resize(src, region, ow, oh)
        err = (gpu - cpu).abs().max().item()
        assert err < 2e-3, f"{region} err {err}"


def test_blend_tile_matches_cpu(extmod):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(5)
    canvas = torch.rand(1, 96, 96, 3)
    tile = torch.rand(1, 48, 48, 3)
    region = (16, 16, 60, 60)
    rect = (24, 24, 56, 56)
    cg = canvas.cuda().contiguous()
    dispatch.blend_tile(cg, tile.cuda(), region, rect, 4.0)
    cc = canvas.clone()
    dispatch.blend_tile(cc, tile, region, rect, 4.0)
    err = (cg.cpu() - cc).abs().max().item()
    assert err < 2e-3, err


def test_native_extension_is_loaded(extmod):
    """Paper trail: the in-tree .so is what's loaded."""
    from comfyui_distributed_amd.ops import ext

    assert ext.SO_PATH.exists()
    assert ext.get_ext(required=True) is not None


# ---------------------------------------------------------------------------
# derived per-element bounds (tests/kernel_bounds.py) at shapes and code
# paths the tests above do not reach. Each prints max(err / bound).
# ---------------------------------------------------------------------------


def _dev_bf16(t):
    return t.to(torch.bfloat16).cuda()


@pytest.mark.parametrize("name,inp,kw", kb.attn_new_cases(),
                         ids=[c[0] for c in kb.attn_new_cases()])
def test_attention_packed_bound(extmod, name, inp, kw):
    """attention_packed with q, k ~ randn (logit std ~1, so one lost or
    misplaced key is worth tens of bounds): head dims that fill their pad
    class only partly, q-row counts around the 16-row fragment and the
    128-row block, an explicit scale, and GQA over several q-blocks with
    B*H = 8 (renumbered workgroups)."""
    from comfyui_distributed_amd.ops import dispatch

    q, k, v = kb.attn_inputs(**inp)
    heads, kv_heads = kw["heads"], kw.get("kv_heads", kw["heads"])
    ref, bound = kb.attention_ref(q, k, v, **kw)
    out = dispatch.attention_packed(
        _dev_bf16(kb.merge_heads(q, heads)),
        _dev_bf16(kb.merge_heads(k, kv_heads)),
        _dev_bf16(kb.merge_heads(v, kv_heads)),
        heads=heads, kv_heads=kv_heads, scale=kw.get("scale"))
    assert out.dtype == torch.bfloat16
    kb.check(out, kb.merge_heads(ref, heads), kb.merge_heads(bound, heads),
             f"attention_packed {name}")


@pytest.mark.parametrize("c,rs,silu", kb.SMALLC_CASES)
def test_conv_smallc_bound(extmod, c, rs, silu):
    """conv_smallc for every (C, RS) instantiation, with and without SiLU,
    K = 40 (8 k-slots of 5) and a last block of 30 pixels."""
    s = kb.SMALLC_SHAPE
    x, wk, bias = kb.conv_inputs(c * 100 + s["k"] + rs, s["b"], c, s["h"],
                                 s["w"], s["k"], rs)
    ref, bound = kb.conv_ref(x, wk, bias, silu=silu)
    y = extmod.conv_smallc(_dev_bf16(x), _dev_bf16(kb.repack_weight(wk)),
                           bias.cuda(), s["b"], s["h"], s["w"], c, s["k"], rs,
                           silu)
    kb.check(y, ref, bound, f"conv_smallc C={c} rs={rs} silu={silu}")


def _gn_fused(extmod, shape, groups, silu, seed, **kw):
    x, w, b = kb.norm_inputs(seed, shape, **kw)
    ref, bound = kb.group_norm_ref(x, groups, w, b, 1e-5, silu)
    y = extmod.group_norm_fused(_dev_bf16(x), groups, w.cuda(), b.cuda(), 1e-5,
                                silu)
    return kb.check(y, ref, bound,
                    f"group_norm_fused {shape} G={groups} silu={silu} {kw}")


@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_nchw_1024_threads(extmod, silu):
    """N*G = 1 < 128 and Cg*HW = 2^21 > 2^20: the launcher picks the
    1024-thread block (16 waves through the 16-float reduction scratch)."""
    shape, groups = kb.GN_NCHW_BIG
    _gn_fused(extmod, shape, groups, silu, shape[1] + groups)


def test_groupnorm_nchw_offset_input(extmod):
    """Input of mean 16, std 1. The kernel takes var = E[x^2] - mean^2 in
    fp32, which loses ~2^-23 * (mean/std)^2 of the variance: 2^-15 here. By
    CPU emulation (test_kernel_bounds_cpu.py) the bound holds at
    mean/std = 16, is left from ~32 on at elements where xhat*w + b cancels
    (3x at 64, 10x at 128), and the typical element is a whole bf16 ulp off
    only near mean/std 256-512. Activations of the models stay far below."""
    shape, groups = kb.GN_OFFSET_CASE
    _gn_fused(extmod, shape, groups, True, shape[1] + groups, **kb.NORM_OFFSET)


@pytest.mark.parametrize("c", kb.LN_CASES)
def test_layernorm_tail_and_wide_rows(extmod, c):
    """Rows whose length is not a multiple of 8 (scalar tail loop), shorter
    than one vector, and longer than one 512-element trip of the wave."""
    x, w, b = kb.norm_inputs(c, (kb.LN_T, c))
    ref, bound = kb.layer_norm_ref(x, w, b, 1e-5)
    y = extmod.layer_norm(_dev_bf16(x), w.cuda(), b.cuda(), 1e-5)
    kb.check(y, ref, bound, f"layer_norm ({kb.LN_T},{c})")


def test_layernorm_offset_input(extmod):
    """Mean 16 / std 1 rows: see test_groupnorm_nchw_offset_input."""
    c = kb.LN_OFFSET_C
    x, w, b = kb.norm_inputs(c, (kb.LN_T, c), **kb.NORM_OFFSET)
    ref, bound = kb.layer_norm_ref(x, w, b, 1e-5)
    y = extmod.layer_norm(_dev_bf16(x), w.cuda(), b.cuda(), 1e-5)
    kb.check(y, ref, bound, f"layer_norm ({kb.LN_T},{c}) mean 16")


@pytest.mark.parametrize("shape", kb.ACT_MUL_SHAPES, ids=str)
@pytest.mark.parametrize("gelu", [False, True])
def test_act_mul_sizes(extmod, shape, gelu):
    """Sizes below one vector, with a tail, 3-D, and past one full grid
    (second trip of the grid-stride loop plus a tail of 5)."""
    a, b = kb.act_mul_inputs(len(shape) + shape[0] % 1000, shape)
    ref, bound = kb.act_mul_ref(a, b, gelu)
    y = extmod.act_mul(_dev_bf16(a), _dev_bf16(b), gelu)
    assert y.shape == a.shape
    kb.check(y, ref, bound, f"act_mul {shape} gelu={gelu}")


# ---------------------------------------------------------------------------
# tile kernels vs the dispatch CPU path (2e-3, as above)
# ---------------------------------------------------------------------------

TILE_TOL = 2e-3
_RS_H, _RS_W = 90, 96
# (region, ow, oh, what)
RESIZE_CASES = [
    ((5, 4, 83, 82), 30, 30, "down 2.6x (filter clamp just past 2.5x)"),
    ((3, 0, 93, 90), 30, 30, "down 3x"),
    ((8, 5, 88, 85), 16, 16, "down 5x"),
    ((3, 10, 93, 40), 30, 30, "3x in x, 1x in y"),
    ((40, 30, 56, 46), 64, 64, "up 4x"),
    ((0, 0, _RS_W, _RS_H), 48, 45, "whole image"),
    ((_RS_W - 9, _RS_H - 9, _RS_W, _RS_H), 27, 27, "bottom-right corner"),
    ((-4, -6, 40, 38), 44, 44, "region starts outside the image"),
]


@pytest.mark.parametrize("region,ow,oh,what", RESIZE_CASES,
                         ids=[c[3] for c in RESIZE_CASES])
@pytest.mark.parametrize("c", [1, 4, 8])
def test_extract_resize_cases(extmod, region, ow, oh, what, c):
    from comfyui_distributed_amd.ops import dispatch

    g = torch.Generator().manual_seed(ow * 10 + c)
    src = torch.rand(2, _RS_H, _RS_W, c, generator=g)
    gpu = dispatch.extract_resize(src.cuda(), region, ow, oh).cpu()
    cpu = dispatch.extract_resize(src, region, ow, oh)
    assert gpu.shape == cpu.shape == (2, oh, ow, c)
    err = (gpu - cpu).abs().max().item()
    print(f"extract_resize {what} C={c}: max err {err:.2e}")
    assert err < TILE_TOL, f"{what} C={c}: err {err}"
    # batch 1 is its own image, not a copy of batch 0
    assert (cpu[0] - cpu[1]).abs().max().item() > 0.05


@pytest.mark.parametrize("region,ow,oh,what", RESIZE_CASES,
                         ids=[c[3] for c in RESIZE_CASES])
def test_extract_resize_constant_image(extmod, region, ow, oh, what):
    """The tap weights are renormalised to sum 1, so a constant image stays
    constant up to fp32 rounding over at most 16x16 taps."""
    from comfyui_distributed_amd.ops import dispatch

    src = torch.full((1, _RS_H, _RS_W, 3), 0.7)
    out = dispatch.extract_resize(src.cuda(), region, ow, oh).cpu()
    err = (out - 0.7).abs().max().item()
    print(f"extract_resize constant {what}: max |out - 0.7| {err:.2e}")
    assert err < 1e-4, f"{what}: {err}"


# (B, canvas H, W, tile h, w, region, mask rect, sigma, what)
BLEND_CASES = [
    (1, 96, 96, 44, 44, (16, 16, 60, 60), (24, 24, 56, 56), 0.0,
     "sigma 0: hard mask"),
    (2, 96, 96, 44, 44, (16, 16, 60, 60), (24, 24, 56, 56), 4.0, "B=2"),
    (1, 96, 96, 64, 64, (20, 30, 52, 62), (24, 34, 48, 58), 3.0,
     "tile twice the region size"),
    (1, 80, 96, 32, 32, (64, 48, 96, 80), (68, 52, 96, 80), 4.0,
     "region flush with the bottom-right corner"),
    (2, 80, 96, 32, 32, (0, 0, 32, 32), (0, 0, 28, 28), 0.0,
     "region flush with the top-left corner, sigma 0"),
    (1, 96, 96, 40, 40, (30, 30, 70, 70), (20, 40, 60, 90), 5.0,
     "mask rect partly outside the region"),
]


@pytest.mark.parametrize("b,ch,cw,th,tw,region,rect,sigma,what", BLEND_CASES,
                         ids=[c[8] for c in BLEND_CASES])
def test_blend_tile_cases(extmod, b, ch, cw, th, tw, region, rect, sigma, what):
    from comfyui_distributed_amd.ops import dispatch

    g = torch.Generator().manual_seed(th + cw)
    canvas = torch.rand(b, ch, cw, 3, generator=g)
    tile = torch.rand(b, th, tw, 3, generator=g)
    cg = canvas.cuda().contiguous()
    dispatch.blend_tile(cg, tile.cuda(), region, rect, sigma)
    cg = cg.cpu()
    cc = canvas.clone()
    dispatch.blend_tile(cc, tile, region, rect, sigma)
    err = (cg - cc).abs().max().item()
    print(f"blend_tile {what}: max err {err:.2e}")
    assert err < TILE_TOL, f"{what}: err {err}"
    x1, y1, x2, y2 = region
    assert (cc[:, y1:y2, x1:x2] - canvas[:, y1:y2, x1:x2]).abs().max() > 0.05
    # outside the region the canvas is untouched, bit for bit
    outside = torch.ones(ch, cw, dtype=torch.bool)
    outside[y1:y2, x1:x2] = False
    assert torch.equal(cg[:, outside], canvas[:, outside]), what
    if sigma <= 0:
        # hard mask: untouched outside the rect too, the tile inside it
        keep = torch.ones(ch, cw, dtype=torch.bool)
        keep[rect[1]:rect[3], rect[0]:rect[2]] = False
        assert torch.equal(cg[:, keep], canvas[:, keep]), what
