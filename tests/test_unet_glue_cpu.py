"""CPU side of the UNet glue changes: the GroupNorm addend argument, the
ResBlock that uses it, LayerNorm parameters handed over in fp32, and the
caches derived from parameters (fp32 copies, repacked conv weights, fused
QKV / KV weights), which follow in-place updates of their source. Every check
is exact: on CPU tensors the new argument is the old broadcast add."""

import pytest
import torch
import torch.nn.functional as F

from comfyui_distributed_amd.models.unet import (CrossAttention, FusedGroupNorm,
                                                ResBlock)
from comfyui_distributed_amd.ops import dispatch


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("silu", [False, True])
def test_group_norm_addend_is_the_broadcast_add(dtype, silu):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 64, 5, 7, generator=g).to(dtype)
    e = torch.randn(3, 64, generator=g).to(dtype)
    w = torch.randn(64, generator=g).to(dtype)
    b = torch.randn(64, generator=g).to(dtype)
    for xx in (x, x.contiguous(memory_format=torch.channels_last)):
        got = dispatch.group_norm_silu(xx, 32, w, b, 1e-5, silu, addend=e)
        want = dispatch.group_norm_silu(xx + e[:, :, None, None], 32, w, b,
                                        1e-5, silu)
        assert got.dtype == dtype and torch.equal(got, want)
    # a wrong batch row would pass a test whose rows are equal
    assert not torch.equal(e[0], e[1])


def test_fused_group_norm_forwards_addend():
    torch.manual_seed(5)
    norm = FusedGroupNorm(64, silu=True)
    with torch.no_grad():
        norm.weight.normal_()
        norm.bias.normal_()
    x, e = torch.randn(2, 64, 4, 4), torch.randn(2, 64)
    with torch.no_grad():
        assert torch.equal(norm(x, addend=e), norm(x + e[:, :, None, None]))
        assert torch.equal(norm(x, None), norm(x))


def _resblock_forward_before(block, x, emb):
    """ResBlock.forward as it was before norm2 took the projection as an
    addend, written out."""
    h = block.conv1(block.norm1(x))
    h = h + block.emb_proj(F.silu(emb))[:, :, None, None]
    h2 = block.norm2(h)
    return block.conv2(h2) + block.skip(x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 96)])
def test_resblock_matches_previous_forward(dtype, cin, cout):
    torch.manual_seed(7)
    block = ResBlock(cin, 32, cout).to(dtype)
    x = torch.randn(3, cin, 6, 5).to(dtype)
    emb = torch.randn(3, 32).to(dtype)
    with torch.no_grad():
        got = block(x, emb)
        want = _resblock_forward_before(block, x, emb)
    assert got.shape == (3, cout, 6, 5)
    assert torch.equal(got, want)


def test_layer_norm_fp32_parameter_copies():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(5, 324, generator=g).to(torch.bfloat16)
    w = torch.randn(324, generator=g).to(torch.bfloat16)
    b = torch.randn(324, generator=g).to(torch.bfloat16)
    got = dispatch.layer_norm(x, w, b, 1e-5)
    want = dispatch.layer_norm(x, w.float(), b.float(), 1e-5)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)


def test_f32_cache_is_exact_and_reused():
    """What dispatch.layer_norm hands the kernel on the GPU path: the exact
    fp32 values of the bf16 parameter, the same tensor on every call."""
    w = torch.nn.Parameter(torch.randn(40).to(torch.bfloat16))
    c1, c2 = dispatch._f32(w), dispatch._f32(w)
    assert c1 is c2 and c1.dtype == torch.float32
    assert torch.equal(c1, w.detach().float())
    f = torch.randn(8)
    assert dispatch._f32(f) is f


# ---------------------------------------------------------------------------
# caches derived from parameters follow in-place updates of their source
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("context_dim", [None, 48])
def test_cross_attention_follows_load_state_dict(context_dim):
    """forward, load_state_dict of a differently seeded twin, forward: the
    result is the twin's, bit for bit (self-attention: the cached fused QKV
    weight; cross-attention: the cached fused KV weight)."""
    torch.manual_seed(21)
    a = CrossAttention(64, context_dim, 2, 32)
    torch.manual_seed(22)
    b = CrossAttention(64, context_dim, 2, 32)
    x = torch.randn(2, 9, 64)
    ctx = None if context_dim is None else torch.randn(2, 5, context_dim)
    with torch.no_grad():
        before = a(x, ctx)
        want = b(x, ctx)
        assert not torch.equal(before, want)
        name = "_wqkv" if context_dim is None else "_wkv"
        cached = getattr(a, name)
        a.load_state_dict(b.state_dict())
        assert torch.equal(a(x, ctx), want)
        # refreshed in place, and left alone while nothing changes
        assert getattr(a, name) is cached
        assert a(x, ctx) is not None and getattr(a, name) is cached


def test_f32_cache_follows_inplace_update():
    w = torch.nn.Parameter(torch.randn(40).to(torch.bfloat16))
    c1 = dispatch._f32(w)
    with torch.no_grad():
        w.mul_(2)
    c2 = dispatch._f32(w)
    assert torch.equal(c2, w.detach().float())
    assert c2 is c1 and dispatch._f32(w) is c1


def test_repacked_weight_follows_inplace_update():
    torch.manual_seed(23)
    conv = torch.nn.Conv2d(32, 16, 3, padding=1)
    new = torch.randn_like(conv.weight)
    wt1 = dispatch._repacked_weight(conv)
    assert dispatch._repacked_weight(conv) is wt1
    with torch.no_grad():
        conv.weight.copy_(new)
    wt2 = dispatch._repacked_weight(conv)
    want = new.permute(0, 2, 3, 1).reshape(16, -1).to(torch.bfloat16)
    assert wt2.shape == (16, 9 * 32) and torch.equal(wt2, want)
    assert wt2 is wt1
