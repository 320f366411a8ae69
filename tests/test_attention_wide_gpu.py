"""attn_wide_kernel (head dims 168..512) against the fp64 reference, inside
the unchanged attention bound of kernel_bounds (the kernel has the arithmetic
it was derived for: bf16 P, fp32 accumulation over Nk and D, one output
rounding). q, k ~ randn at the default scale: one lost or misplaced key or
D-fragment is worth tens of bounds.
"""

import math

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def extmod():
    from comfyui_distributed_amd.ops import ext

    return ext.get_ext(required=True)


def _legacy(extmod, seed, b, h, nq, nk, d, hkv=None, qk_std=1.0, scale=None):
    """dispatch.attention on [B*H, N, D] against kb.attention_ref."""
    from comfyui_distributed_amd.ops import dispatch

    hkv = hkv or h
    q, k, v = kb.attn_inputs(seed, b * h, b * hkv, nq, nk, d, qk_std)
    out = dispatch.attention(q.cuda().to(BF), k.cuda().to(BF), v.cuda().to(BF),
                             heads=h, kv_heads=hkv, scale=scale)
    ref, bound = kb.attention_ref(q, k, v, h, hkv, scale)
    kb.check(out, ref, bound, f"wide b{b} h{h}/{hkv} nq{nq} nk{nk} d{d}")


# first D above the old cap, partial and exact fill of both pad classes; a
# second key tile with a tail
@pytest.mark.parametrize("h", [1, 2])
@pytest.mark.parametrize("d", [168, 200, 256, 264, 384, 504, 512])
def test_head_dims(extmod, d, h):
    _legacy(extmod, d + h, 2, h, 40, 77, d)


# R = 64 q rows per workgroup (W_QROWS): 1, 17, R-1, R, R+1, 2R+5
@pytest.mark.parametrize("nq", [1, 17, 63, 64, 65, 133])
def test_q_rows(extmod, nq):
    _legacy(extmod, 500 + nq, 2, 1, nq, 65, 512)


# KT = 32 keys per tile (W_KT): 1, KT-1, KT, KT+1, 2KT+3
@pytest.mark.parametrize("nk", [1, 31, 32, 33, 67])
def test_keys(extmod, nk):
    _legacy(extmod, 600 + nk, 2, 1, 40, nk, 264)


@pytest.mark.parametrize("d,h", [(512, 1), (256, 2)])
@pytest.mark.parametrize("entry", ["attention", "packed", "qkv", "q_kv"])
def test_entries(extmod, entry, d, h):
    """Row strides H*D, 3*H*D and 2*H*D and the k / v base offsets."""
    from comfyui_distributed_amd.ops import dispatch

    b, n = 2, 150
    if entry == "attention":
        return _legacy(extmod, 7, b, h, n, n, d)
    q, k, v = (kb.merge_heads(u, h)
               for u in kb.attn_inputs(8, b * h, b * h, n, n, d))
    dev = lambda u: u.cuda().to(BF)  # noqa: E731
    if entry == "packed":
        out = dispatch.attention_packed(dev(q), dev(k), dev(v), heads=h)
        ref, bound = kb.attention_packed_ref(q, k, v, h)
    elif entry == "qkv":
        qkv = torch.cat([q, k, v], dim=-1)
        out = dispatch.attention_qkv(dev(qkv), heads=h)
        ref, bound = kb.attention_qkv_ref(qkv, h)
    else:
        kv = torch.cat([k, v], dim=-1)
        out = dispatch.attention_q_kv(dev(q), dev(kv), heads=h)
        ref, bound = kb.attention_q_kv_ref(q, kv, h)
    kb.check(out, ref, bound, f"wide {entry} d{d} h{h}")


def test_gqa(extmod):
    """B*H % 8 == 0: the renumbered grid; query head h reads kv head h // 4."""
    _legacy(extmod, 9, 1, 8, 300, 300, 256, hkv=2)


@pytest.mark.parametrize("mult", kb.ATTN_SCALE_MULT)
def test_explicit_scale(extmod, mult):
    _legacy(extmod, 70 + int(2 * mult), 2, 1, 40, 77, 512,
            qk_std=mult ** -0.5, scale=mult / math.sqrt(512))


def test_bit_identical(extmod):
    from comfyui_distributed_amd.ops import dispatch

    q, k, v = (u.cuda().to(BF) for u in kb.attn_inputs(11, 2, 2, 300, 300, 512))
    a = dispatch.attention(q, k, v, heads=1)
    b = dispatch.attention(q, k, v, heads=1)
    assert torch.equal(a, b)
