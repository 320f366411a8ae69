"""DiT glue ops (qk_norm_rope / norm_modulate / rms_norm / gated_residual):
the dispatch CPU paths must reproduce, bit for bit, the op sequences the WAN
and Flux models ran inline before the ops existed. The formulas below are
literal copies of those model methods."""

import pytest
import torch

from comfyui_distributed_amd.ops import dispatch


# --- the models' former inline formulas -----------------------------------

def wan_rmsnorm(x, weight, eps):
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (y * weight.float()).to(x.dtype)


def wan_apply_rope(x, cos, sin):
    """x: [B, N, H, D] (head-split view); rotate (even, odd) pairs of D."""
    x1, x2 = x[..., 0::2], x[..., 1::2]
    c = cos[None, : x.shape[1], None, :].to(x.dtype)
    s = sin[None, : x.shape[1], None, :].to(x.dtype)
    out = torch.empty_like(x)
    out[..., 0::2] = x1 * c - x2 * s
    out[..., 1::2] = x1 * s + x2 * c
    return out


def flux_rms(x, scale, heads):
    b, n, hd = x.shape
    d = hd // heads
    xv = x.view(b, n, heads, d).float()
    xv = xv * torch.rsqrt(xv.pow(2).mean(-1, keepdim=True) + 1e-6)
    return (xv * scale.float()).reshape(b, n, hd).to(x.dtype)


def flux_apply_rope_packed(x, cos, sin, heads):
    b, n, hd = x.shape
    d = hd // heads
    xv = x.view(b, n, heads, d // 2, 2)
    x1, x2 = xv[..., 0], xv[..., 1]
    c = cos[None, :, None, :]
    s = sin[None, :, None, :]
    out = torch.stack([x1 * c - x2 * s, x1 * s + x2 * c], dim=-1)
    return out.reshape(b, n, hd)


def flux_mod(x, shift, scale):
    return x * (1 + scale[:, None]) + shift[:, None]


# --- helpers ---------------------------------------------------------------

def _tables(npos, d, g):
    ang = torch.rand(npos, d // 2, generator=g) * 6.28
    return ang.cos(), ang.sin()


def _qk(b, n, h, d, g):
    """q, k as chunks of one fused [B, N, 3*H*D] projection output."""
    qkv = torch.randn(b, n, 3 * h * d, generator=g)
    q, k, _ = qkv.chunk(3, dim=-1)
    return q, k, torch.randn(d, generator=g), torch.randn(d, generator=g)


# --- tests -----------------------------------------------------------------

@pytest.mark.parametrize("b,n,h,d", [(2, 5, 2, 32), (1, 7, 3, 64), (2, 3, 2, 96)])
def test_qk_norm_rope_matches_wan_sequence(b, n, h, d):
    g = torch.Generator().manual_seed(0)
    q, k, wq, wk = _qk(b, n, h, d, g)
    cos, sin = _tables(n + 2, d, g)
    eps = 1e-6
    oq, ok = dispatch.qk_norm_rope(q, k, wq, wk, cos, sin, h, eps)
    hs = (b, n, h, d)
    rq = wan_apply_rope(wan_rmsnorm(q.reshape(hs), wq, eps), cos, sin)
    rk = wan_apply_rope(wan_rmsnorm(k.reshape(hs), wk, eps), cos, sin)
    assert oq.shape == (b, n, h * d) and oq.is_contiguous()
    assert torch.equal(oq, rq.reshape(b, n, -1))
    assert torch.equal(ok, rk.reshape(b, n, -1))
    assert not torch.equal(oq, ok)


@pytest.mark.parametrize("b,n,h,d", [(2, 5, 2, 32), (1, 7, 3, 64)])
def test_qk_norm_rope_matches_flux_sequence(b, n, h, d):
    g = torch.Generator().manual_seed(1)
    q, k, wq, wk = _qk(b, n, h, d, g)
    cos, sin = _tables(n, d, g)
    oq, ok = dispatch.qk_norm_rope(q, k, wq, wk, cos, sin, h, 1e-6)
    assert torch.equal(
        oq, flux_apply_rope_packed(flux_rms(q, wq, h), cos, sin, h))
    assert torch.equal(
        ok, flux_apply_rope_packed(flux_rms(k, wk, h), cos, sin, h))


def test_qk_norm_rope_token_offset_builds_joint_buffer():
    """Flux double-stream: txt at offset 0 and img at offset nt written into
    one buffer equal cat -> rope over the joint sequence; rows outside the
    written window keep their contents."""
    g = torch.Generator().manual_seed(2)
    b, nt, ni, h, d = 2, 3, 4, 2, 32
    tq, tk, wq_t, wk_t = _qk(b, nt, h, d, g)
    iq, ik, wq_i, wk_i = _qk(b, ni, h, d, g)
    pad = 2
    cos, sin = _tables(nt + ni + pad, d, g)
    sentinel = -77.0
    oq = torch.full((b, nt + ni + pad, h * d), sentinel)
    ok = torch.full((b, nt + ni + pad, h * d), sentinel)

    dispatch.qk_norm_rope(iq, ik, wq_i, wk_i, cos, sin, h, 1e-6,
                          token_offset=nt, out=(oq, ok))
    # only the img window is written so far
    assert (oq[:, :nt] == sentinel).all() and (ok[:, :nt] == sentinel).all()
    assert (oq[:, nt + ni:] == sentinel).all()
    assert (oq[:, nt:nt + ni] != sentinel).all()
    r = dispatch.qk_norm_rope(tq, tk, wq_t, wk_t, cos, sin, h, 1e-6,
                              token_offset=0, out=(oq, ok))
    assert r[0] is oq and r[1] is ok
    assert (oq[:, nt + ni:] == sentinel).all()
    assert (ok[:, nt + ni:] == sentinel).all()

    c, s = cos[:nt + ni], sin[:nt + ni]
    ref_q = flux_apply_rope_packed(
        torch.cat([flux_rms(tq, wq_t, h), flux_rms(iq, wq_i, h)], dim=1), c, s, h)
    ref_k = flux_apply_rope_packed(
        torch.cat([flux_rms(tk, wk_t, h), flux_rms(ik, wk_i, h)], dim=1), c, s, h)
    assert torch.equal(oq[:, :nt + ni], ref_q)
    assert torch.equal(ok[:, :nt + ni], ref_k)


@pytest.mark.parametrize("d", [12, 264])
def test_qk_norm_rope_rejects_head_dim(d):
    q = torch.randn(1, 2, 2 * d)
    w = torch.ones(d)
    cs = torch.ones(2, d // 2)
    with pytest.raises(ValueError):
        dispatch.qk_norm_rope(q, q, w, w, cs, cs, 2)


def test_qk_norm_rope_rejects_bad_windows():
    q = torch.randn(1, 4, 64)
    w = torch.ones(32)
    cs = torch.ones(5, 16)
    out = (torch.zeros(1, 5, 64), torch.zeros(1, 5, 64))
    with pytest.raises(ValueError):  # rows [2, 6) of a 5-row buffer
        dispatch.qk_norm_rope(q, q, w, w, cs, cs, 2, token_offset=2, out=out)
    with pytest.raises(ValueError):  # an offset with nowhere to put it
        dispatch.qk_norm_rope(q, q, w, w, cs, cs, 2, token_offset=1)
    with pytest.raises(ValueError):  # tables shorter than the window
        dispatch.qk_norm_rope(q, q, w, w, cs[:3], cs[:3], 2)


def test_norm_modulate_rms_matches_wan_sequence():
    g = torch.Generator().manual_seed(3)
    b, n, c = 2, 7, 72
    x = torch.randn(b, n, c, generator=g)
    w = torch.randn(c, generator=g)
    m = torch.randn(b, 6, c, generator=g)
    shift, scale = m.unbind(1)[:2]
    y = dispatch.norm_modulate(x, "rms", w, scale, shift, 1e-6)
    ref = wan_rmsnorm(x, w, 1e-6) * (1 + scale[:, None]) + shift[:, None]
    assert torch.equal(y, ref)
    # no modulation == plain RMSNorm == rms_norm, any leading shape
    assert torch.equal(dispatch.norm_modulate(x, "rms", w), wan_rmsnorm(x, w, 1e-6))
    assert torch.equal(dispatch.rms_norm(x, w, 1e-6), wan_rmsnorm(x, w, 1e-6))
    x4 = x.reshape(b, n, 3, 24)
    w4 = w[:24]
    assert torch.equal(dispatch.rms_norm(x4, w4, 1e-5), wan_rmsnorm(x4, w4, 1e-5))


def test_norm_modulate_layer_matches_flux_sequence():
    g = torch.Generator().manual_seed(4)
    b, n, c = 2, 7, 72
    x = torch.randn(b, n, c, generator=g) * 0.5 + 3.0
    shift, scale, _ = torch.randn(b, 3 * c, generator=g).chunk(3, dim=-1)
    ln = torch.nn.LayerNorm(c, elementwise_affine=False)
    y = dispatch.norm_modulate(x, "layer", None, scale, shift, ln.eps)
    assert torch.equal(y, flux_mod(ln(x), shift, scale))
    # eps defaults to nn.LayerNorm's
    assert torch.equal(dispatch.norm_modulate(x, "layer"), ln(x))


def test_norm_modulate_rejects_bad_arguments():
    x = torch.randn(1, 2, 8)
    w = torch.ones(8)
    s = torch.ones(1, 8)
    with pytest.raises(ValueError):
        dispatch.norm_modulate(x, "group", w)
    with pytest.raises(ValueError):
        dispatch.norm_modulate(x, "rms")
    with pytest.raises(ValueError):
        dispatch.norm_modulate(x, "layer", w)
    with pytest.raises(ValueError):
        dispatch.norm_modulate(x, "rms", w, scale=s)


def test_gated_residual_matches_inline_form():
    g = torch.Generator().manual_seed(5)
    b, n, c = 2, 9, 72
    x = torch.randn(b, n, c, generator=g)
    y = torch.randn(b, n, c, generator=g)
    gate = torch.randn(b, 6, c, generator=g).unbind(1)[2]
    assert not gate.is_contiguous()
    assert torch.equal(dispatch.gated_residual(x, gate, y),
                       x + gate[:, None] * y)


def test_ops_package_exports_dit_ops():
    from comfyui_distributed_amd import ops

    for name in ("qk_norm_rope", "norm_modulate", "rms_norm", "gated_residual"):
        assert getattr(ops, name) is getattr(dispatch, name)
        assert name in ops.__all__
