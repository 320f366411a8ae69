"""FP8 attention (ops.attention_fp8): the torch definition on an exact
construction, and the routing of the WAN / Flux blocks under ``attn_dtype``.
"""

import pytest
import torch

from comfyui_distributed_amd.models import quant
from comfyui_distributed_amd.ops import dispatch

D = dispatch.ATTN_FP8_D
R = 256   # q rows per workgroup of attn_fp8_kernel (ext.ATTN_FP8_QROWS)
# (b, h, nq, nk): nk around the 128-key tile, nq around the q-block; nq >= nk
# so that every key is selected; the last case has B*H = 8 (renumbered grid)
SELECT_CASES = [(2, 2, 1, 1), (2, 2, R - 1, 127), (2, 2, R, 128),
                (2, 2, R + 1, 129), (2, 2, 2 * R + 5, 261), (4, 2, R + 1, 129)]


def selection_case(b, h, nq, nk, seed=0):
    """q_i = k_pi(i): K rows are random +-2 vectors, so the matching logit is
    4 * 128 / sqrt(128) = 45 and every other ~N(0, 4): p' is 2^SP for one key
    and 0 for the rest. V is integer-valued in [-16, 16] with one +-448 per
    (batch, head, channel): its scale is exactly 1 and its codes are V.
    -> q, k, v (fp32, bf16-exact) and want = v[pi]."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 2, (b, nk, h * D), generator=g).float() * 4 - 2
    pi = torch.stack([torch.cat([torch.randperm(nk, generator=g),
                                 torch.randint(0, nk, (nq,), generator=g)])[:nq]
                      for _ in range(b)])
    pi = pi[:, torch.randperm(nq, generator=g)]
    v = torch.randint(-16, 17, (b, nk, h * D), generator=g).float()
    top = torch.randint(0, nk, (b, 1, h * D), generator=g)
    sign = torch.randint(0, 2, (b, 1, h * D), generator=g).float() * 2 - 1
    v.scatter_(1, top, 448.0 * sign)
    idx = pi[:, :, None].expand(-1, -1, h * D)
    return k.gather(1, idx), k, v, v.gather(1, idx)


@pytest.mark.parametrize("b,h,nq,nk", SELECT_CASES)
def test_definition_selects_exactly(b, h, nq, nk):
    q, k, v, want = selection_case(b, h, nq, nk)
    a = dispatch.quantize_attn_qkv(q, k, v, h)
    assert torch.equal(a.v_scale, torch.ones_like(a.v_scale))
    qd, kd, vd = a.dequant()
    assert torch.equal(vd, v)
    if nk > 1:   # the gap in nats between the match and the runner-up
        s = torch.einsum("bqhd,bkhd->bhqk", qd.reshape(b, nq, h, D),
                         kd.reshape(b, nk, h, D)) / D ** 0.5
        top2 = s.topk(2, dim=-1).values
        gap = (top2[..., 0] - top2[..., 1]).min().item()
        print(f"min logit gap {gap:.1f} nats")
        # 2^-(SP + 10) is half of p's smallest e4m3 step: 11.1 nats
        assert gap > 20.0
    assert torch.equal(dispatch.attention_fp8(q, k, v, h), want)
    assert torch.equal(dispatch.attention_fp8(a), want)


def test_errors():
    q = torch.zeros(1, 4, 2 * D)
    with pytest.raises(ValueError):
        dispatch.attention_fp8(q[..., :128], q[..., :128], q[..., :128], 2)
    with pytest.raises(ValueError):
        dispatch.attention_fp8(q, q[..., :D], q[..., :D], 2)   # kv heads
    with pytest.raises(ValueError):
        dispatch.attention_fp8(q, q, q, 2, scale=0.0)
    with pytest.raises(ValueError):
        dispatch.attention_fp8(q, q, q[:, :3], 2)
    with pytest.raises(ValueError):
        quant.resolve_attn_dtype("fp4")


def _tiny(family):
    """One-layer WAN / Flux models with head dim 128 and their inputs."""
    g = torch.Generator().manual_seed(3)
    torch.manual_seed(0)
    if family == "wan":
        from comfyui_distributed_amd.models.wan import WanConfig, WanModel

        model = WanModel(WanConfig(dim=256, ffn_dim=256, num_layers=1,
                                   num_heads=2, text_dim=32, in_channels=4,
                                   out_channels=4)).eval()
        return model, (torch.randn(1, 4, 1, 6, 8, generator=g),
                       torch.tensor([300.0]),
                       torch.randn(1, 5, 32, generator=g)), 1
    from comfyui_distributed_amd.models.flux import FluxConfig, FluxModel

    model = FluxModel(FluxConfig(dim=256, depth_double=1, depth_single=1,
                                 heads=2, context_dim=32, vec_dim=16,
                                 axes_dim=(16, 56, 56),
                                 guidance_embed=False)).eval()
    return model, (torch.randn(1, 16, 8, 8, generator=g), torch.tensor([500.0]),
                   torch.randn(1, 5, 32, generator=g),
                   torch.randn(1, 16, generator=g)), 2


@pytest.mark.parametrize("family", ["wan", "flux"])
def test_routing(family, monkeypatch):
    model, inputs, self_attns = _tiny(family)
    calls = {"fp8": 0, "packed": 0}
    fp8, packed = dispatch.attention_fp8, dispatch.attention_packed

    def count(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapped

    monkeypatch.setattr(dispatch, "attention_fp8", count("fp8", fp8))
    monkeypatch.setattr(dispatch, "attention_packed", count("packed", packed))
    cross = 1 if family == "wan" else 0
    with torch.no_grad():
        y0 = model(*inputs)
        assert calls == {"fp8": 0, "packed": self_attns + cross}
        assert quant.set_attn_dtype(model, "fp8") == self_attns
        calls.update(fp8=0, packed=0)
        y1 = model(*inputs)
    assert calls == {"fp8": self_attns, "packed": cross}
    rel = ((y1 - y0).norm() / y0.norm()).item()
    print(f"{family}: fp8 attention vs default, relative distance {rel:.4f}")
    assert torch.isfinite(y1).all() and rel == rel


def test_head_dim_is_checked_when_routing(monkeypatch):
    from comfyui_distributed_amd.models import create_diffusion_stack

    monkeypatch.setenv("DISTGPU_ATTN_DTYPE", "fp8")
    assert create_diffusion_stack("wan_tiny").attn_dtype is None  # head dim 32
    monkeypatch.delenv("DISTGPU_ATTN_DTYPE")
    with pytest.raises(ValueError):
        create_diffusion_stack("wan_tiny", attn_dtype="fp8")
    with pytest.raises(ValueError):
        create_diffusion_stack("sd15_tiny", attn_dtype="fp8")
