"""FP8 Linear path without a GPU: the bounds of fp8_bounds.py hold for a
faithful fp32 emulation and reject seeded defects; dispatch.linear_fp8's CPU
path computes the reference; quantize_linears / create_diffusion_stack /
CheckpointLoader route the right layers.

Measured here (CPU): emulation at 0.40-0.49 of the GEMM bound; a dropped
32-wide K block leaves it by 151-1552x, weight scales shifted by one channel
by 4300x and more, a row scale from the neighbouring row by 2000x and more;
the torch quantiser sits at 0.99998 of its bound, a truncating one at 2.0.
"""

import pytest
import torch
from torch import nn

import fp8_bounds as fb
from comfyui_distributed_amd.ops import dispatch

SHAPES = [(5, 24, 128), (300, 130, 384), (257, 200, 1280)]   # (M, N, K)


def _quantised(m, n, k, seed=0):
    x, w, bias = fb.linear_inputs(m, n, k, seed)
    qa, sa = fb.quant_ref(x)
    qw, sw = fb.quant_ref(w)
    return x, w, bias, qa, sa, qw, sw


@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("act", fb.ACTS)
def test_emulation_inside_gemm_bound(m, n, k, act):
    _, _, bias, qa, sa, qw, sw = _quantised(m, n, k)
    for b in (None, bias):
        ref, bound = fb.linear_fp8_bound(qa, sa, qw, sw, b, act)
        r = fb.check(fb.emulate_gemm(qa, sa, qw, sw, b, act), ref, bound,
                     f"emulation {m, n, k} act={act} bias={b is not None}")
        assert r <= 0.75


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_seeded_gemm_defects_leave_bound(m, n, k):
    _, _, bias, qa, sa, qw, sw = _quantised(m, n, k)
    ref, bound = fb.linear_fp8_bound(qa, sa, qw, sw, bias)
    defects = {
        "dropped K block": dict(drop_k=k - 64),
        "weight scales shifted": dict(sw_shift=1),
        "row scale from neighbour": dict(sa_shift=1),
    }
    for name, kw in defects.items():
        r = fb.err_ratio(fb.emulate_gemm(qa, sa, qw, sw, bias, **kw), ref, bound)
        print(f"{name} {m, n, k}: err/bound {r:.1f}")
        assert r > 10, (name, r)


@pytest.mark.parametrize("m,k", [(5, 128), (70, 384), (3, 5120)])
def test_quantiser_bound_and_truncation(m, k):
    x, _, _ = fb.linear_inputs(m, 8, k, seed=1)
    x[m // 2] = 0                                   # an all-zero row
    q, scale = fb.quant_ref(x)
    r = fb.quant_ratio(q, x, scale)
    print(f"torch quantiser {m, k}: {r:.5f}")
    assert r <= 1.0
    assert (q[m // 2].float() == 0).all() and scale[m // 2] > 0
    qt, st = fb.quant_truncating(x)
    rt = fb.quant_ratio(qt, x, st)
    print(f"truncating quantiser {m, k}: {rt:.3f}")
    assert rt > 1.5


def test_dispatch_quantisers_match_reference():
    x, w, _ = fb.linear_inputs(9, 40, 256, seed=2)
    q, s = dispatch.quant_rows_fp8(x)
    qr, sr = fb.quant_ref(x)
    assert torch.equal(s, sr)
    assert torch.equal(q.view(torch.uint8), qr.view(torch.uint8))
    qw, sw = dispatch.quantize_weight_fp8(w)
    qwr, swr = fb.quant_ref(w)
    assert qw.dtype == torch.float8_e4m3fn and sw.dtype == torch.float32
    assert torch.equal(sw, swr)
    assert torch.equal(qw.view(torch.uint8), qwr.view(torch.uint8))


@pytest.mark.parametrize("act", fb.ACTS)
def test_dispatch_linear_fp8_cpu(act):
    m, n, k = 300, 130, 384
    x, w, bias = fb.linear_inputs(m, n, k, seed=3)
    qw, sw = dispatch.quantize_weight_fp8(w)
    y = dispatch.linear_fp8(x.reshape(3, 100, k), qw, sw, bias, act)
    assert y.shape == (3, 100, n) and y.dtype == x.dtype
    qa, sa = fb.quant_ref(x)
    ref, bound = fb.linear_fp8_bound(qa, sa, qw, sw, bias, act)
    fb.check(y.reshape(m, n), ref, bound, f"dispatch.linear_fp8 cpu act={act}")


def test_linear_fp8_rejects_unsupported_shapes():
    qw, sw = dispatch.quantize_weight_fp8(torch.randn(16, 128))
    with pytest.raises(ValueError):
        dispatch.linear_fp8(torch.randn(4, 64), qw[:, :64].contiguous(), sw)
    with pytest.raises(ValueError):
        dispatch.linear_fp8(torch.randn(4, 256), qw, sw)      # K mismatch
    big = torch.zeros(1, 16384 + 128)
    with pytest.raises(ValueError):
        dispatch.linear_fp8(big, big.to(torch.float8_e4m3fn), sw[:1])
    with pytest.raises(ValueError):
        dispatch.linear_fp8(torch.randn(4, 128), qw, sw, act="relu")


# ---------------------------------------------------------------------------
# model layer and public interface
# ---------------------------------------------------------------------------


def _fp8_names(module):
    from comfyui_distributed_amd.models.quant import Fp8Linear

    return {n for n, m in module.named_modules() if isinstance(m, Fp8Linear)}


def _linear_names(module):
    return {n for n, m in module.named_modules() if isinstance(m, nn.Linear)}


def test_quantize_linears_wan_block():
    from comfyui_distributed_amd.models.quant import quantize_linears, weight_bytes
    from comfyui_distributed_amd.models.wan import WanBlock, WanConfig, rope_3d

    cfg = WanConfig(dim=128, ffn_dim=256, num_layers=1, num_heads=2,
                    text_dim=128, in_channels=4, out_channels=4)
    torch.manual_seed(0)
    blk = WanBlock(cfg).eval()
    ref_blk = WanBlock(cfg).eval()
    ref_blk.load_state_dict(blk.state_dict())
    before = weight_bytes(blk)
    assert quantize_linears(blk) == 10
    assert _fp8_names(blk) == {"q", "k", "v", "o", "cq", "ck", "cv", "co",
                               "ffn1", "ffn2"}
    assert not _linear_names(blk)
    assert blk.ffn1.act == "silu" and blk.ffn2.act is None
    assert blk.q.qweight.dtype == torch.float8_e4m3fn
    assert not hasattr(blk.q, "weight")
    assert weight_bytes(blk) < 0.35 * before            # fp32 -> e4m3 here
    # dtype casts leave the e4m3 weight and the fp32 scales alone
    blk.to(torch.bfloat16)
    assert blk.q.qweight.dtype == torch.float8_e4m3fn
    assert blk.q.wscale.dtype == torch.float32
    blk.to(torch.float32)

    x = torch.randn(2, 12, 128)
    emb6 = torch.randn(2, 6, 128) * 0.1
    ctx = torch.randn(2, 5, 128)
    cs = rope_3d(1, 3, 4, 64, "cpu")
    with torch.no_grad():
        y, y_ref = blk(x, emb6, ctx, cs), ref_blk(x, emb6, ctx, cs)
    assert y.shape == y_ref.shape and torch.isfinite(y).all()
    rel = ((y - y_ref).norm() / y_ref.norm()).item()
    print(f"WAN block fp8 vs fp32, relative Frobenius distance {rel:.4f}")
    # one fp8 Linear is 3.5-4.8 % from its bf16 result; a broken layer (a
    # doubled SiLU, a swapped weight) moves the block output by order 1
    assert rel < 0.25

    # a predicate vetoes layers by name
    blk2 = WanBlock(cfg)
    assert quantize_linears(blk2, lambda name, lin: name.startswith("c")) == 4
    assert _fp8_names(blk2) == {"cq", "ck", "cv", "co"}


def test_quantize_linears_flux_tiny_and_wan_tiny(monkeypatch):
    from comfyui_distributed_amd.models import create_diffusion_stack

    monkeypatch.delenv("DISTGPU_LINEAR_DTYPE", raising=False)
    base = create_diffusion_stack("flux_tiny", seed=3)
    assert base.linear_dtype is None and base.fp8_linears == 0
    assert not _fp8_names(base.model)

    stack = create_diffusion_stack("flux_tiny", seed=3, linear_dtype="fp8")
    want = {f"double_blocks.0.{p}_{n}" for p in ("img", "txt")
            for n in ("qkv", "proj", "mlp.0", "mlp.2")}
    want |= {"single_blocks.0.linear1", "single_blocks.0.linear2"}
    assert stack.fp8_linears == 10 and _fp8_names(stack.model) == want
    # embedders, modulation and the output head stay nn.Linear
    assert _linear_names(stack.model) == _linear_names(base.model) - want
    blk = stack.model.double_blocks[0]
    assert blk.img_mlp[0].act == "gelu_tanh"
    assert isinstance(blk.img_mlp[1], nn.Identity)
    assert stack.model.single_blocks[0].linear1.act is None
    assert stack.parameters_bytes() < base.parameters_bytes()

    x = torch.randn(1, 16, 8, 8)
    t = torch.tensor([500.0])
    cond = base.make_conditioning(0)
    with torch.no_grad():
        y = stack.model(x, t, cond["context"], cond["vec"])
        y_ref = base.model(x, t, cond["context"], cond["vec"])
    assert y.shape == y_ref.shape and torch.isfinite(y).all()
    rel = ((y - y_ref).norm() / y_ref.norm()).item()
    print(f"flux_tiny fp8 vs fp32, relative Frobenius distance {rel:.4f}")
    assert rel < 0.25

    # wan_tiny (dim 64): nothing fits the kernel's contract, nothing converts
    wan = create_diffusion_stack("wan_tiny", linear_dtype="fp8")
    assert wan.fp8_linears == 0 and not _fp8_names(wan.model)


def test_linear_dtype_env_default_and_unet_error(monkeypatch):
    from comfyui_distributed_amd.models import create_diffusion_stack

    monkeypatch.setenv("DISTGPU_LINEAR_DTYPE", "fp8")
    assert create_diffusion_stack("flux_tiny").fp8_linears == 10
    # the env default is only read by the families that act on it
    create_diffusion_stack("tiny")
    monkeypatch.setenv("DISTGPU_LINEAR_DTYPE", "int3")
    with pytest.raises(ValueError):
        create_diffusion_stack("flux_tiny")
    monkeypatch.delenv("DISTGPU_LINEAR_DTYPE")
    assert create_diffusion_stack("flux_tiny").fp8_linears == 0
    with pytest.raises(ValueError, match="UNet"):
        create_diffusion_stack("tiny", linear_dtype="fp8")
    with pytest.raises(ValueError):
        create_diffusion_stack("flux_tiny", linear_dtype="fp4")


def test_checkpoint_loader_weight_dtype(monkeypatch):
    from comfyui_distributed_amd.graph.builtin_nodes import (
        _STACK_CACHE, CheckpointLoader)

    monkeypatch.delenv("DISTGPU_LINEAR_DTYPE", raising=False)
    spec = CheckpointLoader.INPUT_TYPES()
    assert "weight_dtype" in spec["optional"]
    assert "weight_dtype" not in spec["required"]
    node = CheckpointLoader()
    node.set_context({"device": "cpu"})
    fp8, _, _ = node.load("flux_tiny", weight_dtype="fp8_e4m3fn")
    plain, _, _ = node.load("flux_tiny")
    assert fp8 is not plain
    assert fp8.fp8_linears == 10 and plain.fp8_linears == 0
    assert _STACK_CACHE[("flux_tiny", "cpu")] is plain
    assert _STACK_CACHE[("flux_tiny", "cpu", "fp8_e4m3fn")] is fp8
    assert node.load("flux_tiny", weight_dtype="fp8_e4m3fn")[0] is fp8
    with pytest.raises(ValueError):
        node.load("flux_tiny", weight_dtype="int4")
