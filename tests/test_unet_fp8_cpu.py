"""The FP8 ops for the UNet's Linear widths without a GPU: the padded
quantiser's contract and the CPU definitions of the new ops against fp64."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import fp8_bounds as fb
from comfyui_distributed_amd.models.quant import Fp8GegluLinear, Fp8Linear
from comfyui_distributed_amd.ops import dispatch


def test_quantize_rows_pad_contract():
    x = torch.randn(2, 3, 320)
    with pytest.raises(ValueError):
        dispatch.quantize_rows(x)  # the default keeps the K % 128 contract
    for bad in (torch.randn(3, 96), torch.randn(1, 16384 + 64)):
        with pytest.raises(ValueError):
            dispatch.quantize_rows(bad, pad_k=True)
    rows = dispatch.quantize_rows(x, pad_k=True)
    assert rows.q.shape == (2, 3, 384) and rows.scale.shape == (2, 3)
    assert not rows.q.view(torch.uint8)[..., 320:].any()
    q, s = fb.quant_ref(x.reshape(-1, 320))
    assert torch.equal(rows.scale.reshape(-1), s)
    assert torch.equal(rows.q.view(torch.uint8)[..., :320].reshape(-1, 320),
                       q.view(torch.uint8))
    assert dispatch.quantize_rows(torch.randn(4, 256), pad_k=True).q.shape == (4, 256)


def test_cpu_definitions_against_fp64():
    m, k, inner = 9, 320, 48
    x, w, bias = fb.linear_inputs(m, 2 * inner, k, seed=5)
    g = torch.Generator().manual_seed(1)
    lw, lb = torch.randn(k, generator=g), torch.randn(k, generator=g)
    # layer_norm_fp8 = the padded quantiser of the LayerNorm
    rows = dispatch.layer_norm_fp8(x, lw, lb, 1e-5)
    ln = dispatch.layer_norm(x, lw, lb, 1e-5)
    ln64 = F.layer_norm(x.double(), (k,), lw.double(), lb.double(), 1e-5)
    assert (ln.double() - ln64).abs().max() <= 1e-5
    assert rows.q.shape == (m, 384)
    assert fb.quant_ratio(rows.q[:, :k], ln, rows.scale) <= 1.0
    assert torch.equal(rows.scale, fb.scale_ref(ln.abs().amax(dim=1)))
    # linear_geglu_fp8 on those rows = fp64 GEGLU of the quantised operands
    qw, sw = dispatch.quantize_weight_fp8(w, pad_k=True)
    pre, _ = fb.linear_fp8_pre(rows.q, rows.scale, qw, sw, bias)
    ref = pre[:, :inner] * F.gelu(pre[:, inner:], approximate="tanh")
    y = dispatch.linear_geglu_fp8(
        rows, *dispatch.pack_geglu_weight_fp8(w, bias, pad_k=True))
    assert y.shape == (m, inner)
    assert (y.double() - ref).abs().max() <= 1e-5 * ref.abs().max()
    # the modules: the same numbers from a tensor and from its rows
    lin = nn.Linear(k, 2 * inner)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(bias)
    gg = Fp8GegluLinear(lin, pad_k=True)
    assert gg.pad_k and gg.out_features == inner
    assert torch.equal(gg(rows), y) and torch.equal(gg(ln), y)
    f8 = Fp8Linear(lin, pad_k=True)
    assert (f8(ln).double() - pre).abs().max() <= 1e-5 * pre.abs().max()
    with pytest.raises(ValueError):
        Fp8Linear(lin)  # without pad_k the K % 128 contract holds

