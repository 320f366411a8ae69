"""GEGLU-fused Linear without a GPU: pairing, CPU composition, flag-off route."""

import pytest
import torch
import torch.nn.functional as F

from comfyui_distributed_amd.models.unet import GEGLUFeedForward
from comfyui_distributed_amd.ops import dispatch


@pytest.mark.parametrize("inner", [16, 48, 1280])
def test_pack_pairs_value_and_gate_rows(inner):
    rows = torch.arange(2.0 * inner)  # row r holds r: packed rows name sources
    wp, bp = dispatch.pack_geglu_weight(rows[:, None].repeat(1, 3), rows)
    j = torch.arange(inner)
    value_at, gate_at = 32 * (j // 16) + j % 16, 32 * (j // 16) + 16 + j % 16
    for packed in (wp[:, 0], wp[:, 2], bp):
        assert torch.equal(packed[value_at], rows[:inner])
        assert torch.equal(packed[gate_at], rows[inner:])
    assert dispatch.pack_geglu_weight(rows[:, None])[1].numel() == 0


@pytest.mark.parametrize("with_bias", [True, False])
def test_linear_geglu_cpu_is_the_three_steps(with_bias):
    torch.manual_seed(5)
    x, w = torch.randn(3, 7, 24), torch.randn(96, 24)
    b = torch.randn(96) if with_bias else None
    a, gate = F.linear(x, w, b).chunk(2, dim=-1)
    want = a * F.gelu(gate, approximate="tanh")
    assert torch.equal(dispatch.linear_geglu(x, w, b), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_feed_forward_flag_off_is_parent_formula(dtype, monkeypatch):
    monkeypatch.setattr(dispatch, "_GEGLU_GEMM", False)
    torch.manual_seed(11)
    ff, x = GEGLUFeedForward(dim=16).to(dtype), torch.randn(2, 9, 16).to(dtype)
    a, gate = F.linear(x, ff.proj_in.weight, ff.proj_in.bias).chunk(2, dim=-1)
    h = (a.float() * F.gelu(gate.float(), approximate="tanh")).to(dtype)
    assert torch.equal(ff(x), F.linear(h, ff.proj_out.weight, ff.proj_out.bias))
