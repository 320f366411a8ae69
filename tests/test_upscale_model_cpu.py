"""The RRDBNet upscale model without a GPU: conv3x3_dense's CPU formula on
slice-in-place operands, the dense-buffer forward against the textbook one,
the checkpoint key set and the two graph nodes."""

from __future__ import annotations

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from comfyui_distributed_amd.graph.executor import Executor, default_registry
from comfyui_distributed_amd.models.upscaler import create_upscale_model
from comfyui_distributed_amd.ops import dispatch

SENTINEL = 7.0


@pytest.mark.parametrize("case", ["lrelu", "residuals", "up2"])
def test_conv3x3_dense_cpu_in_place(case):
    torch.manual_seed(3)
    c, k, up2 = 64, 32, case == "up2"
    conv = nn.Conv2d(c, k, 3, 1, 1)
    x = torch.randn(2, 5, 7, c)
    ho, wo = (10, 14) if up2 else (5, 7)
    # x and out in one buffer unless the sizes differ
    buf = torch.full((2, ho, wo, 192), SENTINEL)
    out = buf[..., c:c + k]
    if up2:
        xv = x
    else:
        buf[..., :c] = x
        xv = buf[..., :c]
    kw, res1 = {}, None
    if case == "lrelu":
        kw = dict(lrelu=0.2)
    elif case == "residuals":     # out aliases res2
        res1 = torch.randn(2, ho, wo, k)
        out.copy_(torch.randn(2, ho, wo, k))
        kw = dict(alpha=0.04, res1=res1, beta1=0.2, res2=out)
    res2 = out.clone()
    t = F.conv2d(F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2)
                 if up2 else x.permute(0, 3, 1, 2),
                 conv.weight, conv.bias, padding=1).permute(0, 2, 3, 1)
    if case == "lrelu":
        t = F.leaky_relu(t, 0.2)
    if case == "residuals":
        t = 0.04 * t + 0.2 * res1 + res2
    with torch.no_grad():
        got = dispatch.conv3x3_dense(xv, conv, out, up2=up2, **kw)
    assert got is out
    torch.testing.assert_close(out, t.detach(), rtol=1e-5, atol=1e-5)
    assert (buf[..., c + k:] == SENTINEL).all()
    if up2:
        assert (buf[..., :c] == SENTINEL).all()
    else:
        assert torch.equal(buf[..., :c], x)


def test_dense_forward_matches_textbook_cpu():
    model = create_upscale_model("rrdb_tiny", seed=5)
    x = torch.rand(2, 6, 9, 3, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        dense = model(x, route="dense")
        cat = model(x, route="cat")
    assert dense.shape == cat.shape == (2, 24, 36, 3)
    scale = cat.abs().max().item()
    assert scale > 0
    # two fp32 evaluations of ~40 convs in different summation orders
    assert (dense - cat).abs().max().item() <= 1e-4 * scale


def test_state_dict_keys_follow_the_public_layout():
    model = create_upscale_model("rrdb_tiny")
    convs = ["conv_first", "conv_body", "conv_up1", "conv_up2", "conv_hr",
             "conv_last"]
    convs += [f"body.{i}.rdb{r}.conv{j}" for i in range(2) for r in (1, 2, 3)
              for j in range(1, 6)]
    assert set(model.state_dict()) == {f"{c}.{p}" for c in convs
                                       for p in ("weight", "bias")}
    assert model.body[0].rdb2.conv4.weight.shape == (32, 160, 3, 3)
    assert model.body[1].rdb3.conv5.weight.shape == (64, 192, 3, 3)


def test_upscale_nodes_run_in_a_graph():
    reg = default_registry()
    loader, upscale = reg.get("UpscaleModelLoader"), reg.get("ImageUpscaleWithModel")
    assert loader.RETURN_TYPES == ("UPSCALE_MODEL",)
    assert upscale.INPUT_TYPES()["required"].keys() == {"upscale_model", "image"}
    prompt = {
        "1": {"class_type": "LoadImage", "inputs": {"image": "synthetic:10x6"}},
        "2": {"class_type": "UpscaleModelLoader",
              "inputs": {"model_name": "rrdb_tiny"}},
        "3": {"class_type": "ImageUpscaleWithModel",
              "inputs": {"upscale_model": ["2", 0], "image": ["1", 0]}},
    }
    out = Executor(context={"device": "cpu"}).execute(prompt)["3"][0]
    assert out.shape == (1, 24, 40, 3)
    assert torch.isfinite(out).all() and out.min() >= 0 and out.max() <= 1
