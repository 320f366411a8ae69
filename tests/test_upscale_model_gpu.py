"""RRDBNet (rrdb_tiny, bf16) on the GPU against a written-out fp64 functional
forward built from ``state_dict()`` by name; it calls no ``forward`` and no
``ops.dispatch``. Metric and margins as in test_module_bounds_gpu.py:
``e_rms`` / ``e_max`` of module_refs, allowed 2x / 3x of the yardstick, which
is the same forward with a bf16 rounding wherever the eager model stores a
tensor (each conv, LeakyReLU, scale and add). The dense route rounds at fewer
places (its epilogues fuse scale and add), so a healthy run sits at or under
1x; the ``DISTGPU_RRDB_HIP=0`` route is the eager model itself."""

import pytest
import torch
import torch.nn.functional as F

import module_refs as mr
from comfyui_distributed_amd.models.upscaler import create_upscale_model
from comfyui_distributed_amd.ops import dispatch

pytestmark = pytest.mark.gpu

RMS_LIMIT, MAX_LIMIT = 2.0, 3.0


def rrdbnet_ref(P, x, nb, rnd):
    """x [B, 3, H, W] fp64 -> [B, 3, 4H, 4W]."""
    def conv(name, t):
        return rnd(F.conv2d(t, P[name + ".weight"], P[name + ".bias"],
                            padding=1))

    def lrelu(t):
        return rnd(F.leaky_relu(t, 0.2))

    def up(t):
        return F.interpolate(t, scale_factor=2, mode="nearest")

    feat = h = conv("conv_first", x)
    for i in range(nb):
        x_rrdb = h
        for r in (1, 2, 3):
            feats = [h]
            for j in (1, 2, 3, 4):
                feats.append(lrelu(conv(f"body.{i}.rdb{r}.conv{j}",
                                        torch.cat(feats, 1))))
            t = conv(f"body.{i}.rdb{r}.conv5", torch.cat(feats, 1))
            h = rnd(rnd(t * 0.2) + h)
        h = rnd(rnd(h * 0.2) + x_rrdb)
    h = rnd(feat + conv("conv_body", h))
    h = lrelu(conv("conv_up1", up(h)))
    h = lrelu(conv("conv_up2", up(h)))
    return conv("conv_last", lrelu(conv("conv_hr", h)))


@pytest.fixture(scope="module")
def setup():
    model = create_upscale_model("rrdb_tiny", seed=7)
    x = mr.randn_bf16(21, 2, 12, 20, 3).mul_(0.25).add_(0.5).clamp_(0, 1)
    x = x.to(mr.BF).float()
    P = mr.params_of(model)
    x64 = x.to(mr.F64).permute(0, 3, 1, 2)
    with torch.no_grad():
        ref = rrdbnet_ref(P, x64, 2, mr.ident).permute(0, 2, 3, 1)
        yard = rrdbnet_ref(P, x64, 2, mr.bf16).permute(0, 2, 3, 1)
    return model.to(mr.BF).cuda(), x.cuda(), ref, mr.errors(yard, ref)


@pytest.mark.parametrize("hip", [True, False], ids=["dense", "rrdb_hip_0"])
def test_rrdb_tiny_against_fp64(setup, monkeypatch, hip):
    model, x, ref, (y_rms, y_max) = setup
    assert dispatch.hip_available() and dispatch._RRDB_HIP
    monkeypatch.setattr(dispatch, "_RRDB_HIP", hip)
    with torch.no_grad():
        y = model(x)
        img = model.upscale(x)
    torch.cuda.synchronize()
    e_rms, e_max = mr.errors(y, ref)
    print(f"RRDB hip={hip} e_rms {e_rms:.3e} ({e_rms / y_rms:.3f}x yardstick) "
          f"e_max {e_max:.3e} ({e_max / y_max:.3f}x)")
    assert e_rms <= RMS_LIMIT * y_rms and e_max <= MAX_LIMIT * y_max
    assert img.shape == (2, 48, 80, 3) and img.dtype == torch.float32
    assert torch.isfinite(img).all() and img.min() >= 0 and img.max() <= 1
