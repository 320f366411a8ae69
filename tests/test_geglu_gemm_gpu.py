"""gemm_geglu on the GPU against geglu_ref, every element, and its module route.
bf16-exact x ~ N(0, 1), Wa ~ N(0, 1/K), Wg ~ N(0, 2.25/K), bias ~ N(0, 0.25)."""

from collections import Counter

import pytest
import torch

import kernel_bounds as kb
from geglu_ref import geglu_ref
from comfyui_distributed_amd.models.unet import GEGLUFeedForward
from comfyui_distributed_amd.ops import dispatch

pytestmark = pytest.mark.gpu

KERNEL_CASES = [  # (M, K, inner, bn); bn None: the unpinned entry
    (256, 64, 16, 128),     # one K-tile, packed N = 32 far under the tile
    (300, 192, 144, 128), (300, 192, 144, 256),  # M, N tails; three K-tiles
    (513, 320, 272, 128), (513, 320, 272, 256),  # inner/16 odd; the real K
    (1100, 128, 1280, None),  # many N blocks, chooser
]


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("m,k,inner,bn", KERNEL_CASES)
def test_kernel_against_fp64(m, k, inner, bn, with_bias):
    g = torch.Generator().manual_seed(1000 * m + inner + (bn or 0))
    x = kb.bf16_exact(torch.randn(m, k, generator=g))
    std = torch.tensor([1.0, 1.5]).repeat_interleave(inner)[:, None] / k ** 0.5
    w = kb.bf16_exact(torch.randn(2 * inner, k, generator=g) * std)
    b = kb.bf16_exact(0.5 * torch.randn(2 * inner, generator=g))
    b = b if with_bias else None
    ref, bound = geglu_ref(x, w, b)
    wp, bp = dispatch.pack_geglu_weight(w.to(kb.BF).cuda(),
                                        None if b is None else b.cuda())
    ext, xg = dispatch.ext.get_ext(True), x.to(kb.BF).cuda()
    y = (ext.gemm_geglu(xg, wp, bp) if bn is None
         else ext.gemm_geglu_ex(xg, wp, bp, bn))
    kb.check(y, ref, bound, f"gemm_geglu {m} {k} {inner} bn{bn} b{with_bias}")


@pytest.fixture()
def calls(monkeypatch):
    counter, real = Counter(), dispatch.ext.get_ext

    class Proxy:
        def __getattr__(self, name):
            def counted(*args):
                counter[name] += 1
                return getattr(real(True), name)(*args)
            return counted

    monkeypatch.setattr(dispatch.ext, "get_ext", lambda required=None: Proxy())
    return counter


def _check_ff(ff, x, y, what):
    # proj_out in fp64 on the GEGLU reference; its bound carried through it
    p = {n: t.detach().float().cpu() for n, t in ff.named_parameters()}
    h_ref, h_bound = geglu_ref(x.float().reshape(-1, 64),
                               p["proj_in.weight"], p["proj_in.bias"])
    ref, bound = kb.linear_ref(h_ref, p["proj_out.weight"], p["proj_out.bias"])
    carried = h_bound @ p["proj_out.weight"].double().abs().t()
    rel = 1 + 2 * kb.U + (h_ref.shape[1] + 1) * 2.0 ** -23
    kb.check(y.reshape(-1, 64), ref, bound + rel * carried, what)


def test_module_route_output_and_parameter_update(calls, monkeypatch):
    torch.manual_seed(3)
    ff, x = GEGLUFeedForward(64).to(kb.BF).cuda(), torch.randn(2, 600, 64).to(kb.BF)
    monkeypatch.setattr(dispatch, "_GEGLU_GEMM", False)
    ff(x.cuda())
    assert calls["act_mul"] == 1 and calls["gemm_geglu"] == 0, dict(calls)
    monkeypatch.setattr(dispatch, "_GEGLU_GEMM", True)
    y = ff(x.cuda())
    assert calls["gemm_geglu"] == 1 and calls["act_mul"] == 1, dict(calls)
    _check_ff(ff, x, y, "GEGLUFeedForward, fused")
    packed = ff.proj_in.weight._distgpu_geglu[0]  # refreshed in place below
    ptr = packed.data_ptr()
    with torch.no_grad():
        ff.proj_in.weight.mul_(2)
        ff.proj_in.bias.copy_(torch.linspace(-1, 1, 512))
    _check_ff(ff, x, ff(x.cuda()), "GEGLUFeedForward after in-place update")
    assert ff.proj_in.weight._distgpu_geglu[0] is packed and packed.data_ptr() == ptr
