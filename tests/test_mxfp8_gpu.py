"""MXFP8 kernels (ops/hip/gemm_mxfp8.hip) on the GPU: the quantiser bit for
bit against the CPU definition, the GEMM's lane-to-block map and scale routing
with exactly representable data, random data inside gemm_fp8's bound, and the
emitting epilogue bit for bit against the quantiser."""

import pytest
import torch

import fp8_bounds as fb
import mxfp8_cases as mc
from comfyui_distributed_amd.ops import dispatch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("k", [128, 384])
def test_quantiser_matches_definition(m, k):
    x = mc.rows(m, k, seed=10 * m + k)
    q_ref, e_ref = dispatch.quant_rows_mxfp8(x)
    q, e = dispatch.quant_rows_mxfp8(x.to(DEV))
    assert torch.equal(e.cpu(), e_ref) and mc.same_bytes(q, q_ref)


def _integer_case(m, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    qa = torch.randint(-8, 9, (m, k), generator=g).float().to(mc.FP8)
    qw = torch.randint(-8, 9, (n, k), generator=g).float().to(mc.FP8)
    ea = (127 + torch.randint(-3, 4, (m, k // 32), generator=g)).to(torch.uint8)
    sw = 2.0 ** torch.randint(-2, 3, (n,), generator=g).float()
    bias = torch.randint(-64, 65, (n,), generator=g).float()
    return qa, ea, qw, sw, bias


@pytest.mark.parametrize("n", [8, 260])
@pytest.mark.parametrize("m", [1, 255, 257])
@pytest.mark.parametrize("k", [128, 384])
def test_gemm_integer_exact(k, m, n):
    """Codes in [-8, 8], block exponents in [-3, 3] differing between
    neighbouring blocks and rows, power-of-two channel scales, integer bias:
    every partial sum is a multiple of 2^-3 below 384 * 64 * 8 < 2^18, exact
    in fp32, so the result is the fp64 reference rounded once to bf16."""
    qa, ea, qw, sw, bias = _integer_case(m, n, k, seed=k + m + n)
    ref = (dispatch.mx_dequant(qa, ea).double() @ qw.float().double().t()
           ) * sw.double() + bias.double()
    y = dispatch.gemm_mxfp8(qa.to(DEV), ea.to(DEV), qw.to(DEV), sw.to(DEV),
                            bias.to(DEV))
    assert y.dtype == torch.bfloat16 and y.shape == (m, n)
    assert mc.same_bytes(y.view(torch.int16), ref.bfloat16().view(torch.int16))


def _random_case():
    m, n, k = 257, 264, 256
    x, w, bias = fb.linear_inputs(m, n, k, seed=7)
    qa, ea = dispatch.quant_rows_mxfp8(x.bfloat16())
    qw, sw = dispatch.quantize_weight_fp8(w)
    return qa, ea, qw, sw, bias


@pytest.mark.parametrize("act", fb.ACTS)
def test_gemm_random_inside_fp8_bound(act):
    qa, ea, qw, sw, bias = _random_case()
    ref, bound = fb.linear_fp8_bound(dispatch.mx_dequant(qa, ea),
                                     torch.ones(qa.shape[0]), qw, sw, bias, act)
    y = dispatch.gemm_mxfp8(qa.to(DEV), ea.to(DEV), qw.to(DEV), sw.to(DEV),
                            bias.to(DEV), act)
    fb.check(y, ref, bound, f"gemm_mxfp8 act={act}")


@pytest.mark.parametrize("act", fb.ACTS)
@pytest.mark.parametrize("n", [32, 288])
@pytest.mark.parametrize("m", [1, 257])
def test_emit_matches_quantiser(m, n, act):
    """The emitting epilogue against the definition applied to the bf16 result
    of the plain launch (the CPU definition: the GPU quantiser, bit-equal to
    it above, takes K % 128 == 0 only). Zero weight rows give a zero block
    (the last one, where there is more than one)."""
    x, w, bias = fb.linear_inputs(m, n, 128, seed=m + n)
    zero = slice(n - 32, n) if n > 32 else slice(0, 0)
    w[zero] = 0
    bias[zero] = 0
    qa, ea = dispatch.quant_rows_mxfp8(x.bfloat16())
    qw, sw = dispatch.quantize_weight_fp8(w)
    args = [t.to(DEV) for t in (qa, ea, qw, sw, bias)]
    y = dispatch.gemm_mxfp8(*args, act)
    q, e = dispatch.gemm_mxfp8(*args, act, emit=True)
    q_ref, e_ref = dispatch._mx_quant(y.cpu())
    assert torch.equal(e.cpu(), e_ref) and mc.same_bytes(q, q_ref)
    assert not q.cpu().view(torch.uint8)[:, zero].any()
    assert n == 32 or not e.cpu()[:, -1].any()
