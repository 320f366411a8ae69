"""attn_fp8_kernel and its quantiser (ops/hip/attention_fp8.hip) on the GPU,
against the torch definition (exact cases, quantiser bits) and against fp64
attention over the dequantised operands (derived bound)."""

import math

import pytest
import torch

import kernel_bounds as kb
from comfyui_distributed_amd.ops import dispatch, ext
from test_attention_fp8_cpu import SELECT_CASES, R, selection_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
D = dispatch.ATTN_FP8_D
SP = dispatch.ATTN_FP8_SP


def _dev(*ts):
    return [t.to(BF).to(DEV) for t in ts]


def test_constants_match_the_extension():
    e = ext.get_ext(True)
    assert e.ATTN_FP8_QROWS == R and e.ATTN_FP8_SP == SP


@pytest.mark.parametrize("b,h,nq,nk", SELECT_CASES)
def test_kernel_selects_exactly(b, h, nq, nk):
    """One key per query carries all the weight (test_attention_fp8_cpu
    checks the construction): the output is that key's V row, bit for bit.
    A lost or misplaced key, a wrong V^T position, V column, head or batch
    stride returns another row or a mixture."""
    q, k, v, want = selection_case(b, h, nq, nk)
    out = dispatch.attention_fp8(*_dev(q, k, v), h)
    assert out.dtype == BF and torch.equal(out.float().cpu(), want)


def _ref_and_bound(a, nk, scale):
    """fp64 attention over a.dequant() and the bound on the kernel's error:
      2^-8 |ref|                 the bf16 rounding of the output
      2^-4 P@|V|                 e4m3 has 3 mantissa bits: every normal weight
                                 is off by at most 2^-4 of itself
      Nk 2^-(SP+10) max_j|v_jd|  a weight under 2^-6 / 2^SP is subnormal in
                                 e4m3: step 2^-9, error 2^-10, before the 2^SP;
                                 the maximum over the keys j of the element's
                                 own V channel d
      (Nk+D+16) 2^-23 P@|V|      fp32 sums, as kernel_bounds.attention_ref"""
    h = a.heads
    q, k, v = (kb.split_heads(t.double().cpu(), h) for t in a.dequant())
    p = torch.softmax(torch.bmm(q, k.transpose(1, 2)) * scale, dim=-1)
    ref, pav = torch.bmm(p, v), torch.bmm(p, v.abs())
    bound = (2.0 ** -8 * ref.abs() + 2.0 ** -4 * pav
             + nk * 2.0 ** -(SP + 10) * v.abs().amax(dim=1, keepdim=True)
             + (nk + D + 16) * 2.0 ** -23 * pav)
    return kb.merge_heads(ref, h), kb.merge_heads(bound, h)


# the shapes of the exact cases at the default scale, and nk = 77 (51 pad
# keys under the tail mask) at the default and at the explicit scales
RANDOM_CASES = [(b, h, nq, nk, 1.0) for b, h, nq, nk in SELECT_CASES] + [
    (2, 2, 40, 77, m) for m in [1.0] + kb.ATTN_SCALE_MULT]


@pytest.mark.parametrize("b,h,nq,nk,mult", RANDOM_CASES)
def test_kernel_random_within_bound(b, h, nq, nk, mult):
    q, k, v = kb.attn_inputs(nq + nk, b, b, nq, nk, h * D,
                             qk_std=mult ** -0.5)
    scale = mult / math.sqrt(D)
    a = dispatch.quantize_attn_qkv(*_dev(q, k, v), h)
    out = dispatch.attention_fp8(a, scale=scale)
    ref, bound = _ref_and_bound(a, nk, scale)
    kb.check(out, ref, bound, f"attention_fp8 nq={nq} nk={nk} mult={mult}")


def _bits(t):
    return t.cpu().view(torch.uint8) if t.dtype == torch.float8_e4m3fn \
        else t.cpu()


@pytest.mark.parametrize("n", [1, 127, 129, 300])
def test_quantiser_bits(n):
    """Codes, scales and the K mean equal the torch definition bit for bit
    (the definition sums the mean in the kernel's order). K has a channel
    offset of 8 at std 1: without the mean removal its codes would differ."""
    b, h = 2, 2
    g = torch.Generator().manual_seed(n)
    q = kb.bf16_exact(torch.randn(b, n, h * D, generator=g))
    k = kb.bf16_exact(torch.randn(b, n, h * D, generator=g) + 8.0)
    v = kb.bf16_exact(torch.randn(b, n, h * D, generator=g))
    got = dispatch.quantize_attn_qkv(*_dev(q, k, v), h)
    want = dispatch.quantize_attn_qkv(q, k, v, h)
    for name in ("k_mean", "q_scale", "k_scale", "v_scale", "q", "k", "v"):
        x, y = getattr(got, name), getattr(want, name)
        assert x.shape == y.shape and x.dtype == y.dtype, name
        assert torch.equal(_bits(x), _bits(y)), name
    if n > 1:
        assert (want.k_mean - 8).abs().max() < 4 and \
            want.k_scale.max() < 6.0 / 448


def test_accuracy_against_unquantised_attention():
    """Relative rms error against fp64 attention on the bf16 inputs: the
    kernel within 1.25x of the torch definition (the margin is for the running
    maximum the kernel rounds against)."""
    b, h, n = 1, 2, 1024
    q, k, v = kb.attn_inputs(5, b, b, n, n, h * D)
    ref, _ = kb.attention_packed_ref(q, k, v, h)
    out = dispatch.attention_fp8(*_dev(q, k, v), h).double().cpu()
    cpu = dispatch.attention_fp8(q.to(BF), k.to(BF), v.to(BF), h).double()
    e_gpu = ((out - ref).norm() / ref.norm()).item()
    e_cpu = ((cpu - ref).norm() / ref.norm()).item()
    print(f"relative rms error: kernel {e_gpu:.5f}, definition {e_cpu:.5f}")
    assert e_gpu <= 1.25 * e_cpu
