"""References and per-element error bounds for the FP8 Linear path
(ops/hip/gemm_fp8.hip, dispatch.linear_fp8). Plain torch on the CPU, float64;
imported by test_fp8_linear_cpu.py and test_fp8_linear_gpu.py.

Quantiser (quant_rows_fp8): scale = max(amax, 2^-126 * 448) * (1/448) as one
fp32 multiply, q = rne_e4m3(clamp(x / scale, +-448)).

    quant_bound   with v = x / scale in fp64, from the scale the code under
                  test reports,
                      |q - v| <= hs(v) * (1 + 2^-20) + 2^-20 * |v|
                  hs(v) = 2^(clamp(floor(log2|v|), -6, 8) - 4) is half an e4m3
                  step at v: e4m3 keeps 3 mantissa bits, so the step in the
                  binade 2^e is 2^(e-3); below 2^-6 the format is subnormal
                  with step 2^-9, and 448 lies in the binade 2^8. The 2^-20
                  terms allow the fp32 evaluation of x * (1/scale) (two
                  roundings of 2^-24 each) in front of the one e4m3 rounding;
                  a second rounding or a truncation does not fit.

GEMM (gemm_fp8): ref = (Qa . Qw^T) * sa * sw + bias in fp64 from the exact
quantised operands the kernel receives, then the activation.

    linear_fp8_bound   |err| <= 2U * |ref| + (K + 1) * 2^-23 * mag,
                       mag = (|Qa| . |Qw|^T) * sa * sw + |bias|, U = 2^-8:
                       the project's dot-product bound (kernel_bounds.py): the
                       bf16 store, and the worst case of an fp32 chain of K
                       products and the bias. x1.1 on the second term with an
                       activation fused (|silu'| <= 1.1).
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

U = 2.0 ** -8
E4M3_MAX = 448.0
AMAX_FLOOR = 2.0 ** -126 * E4M3_MAX
FP8 = torch.float8_e4m3fn
ACTS = (None, "silu", "gelu_tanh")


def scale_ref(amax: torch.Tensor) -> torch.Tensor:
    """fp32, bit for bit what the kernel computes from a row's absmax."""
    inv = torch.tensor(1.0 / E4M3_MAX, dtype=torch.float32)
    return amax.float().clamp_min(AMAX_FLOOR) * inv


def quant_ref(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """x [M, K] (values exact in fp32) -> (q float8_e4m3fn, scale fp32 [M])."""
    x = x.float()
    scale = scale_ref(x.abs().amax(dim=1))
    q = (x / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(FP8)
    return q, scale


def half_step(v: torch.Tensor) -> torch.Tensor:
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -40)))
    return torch.exp2(e.clamp(-6, 8) - 4)


def quant_bound(x: torch.Tensor, scale: torch.Tensor):
    """(v, bound): v = x / scale in fp64, bound on |q - v| per element."""
    v = x.double() / scale.double()[:, None]
    return v, half_step(v) * (1 + 2.0 ** -20) + 2.0 ** -20 * v.abs()


def quant_ratio(q: torch.Tensor, x: torch.Tensor, scale: torch.Tensor) -> float:
    """max(|q - v| / bound) over the elements."""
    qd = q.detach().cpu().to(torch.float32).double()
    if not torch.isfinite(qd).all():
        return math.inf
    v, bound = quant_bound(x.detach().cpu(), scale.detach().cpu())
    return ((qd - v).abs() / bound).max().item()


def _act(y: torch.Tensor, act: str | None) -> torch.Tensor:
    if act == "silu":
        return F.silu(y)
    if act == "gelu_tanh":
        return F.gelu(y, approximate="tanh")
    assert act is None, act
    return y


def linear_fp8_pre(qa, sa, qw, sw, bias=None):
    """(pre-activation ref, mag) in fp64."""
    a, w = qa.cpu().to(torch.float32).double(), qw.cpu().to(torch.float32).double()
    s = sa.cpu().double()[:, None] * sw.cpu().double()[None, :]
    ref = (a @ w.t()) * s
    mag = (a.abs() @ w.abs().t()) * s
    if bias is not None:
        ref = ref + bias.cpu().double()
        mag = mag + bias.cpu().double().abs()
    return ref, mag


def linear_fp8_ref(qa, sa, qw, sw, bias=None, act=None) -> torch.Tensor:
    return _act(linear_fp8_pre(qa, sa, qw, sw, bias)[0], act)


def bound_from(ref_act: torch.Tensor, mag: torch.Tensor, k: int, act) -> torch.Tensor:
    return 2 * U * ref_act.abs() + (1.1 if act else 1.0) * (k + 1) * 2.0 ** -23 * mag


def linear_fp8_bound(qa, sa, qw, sw, bias=None, act=None):
    """(ref, bound) of act((Qa . Qw^T) * sa * sw + bias)."""
    pre, mag = linear_fp8_pre(qa, sa, qw, sw, bias)
    ref = _act(pre, act)
    return ref, bound_from(ref, mag, qa.shape[1], act)


def err_ratio(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    out = out.detach().cpu().to(torch.float32).double()
    assert out.shape == ref.shape, (tuple(out.shape), tuple(ref.shape))
    if not torch.isfinite(out).all():
        return math.inf
    err = (out - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err),
                        err / bound.clamp_min(1e-300))
    return ratio.max().item()


def check(out, ref, bound, what: str) -> float:
    r = err_ratio(out, ref, bound)
    print(f"{what}: max|ref| {ref.abs().max().item():.3e}  "
          f"max(err/bound) {r:.3f}")
    assert r <= 1.0, f"{what}: err/bound {r:.3f} > 1"
    return r


# ---------------------------------------------------------------------------
# input recipes
# ---------------------------------------------------------------------------


def linear_inputs(m: int, n: int, k: int, seed: int):
    """bf16-exact x [M, K] whose rows span 1e-2 .. 10 in magnitude, w [N, K]
    whose channels span 0.02 .. 0.5 (neighbouring rows / channels differ, so a
    scale taken from the wrong one shows), fp32 bias [N]."""
    g = torch.Generator().manual_seed(seed)
    row_mag = 10.0 ** (-2 + 3 * torch.rand(m, 1, generator=g))
    x = (torch.randn(m, k, generator=g) * row_mag).bfloat16().float()
    ch_mag = 0.02 * 25.0 ** torch.rand(n, 1, generator=g)
    w = (torch.randn(n, k, generator=g) * ch_mag).bfloat16().float()
    bias = torch.randn(n, generator=g)
    return x, w, bias


def emulate_gemm(qa, sa, qw, sw, bias=None, act=None, drop_k=None,
                 sw_shift=0, sa_shift=0) -> torch.Tensor:
    """fp32 emulation of the kernel: fp32 accumulation of the e4m3 products,
    row scale, channel scale, bias, activation, one bf16 rounding. The
    keyword arguments seed defects: ``drop_k`` zeroes one 32-wide K block,
    ``sw_shift`` / ``sa_shift`` take the scales from a neighbour."""
    a, w = qa.to(torch.float32), qw.to(torch.float32)
    if drop_k is not None:
        a = a.clone()
        a[:, drop_k:drop_k + 32] = 0
    y = (a @ w.t()) * sa.roll(sa_shift)[:, None] * sw.roll(sw_shift)[None, :]
    if bias is not None:
        y = y + bias.float()
    return _act(y, act).bfloat16()


def quant_truncating(x: torch.Tensor):
    """Defect: e4m3 by truncation toward zero instead of round-to-nearest."""
    x = x.float()
    scale = scale_ref(x.abs().amax(dim=1))
    v = (x / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX)
    step = 2 * half_step(v.double()).float()
    return (torch.trunc(v / step) * step).to(FP8), scale
