"""Reference and bounds for norm_modulate_fp8 (ops/hip/dit_ops.hip,
dispatch.norm_modulate_fp8). Plain torch on the CPU, float64; imported by
test_norm_fp8_cpu.py and test_norm_fp8_gpu.py.

norm_modulate_fp8 is defined as quant_rows_fp8(norm_modulate(x, ...)), so its
bound is the single-rounding norm bound of kernel_bounds.norm_modulate_ref
pushed through the quantiser bound of fp8_bounds. Let (h, eh) be that
reference and bound, s the scale the code under test reports, v = h / s and
e = eh / s.

    scale    448 * s lies in [max_row(|h| - eh), max_row(|h| + eh)], both ends
             floored at 2^-126 * 448 and widened by a relative 2^-22 (the one
             fp32 multiply by 1/448 and the fp64 comparison of it)
    values   |q - v| <= hs(|v| + e) * (1 + 2^-20) + 2^-20 * |v| + e
             hs = fp8_bounds.half_step: the quantiser's own bound, with the
             norm's error e added and hs taken at |v| + e, so a value that e
             nudges across a binade edge is covered

Neither term holds a constant of its own. The eager CPU order of
dispatch.norm_modulate (norm rounded to bf16 before the modulation) is 12-83
bounds out, so this bound is for the GPU kernel and for the emulation below,
not for the CPU dispatch path.
"""

from __future__ import annotations

import math

import torch

import fp8_bounds as fb
import kernel_bounds as kb

BF = torch.bfloat16


def reference(inp: dict, modulated: bool = True):
    """(h, eh) fp64 [B, N, C] of a kernel_bounds.nm_inputs dict."""
    sc, sh = (inp["scale"], inp["shift"]) if modulated else (None, None)
    return kb.norm_modulate_ref(inp["x"], inp["mode"], inp["w"], sc, sh)


def scale_interval(h: torch.Tensor, eh: torch.Tensor):
    """(lo, hi) fp64 [B, N] for 448 * scale."""
    lo = (h.abs() - eh).amax(dim=-1).clamp_min(fb.AMAX_FLOOR)
    hi = (h.abs() + eh).amax(dim=-1).clamp_min(fb.AMAX_FLOOR)
    return lo * (1 - 2.0 ** -22), hi * (1 + 2.0 ** -22)


def scale_ok(scale: torch.Tensor, h: torch.Tensor, eh: torch.Tensor) -> bool:
    s = scale.detach().cpu().double() * fb.E4M3_MAX
    lo, hi = scale_interval(h, eh)
    return bool(torch.isfinite(s).all() and ((s >= lo) & (s <= hi)).all())


def value_ratio(q: torch.Tensor, scale: torch.Tensor, h: torch.Tensor,
                eh: torch.Tensor) -> float:
    """max(|q - v| / bound) over the elements."""
    qd = q.detach().cpu().to(torch.float32).double()
    if not torch.isfinite(qd).all():
        return math.inf
    s = scale.detach().cpu().double()[..., None]
    v, e = h / s, eh / s
    bound = (fb.half_step(v.abs() + e) * (1 + 2.0 ** -20)
             + 2.0 ** -20 * v.abs() + e)
    return ((qd - v).abs() / bound).max().item()


def check(q, scale, h, eh, what: str) -> float:
    ok = scale_ok(scale, h, eh)
    r = value_ratio(q, scale, h, eh)
    print(f"{what}: scale inside {ok}  max(err/bound) {r:.4f}")
    assert ok, f"{what}: scale outside its interval"
    assert r <= 1.0, f"{what}: err/bound {r:.4f} > 1"
    return r


def outside(q, scale, h, eh) -> bool:
    """True when either check fails."""
    return not scale_ok(scale, h, eh) or value_ratio(q, scale, h, eh) > 1.0


def emulate(inp: dict, modulated: bool = True, defect: str | None = None):
    """fp32 emulation of the kernel: the modulated value in fp32, one bf16
    rounding, then the reference quantiser on the bf16 row. -> (q, scale) of
    shapes [B, N, C], [B, N]. ``defect`` seeds one:
      "amax without tail"   the absmax skips the last 8 channels
      "neighbour scale"     a row reports and uses the next row's scale
      "previous batch"      scale/shift of batch b - 1
      "truncation"          e4m3 by truncation toward zero
    """
    x, mode = inp["x"].float(), inp["mode"]
    b, n, c = x.shape
    eps = 1e-6 if mode == "rms" else 1e-5
    if mode == "rms":
        g = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
        g = g * inp["w"].float()
    else:
        d = x - x.mean(-1, keepdim=True)
        g = d * torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + eps)
    if modulated:
        sc, sh = inp["scale"].float(), inp["shift"].float()
        if defect == "previous batch":
            sc, sh = sc.roll(1, 0), sh.roll(1, 0)
        g = g * (1.0 + sc[:, None]) + sh[:, None]
    y = g.to(BF).float().reshape(b * n, c)
    if defect == "truncation":
        q, s = fb.quant_truncating(y)
    else:
        amax = (y[:, :-8] if defect == "amax without tail" else y).abs().amax(1)
        s = fb.scale_ref(amax)
        if defect == "neighbour scale":
            s = s.roll(-1)
        q = (y / s[:, None]).clamp(-fb.E4M3_MAX, fb.E4M3_MAX).to(fb.FP8)
    return q.reshape(b, n, c), s.reshape(b, n)


# --- cases -----------------------------------------------------------------

# C -> ITERS of norm_modulate_kernel: 1, 2, 2, 4, 6, 6, 8, 10, 10, 12, 16, 16
GPU_C = [128, 640, 1024, 1152, 2688, 3072, 3712, 4736, 5120, 5760, 6272, 8192]
MODES = [("rms", True), ("rms", False), ("layer", True)]   # (mode, modulated)


def gpu_case(i: int, c: int, mode: str) -> dict:
    """nm_inputs kwargs of GPU case i: (B, N) cycles through
    kernel_bounds.NM_BN (T % 4 != 0, B > 1); C = 1152 is the tail=8 recipe."""
    bn = kb.NM_BN[i % len(kb.NM_BN)]
    return dict(b=bn[0], n=bn[1], c=c, mode=mode, seed=4000 + c,
                tail=8.0 if c == 1152 else 1.0)


# CPU emulation sweep: (C, extra nm_inputs kwargs)
CPU_CASES = (
    [(c, {}) for c in (128, 640, 1152, 1536, 3072, 5120, 8192)]
    + [(1152, dict(mean=3.0, std=0.5)), (1152, dict(mean=128.0)),
       (1152, dict(tail=8.0)), (640, dict(const=True))])
