"""Inputs and the fp64 reference of the MXFP8 row format (ops/hip/
gemm_mxfp8.hip, dispatch.quant_rows_mxfp8). Plain torch on the CPU; imported
by test_mxfp8_cpu.py and test_mxfp8_gpu.py."""

from __future__ import annotations

import torch

FP8 = torch.float8_e4m3fn
BF16_MAX = 2.0 ** 127 * (2 - 2.0 ** -7)


def _block(amax: float, seed: int) -> torch.Tensor:
    """32 bf16 values in [-amax, amax] with -amax among them."""
    g = torch.Generator().manual_seed(seed)
    b = ((torch.rand(32, generator=g) * 2 - 1) * amax).bfloat16()
    b[seed % 32] = -amax
    return b


def edge_blocks() -> torch.Tensor:
    """[n, 32] bf16, the blocks on which the exponent rule or the rounding
    can go wrong (the row count is a multiple of 4: K = 128 rows)."""
    blocks = [torch.zeros(32, dtype=torch.bfloat16)]
    for j in (-3, 0, 5):
        blocks.append(_block(448.0 * 2.0 ** j, 4 + j))      # m = 1.75 exactly
        blocks.append(_block(450.0 * 2.0 ** j, 14 + j))     # one bf16 ulp above
    blocks.append(_block(BF16_MAX, 20))
    blocks.append(_block(2.0 ** -125, 21))                  # exp clamps to -127
    blocks.append(_block(2.0 ** -130, 22))                  # bf16 subnormals
    # e4m3 ties under exp = 0 (amax 448): halfway between neighbours in the
    # normal binades, at the subnormal step 2^-9 and at the clamp
    ties = torch.tensor([448.0, 1.0625, -1.1875, 17.0, -19.0, 2.0 ** -10,
                         3 * 2.0 ** -10, -(2.0 ** -10), 432.0, 0.0] + [0.5] * 22)
    blocks.append(ties.bfloat16())
    blocks.append(_block(1.0, 23))
    assert len(blocks) % 4 == 0
    return torch.stack(blocks)


def rows(m: int, k: int, seed: int) -> torch.Tensor:
    """[m, k] bf16: the edge blocks, then seeded random data whose blocks span
    many binades; m * k / 32 blocks in all."""
    g = torch.Generator().manual_seed(seed)
    nb = m * k // 32
    mag = 2.0 ** torch.randint(-12, 12, (nb, 1), generator=g).float()
    x = (torch.randn(nb, 32, generator=g) * mag).bfloat16()
    e = edge_blocks()[:nb]
    x[:e.shape[0]] = e
    return x.reshape(m, k)


def quant_ref64(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(q float8, e uint8, v fp64) of x [M, K] from the issue's rule in fp64:
    amax = m * 2^E, exp = E - 8 (m <= 1.75) or E - 7, -127 for amax = 0,
    clamped; v = x * 2^-exp, q = e4m3(clamp(v))."""
    m, k = x.shape
    xb = x.double().reshape(m, k // 32, 32)
    amax = xb.abs().amax(-1)
    mant, ex = torch.frexp(amax)                 # amax = mant * 2^ex, mant in [.5, 1)
    exp = (ex - 1) - 8 + (mant > 0.875).int()
    exp = torch.where(amax == 0, torch.full_like(exp, -127), exp).clamp(-127, 127)
    v = torch.ldexp(xb, -exp[..., None])
    q = v.clamp(-448, 448).float().to(FP8).reshape(m, k)
    return q, (exp + 127).to(torch.uint8), v.reshape(m, k)


def same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))
