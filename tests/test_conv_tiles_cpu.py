"""The split-K arithmetic of conv256_nhwc_ex stays inside the dot-product
bound, and its characteristic defects leave it, shown without a GPU.

Emulation of what the kernels do: each slice accumulates its contiguous range
of 64-deep K-tiles (k = tap*C + c, tap-major) in fp32 and stores the raw fp32
partial; the reduce pass adds the partials in slice order in fp32, then adds
the bias, applies SiLU, adds the residual and rounds to bf16 once. The slice
ranges are conv_tiles_cases.slice_ranges: lengths differing by at most one.

On the split cases of conv_tiles_cases.SPLIT_CASES the emulation must stay
within 0.75 of kernel_bounds.conv_ref's bound, and each seeded defect must
leave the bound on every case:

  one slice dropped            (a slab the reduce pass does not read)
  one K-tile in two slices     (overlapping ranges)
  bias added per slice         (epilogue run by the slices)
  SiLU applied per slice       (the same, on the SiLU cases)
"""

import pytest
import torch
import torch.nn.functional as F

import conv_tiles_cases as ct
import kernel_bounds as kb

EMU_MAX = 0.75


def _bf(x):
    return x.to(torch.bfloat16).float()


def _silu32(x):
    return x / (1.0 + torch.exp(-x))


def im2col(x_nhwc, rs, stride):
    """[B,H,W,C] -> ([M, RS*C] fp32 with k = tap*C + c, (B, Ho, Wo))."""
    b, h, w, c = x_nhwc.shape
    r = 3 if rs == 9 else 1
    xf = x_nhwc.float().permute(0, 3, 1, 2)
    cols = F.unfold(xf, r, padding=r // 2, stride=stride)   # [B, C*rs, L]
    ho = (h + 2 * (r // 2) - r) // stride + 1
    wo = (w + 2 * (r // 2) - r) // stride + 1
    cols = cols.reshape(b, c, rs, ho * wo).permute(0, 3, 2, 1)
    return cols.reshape(b * ho * wo, rs * c).contiguous(), (b, ho, wo)


def emulate_split_conv(x, wk, bias, rs, stride, split, silu=False,
                       residual=None, defect=None):
    a, (b, ho, wo) = im2col(x, rs, stride)
    wt = kb.repack_weight(wk).float()                # [K, RS*C]
    ranges = ct.slice_ranges(a.shape[1] // ct.BK, split)
    if defect == "tile twice" and len(ranges) > 1:
        # the second slice starts one K-tile early
        ranges[1] = (ranges[1][0] - 1, ranges[1][1])
    partials = []
    for (t0, t1) in ranges:
        k0, k1 = t0 * ct.BK, t1 * ct.BK
        p = a[:, k0:k1] @ wt[:, k0:k1].t()           # fp32 accumulation
        if defect == "bias per slice":
            p = p + bias.float()
        if defect == "silu per slice":
            p = _silu32(p + bias.float())
        partials.append(p)
    if defect == "slice dropped":
        partials = partials[:-1]
    y = partials[0].clone()
    for p in partials[1:]:                           # fixed order, fp32
        y = y + p
    if defect not in ("bias per slice", "silu per slice"):
        y = y + bias.float()
        if silu:
            y = _silu32(y)
    y = y.reshape(b, ho, wo, -1)
    if residual is not None:
        y = y + residual.float()
    return _bf(y)


def _inputs(case):
    b, c, h, w, k, rs, stride, silu, residual, bn, split = case
    x, wk, bias = kb.conv_inputs(ct.seed_of(c, k, rs), b, c, h, w, k, rs)
    res = None
    if residual:
        ho = h if stride == 1 else (h - 1) // 2 + 1
        wo = w if stride == 1 else (w - 1) // 2 + 1
        g = torch.Generator().manual_seed(ct.seed_of(c, k, rs) + 1)
        res = kb.bf16_exact(torch.randn(b, ho, wo, k, generator=g))
    ref, bound = kb.conv_ref(x, wk, bias, stride=stride, silu=silu,
                             residual=res)
    return x, wk, bias, res, ref, bound


def test_slice_ranges():
    assert ct.slice_ranges(9, 2) == [(0, 5), (5, 9)]
    assert ct.slice_ranges(9, 4) == [(0, 3), (3, 5), (5, 7), (7, 9)]
    assert ct.slice_ranges(9, 16) == [(i, i + 1) for i in range(9)]
    assert ct.slice_ranges(18, 4) == [(0, 5), (5, 10), (10, 14), (14, 18)]
    assert ct.slice_ranges(2, 2) == [(0, 1), (1, 2)]


@pytest.mark.parametrize("case", ct.SPLIT_CASES, ids=str)
def test_split_emulation_inside_defects_outside(case):
    b, c, h, w, k, rs, stride, silu, residual, bn, split = case
    x, wk, bias, res, ref, bound = _inputs(case)
    kw = dict(rs=rs, stride=stride, split=split, silu=silu, residual=res)
    r = kb.err_ratio(emulate_split_conv(x, wk, bias, **kw), ref, bound)
    # the unsplit chain through the same code: the split must not cost more
    # than the bound allows either way
    r1 = kb.err_ratio(emulate_split_conv(x, wk, bias, **dict(kw, split=1)),
                      ref, bound)
    defects = ["slice dropped", "tile twice", "bias per slice"]
    if silu:
        defects.append("silu per slice")
    rd = {d: kb.err_ratio(emulate_split_conv(x, wk, bias, defect=d, **kw),
                          ref, bound) for d in defects}
    print(f"split {split} bn{bn} {(b, c, h, w)}->{k} rs{rs} s{stride} "
          f"silu={silu} res={residual}: emulation {r:.3f} (unsplit {r1:.3f})  "
          + "  ".join(f"{d} {v:.0f}" for d, v in rd.items()))
    assert r <= EMU_MAX and r1 <= EMU_MAX, (r, r1)
    for d, v in rd.items():
        assert v > 1.0, (d, v)
