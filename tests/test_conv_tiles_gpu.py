"""conv256_nhwc_ex with the variant pinned: N-tile widths 128 and 320, the K
split with its fp32 slabs and reduce pass, and the launcher's chooser.

Reference and bound: kernel_bounds.conv_ref, |err| <= 2U|ref| + n*2^-23*mag
with n = RS*C + 1, which holds for any order of the fp32 additions, so the
split cases use it unchanged. Bias is N(0, 1) (kernel_bounds.conv_inputs): a
bias added once per slice, or a SiLU applied per slice, lands tens of bounds
out (test_conv_tiles_cpu.py shows by how much).

Measured max(err/bound) on MI355X: see profiles/r07_conv_tiles.md.
"""

import pytest
import torch

import conv_tiles_cases as ct
import kernel_bounds as kb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def extmod():
    from comfyui_distributed_amd.ops import ext

    return ext.get_ext(required=True)


def _dev_bf16(t):
    return t.to(torch.bfloat16).cuda()


def _nores():
    return torch.empty(0, device="cuda", dtype=torch.bfloat16)


_REFS = {}


def _case(b, c, h, w, k, rs, stride=1, up2=False, silu=False, residual=False):
    """Inputs on the device + (ref, bound), computed once per distinct case."""
    key = (b, c, h, w, k, rs, stride, up2, silu, residual)
    if key not in _REFS:
        x, wk, bias = kb.conv_inputs(ct.seed_of(c, k, rs), b, c, h, w, k, rs)
        res = None
        if residual:
            ho = 2 * h if up2 else (h if stride == 1 else (h - 1) // 2 + 1)
            wo = 2 * w if up2 else (w if stride == 1 else (w - 1) // 2 + 1)
            g = torch.Generator().manual_seed(ct.seed_of(c, k, rs) + 1)
            res = kb.bf16_exact(torch.randn(b, ho, wo, k, generator=g))
        ref, bound = kb.conv_ref(x, wk, bias, stride=stride, up2=up2,
                                 silu=silu, residual=res)
        dev = (_dev_bf16(x), _dev_bf16(kb.repack_weight(wk)), bias.cuda(),
               _dev_bf16(res) if residual else _nores())
        _REFS[key] = (dev, ref, bound)
    return _REFS[key]


def _run(extmod, dev, b, c, h, w, k, rs, stride, up2, silu, bn, split):
    x, wt, bias, res = dev
    return extmod.conv256_nhwc_ex(x, wt, bias, res, b, h, w, c, k, rs, stride,
                                  up2, silu, bn, split)


@pytest.mark.parametrize("case", ct.BN320_CASES + ct.BN128_CASES, ids=str)
def test_conv256_tile_width(extmod, case):
    """bn = 320: five fragments per wave, a 40 KiB B image staged by five
    glds; bn = 128: two fragments, two MFMA clusters per K-tile. M tails,
    full / whole-fragment / half-fragment last N-blocks, M below one tile,
    the 16x16 pixel tiling, stride 2, fused upsample, SiLU and residual."""
    b, c, h, w, k, rs, stride, up2, silu, residual, bn = case
    dev, ref, bound = _case(b, c, h, w, k, rs, stride, up2, silu, residual)
    y = _run(extmod, dev, b, c, h, w, k, rs, stride, up2, silu, bn, 1)
    kb.check(y, ref, bound, f"conv256 bn{bn} {(b, c, h, w)}->{k} rs{rs} "
             f"s{stride} up2={up2} silu={silu} res={residual}")


@pytest.mark.parametrize("case", ct.SPLIT_CASES, ids=str)
def test_conv256_split_k(extmod, case):
    """Slices of uneven K-tile counts, one tile per slice, a split above the
    K-tile count (clamped), both wide tiles, 1x1, stride 2; bias, SiLU and
    residual must be applied once, by the reduce pass."""
    b, c, h, w, k, rs, stride, silu, residual, bn, split = case
    dev, ref, bound = _case(b, c, h, w, k, rs, stride, False, silu, residual)
    y = _run(extmod, dev, b, c, h, w, k, rs, stride, False, silu, bn, split)
    kb.check(y, ref, bound, f"conv256 bn{bn} split{split} {(b, c, h, w)}->{k} "
             f"rs{rs} s{stride} silu={silu} res={residual}")


def test_split_k_clamp_equals_one_tile_per_slice(extmod):
    """split_k = 16 on 9 K-tiles runs as 9: same slices, same bits."""
    args = (1, 64, 9, 9, 96, 9)
    dev, _, _ = _case(*args)
    y9 = _run(extmod, dev, *args, 1, False, False, 256, 9)
    y16 = _run(extmod, dev, *args, 1, False, False, 256, 16)
    assert torch.equal(y9, y16)


def test_split_k_repeats_bit_for_bit(extmod):
    """Same call twice; then a call of another shape and split (its slabs
    land in the memory the allocator just got back), then the first call
    again: all three equal. Stale slab contents would show here."""
    args = (2, 128, 9, 9, 320, 9)
    dev, _, _ = _case(*args)
    y1 = _run(extmod, dev, *args, 1, False, False, 256, 4)
    y2 = _run(extmod, dev, *args, 1, False, False, 256, 4)
    assert torch.equal(y1, y2)
    other = (1, 64, 9, 9, 96, 9)
    odev, _, _ = _case(*other)
    _run(extmod, odev, *other, 1, False, False, 256, 9)
    y3 = _run(extmod, dev, *args, 1, False, False, 256, 4)
    assert torch.equal(y1, y3)


def test_split_k_under_graph_capture(extmod):
    """One split call captured on one stream (no branches) and replayed
    twice: the slabs come from torch's allocator, so capture is legal and
    both replays equal the eager result."""
    args = (2, 128, 9, 9, 320, 9)
    dev, ref, bound = _case(*args)
    eager = _run(extmod, dev, *args, 1, False, False, 256, 4)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = _run(extmod, dev, *args, 1, False, False, 256, 4)
    outs = []
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        outs.append(y.clone())
    assert torch.equal(outs[0], eager) and torch.equal(outs[1], eager)
    kb.check(outs[0], ref, bound, "conv256 split4 replayed")


# ---------------------------------------------------------------------------
# chooser
# ---------------------------------------------------------------------------

# (M, K_out, Kdim) -> (bn, split_k) measured best on MI355X for the flagship
# convs (profiles/r07_conv_tiles.md, microbench table). M = 32 * Ho * Wo.
FLAGSHIP_PLANS = {
    # 68x68 level
    (32 * 68 * 68, 320, 9 * 320): (320, 1),
    (32 * 68 * 68, 320, 9 * 640): (320, 1),
    (32 * 68 * 68, 320, 9 * 960): (320, 1),
    # 34x34 level: two rounds either way, the wider tile's are longer
    (32 * 34 * 34, 640, 9 * 640): (256, 1),
    # 17x17 level: one round either way
    (32 * 17 * 17, 1280, 9 * 1280): (256, 1),
    (32 * 17 * 17, 1280, 9 * 2560): (256, 1),
    # 9x9 level: 44 tiles of 320, five slices of 36 / 72 K-tiles
    (32 * 9 * 9, 1280, 9 * 1280): (320, 5),
    (32 * 9 * 9, 1280, 9 * 2560): (320, 5),
    # its 1x1 skip conv, 40 K-tiles: 55 tiles of 256, four slices of 10
    (32 * 9 * 9, 1280, 2560): (256, 4),
    # stride-2 downsample to 17x17: 74 tiles of 320, three slices of 30
    (32 * 17 * 17, 640, 9 * 640): (320, 3),
    # fused 2x upsample to 34x34, K_out 1280: three rounds either way
    (32 * 34 * 34, 1280, 9 * 1280): (256, 1),
    # the UNet's K_out = 4 output conv
    (32 * 68 * 68, 4, 9 * 320): (128, 1),
    # fused 2x upsample to 68x68, K_out 640: 1156 tiles of 320 against 1734
    (32 * 68 * 68, 640, 9 * 640): (320, 1),
    # VAE 128-wide full-resolution level
    (16 * 544 * 544, 128, 9 * 128): (128, 1),
}


@pytest.mark.parametrize("triple,plan", FLAGSHIP_PLANS.items(), ids=str)
def test_plan_flagship(extmod, triple, plan):
    assert tuple(extmod.conv256_plan(*triple)) == plan


def test_plan_never_splits_a_full_round(extmod):
    """split_k is 1 wherever the plain grid already has >= 256 workgroups,
    a slice never has fewer K-tiles than it would at split 1 / the floor
    allows, and tiles * split_k fills at most one round."""
    for m in (81, 2592, 9248, 36992, 147968, 16 * 544 * 544):
        for k_out in (4, 64, 128, 320, 640, 1280):
            for kdim in (64, 576, 2880, 11520, 23040):
                bn, split = extmod.conv256_plan(m, k_out, kdim)
                assert bn in (128, 256, 320) and split >= 1
                tiles = -(-m // 256) * -(-k_out // bn)
                if tiles >= 256:
                    assert split == 1, (m, k_out, kdim, bn, split)
                else:
                    assert tiles * split <= 256, (m, k_out, kdim, bn, split)
                assert split <= kdim // 64


def test_default_entry_is_the_chooser(extmod):
    """conv256_nhwc and conv256_nhwc_ex(..., 0, 0) agree bit for bit, on a
    shape the chooser splits and on one it does not."""
    for args in ((2, 128, 9, 9, 320, 9), (2, 64, 17, 19, 320, 9)):
        dev, ref, bound = _case(*args)
        x, wt, bias, res = dev
        b, c, h, w, k, rs = args
        y0 = extmod.conv256_nhwc(x, wt, bias, res, b, h, w, c, k, rs, 1,
                                 False, False)
        y1 = _run(extmod, dev, *args, 1, False, False, 0, 0)
        assert torch.equal(y0, y1)
        kb.check(y0, ref, bound, f"conv256 chooser {args}")
