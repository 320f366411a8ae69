"""The K-tile order of the bf16 256-tile kernels (gemm_tile.h tile_ktile_once:
k-step outer, mq inner, every LDS fragment read once), at the smallest shapes
that reach each path of gemm256_tile.

Per case: the fp64 reference under the conv / GEMM bound of kernel_bounds (the
GEGLU rows under geglu_ref's), two calls bit-identical, and the SHA-256 of the
raw output words equal to tests/golden/gemm_ktile_digests.json, which was
recorded on MI355X from the build BEFORE the reorder. An accumulator still
gets k-step 0 before k-step 1, so the reorder moves no bit; a fragment paired
with the wrong half, a B fragment of the other k-step kept for mq = 1 or a
k-step run twice changes the digest and, on N(0, 1) bias and these operand
scales, leaves the bound by orders of magnitude. Inputs are seeded on the CPU.

Before every call the caching allocator is poisoned as in
test_unet_glue_gpu.py: NaN-filled tensors of the sizes the call allocates are
created and freed, so the output, the split-K slabs and the stream-K slots
come back holding NaN and anything left unwritten reaches the output.
"""

import functools
import hashlib
import json
from pathlib import Path

import pytest
import torch

import kernel_bounds as kb
from geglu_ref import geglu_ref

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "gemm_ktile_digests.json"

# conv cases: (b, c, h, w, k, rs, stride, up2, silu, residual, bn, mode, arg)
#   mode "ex": conv256_nhwc_ex(bn, split_k = arg)
#   mode "sk": conv256_nhwc_sk(bn, dp_tiles, sk_wgs = arg)
_S = (2, 13, 13)   # B, H, W: M = 338, one full and one partial 256-row tile


def _conv(c, k, rs, bn, mode="ex", arg=1, b=_S[0], h=_S[1], w=_S[2], stride=1,
          up2=False, silu=False, residual=False):
    return ("conv", b, c, h, w, k, rs, stride, up2, silu, residual, bn, mode,
            arg)


CASES = (
    # 1x1: one K-tile (the prologue's stage only), two, three (both buffer
    # parities as source and as target), at every width
    [_conv(c, 100, 1, bn) for c in (64, 128, 192) for bn in (128, 256, 320)]
    # 3x3, C = 64 (9 K-tiles, border taps on the zero page): masked N tail,
    # the exact 320 block, a second N block, at every width
    + [_conv(64, k, 9, bn) for k in (4, 100, 320, 336)
       for bn in (128, 256, 320)]
    # the epilogue's other inputs, once each
    + [_conv(64, 100, 9, 256, silu=True),
       _conv(64, 336, 9, 320, residual=True)]
    # split-K: slices of 5 + 4 and of 3 + 3 + 3 K-tiles (a slice starts at
    # either buffer parity of the unsplit loop, always at parity 0 of its own)
    + [_conv(64, 100, 9, bn, arg=2) for bn in (128, 256, 320)]
    + [_conv(64, 336, 9, 320, arg=3)]
    # stream-K, schedule pinned: (dp_tiles, ranges). 256: 4 tiles, one whole,
    # 27 units in 5 ranges; 320: 4 tiles, 36 units in 3 ranges (12 each: a
    # range crosses a tile edge mid-way); 128: 2 tiles, 18 units in 4 ranges
    + [_conv(64, 336, 9, 256, "sk", (1, 5)),
       _conv(64, 336, 9, 320, "sk", (0, 3), silu=True),
       _conv(64, 100, 9, 128, "sk", (0, 4))]
    # stride 2 (14x14 -> 7x7, M = 98) and the fused 2x upsample (8x8 -> 16x16,
    # the 16x16-pixel tile map)
    + [_conv(64, 100, 9, 256, b=2, h=14, w=14, stride=2),
       _conv(64, 100, 9, 320, b=2, h=8, w=8, up2=True)]
    # the plain GEMM entry and the GEGLU-fused Linear (bn 0: its chooser)
    + [("gemm", 300, 192, 144, False), ("gemm", 300, 192, 144, True),
       ("geglu", 513, 320, 272, 0), ("geglu", 513, 320, 272, 128),
       ("geglu", 513, 320, 272, 256)]
)


def case_id(case):
    return "-".join(str(v).replace(" ", "") for v in case)


def _seed(case):
    return int(hashlib.sha256(case_id(case[:8] if case[0] == "conv" else case[:4])
                              .encode()).hexdigest()[:8], 16)


def _out_hw(h, w, stride, up2):
    return (2 * h, 2 * w) if up2 else ((h - 1) // stride + 1,
                                       (w - 1) // stride + 1)


@functools.lru_cache(maxsize=None)
def _conv_case(b, c, h, w, k, rs, stride, up2, silu, residual):
    """CPU-seeded operands on the device + (ref, bound), once per problem."""
    seed = _seed(("conv", b, c, h, w, k, rs, stride))
    x, wk, bias = kb.conv_inputs(seed, b, c, h, w, k, rs)
    res = None
    if residual:
        ho, wo = _out_hw(h, w, stride, up2)
        g = torch.Generator().manual_seed(seed + 1)
        res = kb.bf16_exact(torch.randn(b, ho, wo, k, generator=g))
    ref, bound = kb.conv_ref(x, wk, bias, stride=stride, up2=up2, silu=silu,
                             residual=res)
    dev = (x.to(kb.BF).cuda(), kb.repack_weight(wk).to(kb.BF).cuda(),
           bias.cuda(),
           res.to(kb.BF).cuda() if residual
           else torch.empty(0, device="cuda", dtype=kb.BF))
    return dev, ref, bound


@functools.lru_cache(maxsize=None)
def _gemm_case(m, k, n, silu):
    g = torch.Generator().manual_seed(_seed(("gemm", m, k, n)))
    x = kb.bf16_exact(torch.randn(m, k, generator=g) / 4)
    w = kb.bf16_exact(torch.randn(n, k, generator=g) / 4)
    bias = kb.bf16_exact(torch.randn(n, generator=g))
    ref, bound = kb.linear_ref(x, w, bias, silu=silu)
    return (x.to(kb.BF).cuda(), w.to(kb.BF).cuda(), bias.cuda()), ref, bound


@functools.lru_cache(maxsize=None)
def _geglu_case(m, k, inner):
    from comfyui_distributed_amd.ops import dispatch

    g = torch.Generator().manual_seed(_seed(("geglu", m, k, inner)))
    x = kb.bf16_exact(torch.randn(m, k, generator=g))
    std = torch.tensor([1.0, 1.5]).repeat_interleave(inner)[:, None] / k ** 0.5
    w = kb.bf16_exact(torch.randn(2 * inner, k, generator=g) * std)
    b = kb.bf16_exact(0.5 * torch.randn(2 * inner, generator=g))
    ref, bound = geglu_ref(x, w, b)
    wp, bp = dispatch.pack_geglu_weight(w.to(kb.BF).cuda(), b.cuda())
    return (x.to(kb.BF).cuda(), wp, bp), ref, bound


def prepare(case):
    """(device operands, ref, bound, [(numel, dtype) the call allocates])."""
    if case[0] == "conv":
        _, b, c, h, w, k, rs, stride, up2, silu, residual, bn, mode, arg = case
        dev, ref, bound = _conv_case(b, c, h, w, k, rs, stride, up2, silu,
                                     residual)
        ho, wo = _out_hw(h, w, stride, up2)
        m = b * ho * wo
        allocs = [(m * k, kb.BF)]
        if mode == "ex" and arg > 1:
            allocs.append((arg * m * k, torch.float32))
        if mode == "sk":
            tiles = -(-m // 256) * -(-k // bn)
            allocs.append(((arg[1] + tiles - arg[0] - 1) * 256 * bn,
                           torch.float32))
        return dev, ref, bound, allocs
    if case[0] == "gemm":
        _, m, k, n, silu = case
        dev, ref, bound = _gemm_case(m, k, n, silu)
        return dev, ref, bound, [(m * n, kb.BF)]
    _, m, k, inner, _ = case
    dev, ref, bound = _geglu_case(m, k, inner)
    return dev, ref, bound, [(m * inner, kb.BF)]


def run(extmod, case, dev):
    if case[0] == "conv":
        _, b, c, h, w, k, rs, stride, up2, silu, _, bn, mode, arg = case
        x, wt, bias, res = dev
        if mode == "ex":
            return extmod.conv256_nhwc_ex(x, wt, bias, res, b, h, w, c, k, rs,
                                          stride, up2, silu, bn, arg)
        return extmod.conv256_nhwc_sk(x, wt, bias, res, b, h, w, c, k, rs,
                                      stride, up2, silu, bn, arg[0], arg[1])
    if case[0] == "gemm":
        x, w, bias = dev
        return extmod.gemm256_bf16(x, w, bias, case[4])
    x, wp, bp = dev
    return extmod.gemm_geglu_ex(x, wp, bp, case[4])


def digest(y):
    """SHA-256 of the output's raw 16-bit words, row-major."""
    words = y.detach().contiguous().view(torch.int16).cpu().numpy()
    return hashlib.sha256(words.tobytes()).hexdigest()


def poison(allocs):
    held = [torch.full((max(int(n), 1),), float("nan"), dtype=dt,
                       device="cuda") for n, dt in allocs]
    torch.cuda.synchronize()
    del held


@pytest.fixture(scope="module")
def extmod():
    from comfyui_distributed_amd.ops import ext

    return ext.get_ext(required=True)


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_case_list():
    """What the list is meant to reach, checked on the list itself."""
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    conv = [c for c in CASES if c[0] == "conv"]
    assert {c[11] for c in conv if c[12] == "ex" and c[13] == 1} \
        == {128, 256, 320}
    assert {c[11] for c in conv if c[12] == "ex" and c[13] > 1} \
        == {128, 256, 320}
    assert {c[11] for c in conv if c[12] == "sk"} == {128, 256, 320}
    assert {c[2] * c[6] // 64 for c in conv if c[6] == 1} == {1, 2, 3}
    assert {c[5] for c in conv if c[6] == 9} >= {4, 100, 320, 336}
    assert any(c[7] == 2 for c in conv) and any(c[8] for c in conv)
    assert _S[0] * _S[1] * _S[2] == 338


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_ktile_case(extmod, golden, case):
    dev, ref, bound, allocs = prepare(case)
    poison(allocs)
    y1 = run(extmod, case, dev)
    poison(allocs[1:])      # y1 is held: the workspace alone
    y2 = run(extmod, case, dev)
    kb.check(y1.reshape(ref.shape), ref, bound, case_id(case))
    assert torch.equal(y1, y2), "two calls differ"
    assert digest(y1) == golden[case_id(case)], \
        "output bits differ from the build before the K-tile reorder"


@pytest.mark.parametrize("case", [
    _conv(64, 336, 9, 320, arg=3),            # two kernels and a workspace
    _conv(192, 100, 1, 256),                  # three K-tiles, plain
], ids=case_id)
def test_ktile_under_graph_capture(extmod, case):
    """One call captured on one stream and replayed three times: each replay
    equals the eager result bit for bit."""
    dev, _, _, allocs = prepare(case)
    eager = run(extmod, case, dev)
    torch.cuda.synchronize()
    poison(allocs)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = run(extmod, case, dev)
    for _ in range(3):
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)
