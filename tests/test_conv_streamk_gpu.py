"""conv256_nhwc_sk: the stream-K tail of the 256-tile conv with its schedule
pinned (width, data-parallel tiles, number of ranges), the reduce pass over
the cut tiles, and the chooser conv256_sched that conv256_nhwc follows.

Reference and bound: kernel_bounds.conv_ref, |err| <= 2U|ref| + n*2^-23*mag
with n = RS*C + 1, which holds for any order of the fp32 additions, so a tile
summed from several segments uses it unchanged. Bias is N(0, 1): a bias added
per segment, or a SiLU applied per segment, lands hundreds of bounds out
(test_conv_streamk_cpu.py shows by how much, and does the same for a dropped
segment, a K-tile in two segments and a slot read from the neighbouring tile).

Measured max(err/bound) on MI355X: profiles/r15_conv_streamk.md, section 7.
"""

import os
import subprocess
import sys

import pytest
import torch

import conv_streamk_cases as sk
import kernel_bounds as kb
from test_conv_tiles_gpu import FLAGSHIP_PLANS

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
        x, wk, bias = kb.conv_inputs(sk.seed_of(c, k, rs), b, c, h, w, k, rs)
        res = None
        if residual:
            ho, wo = sk.out_hw(h, w, stride, up2)
            g = torch.Generator().manual_seed(sk.seed_of(c, k, rs) + 1)
            res = kb.bf16_exact(torch.randn(b, ho, wo, k, generator=g))
        ref, bound = kb.conv_ref(x, wk, bias, stride=stride, up2=up2,
                                 silu=silu, residual=res)
        dev = (_dev_bf16(x), _dev_bf16(kb.repack_weight(wk)), bias.cuda(),
               _dev_bf16(res) if residual else _nores())
        _REFS[key] = (dev, ref, bound)
    return _REFS[key]


def _run_sk(extmod, dev, b, c, h, w, k, rs, stride, up2, silu, bn, dp, wgs):
    x, wt, bias, res = dev
    return extmod.conv256_nhwc_sk(x, wt, bias, res, b, h, w, c, k, rs, stride,
                                  up2, silu, bn, dp, wgs)


def _run_ex(extmod, dev, b, c, h, w, k, rs, stride, up2, silu, bn, split):
    x, wt, bias, res = dev
    return extmod.conv256_nhwc_ex(x, wt, bias, res, b, h, w, c, k, rs, stride,
                                  up2, silu, bn, split)


# ---------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------


def test_cases_reach_what_they_claim():
    """Contributors per tile 1, 2, 3 and >= 4; a range over three tiles; a
    boundary on a tile edge; dp_tiles 0, between, and all widths."""
    seen, three, edge = set(), False, False
    for case in sk.SK_CASES:
        b, c, h, w, k, rs, stride, up2, _, _, bn, dp, wgs = case
        tiles = sk.n_tiles(b, h, w, k, stride, up2, bn)
        segs = sk.sk_segments(tiles, rs * c // sk.BK, dp, wgs)
        seen |= set(sk.contributors(segs).values())
        for j in range(wgs):
            mine = [s for s in segs if s[0] == j]
            three |= len(mine) >= 3
            edge |= bool(mine) and mine[0][2] == 0 and j > 0
    assert {1, 2, 3} <= seen and max(seen) >= 4 and three and edge
    assert {c[10] for c in sk.SK_CASES} == {128, 256, 320}
    assert any(c[11] == 0 for c in sk.SK_CASES)
    assert any(0 < c[11] < sk.n_tiles(c[0], c[2], c[3], c[4], c[6], c[7],
                                      c[10]) for c in sk.SK_CASES)


@pytest.mark.parametrize("case", sk.SK_CASES, ids=str)
def test_conv256_streamk(extmod, case):
    b, c, h, w, k, rs, stride, up2, silu, residual, bn, dp, wgs = case
    dev, ref, bound = _case(b, c, h, w, k, rs, stride, up2, silu, residual)
    y = _run_sk(extmod, dev, b, c, h, w, k, rs, stride, up2, silu, bn, dp, wgs)
    kb.check(y, ref, bound, f"conv256 sk bn{bn} dp{dp} wgs{wgs} {(b, c, h, w)}"
             f"->{k} rs{rs} s{stride} up2={up2} silu={silu} res={residual}")


# ---------------------------------------------------------------------------
# integer-exact
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bn,dp,wgs", [(256, 0, 4), (256, 0, 7), (256, 1, 3),
                                       (320, 0, 5), (128, 1, 20)])
def test_streamk_integer_exact(extmod, bn, dp, wgs):
    """Operands from {-1, 1, 2} x {1, 0.5}, 25 % dense (as
    test_gemm256_integer_exact), no bias: every product is a multiple of 1/4,
    every partial sum is far below 2^24 and |result| < 64, so fp32 sums are
    exact in any order and bf16 holds the result. The pinned tail call must
    equal the plain call and the fp64 conv element for element: a lost or
    doubled K-tile is a wrong integer."""
    b, c, h, w, k, rs = 1, 64, 17, 19, 96, 9
    g = torch.Generator().manual_seed(c * rs)

    def operand(*shape):
        vals = torch.tensor([-1.0, 1.0, 2.0])[
            torch.randint(0, 3, shape, generator=g)]
        keep = torch.rand(*shape, generator=g) < 0.25
        half = torch.where(torch.rand(*shape, generator=g) < 0.5, 0.5, 1.0)
        return vals * keep * half

    x, wk = operand(b, h, w, c), operand(k, c, 3, 3)
    for t in (x, wk):
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    ref, _ = kb.conv_ref(x, wk)
    assert ref.abs().max() < 64
    assert torch.equal(ref.to(torch.bfloat16).double(), ref)
    dev = (_dev_bf16(x), _dev_bf16(kb.repack_weight(wk)), _nores(), _nores())
    y = _run_sk(extmod, dev, b, c, h, w, k, rs, 1, False, False, bn, dp, wgs)
    plain = _run_ex(extmod, dev, b, c, h, w, k, rs, 1, False, False, bn, 1)
    assert torch.equal(y, plain)
    bad = (y.cpu().double() != ref).sum().item()
    assert bad == 0, f"{bad} of {ref.numel()} elements differ from the conv"


# ---------------------------------------------------------------------------
# bit equality and replay
# ---------------------------------------------------------------------------

_BIT = (1, 64, 17, 19, 96, 9)


@pytest.mark.parametrize("case", [
    (1, 64, 17, 19, 96, 9, 1, False, True, True, 256),
    (1, 64, 17, 19, 400, 9, 1, False, False, False, 320),
    (1, 64, 17, 19, 6, 9, 1, False, False, False, 128),
    (2, 64, 16, 16, 96, 9, 1, False, False, False, 256),
    (2, 64, 34, 18, 96, 9, 2, False, False, False, 256),
], ids=str)
def test_all_tiles_data_parallel_equals_plain(extmod, case):
    """dp_tiles = tiles: every tile whole, through the stream-K kernel; the
    bits of conv256_nhwc_ex(..., bn, 1)."""
    b, c, h, w, k, rs, stride, up2, silu, residual, bn = case
    dev, _, _ = _case(b, c, h, w, k, rs, stride, up2, silu, residual)
    tiles = sk.n_tiles(b, h, w, k, stride, up2, bn)
    y = _run_sk(extmod, dev, b, c, h, w, k, rs, stride, up2, silu, bn, tiles,
                3)
    plain = _run_ex(extmod, dev, b, c, h, w, k, rs, stride, up2, silu, bn, 1)
    assert torch.equal(y, plain)


def test_streamk_repeats_bit_for_bit(extmod):
    """Same call twice; then a call of another shape and schedule (its slots
    land in the memory the allocator just got back), then the first call
    again: all three equal. Stale slot contents would show here."""
    dev, _, _ = _case(*_BIT)
    args = _BIT + (1, False, False, 256, 0, 7)
    y1 = _run_sk(extmod, dev, *args)
    y2 = _run_sk(extmod, dev, *args)
    assert torch.equal(y1, y2)
    other = (1, 64, 17, 19, 400, 9)
    odev, _, _ = _case(*other)
    _run_sk(extmod, odev, *other, 1, False, False, 320, 0, 5)
    y3 = _run_sk(extmod, dev, *args)
    assert torch.equal(y1, y3)


def test_streamk_under_graph_capture(extmod):
    """One tail call captured on one stream (no branches) and replayed twice:
    the slots come from torch's allocator, so capture is legal and both
    replays equal the eager result."""
    dev, ref, bound = _case(*_BIT)
    args = _BIT + (1, False, False, 256, 0, 7)
    eager = _run_sk(extmod, dev, *args)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = _run_sk(extmod, dev, *args)
    outs = []
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        outs.append(y.clone())
    assert torch.equal(outs[0], eager) and torch.equal(outs[1], eager)
    kb.check(outs[0], ref, bound, "conv256 sk replayed")


# ---------------------------------------------------------------------------
# range arithmetic
# ---------------------------------------------------------------------------


def test_extension_segments_match_the_mirror(extmod):
    for tiles, kt, dp, wgs in sk.SCHED_GRID:
        got = [tuple(s) for s in extmod.conv256_sk_segments(tiles, kt, dp,
                                                            wgs)]
        assert got == sk.sk_segments(tiles, kt, dp, wgs), (tiles, kt, dp, wgs)


# ---------------------------------------------------------------------------
# chooser
# ---------------------------------------------------------------------------

# (M, K_out, Kdim) -> (bn, split_k, dp_tiles, sk_wgs) measured best on MI355X
# (profiles/r15_conv_streamk.md, section 3). Every triple of FLAGSHIP_PLANS
# that is not listed keeps its round-counting plan with no tail.
FLAGSHIP_TAILS = {
    # 68x68 level: 578 tiles of 320 = two rounds + 66 tiles (L 12 / 24 / 35)
    (32 * 68 * 68, 320, 9 * 320): (320, 1, 512, 256),
    (32 * 68 * 68, 320, 9 * 640): (320, 1, 512, 256),
    (32 * 68 * 68, 320, 9 * 960): (320, 1, 512, 256),
    # 34x34 level: the wider tile now, one round + 34 tiles (L 12)
    (32 * 34 * 34, 640, 9 * 640): (320, 1, 256, 256),
    # 17x17 level: 148 tiles of 320, the whole grid in the tail (L 105 / 209)
    (32 * 17 * 17, 1280, 9 * 1280): (320, 1, 0, 256),
    (32 * 17 * 17, 1280, 9 * 2560): (320, 1, 0, 256),
    # fused 2x upsample to 34x34: 580 tiles of 320, two rounds + 68 (L 48)
    (32 * 34 * 34, 1280, 9 * 1280): (320, 1, 512, 256),
    # the UNet's K_out = 4 output conv: two rounds + 66 tiles of 128 (L 12)
    (32 * 68 * 68, 4, 9 * 320): (128, 1, 512, 256),
}


@pytest.mark.parametrize("triple", FLAGSHIP_PLANS, ids=str)
def test_sched_flagship(extmod, triple):
    m, k_out, kdim = triple
    bn, split = FLAGSHIP_PLANS[triple]
    want = FLAGSHIP_TAILS.get(
        triple, (bn, split, -(-m // 256) * -(-k_out // bn), 0))
    assert tuple(extmod.conv256_sched(*triple)) == want


def test_sched_sweep(extmod):
    """Where the tail path is taken: dp_tiles is a whole number of rounds,
    at most one round of ranges, never together with a K split, the tail is
    neither empty nor nearly a round, and no range is under the floor of 10
    K-tiles (a range is cut where it crosses a tile edge, so its segments
    can be shorter; the floor is on what a workgroup gets). Elsewhere the
    answer is conv256_plan's with every tile data-parallel."""
    taken = 0
    for m in (81, 2592, 9248, 36992, 147968, 16 * 544 * 544):
        for k_out in (4, 64, 128, 320, 640, 1280):
            for kdim in (64, 576, 2880, 11520, 23040):
                bn, split, dp, wgs = extmod.conv256_sched(m, k_out, kdim)
                tiles = -(-m // 256) * -(-k_out // bn)
                if wgs == 0:
                    assert (bn, split) == tuple(
                        extmod.conv256_plan(m, k_out, kdim))
                    assert dp == tiles
                    continue
                taken += 1
                assert split == 1 and bn in (128, 256, 320)
                assert dp % 256 == 0 and wgs <= 256
                assert 0 < tiles - dp < 256
                units = (tiles - dp) * (kdim // 64)
                assert units // wgs >= 10, (m, k_out, kdim, bn, dp, wgs)
    assert taken > 0
    # 65 tiles of 36 K-tiles: the longest range would have 10 K-tiles, the
    # shortest 9, under the floor
    assert tuple(extmod.conv256_sched(321 * 256, 64, 36 * 64)) == (
        128, 1, 321, 0)


def test_default_entry_follows_sched(extmod):
    """conv256_nhwc equals the pinned call of conv256_sched's answer bit for
    bit, on the cheapest shape found on which the chooser takes the tail path
    (328 M-tiles of 128 columns, 36 K-tiles: one round + 72 tiles, ranges of
    10 and 11 K-tiles). It
    is too large for an fp64 reference on the host, so the result is held
    against the plain launch instead."""
    b, c, h, w, k, rs = 1, 256, 64, 1312, 64, 9
    bn, split, dp, wgs = extmod.conv256_sched(b * h * w, k, rs * c)
    assert (bn, split, dp, wgs) == (128, 1, 256, 256)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = (torch.randn(b, h, w, c, device="cuda", generator=g) / 4).bfloat16()
    wt = (torch.randn(k, rs * c, device="cuda", generator=g) / 8).bfloat16()
    dev = (x, wt, torch.randn(k, device="cuda", generator=g), _nores())
    y0 = extmod.conv256_nhwc(*dev, b, h, w, c, k, rs, 1, False, False)
    y1 = _run_sk(extmod, dev, b, c, h, w, k, rs, 1, False, False, bn, dp, wgs)
    assert torch.equal(y0, y1)
    y2 = _run_ex(extmod, dev, b, c, h, w, k, rs, 1, False, False, 0, 0)
    assert torch.equal(y0, y2)
    # against the plain launch: the same fp32 products added in another
    # order, one bf16 rounding each. Either is within U|v| + n*2^-24*mag of the
    # exact value v, mag = conv(|x|, |w|) + |bias|, which the plain launch
    # computes here too (its own bf16 rounding of mag covered by the 1.02)
    plain = _run_ex(extmod, dev, b, c, h, w, k, rs, 1, False, False, bn, 1)
    mag = extmod.conv256_nhwc_ex(x.abs(), wt.abs(), dev[2].abs(), _nores(),
                                 b, h, w, c, k, rs, 1, False, False, bn, 1)
    n = rs * c + 1
    err = (y0.double() - plain.double()).abs()
    bound = (2 * kb.U * torch.maximum(y0.abs(), plain.abs()).double()
             + 1.02 * n * 2.0 ** -23 * mag.double())
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(plain.abs().max()) > 1.0


def test_streamk_switch_off_in_child_process():
    """DISTGPU_CONV_STREAMK=0 is read once per process: in a fresh child
    conv256_sched is conv256_plan plus an empty tail on every flagship row."""
    code = (
        "import sys\n"
        "from comfyui_distributed_amd.ops import ext\n"
        "m = ext.get_ext(required=True)\n"
        f"rows = {list(FLAGSHIP_PLANS)!r}\n"
        "for r in rows:\n"
        "    bn, split = m.conv256_plan(*r)\n"
        "    tiles = -(-r[0] // 256) * -(-r[1] // bn)\n"
        "    assert tuple(m.conv256_sched(*r)) == (bn, split, tiles, 0), r\n"
        "print('ok')\n")
    env = dict(os.environ, DISTGPU_CONV_STREAMK="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]
