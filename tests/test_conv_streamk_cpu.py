"""The stream-K tail schedule of conv256_nhwc_sk covers every (tile, K-tile)
unit once, and its arithmetic stays inside the dot-product bound while its
characteristic defects leave it, shown without a GPU.

Schedule properties, on conv_streamk_cases.sk_segments over SCHED_GRID (ranges
of one unit, more ranges than units, ranges longer than a tile, dp_tiles from
0 to all): every unit of the tail in exactly one segment, each tile's segments
in K order with distinct slots, range lengths within one of each other,
whole-tile segments direct and only those.

Emulation of what the kernels do: a segment accumulates its K-tiles (k =
tap*C + c, tap-major) in fp32 over its tile's rows and columns; a whole-tile
segment adds the bias, applies SiLU, adds the residual and rounds to bf16; any
other stores the raw fp32 partial in its slot, and the reduce pass adds a
tile's slots in K order in fp32 and then does the same once. The emulation
must stay within 0.75 of kernel_bounds.conv_ref's bound and each seeded defect
must leave it on every case:

  one segment dropped            (a slot the reduce pass does not read)
  one K-tile in two segments     (overlapping ranges)
  bias added per segment         (epilogue run by the segments)
  SiLU applied per segment       (the same, on the SiLU cases)
  slot of the neighbouring tile  (reduce pass reads slot + 1 for one part)

Smallest multiple of the bound each defect reached over the cases below
(printed per case with -s): segment dropped 520, K-tile twice 422, bias per
segment 2010, SiLU per segment 734, neighbouring slot 662. The emulation
itself is at 0.440-0.491.
"""

import pytest
import torch

import conv_streamk_cases as sk
import kernel_bounds as kb
from test_conv_tiles_cpu import _bf, _silu32, im2col

EMU_MAX = 0.75


# ---------------------------------------------------------------------------
# schedule
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("tiles,kt,dp,wgs", sk.SCHED_GRID, ids=str)
def test_schedule_covers_every_unit_once(tiles, kt, dp, wgs):
    segs = sk.sk_segments(tiles, kt, dp, wgs)
    seen = {}
    for j, t, k0, k1, slot in segs:
        assert dp <= t < tiles and 0 <= k0 < k1 <= kt
        for k in range(k0, k1):
            assert (t, k) not in seen, ("unit twice", t, k)
            seen[(t, k)] = j
        # direct exactly when the segment is the whole tile
        assert (slot == -1) == (k0 == 0 and k1 == kt)
    assert len(seen) == (tiles - dp) * kt
    lens = sk.range_lengths(segs, wgs)
    assert max(lens) - min(lens) <= 1 and lens == sorted(lens, reverse=True)
    slots = [s for *_, s in segs if s >= 0]
    assert len(slots) == len(set(slots))
    assert all(s < wgs + (tiles - dp) - 1 for s in slots)
    for t in range(dp, tiles):
        mine = [(k0, k1, s) for _, tt, k0, k1, s in segs if tt == t]
        # K order as listed, contiguous from 0 to kt
        assert mine[0][0] == 0 and mine[-1][1] == kt
        for a, b in zip(mine, mine[1:]):
            assert a[1] == b[0]
        if len(mine) > 1:
            # what the reduce pass assumes: consecutive slots in K order
            first = mine[0][2]
            assert [s for *_, s in mine] == list(range(first,
                                                       first + len(mine)))


def test_schedule_examples():
    # (1, 64, 17, 19) -> 96: 2 tiles of 9 K-tiles
    assert sk.sk_segments(2, 9, 0, 3) == [
        (0, 0, 0, 6, 0), (1, 0, 6, 9, 1), (1, 1, 0, 3, 2), (2, 1, 3, 9, 3)]
    assert sk.sk_segments(2, 9, 0, 2) == [(0, 0, 0, 9, -1), (1, 1, 0, 9, -1)]
    c7 = sk.contributors(sk.sk_segments(2, 9, 0, 7))
    assert c7 == {0: 3, 1: 4}
    # a range over three tiles, the middle one whole
    segs = sk.sk_segments(5, 3, 0, 3)
    assert [s for s in segs if s[0] == 1] == [
        (1, 1, 2, 3, 2), (1, 2, 0, 3, -1), (1, 3, 0, 1, 4)]
    assert sk.sk_segments(3, 2, 3, 4) == []


# ---------------------------------------------------------------------------
# numerics
# ---------------------------------------------------------------------------


def emulate_streamk_conv(x, wk, bias, rs, stride, bn, dp_tiles, sk_wgs,
                         silu=False, residual=None, defect=None):
    a, (b, ho, wo) = im2col(x, rs, stride)
    wt = kb.repack_weight(wk).float()
    m, n = a.shape[0], wt.shape[0]
    kt = a.shape[1] // sk.BK
    gx = -(-m // sk.BM)
    tiles = gx * -(-n // bn)
    segs = ([(-1, t, 0, kt, -1) for t in range(dp_tiles)]
            + sk.sk_segments(tiles, kt, dp_tiles, sk_wgs))
    split = [i for i, s in enumerate(segs) if s[4] >= 0]
    if defect == "tile twice" and split:
        # the first cut segment that does not start its tile starts one early
        i = next(i for i in split if segs[i][2] > 0)
        j, t, k0, k1, s = segs[i]
        segs[i] = (j, t, k0 - 1, k1, s)
    res2d = None if residual is None else residual.float().reshape(m, n)

    def finish(acc, rows, cols):
        y = acc + bias.float()[cols]
        if silu:
            y = _silu32(y)
        if res2d is not None:
            y = y + res2d[rows][:, cols]
        return y

    out = torch.zeros(m, n)
    slots = {}
    for i, (j, t, k0, k1, slot) in enumerate(segs):
        rows = slice((t % gx) * sk.BM, min(m, (t % gx + 1) * sk.BM))
        cols = slice((t // gx) * bn, min(n, (t // gx + 1) * bn))
        p = (a[rows, k0 * sk.BK:k1 * sk.BK]
             @ wt[cols, k0 * sk.BK:k1 * sk.BK].t())
        if slot < 0:
            out[rows, cols] = finish(p, rows, cols)
            continue
        if defect == "bias per segment":
            p = p + bias.float()[cols]
        if defect == "silu per segment":
            p = _silu32(p + bias.float()[cols])
        slots[slot] = (t, p)
    by_tile = {}
    for slot in sorted(slots):
        by_tile.setdefault(slots[slot][0], []).append(slot)
    dropped = False
    for t, ss in by_tile.items():
        rows = slice((t % gx) * sk.BM, min(m, (t % gx + 1) * sk.BM))
        cols = slice((t // gx) * bn, min(n, (t // gx + 1) * bn))
        parts = [slots[s][1] for s in ss]
        if defect == "segment dropped" and not dropped:
            parts, dropped = parts[:-1], True
        if defect == "neighbour slot" and not dropped:
            # the last part comes from the next slot in memory (another
            # tile's, or this tile's first when there is none)
            other = slots.get(ss[-1] + 1, slots[ss[0]])[1]
            if other.shape == parts[-1].shape:
                parts, dropped = parts[:-1] + [other], True
        acc = parts[0].clone()
        for p in parts[1:]:
            acc = acc + p
        if defect in ("bias per segment", "silu per segment"):
            y = acc
            if res2d is not None:
                y = y + res2d[rows][:, cols]
            out[rows, cols] = y
        else:
            out[rows, cols] = finish(acc, rows, cols)
    return _bf(out.reshape(b, ho, wo, n)), bool(split)


# the emulation has no upsample or pixel-tiled address mode: both only change
# which rows a tile holds, which the GPU test covers
EMU_CASES = [c for c in sk.SK_CASES
             if not c[7] and not (c[2] % 16 == 0 and c[3] % 16 == 0)]


@pytest.mark.parametrize("case", EMU_CASES, ids=str)
def test_streamk_emulation_inside_defects_outside(case):
    b, c, h, w, k, rs, stride, up2, silu, residual, bn, dp, wgs = case
    x, wk, bias = kb.conv_inputs(sk.seed_of(c, k, rs), b, c, h, w, k, rs)
    res = None
    if residual:
        ho, wo = sk.out_hw(h, w, stride, up2)
        g = torch.Generator().manual_seed(sk.seed_of(c, k, rs) + 1)
        res = kb.bf16_exact(torch.randn(b, ho, wo, k, generator=g))
    ref, bound = kb.conv_ref(x, wk, bias, stride=stride, silu=silu,
                             residual=res)
    kw = dict(rs=rs, stride=stride, bn=bn, dp_tiles=dp, sk_wgs=wgs, silu=silu,
              residual=res)
    y, has_split = emulate_streamk_conv(x, wk, bias, **kw)
    r = kb.err_ratio(y, ref, bound)
    defects = []
    if has_split:
        defects = ["segment dropped", "tile twice", "bias per segment",
                   "neighbour slot"]
        if silu:
            defects.append("silu per segment")
    rd = {d: kb.err_ratio(emulate_streamk_conv(x, wk, bias, defect=d, **kw)[0],
                          ref, bound) for d in defects}
    print(f"bn{bn} dp{dp} wgs{wgs} {(b, c, h, w)}->{k} rs{rs} s{stride} "
          f"silu={silu} res={residual}: emulation {r:.3f}  "
          + "  ".join(f"{d} {v:.0f}" for d, v in rd.items()))
    assert r <= EMU_MAX, r
    for d, v in rd.items():
        assert v > 10.0, (d, v)
