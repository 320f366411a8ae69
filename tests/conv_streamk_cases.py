"""Shared by test_conv_streamk_cpu.py and test_conv_streamk_gpu.py: a Python
mirror of the stream-K tail schedule of conv256_nhwc_sk and the cases.

The schedule (ops/hip/gemm.hip, SkSched): tiles are numbered in launch order,
tile = n_block * m_blocks + m_block. The first ``dp_tiles`` have one workgroup
each. The other R tiles are R * kt units in (tile, K-tile) order, cut into
``sk_wgs`` contiguous ranges whose lengths differ by at most one (longer ones
first). A range is walked as segments, one tile and one K-tile interval each.
A segment that covers a whole tile is direct (slot -1); any other writes its
fp32 accumulators to workspace slot ``range + tile index within the tail``.

The mirror is written from that description, not from the kernel's code: it
lists every unit, deals the units out and groups each range's units by tile.
"""

import kernel_bounds as kb

BK = 64    # K-tile depth
BM = 256   # tile rows


def sk_segments(tiles: int, kt: int, dp_tiles: int, sk_wgs: int):
    """[(range, tile, kt0, kt1, slot)] in range order, then unit order."""
    units = [(t, k) for t in range(dp_tiles, tiles) for k in range(kt)]
    q, r = divmod(len(units), sk_wgs)
    out, pos = [], 0
    for j in range(sk_wgs):
        mine = units[pos:pos + q + (1 if j < r else 0)]
        pos += len(mine)
        for t in sorted({t for t, _ in mine}):
            ks = [k for tt, k in mine if tt == t]
            assert ks == list(range(ks[0], ks[-1] + 1))
            whole = len(ks) == kt
            out.append((j, t, ks[0], ks[-1] + 1,
                        -1 if whole else j + (t - dp_tiles)))
    assert pos == len(units)
    return out


def range_lengths(segs, sk_wgs):
    n = [0] * sk_wgs
    for j, _, k0, k1, _ in segs:
        n[j] += k1 - k0
    return n


def contributors(segs):
    """tile -> number of segments that meet in it."""
    c = {}
    for _, t, _, _, _ in segs:
        c[t] = c.get(t, 0) + 1
    return c


def out_hw(h, w, stride, up2):
    if up2:
        return 2 * h, 2 * w
    return (h, w) if stride == 1 else ((h - 1) // 2 + 1, (w - 1) // 2 + 1)


def n_tiles(b, h, w, k, stride, up2, bn):
    ho, wo = out_hw(h, w, stride, up2)
    return -(-(b * ho * wo) // BM) * -(-k // bn)


def seed_of(c, k, rs):
    return c * 100 + k + rs


# (b, c, h, w, k, rs, stride, up2, silu, residual, bn, dp_tiles, sk_wgs)
# A = (1, 64, 17, 19) -> 96, 3x3: M = 323, two M-tiles (the second with 67
# rows), 96 of 256 columns live, 9 K-tiles; 18 units with dp_tiles = 0.
_A = (1, 64, 17, 19, 96, 9, 1, False)
# P = (1, 192, 33, 35) -> 96, 1x1: M = 1155, five M-tiles, 3 K-tiles.
_P = (1, 192, 33, 35, 96, 1, 1, False)
SK_CASES = [
    # 9 + 9: both tiles whole, the boundary on the tile edge, no slot used
    _A + (False, False, 256, 0, 2),
    # 6 + 6 + 6: the middle range spans two tiles; 2 contributors per tile
    _A + (False, False, 256, 0, 3),
    # 5 + 5 + 4 + 4: 2 and 3 contributors
    _A + (False, False, 256, 0, 4),
    # 3 3 3 3 2 2 2: a boundary on the tile edge, 3 and 4 contributors
    _A + (False, False, 256, 0, 7),
    # one range: both tiles whole in one workgroup, LDS reused between them
    _A + (False, False, 256, 0, 1),
    # more ranges than units: 18 ranges of one K-tile, 2 idle workgroups
    _A + (False, False, 256, 0, 20),
    # dp_tiles = 1: first tile whole, second cut in 4
    _A + (False, False, 256, 1, 4),
    # bias + SiLU + residual, once, by the reduce pass and by a whole tile
    _A + (True, True, 256, 0, 4),
    _A + (True, True, 256, 1, 1),
    # 15 units in 5 + 5 + 5: the middle range has the end of tile 1, tile 2
    # whole and the start of tile 3
    _P + (False, False, 256, 0, 3),
    # dp_tiles = 2 of 5: 9 units in 5 + 4
    _P + (False, False, 256, 2, 2),
    # column-by-column stores: K_out = 6 is no multiple of 4
    (1, 64, 17, 19, 6, 9, 1, False, False, False, 128, 0, 4),
    (1, 64, 17, 19, 6, 9, 1, False, True, True, 256, 0, 3),
    # bn 128: two N-blocks, the second with 64 live columns; 4 tiles, 36 units
    (1, 64, 17, 19, 192, 9, 1, False, False, False, 128, 0, 5),
    (1, 64, 17, 19, 192, 9, 1, False, False, False, 128, 1, 7),
    # bn 320: two N-blocks, the second with 80 live columns
    (1, 64, 17, 19, 400, 9, 1, False, False, False, 320, 0, 5),
    (1, 64, 17, 19, 400, 9, 1, False, True, True, 320, 2, 3),
    # stride 2 -> 17x9 output, two M-tiles
    (2, 64, 34, 18, 96, 9, 2, False, False, False, 256, 0, 4),
    # fused upsample -> 16x16 output: one pixel-tiled tile, 3 contributors
    (1, 64, 8, 8, 96, 9, 1, True, False, False, 256, 0, 3),
    # 16x16 pixel tiles, two images = two tiles, bn 320 and 256
    (2, 64, 16, 16, 96, 9, 1, False, False, False, 256, 0, 3),
    (2, 64, 16, 16, 400, 9, 1, False, False, True, 320, 1, 4),
]

for _c in SK_CASES:
    assert _c[5] * _c[1] <= kb.DOT_BOUND_MAX_RSC, _c
    assert 0 <= _c[11] <= n_tiles(_c[0], _c[2], _c[3], _c[4], _c[6], _c[7],
                                  _c[10]), _c

# the (tiles, kt, dp_tiles, sk_wgs) grid both tests walk
SCHED_GRID = [(t, kt, dp, wgs)
              for t in (1, 2, 3, 5)
              for kt in (1, 2, 3, 9, 10)
              for dp in sorted({0, 1, t // 2, t})
              for wgs in (1, 2, 3, 4, 7, 16, t * kt + 3)]
