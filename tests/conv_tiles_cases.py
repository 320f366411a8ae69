"""Cases shared by test_conv_tiles_gpu.py and test_conv_tiles_cpu.py: the
N-tile widths (bn = 128 / 256 / 320) and the K split of conv256_nhwc_ex.

Every case keeps RS*C <= kernel_bounds.DOT_BOUND_MAX_RSC, so the dot-product
bound of kernel_bounds.conv_ref applies. That bound holds for any order of
the fp32 additions, so a split reduction needs no tolerance of its own.
"""

import kernel_bounds as kb

BK = 64   # K-tile depth of the kernel


def seed_of(c, k, rs):
    return c * 100 + k + rs


def slice_ranges(n_ktiles: int, split: int):
    """K-tile ranges [(begin, end)] the kernel gives its slices: contiguous,
    lengths differing by at most one, longer slices first. ``split`` above
    the K-tile count is clamped to it, as the launcher does."""
    split = min(split, n_ktiles)
    q, r = divmod(n_ktiles, split)
    out, begin = [], 0
    for s in range(split):
        end = begin + q + (1 if s < r else 0)
        out.append((begin, end))
        begin = end
    assert begin == n_ktiles
    return out


# (b, c, h, w, k, rs, stride, up2, silu, residual, bn)
BN320_CASES = [
    # M = 646: 3 M-tiles, the last with 134 rows; one exactly full N-block
    (2, 64, 17, 19, 320, 9, 1, False, False, False, 320),
    # 16x16 -> tile2d, two N-blocks
    (1, 64, 16, 16, 640, 9, 1, False, False, False, 320),
    # M = 81 < one tile; second N-block has 80 live columns (5 fragments)
    (1, 128, 9, 9, 400, 9, 1, False, False, False, 320),
    # last block: one whole live fragment (336) / half a fragment (328)
    (2, 64, 17, 19, 336, 9, 1, False, False, False, 320),
    (2, 64, 17, 19, 328, 9, 1, False, False, False, 320),
    (2, 64, 34, 18, 320, 9, 2, False, False, False, 320),   # stride 2
    (1, 64, 8, 8, 320, 9, 1, True, False, False, 320),      # up2, tile2d
    (2, 64, 17, 19, 320, 9, 1, False, True, False, 320),    # SiLU
    (2, 64, 17, 19, 320, 9, 1, False, False, True, 320),    # residual
]
BN128_CASES = (
    [(2, 64, 17, 19, k, 9, 1, False, False, False, 128) for k in (128, 192, 256)]
    + [(1, 64, 16, 16, k, 9, 1, False, False, False, 128) for k in (128, 192, 256)]
    + [(2, 64, 34, 18, 128, 9, 2, False, False, False, 128),   # stride 2
       (1, 64, 8, 8, 128, 9, 1, True, False, False, 128),      # up2
       (2, 64, 17, 19, 192, 9, 1, False, True, False, 128)]    # SiLU
)

# (b, c, h, w, k, rs, stride, silu, residual, bn, split)
SPLIT_CASES = [
    # 9 K-tiles: 5+4, 3+2+2+2, one tile per slice, 16 clamped to 9
    (1, 64, 9, 9, 96, 9, 1, False, False, 256, 2),
    (1, 64, 9, 9, 96, 9, 1, False, False, 256, 4),
    (1, 64, 9, 9, 96, 9, 1, False, False, 256, 9),
    (1, 64, 9, 9, 96, 9, 1, False, False, 256, 16),
    # 18 K-tiles in 4 slices (5, 5, 4, 4), both wide tiles
    (2, 128, 9, 9, 320, 9, 1, False, False, 256, 4),
    (2, 128, 9, 9, 320, 9, 1, False, False, 320, 4),
    # 1x1: 2 K-tiles, one each
    (2, 128, 12, 12, 64, 1, 1, False, False, 256, 2),
    # stride 2 -> 17x9 output, 9 K-tiles in 3 slices
    (2, 64, 34, 18, 96, 9, 2, False, False, 256, 3),
    (1, 64, 9, 9, 96, 9, 1, True, False, 256, 3),    # SiLU
    (1, 64, 9, 9, 96, 9, 1, False, True, 256, 3),    # residual
    # the narrow tile under a split
    (1, 64, 9, 9, 96, 9, 1, False, False, 128, 3),
]

for _case in BN320_CASES + BN128_CASES + SPLIT_CASES:
    assert _case[5] * _case[1] <= kb.DOT_BOUND_MAX_RSC, _case
