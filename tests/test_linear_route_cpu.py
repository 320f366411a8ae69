"""Linear routing of dispatch.linear_mfma without a GPU: the table lookup for
the flagship shapes, the DISTGPU_GEMM256=0 switch, and the CPU arithmetic of
the residual argument."""

import os
import subprocess
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

from comfyui_distributed_amd.models import unet as U
from comfyui_distributed_amd.ops import dispatch

ROOT = Path(__file__).resolve().parent.parent

# SD1.5 UNet at tile batch 32, 24 and 16 (544x544 tiles: 68x68, 34x34, 17x17
# tokens): (M, N, K) of every Linear of the transformer blocks
FLAGSHIP = [(hw * tb, n, k) for tb in (32, 24, 16)
            for hw, c in ((4624, 320), (1156, 640), (289, 1280))
            for n, k in ((c, c), (3 * c, c), (8 * c, c), (c, 4 * c))] \
    + [(2464, 2 * c, 768) for c in (320, 640, 1280)] \
    + [(32768, 640, 640), (32768, 1920, 640), (32768, 640, 2560)]  # SDXL 64x64


def test_table_is_well_formed():
    assert isinstance(dispatch._LINEAR_ROUTES, tuple)
    seen = set()
    for row in dispatch._LINEAR_ROUTES:
        k, n, m_lo, m_hi, fuse = row
        assert k % 64 == 0 and n > 0 and 0 < m_lo <= m_hi
        assert isinstance(fuse, bool)
        assert (k, n, m_lo) not in seen
        seen.add((k, n, m_lo))


def test_flagship_lookup(monkeypatch):
    """Every row of the table is reached by a flagship Linear, a shape off the
    table stays on hipBLASLt, and the lookup is the table."""
    monkeypatch.setattr(dispatch, "_GEMM256", True)
    hit = set()
    for m, n, k in FLAGSHIP:
        routed, fuse = dispatch.linear_route(m, n, k)
        rows = [r for r in dispatch._LINEAR_ROUTES
                if r[0] == k and r[1] == n and r[2] <= m <= r[3]]
        assert routed == bool(rows)
        assert fuse == (rows[0][4] if rows else False)
        hit.update(rows)
    assert hit == set(dispatch._LINEAR_ROUTES)
    # where this pull request's microbench left hipBLASLt ahead
    assert dispatch.linear_route(147968, 2560, 320) == (False, False)
    assert dispatch.linear_route(9248, 1280, 5120) == (False, False)
    assert dispatch.linear_route(180, 320, 320) == (False, False)
    # the ratio follows the round count, not M: measured behind or level
    assert dispatch.linear_route(110976, 960, 320) == (False, False)
    assert dispatch.linear_route(73984, 320, 320) == (False, False)
    assert dispatch.linear_route(18496, 640, 2560) == (False, False)


def test_switch_off(monkeypatch):
    monkeypatch.setattr(dispatch, "_GEMM256", False)
    for m, n, k in FLAGSHIP:
        assert dispatch.linear_route(m, n, k) == (False, False)


def test_env_switch():
    """DISTGPU_GEMM256=0 is read at import: a fresh interpreter."""
    code = ("from comfyui_distributed_amd.ops import dispatch as d;"
            "print(d._GEMM256, any(d.linear_route(m, n, k)[0] "
            "for k, n, m, _, _ in d._LINEAR_ROUTES))")
    outs = []
    for val in ("0", "1"):
        env = dict(os.environ, DISTGPU_GEMM256=val)
        outs.append(subprocess.run([sys.executable, "-c", code], cwd=ROOT,
                                   env=env, capture_output=True, text=True,
                                   check=True).stdout.split())
    assert outs[0] == ["False", "False"]
    assert outs[1] == ["True", str(bool(dispatch._LINEAR_ROUTES))]


def test_odd_residual_takes_the_separate_add(monkeypatch):
    """A residual that is not the output's shape never reaches the reshape of
    the fused route: the guard is plain Python, checked here on the CPU path's
    arithmetic (broadcast add) for a shape whose row would fuse."""
    monkeypatch.setattr(dispatch, "_GEMM256", True)
    monkeypatch.setattr(dispatch, "_LINEAR_ROUTES", ((64, 48, 1, 10 ** 6, True),))
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 37, 64, generator=g).bfloat16()
    w = torch.randn(48, 64, generator=g).bfloat16()
    r = torch.randn(48, generator=g).bfloat16()
    assert torch.equal(dispatch.linear_mfma(x, w, None, residual=r),
                       F.linear(x, w) + r)


def test_residual_on_cpu_is_linear_plus_add():
    g = torch.Generator().manual_seed(5)
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(2, 37, 64, generator=g).to(dtype)
        w = torch.randn(48, 64, generator=g).to(dtype)
        b = torch.randn(48, generator=g).to(dtype)
        r = torch.randn(2, 37, 48, generator=g).to(dtype)
        assert torch.equal(dispatch.linear_mfma(x, w, b, residual=r),
                           F.linear(x, w, b) + r)
        assert torch.equal(dispatch.linear_mfma(x, w, None, residual=r),
                           F.linear(x, w) + r)
        assert torch.equal(dispatch.linear_mfma(x, w, b, True, residual=r),
                           F.silu(F.linear(x, w, b)) + r)
        assert torch.equal(dispatch.linear_mfma(x, w, b), F.linear(x, w, b))


def test_transformer_block_on_cpu_matches_the_written_out_adds():
    """The residual threaded through the modules is the three skip adds and
    the SpatialTransformer's, value for value."""
    torch.manual_seed(3)
    st = U.SpatialTransformer(64, 32, 2, 32)
    x = torch.randn(2, 64, 5, 6)
    ctx = torch.randn(2, 7, 32)
    with torch.no_grad():
        y = st(x, ctx)
        b, c, h, w = x.shape
        t = st.norm(x).permute(0, 2, 3, 1).reshape(b, h * w, c)
        t = st.proj_in(t)
        for blk in st.blocks:
            t = t + blk.attn1(blk.norm1(t))
            t = t + blk.attn2(blk.norm2(t), ctx)
            t = t + blk.ff(blk.norm3(t))
        t = st.proj_out(t)
        want = x + t.reshape(b, h, w, c).permute(0, 3, 1, 2)
    assert torch.equal(y, want)
