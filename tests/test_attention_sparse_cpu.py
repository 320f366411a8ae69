"""Block-sparse FP8 attention on the CPU: ops.attn_window against the rule token
by token, the definition of attention_fp8(blocks=), the WAN wiring. The mask
table, exact construction and bound are shared with the GPU tests."""

import pytest
import torch

import kernel_bounds as kb
from comfyui_distributed_amd.models import create_diffusion_stack, quant
from comfyui_distributed_amd.ops import dispatch
from test_attention_fp8_cpu import R, _tiny, selection_case

D, KT, SP = dispatch.ATTN_FP8_D, dispatch.ATTN_FP8_KT, dispatch.ATTN_FP8_SP
NQ, NK = 2 * R + 5, 5 * KT + 5       # 3 q-blocks, 6 key tiles, the last partial
MASK_TILES = {                        # allowed key tiles of q-blocks 0, 1, 2
    "full": [range(6)] * 3,
    "band": [(0, 1), (1, 2, 3), (3, 4, 5)],        # 2i-1 .. 2i+1, clipped
    "single": [(2,), (0,), (4,)],
    "pair": [(1, 4), (0, 5), (2, 3)],
    "gaps": [(0, 3, 5)] * 3,
    "last_only": [(5,)] * 3,
    "no_last": [range(5)] * 3,
    "ragged": [(2,), (0, 2, 4), range(6)],
}


def mask_of(name):
    m = torch.zeros(3, 6, dtype=torch.bool)
    for i, tiles in enumerate(MASK_TILES[name]):
        m[i, list(tiles)] = True
    return m


def allowed_keys(mask, nq=NQ, nk=NK):
    """block mask -> bool [nq, nk]"""
    return mask.repeat_interleave(R, 0)[:nq].repeat_interleave(KT, 1)[:, :nk]


def masked_ref_and_bound(a, nk, scale, allowed):
    """test_attention_fp8_gpu._ref_and_bound with the softmax, and so P in
    every term, taken over the allowed keys only."""
    h = a.heads
    q, k, v = (kb.split_heads(t.double().cpu(), h) for t in a.dequant())
    s = torch.bmm(q, k.transpose(1, 2)) * scale
    p = torch.softmax(s.masked_fill(~allowed, float("-inf")), dim=-1)
    ref, pav = torch.bmm(p, v), torch.bmm(p, v.abs())
    bound = (2.0 ** -8 * ref.abs() + 2.0 ** -4 * pav
             + nk * 2.0 ** -(SP + 10) * v.abs().amax(dim=1, keepdim=True)
             + (nk + D + 16) * 2.0 ** -23 * pav)
    return kb.merge_heads(ref, h), kb.merge_heads(bound, h)


def sparse_selection_case(b, h, mask, nq=NQ, nk=NK):
    """selection_case's K and V, q_i = k_pi(i) with pi(i) among the valid keys
    of the tiles q-block i / 256 is allowed, offsets 0..2 of a tile excepted:
    q-block y with a disallowed tile gets a decoy there at offset y, a copy of
    the offset-y key of an allowed tile, which its first query selects. Nobody
    else selects either: the output is v[pi] exactly, and a mixture for that
    query if the disallowed tile is visited. -> q, k, v, want."""
    _, k, v, _ = selection_case(b, h, nq, nk)
    g = torch.Generator().manual_seed(1)
    pi = torch.empty(nq, dtype=torch.long)
    for y in range(mask.shape[0]):
        r0, r1 = y * R, min(nq, y * R + R)
        tiles = mask[y].nonzero().flatten()
        keys = (tiles[:, None] * KT + torch.arange(3, KT)).flatten()
        keys = keys[keys < nk]
        pi[r0:r1] = keys[torch.randint(0, len(keys), (r1 - r0,), generator=g)]
        hidden = (~mask[y]).nonzero().flatten()
        if len(hidden):
            src, decoy = int(tiles[-1]) * KT + y, int(hidden[0]) * KT + y
            k[:, decoy] = k[:, src]
            pi[r0] = src
    idx = pi[None, :, None].expand(b, -1, h * D)
    return k.gather(1, idx), k, v, v.gather(1, idx)


@pytest.mark.parametrize("grid,tile", [((4, 8, 16), (2, 4, 8)),
                                       ((4, 10, 21), (2, 4, 8))])   # ragged
def test_window_lists(grid, tile):
    n = grid[0] * grid[1] * grid[2]
    perm, inv, full = dispatch.attn_window(grid, tile, (9, 9, 9))
    assert torch.equal(perm.sort().values, torch.arange(n))
    assert torch.equal(perm[inv], torch.arange(n))
    assert full.mask.all() and full.density == 1.0
    blk = dispatch.attn_window(grid, tile, (0, 1, 0))[2]
    assert blk.density < 1.0 and blk.mask.any(dim=1).all()
    assert torch.equal(blk.cnt.long(), blk.mask.sum(dim=1))


def test_definition_selects_exactly(name="ragged"):
    mask = mask_of(name)
    q, k, v, want = sparse_selection_case(2, 2, mask)
    a = dispatch.quantize_attn_qkv(q, k, v, 2)
    qd, kd, vd = a.dequant()
    assert torch.equal(vd, v)
    s = torch.einsum("bqhd,bkhd->bhqk", qd.reshape(2, NQ, 2, D),
                     kd.reshape(2, NK, 2, D)) / D ** 0.5
    top2 = s.masked_fill(~allowed_keys(mask), float("-inf")).topk(2).values
    gap = (top2[..., 0] - top2[..., 1]).min().item()
    print(f"{name}: min logit gap over the allowed keys {gap:.1f} nats")
    assert gap > 20.0      # as test_attention_fp8_cpu: 11.1 nats are needed
    blocks = dispatch.attn_blocks(mask)
    assert torch.equal(dispatch.attention_fp8(a, blocks=blocks), want)
    # the decoys are live: unmasked, the result differs
    assert not torch.equal(dispatch.attention_fp8(a), want)


def test_definition_within_bound_and_full_mask_is_dense():
    q, k, v = kb.attn_inputs(NQ + NK, 2, 2, NQ, NK, 2 * D)
    a = dispatch.quantize_attn_qkv(q, k, v, 2)
    for name in ("band", "ragged"):
        mask = mask_of(name)
        out = dispatch.attention_fp8(a, blocks=dispatch.attn_blocks(mask))
        ref, bound = masked_ref_and_bound(a, NK, D ** -0.5, allowed_keys(mask))
        kb.check(out, ref, bound, f"attention_fp8 definition, {name}")
    full = dispatch.attn_blocks(mask_of("full"))
    assert torch.equal(dispatch.attention_fp8(a, blocks=full),
                       dispatch.attention_fp8(a))
    for bad in (mask_of("full")[:2], mask_of("full")[:, :5]):   # wrong shape
        with pytest.raises(ValueError):
            dispatch.attention_fp8(a, blocks=dispatch.attn_blocks(bad))
    empty_row = mask_of("band")
    empty_row[1] = False
    with pytest.raises(ValueError):
        dispatch.attn_blocks(empty_row)


def test_wan_window():
    """Token grid (2, 16, 16), tiles (1, 8, 8): 2 tiles per axis, 2 q-blocks, 4
    key tiles, and every run of 128 tokens holds the same tokens in raster and
    tile-major order, so the K scales agree and a full window only reorders
    fp32 sums. 1e-5 of max|y| is a hundred fp32 roundings; a token leaves it
    only where the reordered K mean (logits move ~1e-7 of themselves) carries
    one of 131k K codes or 524k weights over an e4m3 boundary (steps 2^-4, so
    ~2e-6 each: one token expected, 4 allowed). Such a weight moves by 2^-4 of
    itself and, with random weights and 512 keys, holds under 8/512 of its
    row: 1e-3 of max|y| caps those tokens. Measured: 1 token over 1e-5
    (4.8e-5), median 9e-8."""
    model, (_, t, ctx), _ = _tiny("wan")
    x = torch.randn(1, 4, 2, 32, 32, generator=torch.Generator().manual_seed(5))
    tile = (1, 8, 8)
    with torch.no_grad():
        with pytest.raises(ValueError):          # bf16 attention blocks
            quant.set_attn_window(model, tile, (0, 0, 0))
        quant.set_attn_dtype(model, "fp8")
        y0 = model(x, t, ctx)
        assert quant.set_attn_window(model, tile, (1, 1, 1))
        y1 = model(x, t, ctx)
        quant.set_attn_window(model, tile, (0, 0, 0))    # a q-block sees its t
        y2 = model(x, t, ctx)
        assert not quant.set_attn_window(model, None)
        assert torch.equal(model(x, t, ctx), y0)
    perm, _, blocks = dispatch.attn_window((2, 16, 16), tile, (0, 0, 0))
    assert not torch.equal(perm, torch.arange(512)) and blocks.density == 0.5
    err = (y1 - y0).abs() / y0.abs().max()
    tok = err[0].amax(0).reshape(2, 16, 2, 16, 2).amax(dim=(2, 4)).flatten()
    print(f"full window, of max|y|: median token {tok.median().item():.1e}, "
          f"{(tok > 1e-5).sum().item()} over 1e-5, max {tok.max().item():.1e}")
    assert (tok > 1e-5).sum().item() <= 4 and tok.max().item() <= 1e-3
    rel = ((y2 - y0).norm() / y0.norm()).item()
    assert torch.isfinite(y2).all() and rel > 1e-4, rel
    quant.set_attn_window(model, tile, (0, 0, 0))
    quant.set_attn_dtype(model, None)            # bf16 again: the window goes
    assert model.attn_window is None


def test_window_option_rules(monkeypatch):
    win = ((2, 4, 8), (0, 0, 0))
    for name in ("tiny", "flux_tiny", "wan_tiny"):   # wan_tiny: bf16 attention
        with pytest.raises(ValueError):
            create_diffusion_stack(name, attn_window=win)
    monkeypatch.setenv("DISTGPU_ATTN_WINDOW", "2,4,8:0,0,0")
    assert quant.resolve_attn_window(None) == (win, False)
    assert create_diffusion_stack("wan_tiny").attn_window is None
