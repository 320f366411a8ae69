"""attn_fp8_sparse_kernel on the GPU: exact cases that a visit to a disallowed
tile, or a tile taken by its list position, would spoil; random operands
against fp64 masked attention; the dense kernel on a full list; graph replay."""

import pytest
import torch

import kernel_bounds as kb
from comfyui_distributed_amd.ops import dispatch
from test_attention_sparse_cpu import (MASK_TILES, NK, NQ, allowed_keys,
                                       mask_of, masked_ref_and_bound,
                                       sparse_selection_case)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = dispatch.ATTN_FP8_D
# every mask at B * H = 4, and one at B * H = 8 (the renumbered grid)
CASES = [(2, 2, name) for name in MASK_TILES] + [(4, 2, "band")]


def _dev(*ts):
    return [t.to(torch.bfloat16).to(DEV) for t in ts]


@pytest.mark.parametrize("b,h,name", CASES)
def test_sparse_kernel_selects_exactly(b, h, name):
    """The output is v[pi] bit for bit, unless the kernel visits a tile that
    is not on the list (each q-block has a decoy of one of its selected keys
    there) or takes a K or V^T tile by list position. A K scale taken by
    position goes unseen here (the scales of +-2 keys agree within 2 %); the
    random test below catches that at 2-5 bounds."""
    mask = mask_of(name)
    q, k, v, want = sparse_selection_case(b, h, mask)
    out = dispatch.attention_fp8(*_dev(q, k, v), h,
                                 blocks=dispatch.attn_blocks(mask, DEV))
    assert torch.equal(out.float().cpu(), want)


@pytest.mark.parametrize("b,h,name", CASES)
def test_sparse_kernel_random_within_bound(b, h, name):
    mask = mask_of(name)
    q, k, v = kb.attn_inputs(NQ + NK, b, b, NQ, NK, h * D)
    a = dispatch.quantize_attn_qkv(*_dev(q, k, v), h)
    out = dispatch.attention_fp8(a, blocks=dispatch.attn_blocks(mask, DEV))
    ref, bound = masked_ref_and_bound(a, NK, D ** -0.5, allowed_keys(mask))
    kb.check(out, ref, bound, f"attention_fp8 sparse {name} b={b}")
    if name == "full":   # the same tiles in the same order: the same bits
        assert torch.equal(out, dispatch.attention_fp8(a))


def test_sparse_kernel_under_graph_replay():
    q, k, v = kb.attn_inputs(7, 2, 2, NQ, NK, 2 * D)
    a = dispatch.quantize_attn_qkv(*_dev(q, k, v), 2)
    blocks = dispatch.attn_blocks(mask_of("band"), DEV)
    eager = dispatch.attention_fp8(a, blocks=blocks)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = dispatch.attention_fp8(a, blocks=blocks)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
