"""MXFP8 activation rows on the CPU: the torch definition of the format
against the rule written out in fp64, linear_fp8 with MxRows in and out, and
the quantize_linears routing under DISTGPU_FP8_MX."""

import pytest
import torch

import fp8_bounds as fb
import mxfp8_cases as mc
from comfyui_distributed_amd.models import quant
from comfyui_distributed_amd.ops import dispatch


@pytest.mark.parametrize("m,k", [(4, 128), (5, 384)])
def test_format_definition_on_edge_blocks(m, k):
    x = mc.rows(m, k, seed=m)
    q, e = dispatch.quant_rows_mxfp8(x)
    q_ref, e_ref, v = mc.quant_ref64(x)
    assert q.dtype == mc.FP8 and e.dtype == torch.uint8
    assert e.shape == (m, k // 32) and torch.equal(e, e_ref)
    assert mc.same_bytes(q, q_ref)
    # the exponent is large enough that nothing is clipped, and the smallest
    # such: one less would clip the block's absmax (unless clamped at -127)
    amax = v.abs().reshape(m, k // 32, 32).amax(-1)
    assert (amax <= 448).all()
    assert ((amax > 224) | (e == 0)).all()


@pytest.mark.parametrize("act", fb.ACTS)
def test_linear_fp8_mx_rows_in_and_out(act):
    m, n, k = 37, 128, 256
    x, w, bias = fb.linear_inputs(m, n, k, seed=5)
    qw, sw = dispatch.quantize_weight_fp8(w)
    rows = dispatch.quantize_rows_mx(x.reshape(1, m, k))
    assert isinstance(rows, dispatch.MxRows) and rows.e.shape == (1, m, k // 32)
    ones = torch.ones(m)
    ref, bound = fb.linear_fp8_bound(
        dispatch.mx_dequant(rows.q[0], rows.e[0]), ones, qw, sw, bias, act)
    y = dispatch.linear_fp8(rows, qw, sw, bias, act)
    assert y.shape == (1, m, n) and y.dtype == x.dtype
    fb.check(y[0], ref, bound, f"MxRows in, act={act}")
    # a tensor in place of the rows is quantised to the same rows
    out = dispatch.linear_fp8(x.reshape(1, m, k), qw, sw, bias, act, emit="mx")
    assert isinstance(out, dispatch.MxRows) and out.dtype == x.dtype
    q_ref, e_ref = dispatch.quant_rows_mxfp8(y[0].bfloat16())
    assert mc.same_bytes(out.q[0], q_ref) and torch.equal(out.e[0], e_ref)
    with pytest.raises(ValueError):
        dispatch.linear_fp8(dispatch.quantize_rows(x), qw, sw, emit="mx")


def _rel(y, ref):
    return ((y - ref).norm() / ref.norm()).item()


def _wan_block():
    from comfyui_distributed_amd.models.wan import WanBlock, WanConfig, rope_3d

    cfg = WanConfig(dim=128, ffn_dim=256, num_layers=1, num_heads=2,
                    text_dim=128, in_channels=4, out_channels=4)
    torch.manual_seed(0)
    args = (torch.randn(2, 12, 128), torch.randn(2, 6, 128) * 0.1,
            torch.randn(2, 5, 128), rope_3d(1, 3, 4, 64, "cpu"))
    return (lambda: WanBlock(cfg).eval()), args, (("ffn1", "ffn2"),)


def _flux_block():
    from comfyui_distributed_amd.models import create_diffusion_stack

    base = create_diffusion_stack("flux_tiny", seed=3)
    cond = base.make_conditioning(0)
    torch.manual_seed(1)
    args = (torch.randn(1, 16, 8, 8), torch.tensor([500.0]), cond["context"],
            cond["vec"])
    return (lambda: create_diffusion_stack("flux_tiny", seed=3).model), args, (
        ("double_blocks.0.img_mlp.0", "double_blocks.0.img_mlp.2"),
        ("double_blocks.0.txt_mlp.0", "double_blocks.0.txt_mlp.2"))


@pytest.mark.parametrize("case", [_wan_block, _flux_block])
def test_quantize_linears_mx_pairs(case, monkeypatch):
    make, args, pairs = case()
    torch.manual_seed(2)
    ref, row, mx = make(), make(), make()
    row.load_state_dict(ref.state_dict())
    mx.load_state_dict(ref.state_dict())
    monkeypatch.setattr(quant, "FP8_MX", False)
    n_row = quant.quantize_linears(row)
    monkeypatch.setattr(quant, "FP8_MX", True)
    assert quant.quantize_linears(mx) == n_row
    for a, b in pairs:
        assert quant._get(row, a).emit is None
        assert quant._get(mx, a).emit == "mx" and quant._get(mx, b).emit is None
    with torch.no_grad():
        y_ref, y_row, y_mx = ref(*args), row(*args), mx(*args)
    e_row, e_mx = _rel(y_row, y_ref), _rel(y_mx, y_ref)
    print(f"{case.__name__}: per-row {e_row:.5f}  mx {e_mx:.5f}")
    # Measured relative Frobenius errors against the fp32 block:
    #   WAN block   per-row 0.00888  mx 0.00891   (ratio 1.003)
    #   flux_tiny   per-row 0.00216  mx 0.00217   (ratio 1.005)
    # The margin is derived, not fitted. The routes differ in the input format
    # of the feed-forward pair only (2 of the 10 Linears). A block's scale is
    # at most the row's scale rounded up to a power of two, so the e4m3 step
    # of those inputs grows by a factor below 2 in the worst case: their error
    # variance by below 4. With 10 comparable error terms that is
    # sqrt((10 + 2 * 3) / 10) = 1.26 on the block's error. A scale applied to
    # the wrong block or row moves the output by order 1, far outside it.
    assert e_mx <= 1.26 * e_row
