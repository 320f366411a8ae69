"""norm_modulate_fp8 (ops/hip/dit_ops.hip) on the GPU: every instantiation
against the fp64 bound of norm_fp8_bounds.py and bit for bit against the two
launches it replaces (norm_modulate, then quant_rows_fp8); edge rows; the
Fp8Rows consumer; graph capture; the WAN block and flux_tiny with the fused
routing on against off.

Measured on MI355X (profiles/r12_norm_fp8.md): max(err/bound) 0.9834-0.9997
over the 36 cases (an e4m3 rounding reaches half a step in any row of a few
hundred values), every case bit-identical to the two launches.
"""

import functools

import pytest
import torch

import fp8_bounds as fb
import kernel_bounds as kb
import norm_fp8_bounds as nb
from comfyui_distributed_amd.models import quant
from comfyui_distributed_amd.ops import dispatch
from comfyui_distributed_amd.ops.dispatch import Fp8Rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn

CASES = [(i, c, mode, modulated) for i, c in enumerate(nb.GPU_C)
         for mode, modulated in nb.MODES]


def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


@functools.lru_cache(maxsize=None)
def _case(i, c, mode, modulated):
    """Inputs, device operands, the fp64 reference and both results, once per
    case; the tests below read them and change nothing."""
    inp = kb.nm_inputs(**nb.gpu_case(i, c, mode))
    x = inp["x"].to(BF).to(DEV)
    w = inp["w"].to(DEV) if inp["w"] is not None else None
    sc = sh = None
    if modulated:
        sc, sh = kb.mod_place(inp["scale"], inp["shift"],
                              ("unbind", "mixed")[i % 2], DEV)
    rows = dispatch.norm_modulate_fp8(x, mode, w, sc, sh)
    y = dispatch.norm_modulate(x, mode, w, sc, sh)
    two = dispatch.quant_rows_fp8(y.reshape(-1, c))
    torch.cuda.synchronize()
    return inp, rows, two, nb.reference(inp, modulated)


@pytest.mark.parametrize("i,c,mode,modulated", CASES)
def test_bound(i, c, mode, modulated):
    inp, rows, _, (h, eh) = _case(i, c, mode, modulated)
    b, n = inp["x"].shape[:2]
    assert isinstance(rows, Fp8Rows) and rows.dtype == BF
    assert rows.q.shape == (b, n, c) and rows.q.dtype == FP8
    assert rows.q.is_contiguous()
    assert rows.scale.shape == (b, n) and rows.scale.dtype == torch.float32
    nb.check(rows.q, rows.scale, h, eh,
             f"norm_modulate_fp8 {mode} mod={modulated} {b, n, c}")


@pytest.mark.parametrize("i,c,mode,modulated", CASES)
def test_bit_identical_to_two_launches(i, c, mode, modulated):
    _, rows, (q2, s2), _ = _case(i, c, mode, modulated)
    assert torch.equal(rows.scale.reshape(-1).cpu(), s2.cpu()), "scale bits"
    diff = (_bytes(rows.q).reshape(-1, c) != _bytes(q2)).sum().item()
    assert diff == 0, f"{diff} of {q2.numel()} bytes differ"


def test_edge_rows():
    c = 640
    # plain rms, rows: zero, +-bf16 max, ordinary
    big = torch.finfo(BF).max
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 3, c, generator=g)
    x[0, 0] = 0
    x[0, 1] = torch.where(torch.rand(c, generator=g) < 0.5, -big, big)
    w = torch.ones(c, device=DEV)
    xd = x.to(BF).to(DEV)
    rows = dispatch.norm_modulate_fp8(xd, "rms", w)
    assert (_bytes(rows.q[0, 0]) == 0).all(), "zero row"
    # 2^-126 * 448 * (1/448), the product the kernel forms
    floor = fb.scale_ref(torch.zeros(1))[0]
    assert 0 < floor.item() <= 2.0 ** -126
    assert torch.equal(rows.scale[0, 0].cpu(), floor), "zero row scale bits"
    assert torch.isfinite(rows.scale).all()
    assert torch.isfinite(rows.q.float()).all()
    q2, s2 = dispatch.quant_rows_fp8(
        dispatch.norm_modulate(xd, "rms", w).reshape(-1, c))
    assert torch.equal(rows.scale.reshape(-1), s2)
    assert torch.equal(_bytes(rows.q).reshape(-1, c), _bytes(q2))

    # layer mode, constant rows: the norm is 0, the shift is what is quantised
    inp = kb.nm_inputs(2, 3, c, "layer", seed=1, const=True)
    sc, sh = kb.mod_place(inp["scale"], inp["shift"], "unbind", DEV)
    rows = dispatch.norm_modulate_fp8(inp["x"].to(BF).to(DEV), "layer", None,
                                      sc, sh)
    q_sh, s_sh = fb.quant_ref(inp["shift"])
    for b in range(2):
        for n in range(3):
            assert torch.equal(rows.scale[b, n].cpu(), s_sh[b])
            assert torch.equal(_bytes(rows.q[b, n]), _bytes(q_sh[b]))


def test_contract_errors():
    x = torch.zeros(1, 2, 64, dtype=BF, device=DEV)
    with pytest.raises(ValueError):
        dispatch.norm_modulate_fp8(x, "layer")
    ext = dispatch.ext.get_ext(True)
    empty = torch.empty(0, dtype=BF, device=DEV)
    for c in (64, 192, 8320):
        with pytest.raises(RuntimeError):
            ext.norm_modulate_fp8(torch.zeros(1, 2, c, dtype=BF, device=DEV),
                                  empty, empty, empty, 1e-5)


def _consumer_case():
    m, n, k = 18, 130, 384                     # the M tail and the N tail
    inp = kb.nm_inputs(2, 9, k, "rms", seed=21)
    _, w, bias = fb.linear_inputs(m, n, k, seed=22)
    qw, sw = dispatch.quantize_weight_fp8(w.to(DEV))
    sc, sh = kb.mod_place(inp["scale"], inp["shift"], "unbind", DEV)
    args = (inp["x"].to(BF).to(DEV), "rms", inp["w"].to(DEV), sc, sh)
    return args, qw, sw, bias.to(DEV)


def test_consumer_bit_identical():
    args, qw, sw, bias = _consumer_case()
    for act in fb.ACTS:
        y_rows = dispatch.linear_fp8(dispatch.norm_modulate_fp8(*args), qw, sw,
                                     bias, act)
        y = dispatch.linear_fp8(dispatch.norm_modulate(*args), qw, sw, bias,
                                act)
        assert y_rows.shape == (2, 9, 130) and y_rows.dtype == BF
        assert torch.equal(y_rows, y), act


def test_under_graph_capture():
    args, qw, sw, bias = _consumer_case()
    eager = dispatch.linear_fp8(dispatch.norm_modulate_fp8(*args), qw, sw,
                                bias, "silu")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = dispatch.linear_fp8(dispatch.norm_modulate_fp8(*args), qw, sw,
                                bias, "silu")
    for i in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager), f"replay {i}"


# ---------------------------------------------------------------------------
# models: fused routing on against off, one process
# ---------------------------------------------------------------------------


def _count(monkeypatch, name):
    calls = []
    real = getattr(dispatch, name)

    def counted(*args, **kwargs):
        calls.append(name)
        return real(*args, **kwargs)

    monkeypatch.setattr(dispatch, name, counted)
    return calls


def test_wan_block_on_off(monkeypatch):
    from comfyui_distributed_amd.models.quant import quantize_linears
    from comfyui_distributed_amd.models.wan import WanBlock, WanConfig, rope_3d

    cfg = WanConfig(dim=128, ffn_dim=256, num_layers=1, num_heads=2,
                    text_dim=128, in_channels=4, out_channels=4)
    torch.manual_seed(0)
    blk = WanBlock(cfg).to(DEV, BF).eval()
    assert quantize_linears(blk) == 10
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 24, 128, generator=g).to(DEV, BF)
    emb6 = (torch.randn(2, 6, 128, generator=g) * 0.1).to(DEV, BF)
    ctx = torch.randn(2, 8, 128, generator=g).to(DEV, BF)
    cs = rope_3d(1, 4, 6, 64, DEV)
    gemms = _count(monkeypatch, "gemm_fp8")
    quants = _count(monkeypatch, "quant_rows_fp8")
    out = {}
    for flag in (True, False):
        monkeypatch.setattr(quant, "FP8_FUSED_NORM", flag)
        del gemms[:], quants[:]
        with torch.no_grad():
            out[flag] = blk(x, emb6, ctx, cs)
        assert len(gemms) == 10
        # q k v cq ffn1 take their rows from the norm kernel
        assert len(quants) == (5 if flag else 10)
    assert torch.isfinite(out[True]).all()
    assert torch.equal(out[True], out[False])


def test_flux_tiny_on_off(monkeypatch):
    from comfyui_distributed_amd.models import create_diffusion_stack

    monkeypatch.delenv("DISTGPU_LINEAR_DTYPE", raising=False)
    stack = create_diffusion_stack("flux_tiny", device=DEV, dtype=BF, seed=5,
                                   linear_dtype="fp8")
    assert stack.fp8_linears == 10
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 16, 16, 16, generator=g).to(DEV, BF)
    t = torch.tensor([500.0], device=DEV, dtype=BF)
    cond = stack.make_conditioning(0)
    gemms = _count(monkeypatch, "gemm_fp8")
    quants = _count(monkeypatch, "quant_rows_fp8")
    out = {}
    for flag in (True, False):
        monkeypatch.setattr(quant, "FP8_FUSED_NORM", flag)
        del gemms[:], quants[:]
        with torch.no_grad():
            out[flag] = stack.model(x, t, cond["context"], cond["vec"])
        assert len(gemms) == stack.fp8_linears
        assert len(quants) == (5 if flag else 10)
    assert torch.isfinite(out[True]).all()
    assert torch.equal(out[True], out[False])
