"""FP8 Linear kernels (ops/hip/gemm_fp8.hip) on the GPU, against the fp64
references and bounds of fp8_bounds.py.

The quantiser is checked for its encoding (every finite e4m3 value, bit for
bit against torch's cast), its scale (bit for bit) and its rounding (half an
e4m3 step). The GEMM is checked with exact small-integer data at zero
tolerance (fragment layout, k map, transpose) and with pre-quantised random
operands against the project's dot-product bound, so a GEMM failure cannot
hide behind the quantiser or the other way round.
"""

import functools

import pytest
import torch

import fp8_bounds as fb
from comfyui_distributed_amd.ops import dispatch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn


def _bytes(t):
    return t.detach().cpu().view(torch.uint8)


# ---------------------------------------------------------------------------
# quantiser
# ---------------------------------------------------------------------------


def test_quantiser_encoding_every_e4m3_value():
    """A K = 256 row holding all 254 finite e4m3 values and two zeros (in
    place of the two NaN codes): amax = 448, so the scale is exactly 1 and
    the output bytes must be torch's cast of the row. Rows 1 and 2 are the
    same row times 1/4 and 4 (exact in bf16): same bytes, scale 1/4 and 4.
    An fnuz encoding, a wrong bias or a saturation mistake changes bytes."""
    codes = torch.arange(256, dtype=torch.uint8)
    row = codes.view(FP8).float()
    assert torch.isnan(row).sum() == 2
    row = torch.nan_to_num(row, nan=0.0)
    row = row[torch.randperm(256, generator=torch.Generator().manual_seed(0))]
    x = torch.stack([row, row * 0.25, row * 4.0])
    assert torch.equal(x.to(BF).float(), x)
    q, scale = dispatch.quant_rows_fp8(x.to(BF).to(DEV))
    assert q.dtype == FP8 and scale.dtype == torch.float32
    want_scale = fb.scale_ref(x.abs().amax(dim=1))
    assert want_scale.tolist() == [1.0, 0.25, 4.0]
    assert torch.equal(scale.cpu(), want_scale)
    want = _bytes(row.to(FP8))
    for r in range(3):
        assert torch.equal(_bytes(q[r]), want), f"row {r}"
    assert torch.equal(_bytes(q), _bytes(fb.quant_ref(x)[0]))


def _quant_case(m, k, seed):
    """Rows spanning 1e-2 .. 10 in magnitude. Row 0's absmax is negative and
    sits in the last 8 elements, the chunk of the highest active lane; the
    last row (M >= 2) is all zero."""
    x, _, _ = fb.linear_inputs(m, 8, k, seed)
    x[0, k - 3] = -(x[0].abs().max() * 2).bfloat16().float()
    if m >= 2:
        x[m - 1] = 0
    return x


@pytest.mark.parametrize("m,k", [(5, 128), (3, 5120), (2, 13824), (1, 16384),
                                 (70, 384)])
def test_quantiser_scale_and_bound(m, k):
    x = _quant_case(m, k, seed=k + m)
    q, scale = dispatch.quant_rows_fp8(x.to(BF).to(DEV))
    assert q.shape == (m, k) and scale.shape == (m,)
    amax = x.abs().amax(dim=1)
    assert amax[0] == -x[0, k - 3]
    assert torch.equal(scale.cpu(), fb.scale_ref(amax)), "scale bits"
    r = fb.quant_ratio(q, x, scale)
    print(f"quant_rows_fp8 {m, k}: max(err/bound) {r:.5f}")
    assert r <= 1.0
    if m >= 2:
        assert (_bytes(q[m - 1]) == 0).all(), "zero row"
        assert scale[m - 1].item() > 0


# ---------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------


def _ones(n):
    return torch.ones(n, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("k", [128, 384])
def test_gemm_integer_exact(k):
    """Operands from {-1, 0, 1, 2} x {1, 0.5}, sparse and seeded so that
    every row, column and k position differs; all scales 1. Every product
    is a multiple of 1/4 and every partial sum stays far below 2^24, so the
    fp32 accumulation is exact in any order, and |result| < 64 keeps the
    multiples of 1/4 exact in bf16: the output must EQUAL the matmul. A
    lane's k slots, the A/B fragment pairing and the transposed store are
    all in this one equality."""
    m = n = 256
    g = torch.Generator().manual_seed(k)

    def operand(rows):
        vals = torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (rows, k), generator=g)]
        keep = torch.rand(rows, k, generator=g) < 0.25
        half = torch.where(torch.rand(rows, k, generator=g) < 0.5, 0.5, 1.0)
        return vals * keep * half

    a, w = operand(m), operand(n)
    ref = a.double() @ w.double().t()
    assert ref.abs().max() < 64
    assert torch.equal(ref.to(BF).double(), ref)
    assert not torch.equal(ref, ref.t())
    y = dispatch.gemm_fp8(a.to(FP8).to(DEV), _ones(m), w.to(FP8).to(DEV),
                          _ones(n))
    assert y.dtype == BF and y.shape == (m, n)
    bad = (y.cpu().double() != ref).sum().item()
    assert bad == 0, f"{bad} of {m * n} elements differ from the exact matmul"


GEMM_SHAPES = [(256, 256, 128), (300, 77, 128), (1, 128, 256),
               (257, 264, 384), (513, 520, 1280), (256, 256, 13824)]


@functools.lru_cache(maxsize=None)
def _gemm_case(m, n, k):
    """Operands pre-quantised by the torch reference; device copies; the
    fp64 pre-activation reference and magnitude with and without bias."""
    x, w, bias = fb.linear_inputs(m, n, k, seed=m + n + k)
    qa, sa = fb.quant_ref(x)
    qw, sw = fb.quant_ref(w)
    dev = tuple(t.to(DEV) for t in (qa, sa, qw, sw, bias))
    pre = {False: fb.linear_fp8_pre(qa, sa, qw, sw),
           True: fb.linear_fp8_pre(qa, sa, qw, sw, bias)}
    return dev, pre


@pytest.mark.parametrize("act", fb.ACTS)
@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_bound(m, n, k, act):
    (qa, sa, qw, sw, bias), pre = _gemm_case(m, n, k)
    for with_bias in (False, True):
        y = dispatch.gemm_fp8(qa, sa, qw, sw, bias if with_bias else None, act)
        assert y.dtype == BF and y.shape == (m, n)
        ref = fb._act(pre[with_bias][0], act)
        bound = fb.bound_from(ref, pre[with_bias][1], k, act)
        fb.check(y, ref, bound,
                 f"gemm_fp8 {m, n, k} act={act} bias={with_bias}")


def test_linear_fp8_end_to_end():
    """GPU quantiser + GEMM through dispatch.linear_fp8, against the fp64
    reference built from the kernel's own q and scale."""
    m, n, k = 300, 130, 384
    x, w, bias = fb.linear_inputs(m, n, k, seed=11)
    qw, sw = dispatch.quantize_weight_fp8(w.to(DEV))
    xd = x.to(BF).to(DEV)
    qa, sa = dispatch.quant_rows_fp8(xd)
    assert fb.quant_ratio(qa, x, sa) <= 1.0
    ref, bound = fb.linear_fp8_bound(qa, sa, qw, sw, bias, "silu")
    y = dispatch.linear_fp8(xd.reshape(3, 100, k), qw, sw, bias.to(DEV), "silu")
    assert y.shape == (3, 100, n) and y.dtype == BF
    fb.check(y.reshape(m, n), ref, bound, "linear_fp8 end to end")
    with pytest.raises(ValueError):
        dispatch.linear_fp8(xd.float(), qw, sw)          # fp32 input on GPU
    with pytest.raises(ValueError):
        dispatch.linear_fp8(xd[:, :64], qw[:, :64].contiguous(), sw)


def test_linear_fp8_under_graph_capture():
    """Both launches captured on one stream and replayed twice: current-stream
    launches, torch's allocator, no sync, so capture is legal and the replays
    are bit-identical to the eager call."""
    m, n, k = 300, 130, 384
    x, w, bias = fb.linear_inputs(m, n, k, seed=12)
    qw, sw = dispatch.quantize_weight_fp8(w.to(DEV))
    xd, bd = x.to(BF).to(DEV), bias.to(DEV)
    eager = dispatch.linear_fp8(xd, qw, sw, bd, "gelu_tanh")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = dispatch.linear_fp8(xd, qw, sw, bd, "gelu_tanh")
    for i in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager), f"replay {i}"


# ---------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------

# Relative Frobenius distance between the fp8 and the bf16 model output on the
# same seeded inputs, measured on MI355X (profiles/r08_fp8_linear.md). The
# inputs are seeded, so only accumulation order moves it; the tests assert at
# twice the measured value. They only have to catch a broken layer (distance
# of order 1), not grade fp8.
MEASURED_REL = {"wan_block": 0.00744, "flux_tiny": 0.00484}


def _count_gemm_calls(monkeypatch):
    calls = []
    real = dispatch.gemm_fp8

    def counted(qa, *args, **kwargs):
        assert qa.is_cuda and qa.dtype == FP8
        calls.append(tuple(qa.shape))
        return real(qa, *args, **kwargs)

    monkeypatch.setattr(dispatch, "gemm_fp8", counted)
    return calls


def _rel(y, ref):
    y, ref = y.float(), ref.float()
    return ((y - ref).norm() / ref.norm()).item()


def test_wan_block_fp8(monkeypatch):
    from comfyui_distributed_amd.models.quant import quantize_linears
    from comfyui_distributed_amd.models.wan import WanBlock, WanConfig, rope_3d

    cfg = WanConfig(dim=128, ffn_dim=256, num_layers=1, num_heads=2,
                    text_dim=128, in_channels=4, out_channels=4)
    torch.manual_seed(0)
    ref_blk = WanBlock(cfg).to(DEV, BF).eval()
    blk = WanBlock(cfg).to(DEV, BF).eval()
    blk.load_state_dict(ref_blk.state_dict())
    eligible = quantize_linears(blk)
    assert eligible == 10
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 24, 128, generator=g).to(DEV, BF)
    emb6 = (torch.randn(2, 6, 128, generator=g) * 0.1).to(DEV, BF)
    ctx = torch.randn(2, 8, 128, generator=g).to(DEV, BF)
    cs = rope_3d(1, 4, 6, 64, DEV)
    calls = _count_gemm_calls(monkeypatch)
    with torch.no_grad():
        y = blk(x, emb6, ctx, cs)
        assert len(calls) == eligible
        y_ref = ref_blk(x, emb6, ctx, cs)
    assert len(calls) == eligible            # the bf16 block calls none
    assert y.shape == x.shape and y.dtype == BF and torch.isfinite(y).all()
    rel = _rel(y, y_ref)
    print(f"WAN block fp8 vs bf16: relative Frobenius distance {rel:.5f}")
    assert rel <= 2 * MEASURED_REL["wan_block"]


def test_flux_tiny_fp8(monkeypatch):
    from comfyui_distributed_amd.models import create_diffusion_stack

    monkeypatch.delenv("DISTGPU_LINEAR_DTYPE", raising=False)
    base = create_diffusion_stack("flux_tiny", device=DEV, dtype=BF, seed=5)
    stack = create_diffusion_stack("flux_tiny", device=DEV, dtype=BF, seed=5,
                                   linear_dtype="fp8")
    assert stack.fp8_linears == 10 and base.fp8_linears == 0
    assert stack.parameters_bytes() < base.parameters_bytes()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 16, 16, 16, generator=g).to(DEV, BF)
    t = torch.tensor([500.0], device=DEV, dtype=BF)
    cond = base.make_conditioning(0)
    calls = _count_gemm_calls(monkeypatch)
    with torch.no_grad():
        y = stack.model(x, t, cond["context"], cond["vec"])
        assert len(calls) == stack.fp8_linears
        y_ref = base.model(x, t, cond["context"], cond["vec"])
    assert len(calls) == stack.fp8_linears
    assert y.shape == x.shape and y.dtype == BF and torch.isfinite(y).all()
    rel = _rel(y, y_ref)
    print(f"flux_tiny fp8 vs bf16: relative Frobenius distance {rel:.5f}")
    assert rel <= 2 * MEASURED_REL["flux_tiny"]
