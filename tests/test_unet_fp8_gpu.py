"""The FP8 kernels for the UNet's Linear widths on the GPU: the padded row
quantiser, ``layer_norm_fp8``, the GEGLU epilogue of the FP8 GEMM and padded
operands through ``Fp8Linear``. References are fp64 on the CPU (fp8_bounds,
kernel_bounds); measured ratios are in profiles/r17_unet_fp8.md."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import fp8_bounds as fb
import kernel_bounds as kb
from comfyui_distributed_amd.models.quant import Fp8GegluLinear, Fp8Linear
from comfyui_distributed_amd.ops import dispatch
from test_module_bounds_gpu import calls  # noqa: F401  (the call counter)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


def _u8(q):
    return q.cpu().view(torch.uint8)


@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("k", [64, 192, 320, 16320])
def test_padded_quantiser(k, m):
    x, _, _ = fb.linear_inputs(m, 8, k, seed=k + m)
    if m > 1:
        x[2] = 0  # an all-zero row: the floor scale, codes 0
    rows = dispatch.quantize_rows(x.to(BF).to(DEV), pad_k=True)
    kp = (k + 127) // 128 * 128
    assert rows.q.shape == (m, kp) and rows.q.dtype == fb.FP8
    assert torch.equal(rows.scale.cpu(), fb.scale_ref(x.abs().amax(dim=1)))
    assert fb.quant_ratio(rows.q[:, :k], x, rows.scale) <= 1.0
    assert not _u8(rows.q)[:, k:].any(), "pad bytes are not zero"
    assert m == 1 or not _u8(rows.q)[2].any()


LN_C = [64, 320, 640, 1280, 1984]
LN_EPS = 1e-5


def _ln_case(c, t):
    x, w, b = kb.norm_inputs(c + t, (t, c), mean=0.5)
    return x, w, b, x.to(BF).to(DEV), w.to(DEV), b.to(DEV)


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("c", LN_C)
def test_layer_norm_fp8(c, t, calls):
    """One launch, bit for bit ``quantize_rows(layer_norm(x), pad_k=True)``
    (7 rows leave the last block of 4 waves partial), and against fp64: with
    y the bf16 LayerNorm, |y - ref| <= lb (kernel_bounds), and q the code of
    v = y / scale, |q - v| <= hs(v) (1 + 2^-20) + 2^-20 |v| (fp8_bounds).
    Against v_ref = ref / scale that is the quantiser bound taken at |v_ref| +
    lb / scale, where hs is no smaller, plus lb / scale."""
    x, w, b, xd, wd, bd = _ln_case(c, t)
    rows = dispatch.layer_norm_fp8(xd, wd, bd, LN_EPS)
    assert dict(calls) == {"layer_norm_fp8": 1}
    pair = dispatch.quantize_rows(dispatch.layer_norm(xd, wd, bd, LN_EPS),
                                  pad_k=True)
    assert rows.q.shape == pair.q.shape == (t, (c + 127) // 128 * 128)
    assert torch.equal(rows.scale, pair.scale)
    assert torch.equal(_u8(rows.q), _u8(pair.q))
    ref, lb = kb.layer_norm_ref(x, w, b, LN_EPS)
    s = rows.scale.cpu().double()[:, None]
    v, slack = ref / s, lb / s
    vmax = v.abs() + slack
    bound = fb.half_step(vmax) * (1 + 2.0 ** -20) + 2.0 ** -20 * vmax + slack
    ratio = ((rows.q[:, :c].cpu().float().double() - v).abs() / bound).max()
    print(f"layer_norm_fp8 C={c} T={t}: max(err/bound) {ratio.item():.3f}")
    assert ratio <= 1.0 and not _u8(rows.q)[:, c:].any()


def test_layer_norm_fp8_graph_replay():
    _, _, _, xd, wd, bd = _ln_case(320, 7)
    eager = dispatch.layer_norm_fp8(xd, wd, bd, LN_EPS)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dispatch.layer_norm_fp8(xd, wd, bd, LN_EPS)  # warm the caches
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            rows = dispatch.layer_norm_fp8(xd, wd, bd, LN_EPS)
    for _ in range(3):
        rows.q.view(torch.uint8).fill_(0xFF)
        rows.scale.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rows.scale, eager.scale)
        assert torch.equal(_u8(rows.q), _u8(eager.q))


def _paired(qw, sw, bias):
    """Unpaired quantised GEGLU operands -> what gemm_geglu_fp8 reads."""
    wp, bp = dispatch.pack_geglu_weight(qw.view(torch.uint8), bias)
    sp, _ = dispatch.pack_geglu_weight(sw[:, None])
    return (wp.view(fb.FP8).to(DEV), sp.reshape(-1).to(DEV),
            bp.to(DEV) if bias is not None else None)


def _geglu_bound(pre, mag, k, inner):
    """(ref, bound) from the fp64 projection [M, 2*inner] and its magnitude:
    one rounding of the product (act_mul_ref) plus each factor's fp32
    accumulation floor (K + 1) 2^-23 mag carried through the other, mag_a
    |gelu(g)| + 1.13 |a| mag_g (1.13 >= |gelu_tanh'|)."""
    a, gate = pre[:, :inner], pre[:, inner:]
    ref, act = kb.act_mul_ref(a, gate, True)
    return ref, act + (k + 1) * 2.0 ** -23 * (
        mag[:, :inner] * F.gelu(gate, approximate="tanh").abs()
        + 1.13 * a.abs() * mag[:, inner:])


@pytest.mark.parametrize("k", [128, 384])
def test_geglu_integer_exact(k):
    """test_gemm_integer_exact's operands: every product is a multiple of
    1/4 and the fp32 sums are exact in any order, so a and g are exact. A k
    slot, a fragment pairing or a value/gate row taken from the wrong place
    moves a or g by at least 1/4, three orders of magnitude past the bound's
    accumulation term, which is kept for the gates whose GELU underflows
    fp32."""
    m, inner = 256, 128
    g = torch.Generator().manual_seed(k)

    def operand(rows):
        vals = torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (rows, k), generator=g)]
        keep = torch.rand(rows, k, generator=g) < 0.25
        half = torch.where(torch.rand(rows, k, generator=g) < 0.5, 0.5, 1.0)
        return vals * keep * half

    a, w = operand(m), operand(2 * inner)
    ref, bound = _geglu_bound(a.double() @ w.double().t(),
                              a.double().abs() @ w.double().abs().t(), k, inner)
    wp, sp, _ = _paired(w.to(fb.FP8), torch.ones(2 * inner), None)
    y = dispatch.gemm_geglu_fp8(a.to(fb.FP8).to(DEV), torch.ones(m, device=DEV),
                                wp, sp)
    assert y.dtype == BF and y.shape == (m, inner)
    kb.check(y, ref, bound, f"geglu fp8 integer K={k}")


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("m,k,inner", [(1, 384, 16), (257, 384, 16),
                                       (300, 640, 144), (513, 1280, 272)])
def test_geglu_gemm_bound(m, k, inner, with_bias):
    """M and N tails, gates past 2*inner masked in a tile, two N-blocks."""
    x, w, bias = fb.linear_inputs(m, 2 * inner, k, seed=m + k + inner)
    bias = bias if with_bias else None
    (qa, sa), (qw, sw) = fb.quant_ref(x), fb.quant_ref(w)
    ref, bound = _geglu_bound(*fb.linear_fp8_pre(qa, sa, qw, sw, bias), k,
                              inner)
    y = dispatch.gemm_geglu_fp8(qa.to(DEV), sa.to(DEV), *_paired(qw, sw, bias))
    assert y.shape == (m, inner)
    kb.check(y, ref, bound, f"geglu fp8 {(m, k, inner)} bias={with_bias}")


@pytest.mark.parametrize("n", [320, 960])
def test_padded_linear(n):
    m, k = 300, 320
    x, w, bias = fb.linear_inputs(m, n, k, seed=n)
    lin = nn.Linear(k, n)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(bias)
    f8 = Fp8Linear(lin, pad_k=True).to(DEV)
    assert f8.pad_k and f8.qweight.shape == (n, 384)
    assert not _u8(f8.qweight)[:, k:].any()
    xd = x.to(BF).to(DEV)
    rows = dispatch.quantize_rows(xd, pad_k=True)
    ref, bound = fb.linear_fp8_bound(rows.q, rows.scale, f8.qweight,
                                     f8.wscale, f8.bias)
    fb.check(f8(xd), ref, bound, f"padded Fp8Linear N={n}")
    fb.check(f8(rows), ref, bound, f"padded Fp8Linear N={n} from rows")
    # the same Linear as a GEGLU projection: the module pairs, pads and routes
    gg = Fp8GegluLinear(lin, pad_k=True).to(DEV)
    pre, mag = fb.linear_fp8_pre(rows.q, rows.scale, f8.qweight, f8.wscale,
                                 f8.bias)
    kb.check(gg(xd), *_geglu_bound(pre, mag, 384, n // 2),
             f"padded Fp8GegluLinear inner={n // 2}")
