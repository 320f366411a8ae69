"""conv_dense.hip (dispatch.conv3x3_dense) against an fp64 F.conv2d reference
on the CPU, taken on the bf16-rounded operands:

    t   = conv(x) + bias;  t = lrelu(t);  ref = alpha*t + beta1*res1 + res2

Bound, the conv/GEMM form of kernel_bounds.py with the epilogue's terms:

    |err| <= 2u*|ref| + n * 2^-23 * mag,    n = 9*C_in + 4,
    mag = |alpha| * (|x| (*) |w| + |bias|) + |beta1*res1| + |res2|

(the fp32 chain of 9*C_in products and the bias, then the three epilogue
operations; LeakyReLU only shrinks |t|). x and out are channel slices of one
192-wide buffer wherever C_in + K_out <= 192 (else out sits in a second one):
the channels past C_in hold NaN, so a read outside x poisons the result, and
everything outside out must come back bit for bit.
"""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import kernel_bounds as kb
from comfyui_distributed_amd.ops import dispatch

pytestmark = pytest.mark.gpu

WIDE = 192
SENTINEL = 7.0
# one chunk / odd chunk counts for the staging / every NF / a masked N
CK = [(32, 32), (96, 32), (160, 32), (192, 64), (64, 3)]
# below one tile / not multiples of the 8 x 32 tile, two images
BHW = [(1, 1, 1), (2, 9, 35), (2, 17, 33)]
CASES = [dict(c=c, k=k, bhw=bhw) for c, k in CK for bhw in BHW] + [
    dict(c=96, k=32, bhw=(2, 9, 35), lrelu=0.2),
    dict(c=192, k=64, bhw=(2, 9, 35), alpha=0.04, beta1=0.2, res=True),
    dict(c=64, k=3, bhw=(2, 9, 35), alpha=0.2, beta1=-1.5, res=True),
    dict(c=64, k=64, bhw=(2, 5, 7), lrelu=0.2, up2=True),
    dict(c=64, k=32, bhw=(2, 9, 35), bias=False),
]


def _f32(v: float) -> float:
    """The value the kernel receives for a scalar argument."""
    return torch.tensor(v, dtype=torch.float32).item()


def _reference(x, w, bias, lrelu, alpha, res1, beta1, res2, up2):
    """fp64 (ref, bound), NHWC, of bf16-exact fp32 CPU operands."""
    xd = x.double().permute(0, 3, 1, 2)
    if up2:
        xd = F.interpolate(xd, scale_factor=2, mode="nearest")
    bd = None if bias is None else bias.double()
    t = F.conv2d(xd, w.double(), bd, padding=1)
    mag = F.conv2d(xd.abs(), w.double().abs(),
                   None if bd is None else bd.abs(), padding=1)
    if lrelu is not None:
        t = torch.where(t > 0, t, _f32(lrelu) * t)
    ref = (_f32(alpha) * t).permute(0, 2, 3, 1)
    mag = (abs(alpha) * mag).permute(0, 2, 3, 1)
    if res1 is not None:
        ref = ref + _f32(beta1) * res1.double()
        mag = mag + abs(beta1) * res1.double().abs()
    if res2 is not None:
        ref = ref + res2.double()
        mag = mag + res2.double().abs()
    n = 9 * x.shape[3] + 4
    return ref, 2 * kb.U * ref.abs() + n * 2.0 ** -23 * mag


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("case", CASES, ids=lambda d: "-".join(
    f"{k}{v}" for k, v in d.items()).replace(" ", ""))
def test_conv_dense_bound(case):
    c, k, (b, h, w) = case["c"], case["k"], case["bhw"]
    up2, lrelu = case.get("up2", False), case.get("lrelu")
    alpha, beta1 = case.get("alpha", 1.0), case.get("beta1", 1.0)
    ho, wo = (2 * h, 2 * w) if up2 else (h, w)
    g = torch.Generator().manual_seed(c * 1000 + k + h)
    x = kb.bf16_exact(torch.randn(b, h, w, c, generator=g) / 4)
    wk = kb.bf16_exact(torch.randn(k, c, 3, 3, generator=g) / 8)
    bias = (kb.bf16_exact(torch.randn(k, generator=g))
            if case.get("bias", True) else None)
    res1 = res2 = None
    if case.get("res"):
        res1 = kb.bf16_exact(torch.randn(b, ho, wo, k, generator=g))
        res2 = kb.bf16_exact(torch.randn(b, ho, wo, k, generator=g))

    conv = nn.Conv2d(c, k, 3, 1, 1, bias=bias is not None)
    with torch.no_grad():
        conv.weight.copy_(wk)
        if bias is not None:
            conv.bias.copy_(bias)
    conv = conv.cuda().to(kb.BF)

    xbuf = torch.full((b, h, w, WIDE), float("nan"), dtype=kb.BF, device="cuda")
    xbuf[..., :c] = x.to(kb.BF).cuda()
    xv = xbuf[..., :c]
    if c + k <= WIDE and not up2:
        obuf, o0 = xbuf, c
    else:
        obuf = torch.full((b, ho, wo, WIDE), SENTINEL, dtype=kb.BF,
                          device="cuda")
        o0 = WIDE - 64
    out = obuf[..., o0:o0 + k]
    kw = {}
    if res1 is not None:      # res1 a slice of its own buffer, out aliases res2
        r1buf = torch.full((b, ho, wo, WIDE), float("nan"), dtype=kb.BF,
                           device="cuda")
        r1buf[..., 32:32 + k] = res1.to(kb.BF).cuda()
        out.copy_(res2.to(kb.BF))
        kw = dict(res1=r1buf[..., 32:32 + k], res2=out)
    before = _bits(obuf).clone()
    x_before = _bits(xbuf).clone()

    got = dispatch.conv3x3_dense(xv, conv, out, lrelu=lrelu, alpha=alpha,
                                 beta1=beta1, up2=up2, **kw)
    torch.cuda.synchronize()
    assert got is out

    ref, bound = _reference(x, wk, bias, lrelu, alpha, res1, beta1, res2, up2)
    kb.check(out, ref, bound, f"conv_dense {case}")
    after = _bits(obuf)
    keep = torch.ones(WIDE, dtype=torch.bool, device="cuda")
    keep[o0:o0 + k] = False
    assert torch.equal(after[..., keep], before[..., keep]), \
        "a channel outside out was written"
    if obuf is not xbuf:
        assert torch.equal(_bits(xbuf), x_before)


def test_conv_dense_above_2gib():
    """x [1, 4100, 4096, 64] is 2.15 GB: the last four rows start 2^31 bytes
    in. Reference on those rows (computed from five, the first one's output
    dropped: it would see a zero row where the image continues)."""
    h, w, c, k, tail = 4100, 4096, 64, 3, 4
    torch.manual_seed(11)
    conv = nn.Conv2d(c, k, 3, 1, 1)
    with torch.no_grad():
        conv.weight.copy_(kb.bf16_exact(conv.weight))
        conv.bias.copy_(kb.bf16_exact(conv.bias))
    x = torch.empty(1, h, w, c, dtype=kb.BF, device="cuda").normal_(0, 0.25)
    assert x.numel() * 2 > 2 ** 31 and (h - tail) * w * c * 2 >= 2 ** 31
    out = torch.full((1, h, w, 8), SENTINEL, dtype=kb.BF, device="cuda")
    dispatch.conv3x3_dense(x, conv.cuda().to(kb.BF), out[..., :k])
    torch.cuda.synchronize()
    ref, bound = _reference(x[:, -tail - 1:].float().cpu(),
                            conv.weight.detach().float().cpu(),
                            conv.bias.detach().float().cpu(), None, 1.0, None,
                            1.0, None, False)
    kb.check(out[:, -tail:, :, :k], ref[:, 1:], bound[:, 1:],
             "conv_dense rows past 2 GiB")
    assert (out[:, -tail:, :, k:] == SENTINEL).all()
    # and the far end of the grid did not leave the first rows unwritten
    assert torch.isfinite(out[:, :8, :, :k].float()).all()
    assert (out[:, :8, :, :k] != SENTINEL).any()


@pytest.mark.parametrize("what", ["overlap", "c_in", "k_out"])
def test_conv_dense_contract_errors(what):
    cin, k = {"overlap": (64, 32), "c_in": (48, 32), "k_out": (64, 80)}[what]
    conv = nn.Conv2d(cin, k, 3, 1, 1).cuda().to(kb.BF)
    buf = torch.zeros(1, 4, 4, 256, dtype=kb.BF, device="cuda")
    o0 = 48 if what == "overlap" else 128     # [48, 80) meets x's [0, 64)
    with pytest.raises(ValueError):
        dispatch.conv3x3_dense(buf[..., :cin], conv, buf[..., o0:o0 + k])
