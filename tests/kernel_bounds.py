"""References, per-element error bounds and input recipes for the kernel tests.

Plain torch on the CPU; imported by the GPU tests (test_ops_gpu.py,
test_conv_gpu.py, test_attention_loop_gpu.py, test_dit_ops_gpu.py) and by
test_kernel_bounds_cpu.py, which shows without a GPU that a faithful
emulation of each kernel stays inside its bound and that seeded defects
leave it.

Every reference is computed in float64 from the exact bf16-rounded values the
kernel receives. ``U = 2^-8`` is the bf16 unit roundoff (one ulp relative; a
round-to-nearest store costs at most half of it). Bounds, per element:

rounding-only ops (group_norm*, layer_norm, act_mul)
    |err| <= 2U*|ref| + 2^-16 * mag
    norms: mag = |xhat|*|w| + |b|, which keeps a floor under elements where
    xhat*w + b cancels; act_mul: mag = |ref|. With SiLU fused the same bound
    is taken on the output (|silu'| <= 1.1).

dot-product ops (conv_nhwc, conv256_nhwc, conv_smallc, gemm256_bf16)
    |err| <= 2U*|ref| + n * 2^-23 * mag,   n = RS*C + 1,
    mag = |x| (*) |w| + |bias|  (+ |residual|)
    the textbook worst-case bound of an fp32 accumulation chain of length n;
    x1.1 on the second term with SiLU fused.

attention
    |err| <= U*(|ref| + P@|V|) + (Nk + D + 16) * 2^-23 * (P@|V|)
    P = softmax(scale * Q K^T) in fp64. First term: the kernel's two
    roundings, P to bf16 before PV (each p_j*v_j off by at most U/2 relative,
    so at most (U/2) * P@|V|) and the output store ((U/2)*|ref|), doubled.
    The row sum is taken over unrounded p, so the normalisation adds nothing.
    Second term: the fp32 chains (QK^T over D, row sum and PV over Nk).

DiT glue ops (qk_norm_rope, norm_modulate, gated_residual of dit_ops.hip)
    |err| <= hulp(ref) + 2^-16 * mag  (+ mean term, LayerNorm mode only)
    hulp(r) = 2^(floor(log2|r|) - 8), half a bf16 ulp at r (|r| clamped
    below at 2^-126). These kernels keep everything in fp32 and round once,
    on the store, so the first term is the exact error of rounding the
    reference itself; 2U*|ref| would be four times that and would pass a
    kernel that rounds twice (the eager chains they replaced do). The second
    term is the same fp32 floor as for the rounding-only ops, on the terms of
    the last fp32 expression:
      qk_norm_rope    even channel |y0*c| + |y1*s|, odd |y0*s| + |y1*c|,
                      y = x * rstd * w
      norm_modulate   |norm| * |1 + scale| + |shift|  (|norm| unmodulated)
      gated_residual  |x| + |gate * y|
    A few fp32 roundings of those terms are 2^-24 each, so 2^-16 leaves two
    orders of magnitude and still sits 2^-7 below hulp wherever nothing
    cancels. LayerNorm mode adds
      n * 2^-24 * mean|x| * rstd * |1 + scale|,   n = 8 * ceil(C/512) + 6,
    for the fp32 mean: every partial sum of the row is at most sum|x|, the
    longest chain of additions into one lane's total is 8 per 512-channel
    chunk and then the 6 shuffle levels, so the mean is off by at most
    n * 2^-24 * mean|x|, and that error reaches every element of the row
    times rstd * |1 + scale|. It scales with |mean|, not with mag: at
    mean/std = 128 the elements near the mean have mag ~ 0, and without
    the term a faithful fp32 evaluation leaves the bound there
    (test_layer_bound_needs_its_mean_term: 1.5 at C = 512 .. 3072).

``check`` prints and returns max(err / bound) and asserts that no element
exceeds its bound; ``err_ratio`` only measures.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

U = 2.0 ** -8
BF = torch.bfloat16


def bf16_exact(x: torch.Tensor) -> torch.Tensor:
    """fp32 tensor holding exactly the values a bf16 kernel input has."""
    return x.to(BF).float()


# ---------------------------------------------------------------------------
# the comparison itself
# ---------------------------------------------------------------------------


def err_ratio(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max(err / bound); an element with err == bound == 0 counts as 0."""
    out = out.detach().double().cpu()
    assert out.shape == ref.shape, (tuple(out.shape), tuple(ref.shape))
    if not torch.isfinite(out).all():
        return math.inf
    err = (out - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err),
                        err / bound.clamp_min(1e-300))
    return ratio.max().item() if ratio.numel() else 0.0


def check(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor,
          what: str) -> float:
    r = err_ratio(out, ref, bound)
    err = (out.detach().double().cpu() - ref).abs().max().item() \
        if ref.numel() else 0.0
    print(f"{what}: max err {err:.3e}  max|ref| {ref.abs().max().item():.3e}  "
          f"max(err/bound) {r:.3f}")
    assert r <= 1.0, f"{what}: err/bound {r:.3f} > 1"
    return r


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------


def split_heads(u: torch.Tensor, heads: int) -> torch.Tensor:
    """[B, N, H*D] -> [B*H, N, D]"""
    b, n, hd = u.shape
    d = hd // heads
    return u.reshape(b, n, heads, d).permute(0, 2, 1, 3).reshape(b * heads, n, d)


def merge_heads(o: torch.Tensor, heads: int) -> torch.Tensor:
    """[B*H, N, D] -> [B, N, H*D]"""
    bh, n, d = o.shape
    b = bh // heads
    return o.reshape(b, heads, n, d).permute(0, 2, 1, 3).reshape(b, n, heads * d)


def attention_ref(q, k, v, heads: int = 1, kv_heads: int | None = None,
                  scale: float | None = None):
    """q [B*H, Nq, D], k/v [B*Hkv, Nk, D] -> (ref, bound), fp64 [B*H, Nq, D].
    Query head h reads kv head h // (H / Hkv)."""
    kv_heads = kv_heads or heads
    d, nk = q.shape[-1], k.shape[1]
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    qd, kd, vd = q.double(), k.double(), v.double()
    if kv_heads != heads:
        rep = heads // kv_heads
        b = q.shape[0] // heads
        kd = kd.reshape(b, kv_heads, 1, nk, d).expand(-1, -1, rep, -1, -1) \
            .reshape(b * heads, nk, d)
        vd = vd.reshape(b, kv_heads, 1, nk, d).expand(-1, -1, rep, -1, -1) \
            .reshape(b * heads, nk, d)
    p = torch.softmax(torch.bmm(qd, kd.transpose(1, 2)) * scale, dim=-1)
    ref = torch.bmm(p, vd)
    pav = torch.bmm(p, vd.abs())
    bound = U * (ref.abs() + pav) + (nk + d + 16) * 2.0 ** -23 * pav
    return ref, bound


def attention_packed_ref(q, k, v, heads: int, kv_heads: int | None = None,
                         scale: float | None = None):
    """q [B, Nq, H*D], k/v [B, Nk, Hkv*D] -> (ref, bound) [B, Nq, H*D]."""
    kv_heads = kv_heads or heads
    ref, bound = attention_ref(split_heads(q, heads), split_heads(k, kv_heads),
                               split_heads(v, kv_heads), heads, kv_heads, scale)
    return merge_heads(ref, heads), merge_heads(bound, heads)


def attention_qkv_ref(qkv, heads: int):
    q, k, v = qkv.split(qkv.shape[-1] // 3, dim=-1)
    return attention_packed_ref(q, k, v, heads)


def attention_q_kv_ref(q, kv, heads: int):
    k, v = kv.split(q.shape[-1], dim=-1)
    return attention_packed_ref(q, k, v, heads)


def attn_inputs(seed: int, bq: int, bkv: int, nq: int, nk: int, d: int,
                qk_std: float = 1.0):
    """q [bq, nq, d], k/v [bkv, nk, d] as bf16-exact fp32. qk_std 1 gives
    logits of std ~1 at the default scale, so single keys carry weight."""
    g = torch.Generator().manual_seed(seed)
    q = bf16_exact(torch.randn(bq, nq, d, generator=g) * qk_std)
    k = bf16_exact(torch.randn(bkv, nk, d, generator=g) * qk_std)
    v = bf16_exact(torch.randn(bkv, nk, d, generator=g))
    return q, k, v


ATTN_H = 3          # heads of the packed cases below
ATTN_B = 2
# head dims no other test runs: partial fill inside each pad class
# (48: 8/16/24, 64: 56, 96: 72/88, 128: 104/120, 160: 136/152) and the
# exact class sizes 48 and 96
ATTN_NEW_D = [8, 16, 24, 48, 56, 72, 88, 96, 104, 120, 136, 152]
# q-row counts around the 16-row fragment and the 128-row block
ATTN_NEW_NQ = [1, 15, 16, 17, 127, 128, 129]
# scale = mult / sqrt(D) with q, k ~ N(0, 1/mult): the logits keep std ~1, so
# a kernel that ignored the argument would be off by a factor of 1/mult in them
ATTN_SCALE_MULT = [0.5, 2.0]
ATTN_GQA = dict(b=1, h=8, hkv=2, n=300, d=64)


def attn_new_cases():
    """(name, attn_inputs kwargs, attention kwargs) of the cases added with
    the bound: H=3 heads, nq=40, nk=77 unless the case is about that size."""
    h, b = ATTN_H, ATTN_B
    cases = []
    for d in ATTN_NEW_D:
        cases.append((f"D{d}", dict(seed=d, bq=b * h, bkv=b * h, nq=40, nk=77,
                                    d=d), dict(heads=h)))
    for nq in ATTN_NEW_NQ:
        cases.append((f"nq{nq}", dict(seed=500 + nq, bq=b * h, bkv=b * h,
                                      nq=nq, nk=65, d=40), dict(heads=h)))
    for i, mult in enumerate(ATTN_SCALE_MULT):
        cases.append((f"scale{mult}", dict(seed=70 + i, bq=b * h, bkv=b * h,
                                           nq=40, nk=77, d=40,
                                           qk_std=mult ** -0.5),
                      dict(heads=h, scale=mult / math.sqrt(40))))
    g = ATTN_GQA
    cases.append(("gqa", dict(seed=8, bq=g["b"] * g["h"], bkv=g["b"] * g["hkv"],
                              nq=g["n"], nk=g["n"], d=g["d"]),
                  dict(heads=g["h"], kv_heads=g["hkv"])))
    return cases


# ---------------------------------------------------------------------------
# dot-product ops
# ---------------------------------------------------------------------------


def conv_ref(x_nhwc, w, bias=None, stride: int = 1, up2: bool = False,
             silu: bool = False, residual=None):
    """x [B,H,W,C], w [K,C,R,S] (pad R//2), bias [K], residual [B,Ho,Wo,K]
    -> (ref, bound) NHWC fp64."""
    xd = x_nhwc.double().permute(0, 3, 1, 2)
    if up2:
        xd = F.interpolate(xd, scale_factor=2, mode="nearest")
    wd = w.double()
    bd = bias.double() if bias is not None and bias.numel() else None
    pad = w.shape[-1] // 2
    ref = F.conv2d(xd, wd, bd, stride=stride, padding=pad)
    mag = F.conv2d(xd.abs(), wd.abs(), bd.abs() if bd is not None else None,
                   stride=stride, padding=pad)
    if silu:
        ref = F.silu(ref)
    ref, mag = ref.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1)
    if residual is not None and residual.numel():
        ref = ref + residual.double()
        mag = mag + residual.double().abs()
    n = w.shape[1] * w.shape[2] * w.shape[3] + 1
    bound = 2 * U * ref.abs() + (1.1 if silu else 1.0) * n * 2.0 ** -23 * mag
    return ref, bound


def linear_ref(x, w, bias=None, silu: bool = False):
    """x [M,K], w [N,K] -> (ref, bound) fp64 [M,N]."""
    xd, wd = x.double(), w.double()
    ref = xd @ wd.t()
    mag = xd.abs() @ wd.abs().t()
    if bias is not None and bias.numel():
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
    if silu:
        ref = F.silu(ref)
    n = x.shape[1] + 1
    bound = 2 * U * ref.abs() + (1.1 if silu else 1.0) * n * 2.0 ** -23 * mag
    return ref, bound


# Above this reduction length the accumulation term n*2^-23*mag outgrows the
# rounding term (15x at the median element of a C=1280 3x3 conv) and what the
# bound allows is set by a worst case no fp32 chain comes near: a lost
# 8-channel fragment is 150+ bounds up to here and 2.6 at C=1280. Longer
# reductions keep their relative-max assert alone.
DOT_BOUND_MAX_RSC = 1152


def repack_weight(w: torch.Tensor) -> torch.Tensor:
    """[K,C,R,S] -> [K, R*S*C], c innermost: the layout the kernels read."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def conv_inputs(seed: int, b: int, c: int, h: int, w: int, k: int, rs: int):
    """x [b,h,w,c] ~ N(0, 1/16), weight [k,c,r,s] ~ N(0, 1/64), bias ~ N(0,1),
    all bf16-exact fp32."""
    g = torch.Generator().manual_seed(seed)
    r = 3 if rs == 9 else 1
    x = bf16_exact(torch.randn(b, h, w, c, generator=g) / 4)
    wk = bf16_exact(torch.randn(k, c, r, r, generator=g) / 8)
    bias = bf16_exact(torch.randn(k, generator=g))
    return x, wk, bias


# (b, c, h, w, k, rs, fuse_silu) for ext.conv_nhwc called directly. The
# launcher takes v2 (conv_direct_kernel<RS, 4, 4, true>, 128x128 tile, weights
# staged in LDS) when K % 128 == 0 and M = b*h*w >= 128, else v1
# (conv_direct_kernel<RS, 2, 2, false>, 64x64 tile).
CONV_V1_CASES = [
    # M = 99: one full 64-row tile + a 35-row tail; K = 48 < 64: column tail
    (1, 32, 9, 11, 48, 9, False),
    (1, 32, 9, 11, 48, 1, False),
    # M = 35 < 64, K = 16: a single partial tile, one live fragment column
    (1, 96, 5, 7, 16, 9, False),
    # M = 50, two images inside one tile; K % 128 != 0 -> v1
    (2, 64, 5, 5, 64, 9, True),
    # M = 35, K = 144: three column blocks (blockIdx.y = 0..2), the last
    # with 16 live columns (the UNet's 9x9 level runs twenty)
    (1, 32, 5, 7, 144, 9, False),
]
CONV_V2_CASES = [
    # M = 156 >= 128, K = 128: second M tile holds 28 rows
    (1, 96, 12, 13, 128, 9, False),
    # M = 144, K = 256: two column blocks (blockIdx.y = 0, 1)
    (1, 64, 12, 12, 256, 9, False),
    # M = 256, K = 128, 1x1 template with the SiLU epilogue
    (1, 32, 16, 16, 128, 1, True),
    # M = 162, the UNet's 9x9 level at batch 2: the two images meet inside
    # the first 128-row tile, the second tile holds 34 rows; 3x3 with SiLU
    (2, 32, 9, 9, 128, 9, True),
]
# conv256_nhwc with K_out below one fragment column group (conv_supported
# routes the VAE conv_out K=3, the UNet out conv K=4 and the VAE K=8 here):
# (b, c, h, w, k, rs, stride, up2); H, W % 16 == 0 -> tile2d, else linear
CONV256_SMALLK_CASES = (
    [(1, 64, 16, 16, k, 9, 1, False) for k in (3, 4, 8)]
    + [(2, 64, 17, 19, k, 9, 1, False) for k in (3, 4, 8)]
    + [(2, 64, 34, 18, 4, 9, 2, False),    # stride 2 -> 17x9 output, linear
       (1, 64, 8, 8, 4, 9, 1, True)]       # up2 -> 16x16 output, tile2d
)
# conv_smallc at (2, C, 7, 9) -> 40: M = 126 (4 blocks of 32 pixels, the last
# with 30), K = 40 = 8 k-slots x 5
SMALLC_CASES = [(c, rs, silu) for c in (3, 4, 8) for rs in (9, 1)
                for silu in (False, True)]
SMALLC_SHAPE = dict(b=2, h=7, w=9, k=40)


# ---------------------------------------------------------------------------
# rounding-only ops
# ---------------------------------------------------------------------------


def group_norm_ref(x_nchw, groups: int, w, b, eps: float, silu: bool):
    """x [N,C,...] -> (ref, bound) fp64, same layout."""
    n, c = x_nchw.shape[:2]
    xd = x_nchw.double().reshape(n, groups, -1)
    mean = xd.mean(-1, keepdim=True)
    var = xd.var(-1, unbiased=False, keepdim=True)
    xhat = ((xd - mean) / (var + eps).sqrt()).reshape(x_nchw.shape)
    shape = [1, c] + [1] * (x_nchw.dim() - 2)
    wd, bd = w.double().view(shape), b.double().view(shape)
    ref = xhat * wd + bd
    mag = xhat.abs() * wd.abs() + bd.abs()
    if silu:
        ref = F.silu(ref)
    return ref, 2 * U * ref.abs() + 2.0 ** -16 * mag


def layer_norm_ref(x, w, b, eps: float):
    """x [T,C] -> (ref, bound) fp64."""
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = xd.var(-1, unbiased=False, keepdim=True)
    xhat = (xd - mean) / (var + eps).sqrt()
    ref = xhat * w.double() + b.double()
    mag = xhat.abs() * w.double().abs() + b.double().abs()
    return ref, 2 * U * ref.abs() + 2.0 ** -16 * mag


def act_mul_ref(a, b, gelu: bool):
    bd = b.double()
    act = F.gelu(bd, approximate="tanh") if gelu else F.silu(bd)
    ref = a.double() * act
    return ref, (2 * U + 2.0 ** -16) * ref.abs()


def norm_inputs(seed: int, shape, mean: float = 0.0, std: float = 1.0):
    """x ~ N(mean, std^2) bf16-exact in ``shape`` ([N,C,H,W] or [T,C]);
    fp32 weight/bias ~ N(0,1) over the channel dim."""
    g = torch.Generator().manual_seed(seed)
    x = bf16_exact(torch.randn(*shape, generator=g) * std + mean)
    c = shape[1] if len(shape) == 4 else shape[-1]
    return x, torch.randn(c, generator=g), torch.randn(c, generator=g)


# group_norm_nhwc, (shape NCHW, G): which kernel the launcher picks
GN_NHWC_CASES = [
    ((2, 320, 7, 9), 32),     # two-pass, Cg=10: vectors straddle groups
    ((1, 640, 4, 4), 32),     # two-pass, Cg=20
    ((1, 1280, 2, 2), 32),    # two-pass, Cg=40
    ((1, 256, 5, 5), 32),     # two-pass, Cg=8: vectors align with groups
    ((1, 512, 3, 3), 64),     # two-pass at the G=64 LDS limit
    ((3, 320, 2, 2), 32),     # three images, one stats block each (bpi=1)
    ((1, 64, 6, 6), 32),      # Cg=2 -> per-(n,g) kernel, scalar loop
    ((1, 576, 3, 3), 72),     # G>64 -> per-(n,g) kernel, Cg=8 vector loop
    ((1, 6, 512, 512), 1),    # C%8 != 0, 1.5M elements -> 1024 threads
]
GN_NCHW_BIG = ((1, 8, 512, 512), 1)   # groupnorm_kernel with 1024 threads
# mean 16 / std 1. The kernels take var = E[x^2] - mean^2 in fp32, whose
# error grows as 2^-23 * (mean/std)^2 relative to var, and the fp32 mean is
# off by ~2^-23 * mean. By CPU emulation (test_kernel_bounds_cpu.py) the
# bound holds at mean/std = 16 (0.5-0.6 of it); from mean/std ~ 32 the
# elements where xhat*w + b cancels leave its 2^-16 floor (3x at 64, 10x at
# 128), and near 256-512 the typical element is off by a whole bf16 ulp.
GN_OFFSET_CASE = ((2, 320, 7, 9), 32)
NORM_OFFSET = dict(mean=16.0, std=1.0)
# layer_norm rows of (5, C): C < 8 (tail only), 12 and 324 (vectors + tail
# of 4), 513 (tail of 1, rows start on odd elements), 2568 > 2048 (several
# trips of the 512-wide loop)
LN_T = 5
LN_CASES = [4, 12, 324, 513, 2568]
LN_OFFSET_C = 324

# act_mul sizes: below one vector, tails of 7/1/3, a 3-D GEGLU tensor, and
# one size past the 2048*256*8-element grid, so the grid-stride loop takes a
# second trip and the tail (n % 8 == 5) is written as well
ACT_MUL_GRID = 2048 * 256 * 8
ACT_MUL_SHAPES = [(1,), (7,), (9,), (1003,), (2, 77, 1280),
                  (ACT_MUL_GRID + 2405,)]


def act_mul_inputs(seed: int, shape):
    """a, b ~ N(0,1), b clamped to [-4, 4]. The tanh form of GELU computes
    1 + tanh(.) in fp32, which cancels as b falls: below b ~ -4.5 its 2^-24
    absolute error is more than 2^-8 of the result (itself < 1e-4 there), and
    no relative bound holds for any fp32 evaluation. Among 4M normal samples
    some reach -5; the clamp keeps the inputs where the bound is meaningful."""
    g = torch.Generator().manual_seed(seed)
    return (bf16_exact(torch.randn(*shape, generator=g)),
            bf16_exact(torch.randn(*shape, generator=g).clamp(-4.0, 4.0)))


# ---------------------------------------------------------------------------
# DiT glue ops (dit_ops.hip): fp32 math, one rounding on store
# ---------------------------------------------------------------------------

FP32_FLOOR = 2.0 ** -16
NM_ITERS = (1, 2, 4, 6, 8, 10, 12, 16)   # norm_modulate_kernel<ITERS>
FILLER = 7.0    # what the unused parts of a strided buffer hold


def hulp(r: torch.Tensor) -> torch.Tensor:
    """Half a bf16 ulp at r: 2^(floor(log2|r|) - 8), |r| >= 2^-126."""
    # |r| = m * 2^e with m in [0.5, 1), so floor(log2|r|) = e - 1
    _, e = torch.frexp(r.double().abs().clamp_min(2.0 ** -126))
    return torch.exp2((e - 9).double())


def qk_norm_rope_ref(x, w, cos, sin, heads: int, eps: float,
                     token_offset: int = 0):
    """One side of qk_norm_rope. x [B, N, H*D] bf16-exact, w [D] fp32,
    cos/sin [Npos, D/2] fp32 -> (ref, bound) fp64 [B, N, H*D]; row n is
    rotated by table row token_offset + n."""
    b, n, hd = x.shape
    d = hd // heads
    xd = x.double().reshape(b, n, heads, d)
    rstd = 1.0 / (xd.pow(2).mean(-1, keepdim=True) + eps).sqrt()
    y = xd * rstd * w.double()
    y0, y1 = y[..., 0::2], y[..., 1::2]
    rows = slice(token_offset, token_offset + n)
    c = cos[rows].double()[None, :, None, :]
    s = sin[rows].double()[None, :, None, :]
    ref, mag = torch.empty_like(y), torch.empty_like(y)
    ref[..., 0::2] = y0 * c - y1 * s
    ref[..., 1::2] = y0 * s + y1 * c
    mag[..., 0::2] = (y0 * c).abs() + (y1 * s).abs()
    mag[..., 1::2] = (y0 * s).abs() + (y1 * c).abs()
    ref, mag = ref.reshape(b, n, hd), mag.reshape(b, n, hd)
    return ref, hulp(ref) + FP32_FLOOR * mag


def norm_modulate_ref(x, mode: str, w=None, scale=None, shift=None,
                      eps: float | None = None):
    """x [B, N, C] bf16-exact, w [C] fp32 (rms), scale/shift [B, C]
    bf16-exact or None -> (ref, bound) fp64 [B, N, C]."""
    if eps is None:
        eps = 1e-6 if mode == "rms" else 1e-5
    c = x.shape[-1]
    xd = x.double()
    if mode == "rms":
        rstd = 1.0 / (xd.pow(2).mean(-1, keepdim=True) + eps).sqrt()
        norm = xd * rstd * w.double()
    else:
        mean = xd.mean(-1, keepdim=True)
        rstd = 1.0 / (xd.var(-1, unbiased=False, keepdim=True) + eps).sqrt()
        norm = (xd - mean) * rstd
    if scale is not None:
        gain = (1.0 + scale.double())[:, None]
        ref = norm * gain + shift.double()[:, None]
        mag = norm.abs() * gain.abs() + shift.double().abs()[:, None]
    else:
        gain = torch.ones(1, 1, 1, dtype=torch.float64)
        ref, mag = norm, norm.abs()
    bound = hulp(ref) + FP32_FLOOR * mag
    if mode == "layer":
        n = 8 * ((c + 511) // 512) + 6
        bound = bound + n * 2.0 ** -24 * xd.abs().mean(-1, keepdim=True) \
            * rstd * gain.abs()
    return ref, bound


def gated_residual_ref(x, gate, y):
    """x, y [B, N, C], gate [B, C], bf16-exact -> (ref, bound) fp64."""
    gy = gate.double()[:, None] * y.double()
    ref = x.double() + gy
    return ref, hulp(ref) + FP32_FLOOR * (x.double().abs() + gy.abs())


# --- qk_norm_rope cases ----------------------------------------------------
#
# kernel G (lanes per head): 2 for D=16, 4 to 32, 8 to 64, 16 to 128, 32 to
# 256; a group is padded when D/8 is no power of two.

QK_EPS = 1e-6
QK_NEW_D = [16, 24, 40, 48, 56, 72, 80, 104, 136, 192, 248, 256]
# B*N*H odd: ngroups * G is a multiple of neither 64 nor 256, so the last
# wave holds live and exited groups
QK_BNH = [(1, 5, 3), (3, 3, 3)]
QK_OLD_SHAPES = [(2, 5, 2, 32), (2, 5, 3, 64), (1, 7, 5, 128), (2, 3, 2, 96)]
FLUX_MLP = 40   # width of the fourth part of the Flux-style split


def _qk_cases():
    """name -> dict(b, n, h, d, layout, amp, tail, zero_head, off).
    layout: how q and k reach the kernel (qk_place). amp: input amplitude.
    tail: factor on the last 8 channels of every head, which gives one lane
    of the group weight in the statistics. zero_head: index of a head that is
    all zero. off: token_offset into out buffers of off + n + 2 rows."""
    cases = {}

    def add(name, bnh, d, layout="qkv", amp=1.0, tail=1.0, zero_head=None,
            off=0):
        b, n, h = bnh
        cases[name] = dict(b=b, n=n, h=h, d=d, layout=layout, amp=amp,
                           tail=tail, zero_head=zero_head, off=off,
                           seed=1000 + len(cases))

    for i, d in enumerate(QK_NEW_D):
        add(f"D{d}", QK_BNH[i % 2], d)
    for b, n, h, d in QK_OLD_SHAPES:
        add(f"shape{b}x{n}x{h}x{d}", (b, n, h), d)
    # q out of the fused projection, k a tensor of its own: strides differ
    add("k_separate_D40", QK_BNH[1], 40, layout="k_separate")
    add("k_separate_D128", QK_BNH[0], 128, layout="k_separate")
    # rows 2..2+N of a longer projection: batch stride != N * row stride
    add("row_slice_D16", QK_BNH[1], 16, layout="row_slice")
    add("row_slice_D72", QK_BNH[1], 72, layout="row_slice")
    add("flux_split_D24", QK_BNH[1], 24, layout="flux_split")
    add("flux_split_D128", QK_BNH[0], 128, layout="flux_split")
    add("zero_head_D40", QK_BNH[1], 40, zero_head=1)
    add("zero_head_D64", (2, 5, 3), 64, zero_head=2)
    # mean(x^2) ~ 2^-20 ~ eps: the only recipe in which eps matters
    for i, d in enumerate((16, 40, 128, 256)):
        add(f"amp2^-10_D{d}", QK_BNH[i % 2], d, amp=2.0 ** -10)
    add("offset4_D64", (2, 5, 3), 64, off=4)
    add("offset3_D136_row_slice", QK_BNH[0], 136, layout="row_slice", off=3)
    for i, d in enumerate((24, 40, 104, 248)):
        add(f"tail8_D{d}", QK_BNH[i % 2], d, tail=8.0)
    return cases


QK_CASES = _qk_cases()


def qk_inputs(b, n, h, d, seed, amp=1.0, tail=1.0, zero_head=None, off=0,
              **_):
    """q, k [B, N, H*D] bf16-exact ~ amp * N(0,1), distinct fp32 weights,
    random angles for off + n + 2 table rows."""
    g = torch.Generator().manual_seed(seed)
    sides = []
    for _side in range(2):
        x = torch.randn(b, n, h, d, generator=g) * amp
        x[..., -8:] *= tail
        if zero_head is not None:
            x[:, :, zero_head] = 0
        sides.append(bf16_exact(x.reshape(b, n, h * d)))
    wq = torch.randn(d, generator=g)
    wk = torch.randn(d, generator=g)
    ang = torch.rand(off + n + 2, d // 2, generator=g) * 6.28
    return dict(q=sides[0], k=sides[1], wq=wq, wk=wk, cos=ang.cos(),
                sin=ang.sin(), heads=h, off=off, ntot=off + n + 2)


def qk_refs(inp):
    """((ref_q, bound_q), (ref_k, bound_k)) of qk_inputs' result."""
    return tuple(
        qk_norm_rope_ref(inp[x], inp[w], inp["cos"], inp["sin"], inp["heads"],
                         QK_EPS, inp["off"])
        for x, w in (("q", "wq"), ("k", "wk")))


def qk_place(q, k, layout: str, device):
    """bf16 q and k on ``device`` as the views the models hand over; the
    rest of each buffer holds FILLER."""
    b, n, hd = q.shape
    q, k = q.to(BF).to(device), k.to(BF).to(device)
    if layout == "qkv":                       # chunks of [B, N, 3HD]
        buf = torch.full((b, n, 3 * hd), FILLER, dtype=BF, device=device)
        vq, vk, _ = buf.chunk(3, dim=-1)
    elif layout == "k_separate":              # q a chunk, k contiguous
        buf = torch.full((b, n, 3 * hd), FILLER, dtype=BF, device=device)
        vq, vk = buf.chunk(3, dim=-1)[0], torch.empty_like(k)
    elif layout == "row_slice":               # [:, 2:2+N] of [B, N+4, 3HD]
        buf = torch.full((b, n + 4, 3 * hd), FILLER, dtype=BF, device=device)
        vq, vk, _ = buf[:, 2:2 + n].chunk(3, dim=-1)
    elif layout == "flux_split":              # [d, d, d, mlp] of one Linear
        buf = torch.full((b, n, 3 * hd + FLUX_MLP), FILLER, dtype=BF,
                         device=device)
        vq, vk, _, _ = buf.split([hd, hd, hd, FLUX_MLP], dim=-1)
    else:
        raise ValueError(layout)
    vq.copy_(q)
    vk.copy_(k)
    return vq, vk


# --- norm_modulate cases ---------------------------------------------------

# every instantiation, full (512, 1024, 2048, 6144, 8192 ...) and with dead
# trips (520 -> 2, 1032 -> 4, 2056 -> 6, 3080 -> 8, 4104 -> 10, 5128 -> 12,
# 6152 -> 16), and the limits 8 and 8192
NM_NEW_C = [8, 512, 520, 1024, 1032, 2048, 2056, 3080, 3584, 4096, 4104,
            5128, 6144, 6152, 8192]
# T = B*N: 9, 6, 3, 5 -> T % 4 = 1, 2, 3, 1 (4 rows per block); B = 3; N = 1
NM_BN = [(3, 3), (2, 3), (3, 1), (1, 5)]
NM_OLD_C = [64, 72, 3072, 5120]


def _nm_cases():
    """name -> dict(b, n, c, mode, layout, mean, std, tail, const).
    layout "unbind": scale and shift are rows of one [B, 6, C] tensor;
    "mixed": scale is, shift is a contiguous tensor of its own. const: every
    row holds one value."""
    cases = {}

    def add(name, bn, c, mode, layout="unbind", mean=0.0, std=1.0, tail=1.0,
            const=False):
        cases[name] = dict(b=bn[0], n=bn[1], c=c, mode=mode, layout=layout,
                           mean=mean, std=std, tail=tail, const=const,
                           seed=2000 + len(cases))

    for mode in ("rms", "layer"):
        for i, c in enumerate(NM_NEW_C):
            add(f"{mode}_C{c}", NM_BN[i % 4], c, mode,
                layout=("unbind", "mixed")[i % 2])
        for c in NM_OLD_C:   # the recipe of test_norm_modulate
            add(f"{mode}_C{c}_mean3", (2, 7), c, mode, mean=3.0, std=0.5)
        # the last partial chunk carries a third of the row's sum of squares
        add(f"{mode}_C1032_tail8", (2, 3), 1032, mode, tail=8.0)
    for c in (520, 3080, 8192):
        add(f"layer_C{c}_const", (3, 3), c, "layer", const=True)
    # where a one-pass variance (sumsq - mean^2) breaks down
    for i, c in enumerate((512, 1032, 3072)):
        add(f"layer_C{c}_mean128", NM_BN[i], c, "layer", mean=128.0)
    for i, c in enumerate((520, 3072)):
        add(f"rms_C{c}_mean32", NM_BN[i], c, "rms", mean=32.0)
    return cases


NM_CASES = _nm_cases()


def nm_inputs(b, n, c, mode, seed, mean=0.0, std=1.0, tail=1.0, const=False,
              **_):
    """x [B, N, C] ~ N(mean, std^2), scale/shift [B, C] ~ N(0,1), all
    bf16-exact; fp32 weight [C] ~ N(0,1) in rms mode."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, n, 1 if const else c, generator=g) * std + mean
    x = x.expand(b, n, c).clone()
    x[..., -8:] *= tail
    m = bf16_exact(torch.randn(b, 2, c, generator=g))
    w = torch.randn(c, generator=g) if mode == "rms" else None
    return dict(x=bf16_exact(x), mode=mode, w=w, scale=m[:, 0], shift=m[:, 1])


def mod_place(scale, shift, layout: str, device):
    """bf16 scale and shift [B, C] on ``device`` as strided views."""
    b, c = scale.shape
    buf = torch.full((b, 6, c), FILLER, dtype=BF, device=device)
    vsh, vsc = buf.unbind(1)[3:5]
    if layout == "mixed":
        vsh = torch.empty(b, c, dtype=BF, device=device)
    elif layout != "unbind":
        raise ValueError(layout)
    vsc.copy_(scale.to(BF))
    vsh.copy_(shift.to(BF))
    return vsc, vsh


# --- gated_residual cases --------------------------------------------------

GR_GRID = 4096 * 256 * 8     # elements of one trip of the grid-stride loop
# name -> (b, n, c, gate layout). "offset": the gate starts C + 16 elements
# into its storage and its rows are 3 * (C + 8) apart.
GR_CASES = {
    "one_chunk": (1, 1, 8, "unbind"),
    "shape2x9x72": (2, 9, 72, "unbind"),
    "gate_offset": (3, 5, 136, "offset"),
    # 8,409,096 elements > GR_GRID: a second trip, and both batch boundaries
    # (at 2,803,032 and 5,606,064) fall inside a block's 2048 elements
    "second_trip": (3, 683, 4104, "unbind"),
}
assert 3 * 683 * 4104 > GR_GRID and (683 * 4104) % 2048 != 0


def gr_inputs(name):
    b, n, c, _ = GR_CASES[name]
    g = torch.Generator().manual_seed(3000 + c)
    return (bf16_exact(torch.randn(b, n, c, generator=g)),
            bf16_exact(torch.randn(b, c, generator=g)),
            bf16_exact(torch.randn(b, n, c, generator=g)))


def gate_place(gate, layout: str, device):
    b, c = gate.shape
    if layout == "unbind":
        view = torch.full((b, 6, c), FILLER, dtype=BF,
                          device=device).unbind(1)[2]
    elif layout == "offset":
        view = torch.full((b, 3, c + 8), FILLER, dtype=BF,
                          device=device)[:, 1, 8:]
    else:
        raise ValueError(layout)
    view.copy_(gate.to(BF))
    return view
