"""The bounds of kernel_bounds.py discriminate, shown without a GPU.

For the shapes and input recipes the GPU tests use, a CPU emulation of each
kernel's arithmetic (fp32 math where the kernel has fp32, bf16 where it rounds)
must stay within 0.75 of the bound, and the same emulation with one seeded
defect must leave it:

  attention   last key dropped / two V rows swapped / scale off by 1%
  conv        one 8-channel chunk of one tap missing / border taps not zero
  norms       statistics of the neighbouring group (row)
  LN, act_mul tail elements (past the last 8-wide vector) left unwritten

G=1 group norms have no neighbouring group and sizes that are a multiple of 8
have no tail; those cases run the emulation check only.

The DiT glue ops (dit_ops.hip) round once, and their bound is half a bf16 ulp
of the reference plus an fp32 floor, so there is no 0.75 of headroom to ask
for: their emulations must stay within 1.0 on every case of kernel_bounds'
lists, and every seeded defect (QK_DEFECTS, NM_DEFECTS, GR_DEFECTS below)
must reach 2 bounds on at least one case of its op.
"""

import math

import pytest
import torch
import torch.nn.functional as F

import kernel_bounds as kb

KT = 64                # keys per tile
LOG2E = 1.4426950408889634
DEFER_THR = 8.0
EMU_MAX = 0.75


def _bf(x):
    return x.to(torch.bfloat16).float()


def _silu32(x):
    return x / (1.0 + torch.exp(-x))


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------


def emulate_attention(q, k, v, heads=1, kv_heads=None, scale=None):
    """The tile loop of attention.hip in fp32: 64-key tiles, running max in
    the exp2 domain that moves only when some row of a 16-row group sees its
    tile max pass it by more than 8 (defer-max), row sum over unrounded p,
    p rounded to bf16 for PV, fp32 accumulators, one bf16 store."""
    kv_heads = kv_heads or heads
    bh, nq, d = q.shape
    nk = k.shape[1]
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    if kv_heads != heads:
        rep, b = heads // kv_heads, bh // heads
        k = k.reshape(b, kv_heads, 1, nk, d).expand(-1, -1, rep, -1, -1) \
            .reshape(bh, nk, d)
        v = v.reshape(b, kv_heads, 1, nk, d).expand(-1, -1, rep, -1, -1) \
            .reshape(bh, nk, d)
    nqp = (nq + 15) // 16 * 16
    qf = torch.zeros(bh, nqp, d)
    qf[:, :nq] = q.float()
    kf, vf = k.float(), v.float()
    c = torch.tensor(scale * LOG2E, dtype=torch.float32)
    m_run = torch.full((bh, nqp), -1e30)
    l_run = torch.zeros(bh, nqp)
    o = torch.zeros(bh, nqp, d)
    for k0 in range(0, nk, KT):
        s = torch.bmm(qf, kf[:, k0:k0 + KT].transpose(1, 2))
        mt = s.max(dim=-1).values * c
        need = (mt - m_run) > DEFER_THR * LOG2E
        grp = need.reshape(bh, nqp // 16, 16).any(-1, keepdim=True) \
            .expand(-1, -1, 16).reshape(bh, nqp)
        m_new = torch.where(grp, torch.maximum(m_run, mt), m_run)
        a = torch.exp2(m_run - m_new)
        m_run = m_new
        l_run = l_run * a
        o = o * a[..., None]
        p = torch.exp2(s * c - m_run[..., None])
        l_run = l_run + p.sum(-1)
        o = o + torch.bmm(_bf(p), vf[:, k0:k0 + KT])
    return _bf(o / l_run[..., None])[:, :nq]


@pytest.mark.parametrize("name,inp,kw", kb.attn_new_cases(),
                         ids=[c[0] for c in kb.attn_new_cases()])
def test_attention_emulation_inside_mutations_outside(name, inp, kw):
    q, k, v = kb.attn_inputs(**inp)
    ref, bound = kb.attention_ref(q, k, v, **kw)
    r = kb.err_ratio(emulate_attention(q, k, v, **kw), ref, bound)
    nk = k.shape[1]
    v_swap = v.clone()
    v_swap[:, [3, nk - 2]] = v[:, [nk - 2, 3]]
    scale = kw.get("scale", 1.0 / math.sqrt(q.shape[-1]))
    mut = {
        "drop last key": emulate_attention(q, k[:, :-1], v[:, :-1], **kw),
        "swap V rows": emulate_attention(q, k, v_swap, **kw),
        "scale +1%": emulate_attention(q, k, v, **{**kw, "scale": scale * 1.01}),
    }
    rm = {m: kb.err_ratio(o, ref, bound) for m, o in mut.items()}
    print(f"attention {name}: emulation {r:.3f}  " +
          "  ".join(f"{m} {x:.1f}" for m, x in rm.items()))
    assert r <= EMU_MAX, r
    for m, x in rm.items():
        assert x > 1.0, (m, x)


@pytest.mark.parametrize("d", [40, 64, 80, 128, 160])
@pytest.mark.parametrize("nq,nk", [(64, 64), (77, 77), (1156, 77),
                                   (1024, 1024), (40, 1), (40, 13), (40, 141)])
def test_attention_emulation_flat_logits(d, nq, nk):
    """The recipe of the older tests (q, k ~ randn/2: nearly flat softmax)
    at their shapes: the emulation stays inside the bound there too."""
    g = torch.Generator().manual_seed(d * 1000 + nq)
    q = kb.bf16_exact(torch.randn(4, nq, d, generator=g) / 2)
    k = kb.bf16_exact(torch.randn(4, nk, d, generator=g) / 2)
    v = kb.bf16_exact(torch.randn(4, nk, d, generator=g))
    ref, bound = kb.attention_ref(q, k, v)
    r = kb.err_ratio(emulate_attention(q, k, v), ref, bound)
    print(f"attention flat d={d} nq={nq} nk={nk}: emulation {r:.3f}")
    assert r <= EMU_MAX, r


def test_attention_emulation_peaked_recipes():
    """The hand-built recipes of the older tests: spiked keys in later tiles
    (the defer-max rescale fires mid-stream), one-hot rows, uniform V."""
    g = torch.Generator().manual_seed(9)
    q = torch.randn(2, 256, 64, generator=g) / 4
    k = torch.randn(2, 256, 64, generator=g) / 4
    v = torch.randn(2, 256, 64, generator=g)
    k[:, 140] = q[:, 17] * 40.0
    k[:, 200] = q[:, 33] * 60.0
    spikes = tuple(kb.bf16_exact(t) for t in (q, k, v))

    k = F.normalize(torch.randn(2, 150, 40, generator=g), dim=-1)
    q = kb.bf16_exact(250.0 * k[:, torch.arange(160) % 150])
    one_hot = (q, kb.bf16_exact(k),
               kb.bf16_exact(torch.randn(2, 150, 40, generator=g)))

    uniform = (kb.bf16_exact(torch.randn(2, 100, 64, generator=g)),
               kb.bf16_exact(torch.randn(2, 150, 64, generator=g)),
               torch.ones(2, 150, 64))
    for name, (q, k, v) in dict(spikes=spikes, one_hot=one_hot,
                                uniform_v=uniform).items():
        ref, bound = kb.attention_ref(q, k, v)
        r = kb.err_ratio(emulate_attention(q, k, v), ref, bound)
        print(f"attention {name}: emulation {r:.3f}")
        assert r <= EMU_MAX, (name, r)


def test_attention_flat_logits_lost_key_is_seen():
    """nq=128, nk=1024, d=64 with flat logits: a dropped key moves the output
    by about 0.005, far inside the old 0.03, and outside the derived bound."""
    g = torch.Generator().manual_seed(1)
    q = kb.bf16_exact(torch.randn(2, 128, 64, generator=g) / 2)
    k = kb.bf16_exact(torch.randn(2, 1024, 64, generator=g) / 2)
    v = kb.bf16_exact(torch.randn(2, 1024, 64, generator=g))
    ref, bound = kb.attention_ref(q, k, v)
    out = emulate_attention(q, k[:, :-1], v[:, :-1])
    err = (out.double() - ref).abs().max().item()
    r = kb.err_ratio(out, ref, bound)
    print(f"flat nk=1024 dropped key: max err {err:.4f}  err/bound {r:.2f}")
    assert err < 0.03 and r > 1.0, (err, r)


# ---------------------------------------------------------------------------
# convolution / gemm
# ---------------------------------------------------------------------------


def emulate_conv(x_nhwc, w, bias, stride=1, up2=False, silu=False,
                 residual=None, zero_chunk=None, replicate_border=False):
    """fp32 accumulation, bias, SiLU, residual, one bf16 store.
    zero_chunk=(r, s, c0): the 8 channels from c0 of tap (r, s) are missing.
    replicate_border: out-of-image taps read the nearest pixel, not zero."""
    xf = x_nhwc.float().permute(0, 3, 1, 2)
    if up2:
        xf = F.interpolate(xf, scale_factor=2, mode="nearest")
    wf = w.float().clone()
    if zero_chunk is not None:
        r, s, c0 = zero_chunk
        wf[:, c0:c0 + 8, r, s] = 0
    pad = w.shape[-1] // 2
    if replicate_border and pad:
        xf = F.pad(xf, (pad, pad, pad, pad), mode="replicate")
        pad = 0
    y = F.conv2d(xf, wf, bias.float(), stride=stride, padding=pad)
    if silu:
        y = _silu32(y)
    y = y.permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual.float()
    return _bf(y)


def _conv_cases():
    out = []
    for (b, c, h, w, k, rs, silu) in kb.CONV_V1_CASES + kb.CONV_V2_CASES:
        out.append((b, c, h, w, k, rs, 1, False, silu))
    for (b, c, h, w, k, rs, stride, up2) in kb.CONV256_SMALLK_CASES:
        out.append((b, c, h, w, k, rs, stride, up2, False))
    s = kb.SMALLC_SHAPE
    for (c, rs, silu) in kb.SMALLC_CASES:
        out.append((s["b"], c, s["h"], s["w"], s["k"], rs, 1, False, silu))
    # shapes of the older conv tests that go through the bound
    for (b, c, h, w, k, rs) in [(2, 64, 17, 19, 96, 9), (1, 128, 34, 34, 320, 9),
                                (2, 64, 32, 32, 48, 1), (2, 4, 17, 19, 320, 9)]:
        out.append((b, c, h, w, k, rs, 1, False, False))
    return out


@pytest.mark.parametrize("b,c,h,w,k,rs,stride,up2,silu", _conv_cases())
def test_conv_emulation_inside_mutations_outside(b, c, h, w, k, rs, stride,
                                                 up2, silu):
    x, wk, bias = kb.conv_inputs(c * 100 + k + rs, b, c, h, w, k, rs)
    ref, bound = kb.conv_ref(x, wk, bias, stride, up2, silu)
    kw = dict(stride=stride, up2=up2, silu=silu)
    r = kb.err_ratio(emulate_conv(x, wk, bias, **kw), ref, bound)
    r3 = 3 if rs == 9 else 1
    chunk = (r3 // 2, r3 // 2, max(0, c - 8))
    rm = {"lost chunk": kb.err_ratio(
        emulate_conv(x, wk, bias, zero_chunk=chunk, **kw), ref, bound)}
    if rs == 9:
        rm["border not zero"] = kb.err_ratio(
            emulate_conv(x, wk, bias, replicate_border=True, **kw), ref, bound)
    print(f"conv {(b, c, h, w)}->{k} rs{rs} s{stride} up2={up2} silu={silu}: "
          f"emulation {r:.3f}  " +
          "  ".join(f"{m} {v:.0f}" for m, v in rm.items()))
    assert r <= EMU_MAX, r
    for m, v in rm.items():
        assert v > 1.0, (m, v)


def test_conv_residual_emulation():
    b, c, h, w, k = 2, 64, 20, 20, 96
    x, wk, bias = kb.conv_inputs(9, b, c, h, w, k, 9)
    res = kb.bf16_exact(torch.randn(b, h, w, k,
                                    generator=torch.Generator().manual_seed(10)))
    ref, bound = kb.conv_ref(x, wk, bias, residual=res)
    r = kb.err_ratio(emulate_conv(x, wk, bias, residual=res), ref, bound)
    rm = kb.err_ratio(emulate_conv(x, wk, bias, residual=res,
                                   zero_chunk=(0, 2, 8)), ref, bound)
    print(f"conv + residual: emulation {r:.3f}  lost chunk {rm:.0f}")
    assert r <= EMU_MAX and rm > 1.0, (r, rm)


@pytest.mark.parametrize("m,n,k", [(300, 77, 128), (256, 256, 64),
                                   (1156, 640, 768)])
@pytest.mark.parametrize("silu", [False, True])
def test_gemm_emulation_inside_mutation_outside(m, n, k, silu):
    g = torch.Generator().manual_seed(k)
    x = kb.bf16_exact(torch.randn(m, k, generator=g) / 4)
    w = kb.bf16_exact(torch.randn(n, k, generator=g) / 4)
    b = kb.bf16_exact(torch.randn(n, generator=g))
    ref, bound = kb.linear_ref(x, w, b, silu)

    def emu(wf):
        y = x @ wf.t() + b
        return _bf(_silu32(y) if silu else y)

    r = kb.err_ratio(emu(w), ref, bound)
    w_lost = w.clone()
    w_lost[:, k - 8:] = 0
    rm = kb.err_ratio(emu(w_lost), ref, bound)
    print(f"gemm {m}x{n}x{k} silu={silu}: emulation {r:.3f}  "
          f"lost chunk {rm:.0f}")
    assert r <= EMU_MAX and rm > 1.0, (r, rm)


def test_dot_bound_above_1152():
    """Why the bound stops at RS*C = 1152: at C=1280 3x3 the accumulation
    term n*2^-23*mag is many times the rounding term 2U*|ref|, so what the
    bound allows is set by a worst case no fp32 chain comes near."""
    x, wk, bias = kb.conv_inputs(1280, 1, 1280, 8, 8, 32, 9)
    ref, bound = kb.conv_ref(x, wk, bias)
    acc_term = bound - 2 * kb.U * ref.abs()
    share = (acc_term / (2 * kb.U * ref.abs()).clamp_min(1e-30)).median().item()
    rm = kb.err_ratio(emulate_conv(x, wk, bias, zero_chunk=(1, 1, 0)), ref,
                      bound)
    print(f"C=1280 3x3: accumulation/rounding term median {share:.1f}, "
          f"lost chunk err/bound {rm:.2f}")
    assert 9 * 1280 > kb.DOT_BOUND_MAX_RSC
    assert share > 10.0, share
    assert rm < 10.0, rm   # 150+ for every shape that goes through the bound


# ---------------------------------------------------------------------------
# norms, act_mul
# ---------------------------------------------------------------------------


def _one_pass_stats(xg, eps):
    """mean and rstd from sum and sum of squares in fp32, as the kernels do."""
    n = xg.shape[-1]
    s = xg.sum(-1, keepdim=True, dtype=torch.float32)
    sq = (xg * xg).sum(-1, keepdim=True, dtype=torch.float32)
    mean = s / n
    var = sq / n - mean * mean
    return mean, torch.rsqrt(var.clamp_min(0.0) + eps)


def emulate_group_norm(x, groups, w, b, eps, silu, neighbour=False):
    n, c = x.shape[:2]
    xg = x.float().reshape(n, groups, -1)
    mean, rstd = _one_pass_stats(xg, eps)
    if neighbour:
        mean, rstd = mean.roll(1, 1), rstd.roll(1, 1)
    y = ((xg - mean) * rstd).reshape(x.shape)
    shape = [1, c] + [1] * (x.dim() - 2)
    y = y * w.float().view(shape) + b.float().view(shape)
    return _bf(_silu32(y) if silu else y)


def emulate_layer_norm(x, w, b, eps, neighbour=False, drop_tail=False):
    xf = x.float()
    mean, rstd = _one_pass_stats(xf, eps)
    if neighbour:
        mean, rstd = mean.roll(1, 0), rstd.roll(1, 0)
    y = _bf((xf - mean) * rstd * w.float() + b.float())
    if drop_tail:
        y[:, x.shape[-1] // 8 * 8:] = 0
    return y


GN_ALL = ([(s, g, {}) for s, g in kb.GN_NHWC_CASES + [kb.GN_NCHW_BIG]]
          + [(*kb.GN_OFFSET_CASE, kb.NORM_OFFSET)]
          + [((2, 128, 20, 20), 32, {}), ((2, 33, 7, 7), 3, {})])


@pytest.mark.parametrize("shape,groups,kw", GN_ALL)
@pytest.mark.parametrize("silu", [False, True])
def test_group_norm_emulation_inside_mutation_outside(shape, groups, kw, silu):
    x, w, b = kb.norm_inputs(shape[1] + groups, shape, **kw)
    ref, bound = kb.group_norm_ref(x, groups, w, b, 1e-5, silu)
    r = kb.err_ratio(emulate_group_norm(x, groups, w, b, 1e-5, silu), ref,
                     bound)
    msg = f"group_norm {shape} G={groups} {kw} silu={silu}: emulation {r:.3f}"
    assert r <= EMU_MAX, msg
    if groups > 1:
        rm = kb.err_ratio(
            emulate_group_norm(x, groups, w, b, 1e-5, silu, neighbour=True),
            ref, bound)
        msg += f"  neighbour stats {rm:.1f}"
        assert rm > 1.0, msg
    print(msg)


@pytest.mark.parametrize("c,kw", [(c, {}) for c in kb.LN_CASES]
                         + [(kb.LN_OFFSET_C, kb.NORM_OFFSET),
                            (320, {}), (2048, {})])
def test_layer_norm_emulation_inside_mutations_outside(c, kw):
    x, w, b = kb.norm_inputs(c, (kb.LN_T, c), **kw)
    ref, bound = kb.layer_norm_ref(x, w, b, 1e-5)
    r = kb.err_ratio(emulate_layer_norm(x, w, b, 1e-5), ref, bound)
    rm = {"neighbour stats": kb.err_ratio(
        emulate_layer_norm(x, w, b, 1e-5, neighbour=True), ref, bound)}
    if c % 8:
        rm["tail unwritten"] = kb.err_ratio(
            emulate_layer_norm(x, w, b, 1e-5, drop_tail=True), ref, bound)
    print(f"layer_norm C={c} {kw}: emulation {r:.3f}  " +
          "  ".join(f"{m} {v:.1f}" for m, v in rm.items()))
    assert r <= EMU_MAX, r
    for m, v in rm.items():
        assert v > 1.0, (m, v)


def test_one_pass_statistics_range():
    """How far the one-pass statistics carry: with std 1 the emulation is
    inside the bound at mean 16 and outside it at mean 128, where
    E[x^2] - mean^2 has lost 2^-9 of the variance; the median element is
    still within half a bf16 ulp there."""
    shape, groups = kb.GN_OFFSET_CASE
    ratio, med = {}, {}
    for mean in (16.0, 128.0):
        x, w, b = kb.norm_inputs(0, shape, mean=mean, std=1.0)
        ref, bound = kb.group_norm_ref(x, groups, w, b, 1e-5, True)
        out = emulate_group_norm(x, groups, w, b, 1e-5, True)
        ratio[mean] = kb.err_ratio(out, ref, bound)
        err = (out.double() - ref).abs()
        med[mean] = (err / (kb.U * ref.abs()).clamp_min(1e-30)).median().item()
    print(f"one-pass GN statistics: err/bound {ratio}, median err in ulp {med}")
    assert ratio[16.0] <= EMU_MAX and ratio[128.0] > 1.0, ratio
    assert med[128.0] < 0.5, med


def emulate_act_mul(a, b, gelu, drop_tail=False):
    bf = b.float()
    if gelu:
        act = 0.5 * bf * (1.0 + torch.tanh(
            0.7978845608 * (bf + 0.044715 * bf * bf * bf)))
    else:
        act = _silu32(bf)
    y = _bf(a.float() * act)
    if drop_tail:
        flat = y.reshape(-1)
        flat[flat.numel() // 8 * 8:] = 0
    return y


@pytest.mark.parametrize("shape", kb.ACT_MUL_SHAPES, ids=str)
@pytest.mark.parametrize("gelu", [False, True])
def test_act_mul_emulation_inside_mutation_outside(shape, gelu):
    a, b = kb.act_mul_inputs(len(shape) + shape[0] % 1000, shape)
    ref, bound = kb.act_mul_ref(a, b, gelu)
    r = kb.err_ratio(emulate_act_mul(a, b, gelu), ref, bound)
    msg = f"act_mul {shape} gelu={gelu}: emulation {r:.3f}"
    assert r <= EMU_MAX, msg
    if a.numel() % 8:
        rm = kb.err_ratio(emulate_act_mul(a, b, gelu, drop_tail=True), ref,
                          bound)
        msg += f"  tail unwritten {rm:.0f}"
        assert rm > 1.0, msg
    print(msg)


# ---------------------------------------------------------------------------
# DiT glue ops: emulation <= 1.0 on every case, each seeded defect >= 2 on
# at least one case of its op
# ---------------------------------------------------------------------------

DEFECT_MIN = 2.0


def _xor_tree(p, skip=None):
    """What every lane of a group holds after the __shfl_xor butterfly over
    the last dim (a power of two); ``skip``: an offset whose level is lost."""
    g = p.shape[-1]
    lane = torch.arange(g)
    off = g // 2
    while off:
        if off != skip:
            p = p + p[..., lane ^ off]
        off //= 2
    return p


def emulate_qk_side(x, w, cos, sin, heads, eps, off, defect=None):
    """qk_norm_rope_kernel<G> on one side in fp32: a lane sums the squares of
    its 8 channels, width-G butterfly, rstd, y = x * rstd * w, rotation of
    the (2i, 2i+1) pairs, one bf16 store."""
    b, n, hd = x.shape
    d = hd // heads
    g = 2
    while g * 8 < d:
        g *= 2
    xf = x.float().reshape(b, n, heads, d)
    lanes = torch.zeros(b, n, heads, g * 8)
    lanes[..., :d] = xf
    lanes = lanes.reshape(b, n, heads, g, 8)
    if defect == "last lane of padded group":
        lanes[..., d // 8 - 1, :] = 0
    part = torch.zeros(b, n, heads, g)
    for j in range(8):
        part = part + lanes[..., j] * lanes[..., j]
    tot = _xor_tree(part, g // 2 if defect == "shuffle level" else None)
    e = torch.tensor(0.0 if defect == "eps dropped" else eps,
                     dtype=torch.float32)
    rstd = torch.rsqrt(tot / float(d) + e)
    y = xf * rstd.repeat_interleave(8, -1)[..., :d] * w.float()
    if defect == "norm rounded":
        y = _bf(y)
    first = 0 if defect == "table row n" else off
    c = cos[first:first + n].float()[None, :, None, :]
    s = sin[first:first + n].float()[None, :, None, :]
    if defect == "sin sign":
        s = -s
    out = torch.empty_like(y)
    if defect == "half pairs":
        y0, y1 = y[..., :d // 2], y[..., d // 2:]
        out[..., :d // 2] = y0 * c - y1 * s
        out[..., d // 2:] = y0 * s + y1 * c
    else:
        y0, y1 = y[..., 0::2], y[..., 1::2]
        out[..., 0::2] = y0 * c - y1 * s
        out[..., 1::2] = y0 * s + y1 * c
    return _bf(out).reshape(b, n, hd)


def _qk_ratio(name, defect=None):
    """max(err/bound) over q and k of one case."""
    inp = kb.qk_inputs(**kb.QK_CASES[name])
    out = []
    for side, (ref, bound) in zip("qk", kb.qk_refs(inp)):
        w = inp["wq"] if defect == "k with q's weight" else inp["w" + side]
        o = emulate_qk_side(inp[side], w, inp["cos"], inp["sin"],
                            inp["heads"], kb.QK_EPS, inp["off"], defect)
        out.append(kb.err_ratio(o, ref, bound))
    return max(out)


def _padded(case):
    return case["d"] // 8 & (case["d"] // 8 - 1) != 0


# defect -> which cases can show it
QK_DEFECTS = {
    "k with q's weight": lambda c: True,
    "table row n": lambda c: c["off"] > 0,
    "shuffle level": lambda c: True,
    "last lane of padded group": _padded,
    # without eps an all-zero head is 0 * inf
    "eps dropped": lambda c: c["amp"] < 1.0,
    "half pairs": lambda c: True,
    "sin sign": lambda c: True,
    "norm rounded": lambda c: True,
}


@pytest.mark.parametrize("name", kb.QK_CASES)
def test_qk_norm_rope_emulation_inside(name):
    r = _qk_ratio(name)
    print(f"qk_norm_rope {name}: emulation {r:.3f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("defect", QK_DEFECTS)
def test_qk_norm_rope_defect_outside(defect):
    rs = {n: _qk_ratio(n, defect) for n, c in kb.QK_CASES.items()
          if QK_DEFECTS[defect](c)}
    worst = max(rs, key=rs.get)
    print(f"qk_norm_rope defect '{defect}': {len(rs)} cases, err/bound "
          f"{min(rs.values()):.2f} .. {rs[worst]:.1f} ({worst})")
    assert rs[worst] >= DEFECT_MIN, rs


def emulate_norm_modulate(x, mode, w, scale, shift, eps=None, defect=None):
    """norm_modulate_kernel<ITERS, LAYER> in fp32, in its summation order:
    lane l owns the 8-channel chunks it*64 + l, adds their 8 values one after
    the other, then the xor butterfly over the 64 lanes. Layer mode takes the
    variance around the mean in a second pass over the same chunks."""
    if eps is None:
        eps = 1e-6 if mode == "rms" else 1e-5
    b, n, c = x.shape
    t = b * n
    iters = next(i for i in kb.NM_ITERS if i * 512 >= c)
    xf = x.float().reshape(t, c)
    live = torch.zeros(t, iters * 512)      # 1 where the statistics read
    live[:, :c] = 1
    if defect == "last chunk not in statistics":
        live[:, c - 8:c] = 0
    rows = torch.zeros(t, iters * 512)
    rows[:, :c] = xf
    live = live.reshape(t, iters, 64, 8)
    rows = rows.reshape(t, iters, 64, 8) * live

    def row_sum(v):
        acc = torch.zeros(t, 64)
        for it in range(iters):
            for j in range(8):
                acc = acc + v[:, it, :, j]
        return _xor_tree(acc)[:, :1]

    mean = torch.zeros(t, 1)
    if mode == "layer":
        mean = row_sum(rows) / c
        if defect == "one-pass variance":
            var = row_sum(rows * rows) / c - mean * mean
        else:
            dev = (rows - mean[:, :, None, None]) * live
            var = row_sum(dev * dev) / c
        rstd = torch.rsqrt(var + eps)
    else:
        rstd = torch.rsqrt(row_sum(rows * rows) / c + eps)
        if defect == "rms subtracts mean":
            mean = row_sum(rows) / c
    g = (xf - mean) * rstd
    if mode == "rms":
        g = g * w.float()
    if defect == "norm rounded":
        g = _bf(g)
    if scale is not None:
        sc, sh = scale.float(), shift.float()
        if defect == "batch 0 modulation":
            sc, sh = sc[:1].expand(b, c), sh[:1].expand(b, c)
        if defect == "scale and shift swapped":
            sc, sh = sh, sc
        sc = sc.repeat_interleave(n, 0)
        sh = sh.repeat_interleave(n, 0)
        g = g * (sc if defect == "scale for 1 + scale" else 1.0 + sc) + sh
    return _bf(g).reshape(b, n, c)


def _nm_ratio(case, defect=None, modulated=True):
    inp = kb.nm_inputs(**case)
    sc, sh = (inp["scale"], inp["shift"]) if modulated else (None, None)
    ref, bound = kb.norm_modulate_ref(inp["x"], inp["mode"], inp["w"], sc, sh)
    out = emulate_norm_modulate(inp["x"], inp["mode"], inp["w"], sc, sh,
                                defect=defect)
    return kb.err_ratio(out, ref, bound)


NM_DEFECTS = {
    "batch 0 modulation": lambda c: c["b"] > 1,
    "scale and shift swapped": lambda c: True,
    "scale for 1 + scale": lambda c: True,
    "last chunk not in statistics": lambda c: c["c"] == 1032,
    "norm rounded": lambda c: c["c"] >= 72 and not c["const"],
    "one-pass variance": lambda c: c["mode"] == "layer" and c["mean"] == 128.0,
    "rms subtracts mean": lambda c: c["mode"] == "rms",
}


@pytest.mark.parametrize("name", kb.NM_CASES)
def test_norm_modulate_emulation_inside(name):
    case = kb.NM_CASES[name]
    r = _nm_ratio(case)
    rp = _nm_ratio(case, modulated=False)
    print(f"norm_modulate {name}: emulation modulated {r:.3f} plain {rp:.3f}")
    assert r <= 1.0 and rp <= 1.0, (r, rp)


# (mean, std): the range over which the mean term of the layer bound has to
# carry the fp32 mean, and the rms sum of squares its large common part
NM_OFFSETS = [(0.0, 1.0), (4.0, 1.0), (32.0, 1.0), (128.0, 1.0), (256.0, 2.0)]


@pytest.mark.parametrize("mode", ["rms", "layer"])
@pytest.mark.parametrize("c", [8, 520, 1032, 3072, 8192])
def test_norm_modulate_emulation_offset_sweep(mode, c):
    rs = {}
    for mean, std in NM_OFFSETS:
        case = dict(b=2, n=3, c=c, mode=mode, seed=c + int(mean), mean=mean,
                    std=std)
        rs[(mean, std)] = max(_nm_ratio(case), _nm_ratio(case, modulated=False))
    print(f"norm_modulate {mode} C={c} (mean, std) sweep: " +
          "  ".join(f"{k} {v:.3f}" for k, v in rs.items()))
    assert max(rs.values()) <= 1.0, rs


def test_layer_bound_needs_its_mean_term():
    """Without the mean term the faithful fp32 evaluation leaves the bound at
    mean/std = 128: the term is there for the kernel, not for slack."""
    worst = 0.0
    for c in (512, 1032, 3072):
        inp = kb.nm_inputs(**kb.NM_CASES[f"layer_C{c}_mean128"])
        ref, _ = kb.norm_modulate_ref(inp["x"], "layer", None, inp["scale"],
                                      inp["shift"])
        gain = (1.0 + inp["scale"].double())[:, None]
        xd = inp["x"].double()
        rstd = 1.0 / (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
        mag = ((xd - xd.mean(-1, keepdim=True)) * rstd * gain).abs() \
            + inp["shift"].double().abs()[:, None]
        out = emulate_norm_modulate(inp["x"], "layer", None, inp["scale"],
                                    inp["shift"])
        worst = max(worst, kb.err_ratio(out, ref,
                                        kb.hulp(ref) + kb.FP32_FLOOR * mag))
    print(f"layer mean 128, bound without the mean term: emulation {worst:.2f}")
    assert worst > 1.0, worst


@pytest.mark.parametrize("defect", NM_DEFECTS)
def test_norm_modulate_defect_outside(defect):
    rs = {n: _nm_ratio(c, defect) for n, c in kb.NM_CASES.items()
          if NM_DEFECTS[defect](c)}
    worst = max(rs, key=rs.get)
    print(f"norm_modulate defect '{defect}': {len(rs)} cases, err/bound "
          f"{min(rs.values()):.2f} .. {rs[worst]:.1f} ({worst})")
    assert rs[worst] >= DEFECT_MIN, rs


def test_mean3_std05_does_not_expose_one_pass_variance():
    """The recipe of test_norm_modulate (mean 3 / std 0.5, mean/std = 6) is
    inside the bound with a one-pass variance too; it takes mean/std of 32
    or more, hence the mean-128 cases."""
    for c in kb.NM_OLD_C:
        r = _nm_ratio(kb.NM_CASES[f"layer_C{c}_mean3"], "one-pass variance")
        print(f"layer C={c} mean 3 / std 0.5, one-pass variance: {r:.3f}")
        assert r <= 1.0, (c, r)


def emulate_gated_residual(x, gate, y, defect=None):
    g = gate.float()
    if defect == "batch 0 gate":
        g = g[:1].expand_as(g)
    prod = g[:, None] * y.float()
    if defect == "product rounded":
        prod = _bf(prod)
    out = _bf(x.float() + prod)
    if defect == "last chunk unwritten":
        out.reshape(-1)[-8:] = 0
    return out


GR_DEFECTS = {
    "product rounded": lambda name: True,
    "batch 0 gate": lambda name: kb.GR_CASES[name][0] > 1,
    "last chunk unwritten": lambda name: True,
}


@pytest.mark.parametrize("name", kb.GR_CASES)
def test_gated_residual_emulation_inside(name):
    x, gate, y = kb.gr_inputs(name)
    ref, bound = kb.gated_residual_ref(x, gate, y)
    r = kb.err_ratio(emulate_gated_residual(x, gate, y), ref, bound)
    print(f"gated_residual {name}: emulation {r:.3f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("defect", GR_DEFECTS)
def test_gated_residual_defect_outside(defect):
    rs = {}
    for name in kb.GR_CASES:
        if name == "second_trip" or not GR_DEFECTS[defect](name):
            continue   # the small cases suffice
        x, gate, y = kb.gr_inputs(name)
        ref, bound = kb.gated_residual_ref(x, gate, y)
        rs[name] = kb.err_ratio(emulate_gated_residual(x, gate, y, defect),
                                ref, bound)
    worst = max(rs, key=rs.get)
    print(f"gated_residual defect '{defect}': err/bound "
          f"{min(rs.values()):.2f} .. {rs[worst]:.1f} ({worst})")
    assert rs[worst] >= DEFECT_MIN, rs
