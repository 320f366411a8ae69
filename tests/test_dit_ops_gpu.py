"""DiT glue kernels (ops/hip/dit_ops.hip) on the GPU.

Reference for every op test: the dispatch CPU path on the bf16-rounded inputs
upcast to fp32, so the reference carries no intermediate rounding. One bound
for all of them:

    |gpu - ref| <= 2^-8 * |ref| + 1e-4 * max|ref|

bf16 keeps 8 significand bits, so the single RNE rounding on store is at most
2^-9 relative; 2^-8 leaves one ulp for fp32 values that straddle a rounding
boundary. The absolute term covers fp32 cancellation in the rotation (about
1e-7 x operand magnitude x a few ops) and stays far below any indexing error.

The second half of the file puts every kernel instantiation, the stride and
batch layouts the models use and the shapes above through the fp64 references
and the single-rounding bound of kernel_bounds.py (half a bf16 ulp of the
reference plus an fp32 floor); the case lists live there so that
test_kernel_bounds_cpu.py runs the same recipes through a CPU emulation.
"""

import pytest
import torch

import kernel_bounds as kb
from comfyui_distributed_amd.ops import dispatch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16


def _check(gpu: torch.Tensor, ref: torch.Tensor, what: str):
    gpu = gpu.float().cpu()
    assert gpu.shape == ref.shape, (what, gpu.shape, ref.shape)
    assert torch.isfinite(gpu).all(), what
    err = (gpu - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-4 * ref.abs().max()
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max|ref| "
          f"{ref.abs().max().item():.3e}, worst (err - bound) {worst:.3e}")
    assert (err <= bound).all(), f"{what}: exceeds bound by {worst}"


def _qk_inputs(b, n, h, d, npos, seed):
    """bf16 q/k as chunks of one [B, N, 3HD] tensor, distinct fp32 weights,
    random angles per (position, pair)."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(b, n, 3 * h * d, generator=g).to(BF)
    wq = torch.randn(d, generator=g)
    wk = torch.randn(d, generator=g)
    ang = torch.rand(npos, d // 2, generator=g) * 6.28
    return qkv, wq, wk, ang.cos(), ang.sin()


@pytest.mark.parametrize("b,n,h,d", [(2, 5, 2, 32), (2, 5, 3, 64),
                                     (1, 7, 5, 128), (2, 3, 2, 96)])
def test_qk_norm_rope(b, n, h, d):
    qkv, wq, wk, cos, sin = _qk_inputs(b, n, h, d, n, seed=d)
    q, k, _ = qkv.float().chunk(3, dim=-1)
    ref_q, ref_k = dispatch.qk_norm_rope(q, k, wq, wk, cos, sin, h, 1e-6)

    gq, gk, _ = qkv.to(DEV).chunk(3, dim=-1)
    assert not gq.is_contiguous()
    out_q, out_k = dispatch.qk_norm_rope(
        gq, gk, wq.to(DEV), wk.to(DEV), cos.to(DEV), sin.to(DEV), h, 1e-6)
    assert out_q.dtype == BF and out_q.is_contiguous()
    _check(out_q, ref_q, f"q {b, n, h, d}")
    _check(out_k, ref_k, f"k {b, n, h, d}")
    # the two weights differ, so swapped sides cannot both pass
    assert not torch.allclose(ref_q, ref_k)


def test_qk_norm_rope_token_offset_keeps_other_rows():
    b, n, h, d, off = 2, 5, 3, 64, 4
    ntot = n + 6
    qkv, wq, wk, cos, sin = _qk_inputs(b, n, h, d, ntot, seed=9)
    q, k, _ = qkv.float().chunk(3, dim=-1)
    sentinel = -77.0
    ref = (torch.full((b, ntot, h * d), sentinel),
           torch.full((b, ntot, h * d), sentinel))
    dispatch.qk_norm_rope(q, k, wq, wk, cos, sin, h, 1e-6,
                          token_offset=off, out=ref)

    gq, gk, _ = qkv.to(DEV).chunk(3, dim=-1)
    out = (torch.full((b, ntot, h * d), sentinel, device=DEV, dtype=BF),
           torch.full((b, ntot, h * d), sentinel, device=DEV, dtype=BF))
    dispatch.qk_norm_rope(gq, gk, wq.to(DEV), wk.to(DEV), cos.to(DEV),
                          sin.to(DEV), h, 1e-6, token_offset=off, out=out)
    for o, r, name in zip(out, ref, "qk"):
        o = o.float().cpu()
        assert (o[:, :off] == sentinel).all(), name
        assert (o[:, off + n:] == sentinel).all(), name
        _check(o[:, off:off + n], r[:, off:off + n], f"{name} window")
    # rotated by table rows off.., not 0..: the offset-0 result differs
    ref0, _ = dispatch.qk_norm_rope(q, k, wq, wk, cos, sin, h, 1e-6)
    assert not torch.allclose(ref0, ref[0][:, off:off + n])


def test_qk_norm_rope_copies_unaligned_views():
    """A view whose start is not a multiple of 8 elements goes through a
    contiguous copy in dispatch instead of reaching the kernel."""
    b, n, h, d = 1, 3, 2, 32
    g = torch.Generator().manual_seed(3)
    base = torch.randn(b, n, 2 * h * d + 4, generator=g).to(BF)
    q, k = base[..., 4:4 + h * d], base[..., 4 + h * d:]
    w = torch.randn(d, generator=g)
    ang = torch.rand(n, d // 2, generator=g)
    cos, sin = ang.cos(), ang.sin()
    ref_q, ref_k = dispatch.qk_norm_rope(q.float(), k.float(), w, -w, cos,
                                         sin, h)
    gb = base.to(DEV)
    out_q, out_k = dispatch.qk_norm_rope(
        gb[..., 4:4 + h * d], gb[..., 4 + h * d:], w.to(DEV), -w.to(DEV),
        cos.to(DEV), sin.to(DEV), h)
    _check(out_q, ref_q, "q unaligned")
    _check(out_k, ref_k, "k unaligned")


@pytest.mark.parametrize("mode", ["rms", "layer"])
@pytest.mark.parametrize("c", [64, 72, 3072, 5120])
def test_norm_modulate(mode, c):
    b, n = 2, 7
    g = torch.Generator().manual_seed(c)
    # mean 3 / std 0.5: an offset of 6 std, so a mean taken for 0 or left out
    # of the normalise pass shows. It does not expose a one-pass variance
    # (sumsq - mean^2): by CPU emulation that stays inside any sensible bound
    # until mean/std is about 32; the mean-128 cases of
    # test_norm_modulate_bound are the ones that would catch it.
    x = (torch.randn(b, n, c, generator=g) * 0.5 + 3.0).to(BF)
    m = torch.randn(b, 6, c, generator=g).to(BF)
    w = torch.randn(c, generator=g) if mode == "rms" else None
    shift, scale = m.float().unbind(1)[3:5]
    ref = dispatch.norm_modulate(x.float(), mode, w, scale, shift)
    ref_plain = dispatch.norm_modulate(x.float(), mode, w)

    gm = m.to(DEV)
    gshift, gscale = gm.unbind(1)[3:5]
    gw = w.to(DEV) if w is not None else None
    y = dispatch.norm_modulate(x.to(DEV), mode, gw, gscale, gshift)
    assert y.dtype == BF
    _check(y, ref, f"{mode} C={c} modulated")
    _check(dispatch.norm_modulate(x.to(DEV), mode, gw), ref_plain,
           f"{mode} C={c} plain")
    # per-batch modulation: batch 1 must not have used batch 0's rows
    assert not torch.allclose(scale[0], scale[1])


def test_rms_norm_head_split_view():
    """rms_norm over the last dim of a 4-D head-split tensor."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 5, 3, 64, generator=g).to(BF)
    w = torch.randn(64, generator=g)
    ref = dispatch.rms_norm(x.float(), w, 1e-6)
    _check(dispatch.rms_norm(x.to(DEV), w.to(DEV), 1e-6), ref, "rms_norm 4-D")


def test_gated_residual():
    b, n, c = 2, 9, 72
    g = torch.Generator().manual_seed(2)
    x = torch.randn(b, n, c, generator=g).to(BF)
    y = torch.randn(b, n, c, generator=g).to(BF)
    m = torch.randn(b, 6, c, generator=g).to(BF)
    ref = dispatch.gated_residual(x.float(), m.float().unbind(1)[2], y.float())
    gate = m.to(DEV).unbind(1)[2]
    assert not gate.is_contiguous()
    out = dispatch.gated_residual(x.to(DEV), gate, y.to(DEV))
    assert out.dtype == BF
    _check(out, ref, "gated_residual")


def test_switch_off_runs_eager_sequence(monkeypatch):
    """_DIT_FUSED off: device tensors take the torch sequence of the CPU
    path (bf16 intermediates), the baseline kept for A/B."""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 9, 72, generator=g).to(BF)
    y = torch.randn(2, 9, 72, generator=g).to(BF)
    gate = torch.randn(2, 72, generator=g).to(BF)
    monkeypatch.setattr(dispatch, "_DIT_FUSED", False)
    out = dispatch.gated_residual(x.to(DEV), gate.to(DEV), y.to(DEV))
    assert torch.equal(out.cpu(), x + gate[:, None] * y)


def test_uncovered_shapes_and_dtypes_keep_torch_semantics():
    """Widths the kernels do not cover (C % 8 != 0) and mixed dtypes (an
    fp32 gate / scale beside a bf16 x, where torch promotes) run the torch
    sequence on device, as the models' inline code did."""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 5, 70, generator=g).to(BF).to(DEV)
    y = torch.randn(2, 5, 70, generator=g).to(BF).to(DEV)
    gate = torch.randn(2, 70, generator=g).to(BF).to(DEV)
    w = torch.randn(70, generator=g).to(DEV)
    assert torch.equal(dispatch.gated_residual(x, gate, y),
                       x + gate[:, None] * y)
    out = dispatch.norm_modulate(x, "layer", None, gate, gate)
    ln = torch.nn.functional.layer_norm(x, (70,))
    assert torch.equal(out, ln * (1 + gate[:, None]) + gate[:, None])
    assert dispatch.rms_norm(x, w).shape == x.shape

    x8 = torch.randn(2, 5, 72, generator=g).to(BF).to(DEV)
    y8 = torch.randn(2, 5, 72, generator=g).to(BF).to(DEV)
    gate32 = torch.randn(2, 72, generator=g).to(DEV)
    out = dispatch.gated_residual(x8, gate32, y8)
    assert out.dtype == torch.float32
    assert torch.equal(out, x8 + gate32[:, None] * y8)
    out = dispatch.norm_modulate(x8, "layer", None, gate32, gate32)
    assert out.dtype == torch.float32


# ---------------------------------------------------------------------------
# fp64 references and the single-rounding bound (kernel_bounds.py)
# ---------------------------------------------------------------------------

SENTINEL = -77.0


def _run_qk(inp, gq, gk, out=None):
    return dispatch.qk_norm_rope(
        gq, gk, inp["wq"].to(DEV), inp["wk"].to(DEV), inp["cos"].to(DEV),
        inp["sin"].to(DEV), inp["heads"], kb.QK_EPS,
        token_offset=inp["off"], out=out)


@pytest.mark.parametrize("name", kb.QK_CASES)
def test_qk_norm_rope_bound(name):
    case = kb.QK_CASES[name]
    inp = kb.qk_inputs(**case)
    refs = kb.qk_refs(inp)
    b, n, hd = inp["q"].shape
    off = inp["off"]
    out = None
    if off:
        out = tuple(torch.full((b, inp["ntot"], hd), SENTINEL, device=DEV,
                               dtype=BF) for _ in range(2))
    gq, gk = kb.qk_place(inp["q"], inp["k"], case["layout"], DEV)
    if case["layout"] == "k_separate":
        assert gq.stride() != gk.stride()
    if case["layout"] == "row_slice":
        assert gq.stride(0) != n * gq.stride(1)
    outs = _run_qk(inp, gq, gk, out)
    for o, (ref, bound), side in zip(outs, refs, "qk"):
        assert o.dtype == BF and o.is_contiguous()
        if off:
            assert (o[:, :off] == SENTINEL).all(), side
            assert (o[:, off + n:] == SENTINEL).all(), side
            o = o[:, off:off + n]
        kb.check(o, ref, bound, f"qk_norm_rope {name} {side}")
        if case["zero_head"] is not None:
            d = hd // inp["heads"]
            head = o.reshape(b, n, inp["heads"], d)[:, :, case["zero_head"]]
            assert torch.isfinite(head).all() and (head == 0).all(), side


def test_qk_norm_rope_two_calls_fill_one_buffer():
    """Flux double block: the text stream's q/k go to rows [0, Ntxt) and the
    image stream's to [Ntxt, Ntxt + Nimg) of one buffer. Against the fp64
    reference of the concatenated input; no row keeps the sentinel."""
    b, ntxt, nimg, h, d = 2, 3, 5, 3, 128
    txt = kb.qk_inputs(b, ntxt, h, d, seed=41)
    img = kb.qk_inputs(b, nimg, h, d, seed=42)
    both = kb.qk_inputs(b, ntxt + nimg, h, d, seed=43)   # weights, tables
    both["q"] = torch.cat([txt["q"], img["q"]], dim=1)
    both["k"] = torch.cat([txt["k"], img["k"]], dim=1)
    both["ntot"] = ntxt + nimg
    out = tuple(torch.full((b, ntxt + nimg, h * d), SENTINEL, device=DEV,
                           dtype=BF) for _ in range(2))
    for part, off in ((txt, 0), (img, ntxt)):
        part.update({key: both[key] for key in ("wq", "wk", "cos", "sin")},
                    off=off)
        _run_qk(part, *kb.qk_place(part["q"], part["k"], "flux_split", DEV),
                out)
    for o, (ref, bound), side in zip(out, kb.qk_refs(both), "qk"):
        assert (o != SENTINEL).all(), side
        kb.check(o, ref, bound, f"qk_norm_rope two calls {side}")


@pytest.mark.parametrize("name", kb.NM_CASES)
def test_norm_modulate_bound(name):
    case = kb.NM_CASES[name]
    inp = kb.nm_inputs(**case)
    x, mode, w = inp["x"], inp["mode"], inp["w"]
    gx = x.to(BF).to(DEV)
    gw = w.to(DEV) if w is not None else None
    gsc, gsh = kb.mod_place(inp["scale"], inp["shift"], case["layout"], DEV)
    assert gsc.stride(0) != x.shape[-1]
    assert (case["layout"] == "mixed") == (gsc.stride() != gsh.stride())

    y = dispatch.norm_modulate(gx, mode, gw, gsc, gsh)
    assert y.dtype == BF and y.shape == x.shape
    ref, bound = kb.norm_modulate_ref(x, mode, w, inp["scale"], inp["shift"])
    kb.check(y, ref, bound, f"norm_modulate {name} modulated")
    y_plain = dispatch.norm_modulate(gx, mode, gw)
    ref, bound = kb.norm_modulate_ref(x, mode, w)
    kb.check(y_plain, ref, bound, f"norm_modulate {name} plain")
    if case["const"]:
        # x - mean is exactly 0: the fp32 sum of at most 8192 copies of a
        # bf16 value is exact, and so is its quotient by C
        want = inp["shift"].to(BF)[:, None].expand_as(y)
        assert torch.equal(y.cpu(), want)
        assert (y_plain == 0).all()


def test_rms_norm_head_split_view_bound():
    g = torch.Generator().manual_seed(1)
    x = kb.bf16_exact(torch.randn(2, 5, 3, 64, generator=g))
    w = torch.randn(64, generator=g)
    ref, bound = kb.norm_modulate_ref(x.reshape(1, -1, 64), "rms", w)
    y = dispatch.rms_norm(x.to(BF).to(DEV), w.to(DEV), 1e-6)
    assert y.shape == x.shape and y.dtype == BF
    kb.check(y.reshape(1, -1, 64), ref, bound, "rms_norm 4-D")


def test_norm_modulate_above_8192_keeps_torch_semantics():
    """C = 8200 is past the widest instantiation: the torch sequence runs on
    device, bit for bit what the models' inline code gave."""
    g = torch.Generator().manual_seed(8)
    c = 8200
    x = torch.randn(2, 3, c, generator=g).to(BF).to(DEV)
    scale = torch.randn(2, c, generator=g).to(BF).to(DEV)
    shift = torch.randn(2, c, generator=g).to(BF).to(DEV)
    w = torch.randn(c, generator=g).to(DEV)
    ln = torch.nn.functional.layer_norm(x, (c,))
    assert torch.equal(dispatch.norm_modulate(x, "layer", None, scale, shift),
                       ln * (1 + scale[:, None]) + shift[:, None])
    assert torch.equal(dispatch.norm_modulate(x, "layer"), ln)
    xf = x.float()
    rms = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)
           * w.float()).to(BF)
    assert torch.equal(dispatch.norm_modulate(x, "rms", w, scale, shift),
                       rms * (1 + scale[:, None]) + shift[:, None])
    assert torch.equal(dispatch.rms_norm(x, w), rms)


@pytest.mark.parametrize("name", kb.GR_CASES)
def test_gated_residual_bound(name):
    x, gate, y = kb.gr_inputs(name)
    layout = kb.GR_CASES[name][3]
    ggate = kb.gate_place(gate, layout, DEV)
    assert ggate.stride(0) != x.shape[-1]
    if layout == "offset":
        assert ggate.storage_offset() > 0
    out = dispatch.gated_residual(x.to(BF).to(DEV), ggate, y.to(BF).to(DEV))
    assert out.dtype == BF
    ref, bound = kb.gated_residual_ref(x, gate, y)
    kb.check(out, ref, bound, f"gated_residual {name}")


# ---------------------------------------------------------------------------
# model level: fused vs eager glue against the CPU fp32 forward
# ---------------------------------------------------------------------------


def _rel_err(out_gpu, out_cpu):
    err = (out_gpu.float().cpu() - out_cpu).abs().max().item()
    return err / out_cpu.abs().max().item()


def _model_errors(name, make_inputs, t_dtype, monkeypatch):
    """inputs[1] are the timesteps (100 and 700: exact in bf16 too); the
    samplers hand them to WAN in fp32 and to Flux in the model dtype."""
    from comfyui_distributed_amd.models import create_diffusion_stack

    cpu = create_diffusion_stack(name, device="cpu", dtype=torch.float32, seed=5)
    gpu = create_diffusion_stack(name, device=DEV, dtype=BF, seed=5)
    inputs = make_inputs(cpu)
    dev_inputs = [t.to(DEV, t_dtype if i == 1 else BF)
                  for i, t in enumerate(inputs)]
    errs = {}
    with torch.no_grad():
        ref = cpu.model(*inputs)
        for fused in (True, False):
            monkeypatch.setattr(dispatch, "_DIT_FUSED", fused)
            out = gpu.model(*dev_inputs)
            assert torch.isfinite(out).all()
            errs[fused] = _rel_err(out, ref)
    print(f"{name}: rel max err vs CPU fp32: fused {errs[True]:.5f}, "
          f"eager {errs[False]:.5f}")
    return errs[True], errs[False]


def test_wan_tiny_fused_no_worse_than_eager(monkeypatch):
    def make_inputs(stack):
        g = torch.Generator().manual_seed(11)
        return [torch.randn(2, 4, 3, 8, 8, generator=g),
                torch.tensor([100.0, 700.0]),
                torch.randn(2, 12, stack.model.cfg.text_dim, generator=g)]

    fused, eager = _model_errors("wan_tiny", make_inputs, torch.float32,
                                 monkeypatch)
    assert fused <= 1.5 * eager, (fused, eager)


def test_flux_tiny_fused_no_worse_than_eager(monkeypatch):
    def make_inputs(stack):
        g = torch.Generator().manual_seed(12)
        return [torch.randn(2, 16, 8, 8, generator=g),
                torch.tensor([100.0, 700.0]),
                torch.randn(2, 12, stack.cfg.context_dim, generator=g),
                torch.randn(2, stack.cfg.vec_dim, generator=g)]

    fused, eager = _model_errors("flux_tiny", make_inputs, BF, monkeypatch)
    assert fused <= 1.5 * eager, (fused, eager)
