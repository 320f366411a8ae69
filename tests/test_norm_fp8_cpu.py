"""norm_modulate_fp8 / Fp8Rows without a GPU: the CPU dispatch path is the
two-step composition bit for bit, linear_fp8 takes Fp8Rows, the bound of
norm_fp8_bounds.py holds for an fp32 emulation of the kernel and rejects
seeded defects, and the WAN / Flux blocks hand Fp8Rows to exactly the
Linears a norm feeds, with unchanged outputs.

Measured here (CPU): emulation at 0.9993-0.9997 of the bound; absmax without
the last chunk 29-108 bounds, a neighbour's scale 155-196, the previous
batch's modulation above 28 000, truncation 1.9-2.0.
"""

import pytest
import torch

import fp8_bounds as fb
import kernel_bounds as kb
import norm_fp8_bounds as nb
from comfyui_distributed_amd import ops as ops_pkg
from comfyui_distributed_amd.models import quant
from comfyui_distributed_amd.models.quant import Fp8Linear, quantize_linears
from comfyui_distributed_amd.ops import dispatch
from comfyui_distributed_amd.ops.dispatch import Fp8Rows

FP8 = torch.float8_e4m3fn


def _bytes(t):
    return t.view(torch.uint8)


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------


def test_exported():
    for name in ("Fp8Rows", "quantize_rows", "norm_modulate_fp8"):
        assert getattr(ops_pkg, name) is getattr(dispatch, name)


@pytest.mark.parametrize("b,n,c", [(2, 7, 128), (3, 3, 640)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode,modulated", nb.MODES)
def test_cpu_dispatch_is_the_composition(b, n, c, dtype, mode, modulated):
    inp = kb.nm_inputs(b, n, c, mode, seed=c)
    x = inp["x"].to(dtype)
    sc, sh = ((inp["scale"].to(dtype), inp["shift"].to(dtype)) if modulated
              else (None, None))
    rows = dispatch.norm_modulate_fp8(x, mode, inp["w"], sc, sh)
    y = dispatch.norm_modulate(x, mode, inp["w"], sc, sh)
    q, s = dispatch.quant_rows_fp8(y.reshape(-1, c))
    assert isinstance(rows, Fp8Rows)
    assert rows.q.shape == (b, n, c) and rows.q.dtype == FP8
    assert rows.q.is_contiguous()
    assert rows.scale.shape == (b, n) and rows.scale.dtype == torch.float32
    assert rows.dtype == y.dtype == dtype
    assert torch.equal(_bytes(rows.q).reshape(-1, c), _bytes(q))
    assert torch.equal(rows.scale.reshape(-1), s)
    with pytest.raises(Exception):       # immutable
        rows.q = q


def test_norm_modulate_fp8_errors():
    w = torch.ones(128)
    x = torch.randn(2, 3, 128)
    m = torch.randn(2, 128)
    for c in (64, 16512):
        with pytest.raises(ValueError, match="unsupported"):
            dispatch.norm_modulate_fp8(torch.zeros(1, 2, c), "layer")
    # the argument errors of norm_modulate
    for args in (("group", None), ("rms", None), ("layer", w)):
        with pytest.raises(ValueError):
            dispatch.norm_modulate(x, *args)
        with pytest.raises(ValueError):
            dispatch.norm_modulate_fp8(x, *args)
    with pytest.raises(ValueError, match="come together"):
        dispatch.norm_modulate_fp8(x, "rms", w, scale=m)
    with pytest.raises(ValueError, match="come together"):
        dispatch.norm_modulate_fp8(x, "layer", shift=m)


def test_quantize_rows_and_linear_fp8_rows():
    m, n, k = 15, 130, 384
    x, w, bias = fb.linear_inputs(m, n, k, seed=5)
    x3 = x.reshape(3, 5, k)
    rows = dispatch.quantize_rows(x3)
    q, s = dispatch.quant_rows_fp8(x)
    assert rows.q.shape == (3, 5, k) and rows.scale.shape == (3, 5)
    assert rows.dtype == torch.float32
    assert torch.equal(_bytes(rows.q).reshape(m, k), _bytes(q))
    assert torch.equal(rows.scale.reshape(m), s)
    with pytest.raises(ValueError):
        dispatch.quantize_rows(torch.zeros(2, 3, 64))       # K contract

    qw, sw = dispatch.quantize_weight_fp8(w)
    for act in fb.ACTS:
        y_rows = dispatch.linear_fp8(rows, qw, sw, bias, act)
        y = dispatch.linear_fp8(x3, qw, sw, bias, act)
        assert y_rows.shape == (3, 5, n) and y_rows.dtype == torch.float32
        assert torch.equal(y_rows, y)
    bf_rows = Fp8Rows(rows.q, rows.scale, torch.bfloat16)
    assert dispatch.linear_fp8(bf_rows, qw, sw).dtype == torch.bfloat16
    with pytest.raises(ValueError):
        dispatch.linear_fp8(rows, qw[:, :256].contiguous(), sw)   # K mismatch


def test_linear_fp8_rows_runs_no_quantiser(monkeypatch):
    x, w, _ = fb.linear_inputs(4, 128, 128, seed=6)
    qw, sw = dispatch.quantize_weight_fp8(w)
    rows = dispatch.quantize_rows(x)
    gemms = []
    real = dispatch.gemm_fp8

    def no_quant(*a, **k):
        raise AssertionError("quantiser called for Fp8Rows")

    def counted(*a, **k):
        gemms.append(1)
        return real(*a, **k)

    monkeypatch.setattr(dispatch, "quant_rows_fp8", no_quant)
    monkeypatch.setattr(dispatch, "gemm_fp8", counted)
    dispatch.linear_fp8(rows, qw, sw)
    assert len(gemms) == 1


# ---------------------------------------------------------------------------
# bound: emulation inside, seeded defects outside
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("mode,modulated", [("rms", True), ("rms", False),
                                            ("layer", True), ("layer", False)])
def test_emulation_inside_bound(mode, modulated):
    worst = 0.0
    for c, kw in nb.CPU_CASES:
        inp = kb.nm_inputs(3, 3, c, mode, seed=c + len(kw), **kw)
        h, eh = nb.reference(inp, modulated)
        q, s = nb.emulate(inp, modulated)
        worst = max(worst, nb.check(q, s, h, eh,
                                    f"emulation {mode} mod={modulated} C={c} {kw}"))
    print(f"emulation {mode} mod={modulated}: worst {worst:.4f}")


def _defect_inputs(mode):
    """tail=8 at C = 1152, B = 3; batch 1's gain is 8x the others', so rows of
    neighbouring batches differ in magnitude."""
    inp = kb.nm_inputs(3, 3, 1152, mode, seed=77, tail=8.0)
    inp["scale"][1] = inp["scale"][1] * 8.0 + 8.0
    return inp


@pytest.mark.parametrize("mode", ["rms", "layer"])
@pytest.mark.parametrize("defect", ["amax without tail", "neighbour scale",
                                    "previous batch", "truncation"])
def test_seeded_defects_leave_bound(mode, defect):
    inp = _defect_inputs(mode)
    h, eh = nb.reference(inp)
    q, s = nb.emulate(inp)
    nb.check(q, s, h, eh, f"clean {mode}")
    q, s = nb.emulate(inp, defect=defect)
    r = nb.value_ratio(q, s, h, eh)
    ok = nb.scale_ok(s, h, eh)
    print(f"defect '{defect}' {mode}: scale inside {ok}, err/bound {r:.1f}")
    assert nb.outside(q, s, h, eh)
    if defect == "truncation":      # the scale is right, the values are not
        assert ok and r > 1.5
    if defect == "amax without tail":
        assert r > 10


# ---------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------


def _record_inputs(module, names=None):
    """name -> list of first forward arguments, for every Fp8Linear."""
    seen = {}
    for name, m in module.named_modules():
        if isinstance(m, Fp8Linear):
            seen[name] = []
            m.register_forward_pre_hook(
                lambda mod, args, _l=seen[name]: _l.append(args[0]))
    return seen


def _rows_names(seen):
    return {n for n, xs in seen.items() if any(isinstance(x, Fp8Rows) for x in xs)}


def _wan_cfg(layers=1):
    from comfyui_distributed_amd.models.wan import WanConfig

    return WanConfig(dim=128, ffn_dim=256, num_layers=layers, num_heads=2,
                     text_dim=128, in_channels=4, out_channels=4)


def _wan_block_run(blk, flag, monkeypatch):
    from comfyui_distributed_amd.models.wan import rope_3d

    monkeypatch.setattr(quant, "FP8_FUSED_NORM", flag)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 12, 128, generator=g)
    emb6 = torch.randn(2, 6, 128, generator=g) * 0.1
    ctx = torch.randn(2, 5, 128, generator=g)
    with torch.no_grad():
        return blk(x, emb6, ctx, rope_3d(1, 3, 4, 64, "cpu"))


def test_wan_block_routing(monkeypatch):
    from comfyui_distributed_amd.models.wan import WanBlock

    torch.manual_seed(0)
    blk = WanBlock(_wan_cfg()).eval()
    assert quantize_linears(blk) == 10
    seen = _record_inputs(blk)
    y_on = _wan_block_run(blk, True, monkeypatch)
    assert all(len(xs) == 1 for xs in seen.values())
    assert _rows_names(seen) == {"q", "k", "v", "cq", "ffn1"}
    assert seen["q"][0] is seen["k"][0] is seen["v"][0]
    for name in ("o", "ck", "cv", "co", "ffn2"):
        assert isinstance(seen[name][0], torch.Tensor)
    for xs in seen.values():
        xs.clear()
    y_off = _wan_block_run(blk, False, monkeypatch)
    assert not _rows_names(seen)
    assert torch.equal(y_on, y_off)


def test_wan_block_vetoed_consumer_keeps_bf16(monkeypatch):
    from comfyui_distributed_amd.models.wan import WanBlock

    torch.manual_seed(0)
    blk = WanBlock(_wan_cfg()).eval()
    assert quantize_linears(blk, lambda name, lin: name != "k") == 9
    seen = _record_inputs(blk)
    y_on = _wan_block_run(blk, True, monkeypatch)
    assert _rows_names(seen) == {"cq", "ffn1"}
    assert isinstance(seen["q"][0], torch.Tensor)
    assert isinstance(seen["v"][0], torch.Tensor)
    assert torch.equal(y_on, _wan_block_run(blk, False, monkeypatch))


def test_wan_model_quantises_context_once(monkeypatch):
    from comfyui_distributed_amd.models.wan import WanModel

    torch.manual_seed(0)
    model = WanModel(_wan_cfg(layers=2)).eval()
    assert quantize_linears(model) == 20
    seen = _record_inputs(model)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 4, 1, 6, 8, generator=g)
    t = torch.tensor([300.0])
    ctx = torch.randn(1, 5, 128, generator=g)
    monkeypatch.setattr(quant, "FP8_FUSED_NORM", True)
    with torch.no_grad():
        y_on = model(x, t, ctx)
    ctx_rows = seen["blocks.0.ck"][0]
    assert isinstance(ctx_rows, Fp8Rows)
    for name in ("blocks.0.cv", "blocks.1.ck", "blocks.1.cv"):
        assert seen[name][0] is ctx_rows
    monkeypatch.setattr(quant, "FP8_FUSED_NORM", False)
    for xs in seen.values():
        xs.clear()
    with torch.no_grad():
        y_off = model(x, t, ctx)
    assert not _rows_names(seen)
    assert torch.equal(y_on, y_off)

    # one bf16 ck: the context stays a tensor for every block
    torch.manual_seed(0)
    mixed = WanModel(_wan_cfg(layers=2)).eval()
    quantize_linears(mixed, lambda name, lin: name != "blocks.1.ck")
    seen = _record_inputs(mixed)
    monkeypatch.setattr(quant, "FP8_FUSED_NORM", True)
    with torch.no_grad():
        mixed(x, t, ctx)
    assert isinstance(seen["blocks.0.ck"][0], torch.Tensor)
    assert isinstance(seen["blocks.1.cv"][0], torch.Tensor)


def test_flux_tiny_routing(monkeypatch):
    from comfyui_distributed_amd.models import create_diffusion_stack

    monkeypatch.delenv("DISTGPU_LINEAR_DTYPE", raising=False)
    stack = create_diffusion_stack("flux_tiny", seed=3, linear_dtype="fp8")
    assert stack.fp8_linears == 10
    seen = _record_inputs(stack.model)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 16, 8, 8, generator=g)
    t = torch.tensor([500.0])
    cond = stack.make_conditioning(0)

    def run(flag):
        monkeypatch.setattr(quant, "FP8_FUSED_NORM", flag)
        for xs in seen.values():
            xs.clear()
        with torch.no_grad():
            return stack.model(x, t, cond["context"], cond["vec"])

    y_on = run(True)
    assert _rows_names(seen) == {
        "double_blocks.0.img_qkv", "double_blocks.0.img_mlp.0",
        "double_blocks.0.txt_qkv", "double_blocks.0.txt_mlp.0",
        "single_blocks.0.linear1"}
    y_off = run(False)
    assert not _rows_names(seen)
    assert torch.isfinite(y_on).all() and torch.equal(y_on, y_off)


def test_flag_reads_environment():
    import os
    import subprocess
    import sys

    # this process: on unless the variable says otherwise
    assert quant.FP8_FUSED_NORM == (
        os.environ.get("DISTGPU_FP8_FUSED_NORM", "1") == "1")
    # the variable is read at import, so "0" needs a process of its own
    code = ("from comfyui_distributed_amd.models import quant;"
            "print(quant.FP8_FUSED_NORM)")
    env = dict(os.environ, DISTGPU_FP8_FUSED_NORM="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root,
                         capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "False", (out.stdout, out.stderr)
