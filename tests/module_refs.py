"""Written-out references for the UNet and VAE modules (models/unet.py,
models/vae.py): the layer that decides which kernel runs, in which layout and
with which fused extras.

Every reference is plain functional torch in fp64, built from a module's
``state_dict()`` by parameter name. None calls a module's ``forward`` or
anything in ``ops.dispatch``. Parameters are taken after the bf16 round, so
the reference sees the values the bf16 module holds.

Every reference takes ``rnd``:

* ``rnd=ident``: the fp64 reference.
* ``rnd=bf16``: the **yardstick**, the same arithmetic rounded to bf16 wherever
  the model stores a bf16 tensor: once after each conv (+bias), GroupNorm
  (+SiLU), Linear, LayerNorm, residual add, ``a * act(b)`` and attention
  output, and on the softmax probabilities in front of the PV product (the
  attention kernel feeds them to the MFMA as bf16). Where the GPU path fuses
  two steps into one rounding (conv + residual in the epilogue) the yardstick
  keeps both. The yardstick is not asserted against: its distance from the
  reference says how large a healthy bf16 error is.

Every reference takes ``defect``: None, or the name of one seeded wiring
mistake (``DEFECTS``). The tests never rewrite a module; they show that the
metric separates each defect from the yardstick.

Every reference returns ``(out, inter)``; ``inter`` maps a submodule's name
(as in ``named_modules()``) to the reference value of that submodule's
output, so a failing module can be bisected with forward hooks
(``stage_errors``) without changing anything.

Metric (``errors``), per batch sample, worst sample counting:
``e_rms = rms(y - r) / rms(r)`` and ``e_max = max|y - r| / rms(r)``. For
SpatialTransformer and VAEAttention the untouched input dominates the output,
so both are also taken on the branch, ``y - x`` against ``r - x``.
"""

from __future__ import annotations

import functools
import math
from collections import Counter
from dataclasses import dataclass, field

import torch
import torch.nn as nn
import torch.nn.functional as F

from comfyui_distributed_amd.models import unet as U
from comfyui_distributed_amd.models import vae as V

BF = torch.bfloat16
F64 = torch.float64
EPS = 1e-5

DEFECTS = {
    # ResBlock family
    "drop_addend": "timestep projection not added",
    "addend_wrong_row": "timestep projection of batch row (b + 1) % B",
    "drop_skip": "skip connection dropped",
    "skip_after_norm1": "skip taken from after norm1 instead of from x",
    "no_silu2": "SiLU missing after norm2",
    # transformer family
    "ctx_wrong_row": "context of batch row (b + 1) % B",
    "kv_swap": "K and V exchanged in the cross-attention",
    "kv_swap_self": "K and V exchanged in the self-attention",
    "self_for_cross": "self-attention where cross-attention belongs",
    "geglu_swap": "GEGLU halves exchanged",
    "silu_for_gelu": "SiLU instead of tanh-GELU in the gate",
    "drop_res1": "residual add around attn1 dropped",
    "drop_res2": "residual add around attn2 dropped",
    "drop_res3": "residual add around the feed-forward dropped",
    "drop_proj_out_res": "residual add after proj_out dropped",
    # up / down
    "conv_first": "conv before the upsample instead of after",
    "stride_offset": "stride-2 sampling offset by one pixel",
    "blind_2x": "a blind 2x where output_shape is 2x - 1",
    # VAE
    "no_silu": "norm_out without SiLU",
    "heads1": "one head instead of C / 64",
}


def ident(t: torch.Tensor) -> torch.Tensor:
    return t


def bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(BF).to(F64)


def params_of(module: nn.Module) -> dict:
    """state_dict by name, rounded to bf16, in fp64."""
    return {k: v.detach().to(BF).to(F64) for k, v in module.state_dict().items()}


def sub(P: dict, prefix: str) -> dict:
    return {k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}


def _groups(c: int) -> int:
    return 32 if c % 32 == 0 else math.gcd(c, 32)


# ---------------------------------------------------------------------------
# pieces
# ---------------------------------------------------------------------------


def _gn(P, name, x, silu, rnd, addend=None):
    if addend is not None:
        # the kernel works on the bf16 round of x + addend
        x = rnd(x + addend[:, :, None, None])
    y = F.group_norm(x, _groups(x.shape[1]), P[name + ".weight"],
                     P[name + ".bias"], EPS)
    return rnd(F.silu(y) if silu else y)


def _conv(P, name, x, rnd, stride=1):
    w = P[name + ".weight"]
    return rnd(F.conv2d(x, w, P.get(name + ".bias"), stride=stride,
                        padding=w.shape[-1] // 2))


def _linear(P, name, x, rnd):
    return rnd(F.linear(x, P[name + ".weight"], P.get(name + ".bias")))


def _ln(P, name, x, rnd):
    return rnd(F.layer_norm(x, (x.shape[-1],), P[name + ".weight"],
                            P[name + ".bias"], EPS))


def _attention(q, k, v, heads, rnd):
    """softmax(Q K^T / sqrt(d)) V per head on [B, N, heads * d]."""
    d = q.shape[-1] // heads
    outs = []
    for h in range(heads):
        sl = slice(h * d, (h + 1) * d)
        s = q[..., sl] @ k[..., sl].transpose(1, 2) / math.sqrt(d)
        p = rnd(torch.softmax(s, dim=-1))
        outs.append(p @ v[..., sl])
    return rnd(torch.cat(outs, dim=-1))


def _cross_attention(P, name, x, context, heads, rnd, swap_kv=False):
    src = x if context is None else context
    q = _linear(P, name + ".to_q", x, rnd)
    k = _linear(P, name + ".to_k", src, rnd)
    v = _linear(P, name + ".to_v", src, rnd)
    if swap_kv:
        k, v = v, k
    return _linear(P, name + ".to_out", _attention(q, k, v, heads, rnd), rnd)


# ---------------------------------------------------------------------------
# UNet modules
# ---------------------------------------------------------------------------


def resblock_ref(P, x, emb, rnd=ident, defect=None):
    inter = {}
    n1 = inter["norm1"] = _gn(P, "norm1", x, True, rnd)
    c1 = inter["conv1"] = _conv(P, "conv1", n1, rnd)
    e = inter["emb_proj"] = _linear(P, "emb_proj", rnd(F.silu(emb)), rnd)
    if defect == "addend_wrong_row":
        e = e.roll(-1, 0)
    if defect == "drop_addend":
        e = None
    n2 = inter["norm2"] = _gn(P, "norm2", c1, defect != "no_silu2", rnd,
                              addend=e)
    c2 = inter["conv2"] = _conv(P, "conv2", n2, rnd)
    src = n1 if defect == "skip_after_norm1" else x
    skip = _conv(P, "skip", src, rnd) if "skip.weight" in P else src
    if defect == "drop_skip":
        return c2, inter
    return rnd(c2 + skip), inter


def transformer_block_ref(P, x, context, heads, rnd=ident, defect=None):
    """x [B, N, C], context [B, Nk, Cctx]."""
    inter = {}
    if defect == "ctx_wrong_row":
        context = context.roll(-1, 0)
    a1 = inter["attn1"] = _cross_attention(
        P, "attn1", _ln(P, "norm1", x, rnd), None, heads, rnd,
        swap_kv=defect == "kv_swap_self")
    x = a1 if defect == "drop_res1" else rnd(x + a1)
    n2 = _ln(P, "norm2", x, rnd)
    a2 = inter["attn2"] = _cross_attention(
        P, "attn2", n2, n2 if defect == "self_for_cross" else context, heads,
        rnd, swap_kv=defect == "kv_swap")
    x = a2 if defect == "drop_res2" else rnd(x + a2)
    h = _linear(P, "ff.proj_in", _ln(P, "norm3", x, rnd), rnd)
    a, gate = h.chunk(2, dim=-1)
    if defect == "geglu_swap":
        a, gate = gate, a
    act = (F.silu(gate) if defect == "silu_for_gelu"
           else F.gelu(gate, approximate="tanh"))
    f = inter["ff"] = _linear(P, "ff.proj_out", rnd(a * act), rnd)
    x = f if defect == "drop_res3" else rnd(x + f)
    return x, inter


def spatial_transformer_ref(P, x, context, heads, rnd=ident, defect=None):
    inter = {}
    b, c, h, w = x.shape
    n = inter["norm"] = _gn(P, "norm", x, False, rnd)
    t = n.permute(0, 2, 3, 1).reshape(b, h * w, c)
    t = inter["proj_in"] = _linear(P, "proj_in", t, rnd)
    i = 0
    while f"blocks.{i}.norm1.weight" in P:
        t, bi = transformer_block_ref(sub(P, f"blocks.{i}."), t, context,
                                      heads, rnd, defect)
        inter.update({f"blocks.{i}.{k}": v for k, v in bi.items()})
        inter[f"blocks.{i}"] = t
        i += 1
    t = inter["proj_out"] = _linear(P, "proj_out", t, rnd)
    t = t.reshape(b, h, w, c).permute(0, 3, 1, 2)
    if defect == "drop_proj_out_res":
        return t, inter
    return rnd(x + t), inter


def downsample_ref(P, x, rnd=ident, defect=None):
    if defect == "stride_offset":
        # the taps centred on pixels 1, 3, ... instead of 0, 2, ...
        x = F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:]
    return _conv(P, "conv", x, rnd, stride=2), {}


def upsample_ref(P, x, output_shape=None, rnd=ident, defect=None):
    """Nearest upsample to ``output_shape`` (2x when None), then the conv."""
    h, w = x.shape[2:]
    size = tuple(output_shape) if output_shape is not None else (2 * h, 2 * w)
    if defect == "conv_first":
        return F.interpolate(_conv(P, "conv", x, rnd), size=size,
                             mode="nearest"), {}
    if defect == "blind_2x":
        y = F.interpolate(x, scale_factor=2, mode="nearest")
        return _conv(P, "conv", y, rnd)[:, :, :size[0], :size[1]], {}
    y = F.interpolate(x, size=size, mode="nearest")
    return _conv(P, "conv", y, rnd), {}


def stem_ref(P, x, rnd=ident, defect=None):
    return _conv(P, "conv", x, rnd), {}


def tail_ref(P, x, rnd=ident, defect=None):
    """norm + SiLU, conv: the UNet's out_norm/out_conv and the VAE's
    norm_out/conv_out (the _Tail wrapper below names them norm, conv)."""
    inter = {}
    n = inter["norm"] = _gn(P, "norm", x, defect != "no_silu", rnd)
    return _conv(P, "conv", n, rnd), inter


# ---------------------------------------------------------------------------
# VAE modules
# ---------------------------------------------------------------------------


def vae_resblock_ref(P, x, rnd=ident, defect=None):
    inter = {}
    n1 = inter["norm1"] = _gn(P, "norm1", x, True, rnd)
    c1 = inter["conv1"] = _conv(P, "conv1", n1, rnd)
    n2 = inter["norm2"] = _gn(P, "norm2", c1, True, rnd)
    c2 = inter["conv2"] = _conv(P, "conv2", n2, rnd)
    if defect == "drop_skip":
        return c2, inter
    skip = _conv(P, "skip", x, rnd) if "skip.weight" in P else x
    return rnd(c2 + skip), inter


def vae_attention_ref(P, x, rnd=ident, defect=None):
    inter = {}
    b, c, h, w = x.shape
    heads = 1 if defect == "heads1" or c % 64 else c // 64
    n = inter["norm"] = _gn(P, "norm", x, False, rnd)
    t = n.permute(0, 2, 3, 1).reshape(b, h * w, c)
    inter["qkv"] = _linear(P, "qkv", t, rnd)
    q, k, v = inter["qkv"].chunk(3, dim=-1)
    o = _attention(q, k, v, heads, rnd)
    o = inter["proj"] = _linear(P, "proj", o, rnd)
    return rnd(x + o.reshape(b, h, w, c).permute(0, 3, 1, 2)), inter


def decoder_upsample_ref(P, x, rnd=ident, defect=None):
    return upsample_ref(P, x, None, rnd, defect)


# ---------------------------------------------------------------------------
# compositions: walk the config the way UNetModel / VAEDecoder do
# ---------------------------------------------------------------------------


def unet_layout(cfg):
    """(input_blocks, middle_block, output_blocks): per block a list of layer
    specs ("stem",), ("res", cin, cout), ("st", ch, heads), ("down", ch),
    ("up", ch), in the order UNetModel's constructor appends them."""
    ch0 = cfg.model_channels

    def heads_for(ch):
        return ch // cfg.head_dim if cfg.head_dim is not None else cfg.num_heads

    def st(level, ch):
        if level in cfg.attn_levels and cfg.transformer_depth[level] > 0:
            return [("st", ch, heads_for(ch))]
        return []

    inputs, skip_chans, ch = [[("stem",)]], [ch0], ch0
    last = len(cfg.channel_mult) - 1
    for level, mult in enumerate(cfg.channel_mult):
        for _ in range(cfg.num_res_blocks):
            inputs.append([("res", ch, ch0 * mult)] + st(level, ch0 * mult))
            ch = ch0 * mult
            skip_chans.append(ch)
        if level != last:
            inputs.append([("down", ch)])
            skip_chans.append(ch)
    middle = [("res", ch, ch), ("st", ch, heads_for(ch)), ("res", ch, ch)]
    outputs = []
    for level, mult in reversed(list(enumerate(cfg.channel_mult))):
        for i in range(cfg.num_res_blocks + 1):
            layers = [("res", ch + skip_chans.pop(), ch0 * mult)]
            ch = ch0 * mult
            layers += st(level, ch)
            if level != 0 and i == cfg.num_res_blocks:
                layers.append(("up", ch))
            outputs.append(layers)
    return inputs, middle, outputs


def timestep_sinusoid(t: torch.Tensor, dim: int) -> torch.Tensor:
    """The model's timestep encoding, by its definition in fp32 (it is an
    input encoding, the same bits for the reference and every forward)."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0)
                      * torch.arange(half, dtype=torch.float32) / half)
    args = t.float()[:, None] * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def unet_ref(cfg, P, x, timesteps, context, rnd=ident, defect=None):
    inter = {}
    temb = rnd(timestep_sinusoid(timesteps, cfg.model_channels).to(F64))
    emb = _linear(P, "time_embed.0", temb, rnd)
    emb = inter["time_embed"] = _linear(P, "time_embed.2", rnd(F.silu(emb)),
                                        rnd)
    inputs, middle, outputs = unet_layout(cfg)

    def run(prefix, layers, h, output_shape=None):
        for j, spec in enumerate(layers):
            p = sub(P, f"{prefix}.{j}.")
            if spec[0] == "stem":
                h, _ = stem_ref(p, h, rnd)
            elif spec[0] == "res":
                assert h.shape[1] == spec[1]
                h, _ = resblock_ref(p, h, emb, rnd)
            elif spec[0] == "st":
                h, _ = spatial_transformer_ref(p, h, context, spec[2], rnd)
            elif spec[0] == "down":
                h, _ = downsample_ref(p, h, rnd)
            else:
                h, _ = upsample_ref(p, h, output_shape, rnd)
            inter[f"{prefix}.{j}"] = h
        return h

    hs, h = [], x
    for i, layers in enumerate(inputs):
        h = run(f"input_blocks.{i}", layers, h)
        hs.append(h)
    h = run("middle_block", middle, h)
    for i, layers in enumerate(outputs):
        h = torch.cat([h, hs.pop()], dim=1)
        h = run(f"output_blocks.{i}", layers, h,
                hs[-1].shape[2:] if hs else None)
    out, _ = tail_ref({"norm.weight": P["out_norm.weight"],
                       "norm.bias": P["out_norm.bias"],
                       "conv.weight": P["out_conv.weight"],
                       "conv.bias": P["out_conv.bias"]}, h, rnd)
    return out, inter


def vae_decoder_layout(cfg):
    """(mid, up) layer specs of VAEDecoder: ("res", cin, cout), ("attn", ch),
    ("up", ch)."""
    ch = cfg.base_channels
    cin = ch * cfg.channel_mult[-1]
    mid = [("res", cin, cin), ("attn", cin), ("res", cin, cin)]
    ups = []
    for level, mult in reversed(list(enumerate(cfg.channel_mult))):
        for _ in range(cfg.num_res_blocks + 1):
            ups.append(("res", cin, ch * mult))
            cin = ch * mult
        if level != 0:
            ups.append(("up", cin))
    return mid, ups


def vae_decoder_ref(cfg, P, z, rnd=ident, defect=None):
    inter = {}
    mid, ups = vae_decoder_layout(cfg)
    h, _ = stem_ref(sub(P, "conv_in."), z, rnd)
    inter["conv_in"] = h
    for prefix, layers in (("mid", mid), ("up", ups)):
        for j, spec in enumerate(layers):
            p = sub(P, f"{prefix}.{j}.")
            if spec[0] == "res":
                assert h.shape[1] == spec[1]
                h, _ = vae_resblock_ref(p, h, rnd)
            elif spec[0] == "attn":
                h, _ = vae_attention_ref(p, h, rnd)
            else:
                h, _ = decoder_upsample_ref(p, h, rnd)
            inter[f"{prefix}.{j}"] = h
    out, _ = tail_ref({"norm.weight": P["norm_out.weight"],
                       "norm.bias": P["norm_out.bias"],
                       "conv.weight": P["conv_out.weight"],
                       "conv.bias": P["conv_out.bias"]}, h, rnd)
    return out, inter


# ---------------------------------------------------------------------------
# metric
# ---------------------------------------------------------------------------


def errors(y: torch.Tensor, r: torch.Tensor) -> tuple[float, float]:
    """(e_rms, e_max) of y against r, per batch sample, the worst sample."""
    y = y.detach().to("cpu", F64)
    r = r.to(F64)
    assert y.shape == r.shape, (tuple(y.shape), tuple(r.shape))
    d = (y - r).reshape(r.shape[0], -1)
    rms_r = r.reshape(r.shape[0], -1).pow(2).mean(1).sqrt()
    assert (rms_r > 0).all()
    return ((d.pow(2).mean(1).sqrt() / rms_r).max().item(),
            (d.abs().amax(1) / rms_r).max().item())


def assert_rows_differ(t: torch.Tensor, what: str) -> None:
    for i in range(t.shape[0]):
        for j in range(i + 1, t.shape[0]):
            assert not torch.equal(t[i], t[j]), f"{what}: rows {i}, {j} equal"


def stage_errors(module, call, inter_ref, inter_yard) -> list:
    """Run ``call()`` with a forward hook on every submodule that ``inter_ref``
    names; returns [(name, e_rms / yardstick e_rms, e_max / yardstick e_max)]
    in execution order: the first stage whose ratio jumps is where to look.
    A submodule that the forward bypasses (a conv run through dispatch
    directly) has no row."""
    rows, hooks = [], []

    def hook(name):
        def fn(_m, _i, out):
            if out.shape == inter_ref[name].shape:
                e, y = errors(out, inter_ref[name]), errors(inter_yard[name],
                                                            inter_ref[name])
                rows.append((name, e[0] / max(y[0], 1e-30),
                             e[1] / max(y[1], 1e-30)))
        return fn

    for name, m in module.named_modules():
        if name in inter_ref:
            hooks.append(m.register_forward_hook(hook(name)))
    try:
        call()
    finally:
        for h in hooks:
            h.remove()
    return rows


# ---------------------------------------------------------------------------
# seeded modules and inputs
# ---------------------------------------------------------------------------


class _Tail(nn.Module):
    """``conv(norm(x))`` as UNetModel, VAEEncoder and VAEDecoder end."""

    def __init__(self, c, k_out):
        super().__init__()
        self.norm = U.FusedGroupNorm(c, silu=True)
        self.conv = U.MfmaConv2d(c, k_out, 3, padding=1)

    def forward(self, x):
        return self.conv(self.norm(x))


def seeded(ctor, seed: int) -> nn.Module:
    """ctor() under the seed, fp32, every parameter bf16-representable. Norm
    weights are 1 + 0.3 randn and norm biases 0.3 randn (with ones and zeros a
    dropped affine term is invisible); conv and Linear keep their init."""
    torch.manual_seed(seed)
    m = ctor().eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (U.FusedGroupNorm, U.FusedLayerNorm)):
                n = mod.weight.numel()
                mod.weight.copy_(1 + 0.3 * torch.randn(n, generator=g))
                mod.bias.copy_(0.3 * torch.randn(n, generator=g))
        for p in m.parameters():
            p.copy_(p.to(BF).float())
    return m


def randn_bf16(seed: int, *shape, scale: float = 1.0) -> torch.Tensor:
    """fp32 tensor of bf16-representable values."""
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(BF).float()


RES = ("drop_addend", "addend_wrong_row", "drop_skip", "skip_after_norm1",
       "no_silu2")
RES_B1 = tuple(d for d in RES if d != "addend_wrong_row")
TB = ("ctx_wrong_row", "kv_swap", "kv_swap_self", "geglu_swap",
      "silu_for_gelu", "drop_res1", "drop_res2", "drop_res3")
ST = TB + ("drop_proj_out_res",)


@dataclass(frozen=True)
class Case:
    """One row of the table. ``build``: () -> module (before seeding).
    ``inputs``: () -> tuple of fp32 tensors holding bf16 values, as ``ref``
    takes them after P. ``call``: (module, *inputs) -> output, where the
    module is not simply called on the inputs. ``routes``: the extension
    functions one bf16 channels_last forward on the GPU calls, by count.
    ``branch``: also measure y - x. ``fuse_res``: run on the GPU with
    dispatch._FUSE_RES False and True."""

    name: str
    build: object
    inputs: object
    ref: object
    routes: dict
    defects: tuple = ()
    call: object = None
    branch: bool = False
    fuse_res: bool = False
    # ("conv", M, K_out, Kdim, (bn, split_k) expected) / ("gn", B, HW, C)
    plans: tuple = field(default=())
    why: str = ""


def _res_case(name, cin, cout, emb_dim, shape, routes, defects=RES, **kw):
    b = shape[0]
    return Case(
        name, lambda: U.ResBlock(cin, emb_dim, cout),
        lambda: (randn_bf16(cin + cout, *shape), randn_bf16(7 + cin, b, emb_dim)),
        resblock_ref, routes, defects, **kw)


def _cat_inputs():
    h = randn_bf16(192, 2, 192, 12, 12).contiguous(memory_format=torch.channels_last)
    s = randn_bf16(128, 2, 128, 12, 12).contiguous(memory_format=torch.channels_last)
    return h, s, randn_bf16(64, 2, 64)


def _st_case(name, c, ctx_dim, heads, d, shape, nctx, why):
    return Case(
        name, lambda: U.SpatialTransformer(c, ctx_dim, heads, d),
        lambda: (randn_bf16(c, *shape), randn_bf16(ctx_dim, shape[0], nctx, ctx_dim)),
        lambda P, x, ctx, rnd=ident, defect=None: spatial_transformer_ref(
            P, x, ctx, heads, rnd, defect),
        {"group_norm_nhwc": 1, "layer_norm": 3, "attn_fwd_qkv": 1,
         "attn_fwd_q_kv": 1, "act_mul": 1},
        ST, branch=True, why=why,
        plans=(("gn", shape[0], shape[2] * shape[3], c),))


def _simple(name, build, shape, ref, routes, defects=(), **kw):
    return Case(name, build, lambda: (randn_bf16(sum(shape), *shape),),
                ref, routes, defects, **kw)


UNET_CFG = U.UNetConfig(model_channels=128, channel_mult=(1, 2),
                        num_res_blocks=1, attn_levels=(0, 1),
                        transformer_depth=(1, 1), context_dim=96, num_heads=2)
VAE_CFG = V.VAEConfig(base_channels=128, channel_mult=(1, 2), num_res_blocks=1)

C256, CDIR, GN = "conv256_nhwc", "conv_nhwc", "group_norm_nhwc"


def conv_route(c: int, m: int, up2: bool = False) -> str:
    """The gate of dispatch.conv2d_mfma, as documented: the 256-tile kernel
    for C % 64 == 0 and M = B*H*W (of the input) >= 256, or a fused
    upsample; else the direct kernel."""
    return C256 if c % 64 == 0 and (m >= 256 or up2) else CDIR


def unet_routes(cfg, b, h, w) -> dict:
    """Extension calls of one UNetModel forward on [b, ., h, w], from the
    layout and conv_route."""
    n = Counter()
    inputs, middle, outputs = unet_layout(cfg)
    sizes = []

    def run(layers, hw, output_shape=None):
        for spec in layers:
            m = b * hw[0] * hw[1]
            if spec[0] == "stem":
                n["conv_smallc"] += 1
            elif spec[0] == "res":
                n[GN] += 2
                n[conv_route(spec[1], m)] += 1 + (spec[1] != spec[2])
                n[conv_route(spec[2], m)] += 1
            elif spec[0] == "st":
                n[GN] += 1
                n["layer_norm"] += 3
                n["attn_fwd_qkv"] += 1
                n["attn_fwd_q_kv"] += 1
                n["act_mul"] += 1
            elif spec[0] == "down":
                n[conv_route(spec[1], m)] += 1
                hw = ((hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1)
            else:
                exact = (output_shape is None
                         or tuple(output_shape) == (2 * hw[0], 2 * hw[1]))
                out = tuple(output_shape) if output_shape else (2 * hw[0], 2 * hw[1])
                n[conv_route(spec[1], m if exact else b * out[0] * out[1],
                             up2=exact)] += 1
                hw = out
        return hw

    hw = (h, w)
    for layers in inputs:
        hw = run(layers, hw)
        sizes.append(hw)
    hw = run(middle, hw)
    for layers in outputs:
        sizes.pop()
        hw = run(layers, hw, sizes[-1] if sizes else None)
    n[GN] += 1
    n[conv_route(cfg.model_channels, b * hw[0] * hw[1])] += 1
    return dict(n)


def vae_decoder_routes(cfg, b, h, w) -> dict:
    n = Counter()
    mid, ups = vae_decoder_layout(cfg)
    n["conv_smallc"] += 1
    hw = (h, w)
    for spec in mid + ups:
        m = b * hw[0] * hw[1]
        if spec[0] == "res":
            n[GN] += 2
            n[conv_route(spec[1], m)] += 1 + (spec[1] != spec[2])
            n[conv_route(spec[2], m)] += 1
        elif spec[0] == "attn":
            n[GN] += 1
            n["attn_fwd_packed"] += 1
        else:
            n[conv_route(spec[1], m, up2=True)] += 1
            hw = (2 * hw[0], 2 * hw[1])
    n[GN] += 1
    n[conv_route(cfg.base_channels, b * hw[0] * hw[1])] += 1
    return dict(n)


def _unet_inputs():
    return (randn_bf16(41, 2, 4, 17, 19), torch.tensor([100.0, 700.0]),
            randn_bf16(42, 2, 13, 96))


CASES = [
    _res_case("res128", 128, 128, 64, (2, 128, 12, 12), {C256: 2, GN: 2},
              fuse_res=True,
              plans=(("conv", 288, 128, 1152, (256, 1)), ("gn", 2, 144, 128)),
              why="256-tile conv, M = 288 (32-row tail); two-pass GN with the "
                  "addend in-kernel; identity skip"),
    _res_case("res128_192", 128, 192, 64, (1, 128, 16, 17), {C256: 3, GN: 2},
              RES_B1,
              plans=(("conv", 272, 192, 1152, (256, 1)),
                     ("conv", 272, 192, 128, (256, 1)),
                     ("gn", 1, 272, 192)),
              why="1x1 skip conv on the 256-tile kernel; K_out = 192; B = 1; "
                  "Cg = 6"),
    _res_case("res64_128", 64, 128, 64, (2, 64, 12, 12), {C256: 3, GN: 2},
              why="norm1 at Cg = 2 (per-(n, g) kernel); norm2 (C = 128, two-"
                  "pass) gets the addend"),
    _res_case("res128_64", 128, 64, 64, (2, 128, 12, 12), {C256: 3, GN: 2},
              why="norm2 at Cg = 2: the per-(n, g) fallback gets the addend"),
    _res_case("res320", 320, 320, 64, (2, 320, 9, 9), {CDIR: 2, GN: 2},
              why="M = 162 < 256: direct conv kernel, the flagship 9x9 level"),
    _res_case("res96", 96, 96, 64, (2, 96, 12, 12), {CDIR: 2, GN: 2},
              why="C % 64 != 0: direct kernel although M >= 256; Cg = 3"),
    Case("res_cat320_128", lambda: U.ResBlock(320, 64, 128), _cat_inputs,
         lambda P, h, s, emb, rnd=ident, defect=None: resblock_ref(
             P, torch.cat([h, s], dim=1), emb, rnd, defect),
         {C256: 3, GN: 2}, RES,
         call=lambda m, h, s, emb: m(torch.cat([h, s], dim=1), emb),
         why="the decoder's concat of two channels_last tensors"),
    _simple("down128", lambda: U.Downsample(128), (2, 128, 17, 19),
            downsample_ref, {C256: 1}, ("stride_offset",),
            why="stride-2 address mode, odd sizes"),
    _simple("up128_none", lambda: U.Upsample(128), (1, 128, 9, 9),
            upsample_ref, {C256: 1}, ("conv_first",),
            why="fused up2 at M = 81"),
    Case("up128_18", lambda: U.Upsample(128),
         lambda: (randn_bf16(5, 1, 128, 9, 9),),
         lambda P, x, rnd=ident, defect=None: upsample_ref(P, x, (18, 18), rnd,
                                                           defect),
         {C256: 1}, ("conv_first",),
         call=lambda m, x: m(x, output_shape=(18, 18)),
         why="output_shape exactly 2x: fused up2"),
    Case("up128_17", lambda: U.Upsample(128),
         lambda: (randn_bf16(6, 1, 128, 9, 9),),
         lambda P, x, rnd=ident, defect=None: upsample_ref(P, x, (17, 17), rnd,
                                                           defect),
         {C256: 1}, ("conv_first", "blind_2x"),
         call=lambda m, x: m(x, output_shape=(17, 17)),
         why="2x - 1: interpolate to size, then the 256-tile conv (M = 289)"),
    _st_case("st320", 320, 768, 8, 40, (2, 320, 9, 10), 77,
             "NHWC GN without SiLU, LayerNorm, fused QKV / KV at D = 40, "
             "GEGLU on the chunk views"),
    _st_case("st128", 128, 96, 2, 64, (2, 128, 8, 9), 13,
             "D = 64, short context with a key tail"),
    Case("tblock128", lambda: U.TransformerBlock(128, 128, 2, 64),
         lambda: (randn_bf16(9, 2, 72, 128), randn_bf16(10, 2, 13, 128)),
         lambda P, x, ctx, rnd=ident, defect=None: transformer_block_ref(
             P, x, ctx, 2, rnd, defect),
         {"layer_norm": 3, "attn_fwd_qkv": 1, "attn_fwd_q_kv": 1, "act_mul": 1},
         TB + ("self_for_cross",),
         why="context_dim == dim, so self-for-cross is a possible mistake"),
    _simple("stem4", lambda: U.StemConv(4, 128), (2, 4, 9, 11), stem_ref,
            {"conv_smallc": 1}),
    _simple("stem3", lambda: U.StemConv(3, 128), (1, 3, 9, 11), stem_ref,
            {"conv_smallc": 1}),
    _simple("unet_tail", lambda: _Tail(320, 4), (2, 320, 12, 12), tail_ref,
            {GN: 1, C256: 1}, ("no_silu",),
            plans=(("conv", 288, 4, 2880, (256, 4)),),
            why="K_out = 4 on the 256-tile kernel (K split in 4) after GN+SiLU"),
    _simple("vae_res128", lambda: V.VAEResBlock(128, 128), (1, 128, 16, 18),
            vae_resblock_ref, {GN: 2, C256: 2}, ("drop_skip",), fuse_res=True),
    _simple("vae_res128_256", lambda: V.VAEResBlock(128, 256),
            (1, 128, 16, 18), vae_resblock_ref, {GN: 2, C256: 3},
            ("drop_skip",), fuse_res=True),
    _simple("vae_res256_128", lambda: V.VAEResBlock(256, 128),
            (1, 256, 16, 18), vae_resblock_ref, {GN: 2, C256: 3},
            ("drop_skip",), fuse_res=True),
    _simple("vae_attn512", lambda: V.VAEAttention(512), (1, 512, 8, 9),
            vae_attention_ref, {GN: 1, "attn_fwd_packed": 1}, ("heads1",),
            branch=True, why="8 heads of 64 on .contiguous() chunks"),
    _simple("vae_up128", lambda: V._DecoderUpsample(128), (1, 128, 9, 11),
            decoder_upsample_ref, {C256: 1}, ("conv_first",)),
    _simple("vae_tail128_3", lambda: _Tail(128, 3), (1, 128, 16, 18), tail_ref,
            {GN: 1, C256: 1}, ("no_silu",)),
    _simple("vae_tail512_8", lambda: _Tail(512, 8), (1, 512, 16, 18), tail_ref,
            {GN: 1, C256: 1}, ("no_silu",),
            plans=(("conv", 288, 8, 4608, (256, 7)),),
            why="K_out = 8, K split in 7"),
    Case("unet", lambda: U.UNetModel(UNET_CFG), _unet_inputs,
         lambda P, x, t, ctx, rnd=ident, defect=None: unet_ref(
             UNET_CFG, P, x, t, ctx, rnd, defect),
         unet_routes(UNET_CFG, 2, 17, 19),
         why="skip stack order, concat, 17x19 -> 9x10 -> back with a non-2x "
             "output_shape, emb path"),
    Case("vae_decoder", lambda: V.VAEDecoder(VAE_CFG),
         lambda: (randn_bf16(43, 1, 4, 9, 10),),
         lambda P, z, rnd=ident, defect=None: vae_decoder_ref(VAE_CFG, P, z,
                                                              rnd, defect),
         vae_decoder_routes(VAE_CFG, 1, 9, 10),
         why="decoder composition with the fused upsample"),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


@dataclass(frozen=True)
class CaseData:
    case: Case
    module: nn.Module      # fp32, bf16-representable parameters; do not mutate
    inputs: tuple          # fp32 tensors holding bf16 values (and int tensors)
    ref: torch.Tensor
    yard: torch.Tensor
    inter_ref: dict
    inter_yard: dict
    P: dict

    def x64(self):
        """The input the branch metric subtracts."""
        return self.inputs[0].to(F64)

    def metrics(self, y) -> dict:
        """{"out": (e_rms, e_max)[, "branch": ...]} of y against the reference."""
        m = {"out": errors(y, self.ref)}
        if self.case.branch:
            x = self.x64()
            m["branch"] = errors(y.detach().to("cpu", F64) - x, self.ref - x)
        return m

    def yard_metrics(self) -> dict:
        return self.metrics(self.yard)

    def forward(self, module, inputs):
        if self.case.call is not None:
            return self.case.call(module, *inputs)
        return module(*inputs)


def to64(inputs):
    return tuple(t.to(F64) if t.is_floating_point() else t for t in inputs)


def check_inputs(inputs) -> None:
    """Batch rows of every input with more than one are pairwise different."""
    for i, t in enumerate(inputs):
        if t.shape[0] > 1:
            assert_rows_differ(t, f"input {i}")


@functools.lru_cache(maxsize=None)
def case_data(name: str, seed: int = 0) -> CaseData:
    """Module, inputs, reference and yardstick of a case, computed once and
    shared; nothing in it may be modified."""
    case = CASE[name]
    module = seeded(case.build, 1000 + seed + len(name))
    inputs = case.inputs()
    check_inputs(inputs)
    P = params_of(module)
    with torch.no_grad():
        ref, inter_ref = case.ref(P, *to64(inputs), rnd=ident)
        yard, inter_yard = case.ref(P, *to64(inputs), rnd=bf16)
    return CaseData(case, module, inputs, ref, yard, inter_ref, inter_yard, P)
