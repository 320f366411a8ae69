"""RRDBNet (ESRGAN) upscale model: the ``UpscaleModelLoader`` +
``ImageUpscaleWithModel`` step of the reference's distributed-upscale
workflow, in front of the tiled diffusion upscale.

The network is 23 residual-in-residual dense blocks at the input resolution
(345 3x3 convs) and a 4x nearest-upsample tail. Submodule names follow the
public RRDBNet layout (``conv_first``, ``body.{i}.rdb{1,2,3}.conv{1..5}``,
``conv_body``, ``conv_up1``, ``conv_up2``, ``conv_hr``, ``conv_last``) so a
real checkpoint's ``state_dict`` loads once file IO exists; weights are
random-init under a seed like every other family here.

Two forwards over the same parameters:

* the **dense route** (GPU, bf16, ``DISTGPU_RRDB_HIP`` unset or 1):
  activations stay NHWC; each dense block lives in one ``[B, H, W, nf + 4*gc]``
  buffer whose channel slices ``ops.conv3x3_dense`` (conv_dense.hip) reads and
  writes in place, so none of the 276 concats is a copy; LeakyReLU, the
  ``0.2 * y + x`` of every block and the RRDB residual are conv epilogues; the
  two 2x upsamples of the tail are address modes of their convs. Three
  rotating buffers serve the whole body.
* the **textbook route** (CPU, any dtype, or ``DISTGPU_RRDB_HIP=0``): plain
  ``nn.Conv2d`` calls with ``torch.cat``.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import dispatch as ops

LRELU = 0.2
RES_SCALE = 0.2


@dataclass(frozen=True)
class RRDBConfig:
    in_ch: int = 3
    out_ch: int = 3
    nf: int = 64
    gc: int = 32
    nb: int = 23
    scale: int = 4


UPSCALE_CONFIGS = {
    "esrgan_x4": RRDBConfig(),
    # same widths, so it takes the same kernels; for tests
    "rrdb_tiny": RRDBConfig(nb=2),
}


def _conv(cin: int, cout: int) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, 3, 1, 1)


class ResidualDenseBlock(nn.Module):
    def __init__(self, nf: int, gc: int):
        super().__init__()
        for j in range(1, 5):
            setattr(self, f"conv{j}", _conv(nf + (j - 1) * gc, gc))
        self.conv5 = _conv(nf + 4 * gc, nf)

    def forward(self, x):
        feats = [x]
        for j in range(1, 5):
            feats.append(F.leaky_relu(
                getattr(self, f"conv{j}")(torch.cat(feats, 1)), LRELU))
        return self.conv5(torch.cat(feats, 1)) * RES_SCALE + x


class RRDB(nn.Module):
    def __init__(self, nf: int, gc: int):
        super().__init__()
        self.rdb1 = ResidualDenseBlock(nf, gc)
        self.rdb2 = ResidualDenseBlock(nf, gc)
        self.rdb3 = ResidualDenseBlock(nf, gc)

    def forward(self, x):
        return self.rdb3(self.rdb2(self.rdb1(x))) * RES_SCALE + x


class RRDBNet(nn.Module):
    def __init__(self, cfg: RRDBConfig = RRDBConfig()):
        super().__init__()
        if cfg.scale != 4:
            raise ValueError("RRDBNet: only the 4x layout is implemented")
        self.cfg = cfg
        nf = cfg.nf
        self.conv_first = _conv(cfg.in_ch, nf)
        self.body = nn.ModuleList(RRDB(nf, cfg.gc) for _ in range(cfg.nb))
        self.conv_body = _conv(nf, nf)
        self.conv_up1 = _conv(nf, nf)
        self.conv_up2 = _conv(nf, nf)
        self.conv_hr = _conv(nf, nf)
        self.conv_last = _conv(nf, cfg.out_ch)

    # -- textbook ----------------------------------------------------------

    def forward_cat(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, in_ch, H, W] -> [B, out_ch, 4H, 4W], as the model is
        published."""
        feat = self.conv_first(x)
        h = feat
        for block in self.body:
            h = block(h)
        h = feat + self.conv_body(h)
        h = F.leaky_relu(self.conv_up1(F.interpolate(h, scale_factor=2,
                                                     mode="nearest")), LRELU)
        h = F.leaky_relu(self.conv_up2(F.interpolate(h, scale_factor=2,
                                                     mode="nearest")), LRELU)
        return self.conv_last(F.leaky_relu(self.conv_hr(h), LRELU))

    # -- dense buffers -----------------------------------------------------

    def dense_supported(self) -> bool:
        cfg = self.cfg
        return (cfg.nf % 32 == 0 and cfg.gc % 32 == 0 and cfg.gc <= 64
                and cfg.nf <= 64 and cfg.nf + 4 * cfg.gc <= 512
                and cfg.out_ch <= 64)

    def _first(self, x_nhwc: torch.Tensor) -> torch.Tensor:
        """conv_first (C = 3) -> [B, H, W, nf]: the small-C stem kernel on
        the GPU."""
        x = x_nhwc.permute(0, 3, 1, 2)
        if x.is_cuda and ops._RRDB_HIP and self.cfg.in_ch in (3, 4, 8):
            return ops.conv2d_smallc(x, self.conv_first).permute(0, 2, 3, 1)
        return self.conv_first(x).permute(0, 2, 3, 1)

    def forward_dense(self, x_nhwc: torch.Tensor) -> torch.Tensor:
        """x [B, H, W, in_ch] -> [B, 4H, 4W, out_ch], every 3x3 conv behind
        conv_first through ``ops.conv3x3_dense`` (the HIP kernel on the GPU,
        its fp32 torch formula on the CPU)."""
        cfg = self.cfg
        nf, gc = cfg.nf, cfg.gc
        b, h, w, _ = x_nhwc.shape
        feat = self._first(x_nhwc)
        bufs = [feat.new_empty(b, h, w, nf + 4 * gc) for _ in range(3)]
        bufs[0][..., :nf].copy_(feat)
        for block in self.body:
            x_rrdb = bufs[0][..., :nf]
            for i, rdb in enumerate((block.rdb1, block.rdb2, block.rdb3)):
                cur, nxt = bufs[i], bufs[(i + 1) % 3]
                for j in range(1, 5):
                    c = nf + (j - 1) * gc
                    ops.conv3x3_dense(cur[..., :c], getattr(rdb, f"conv{j}"),
                                      cur[..., c:c + gc], lrelu=LRELU)
                if i < 2:    # 0.2 * t + x, the next block's input
                    ops.conv3x3_dense(cur, rdb.conv5, nxt[..., :nf],
                                      alpha=RES_SCALE, res2=cur[..., :nf])
                else:        # 0.2 * (0.2 * t + x_rdb) + x_rrdb, in place
                    ops.conv3x3_dense(cur, rdb.conv5, x_rrdb,
                                      alpha=RES_SCALE * RES_SCALE,
                                      res1=cur[..., :nf], beta1=RES_SCALE,
                                      res2=x_rrdb)
        trunk = feat.new_empty(b, h, w, nf)
        ops.conv3x3_dense(bufs[0][..., :nf], self.conv_body, trunk, res2=feat)
        del bufs, feat
        up1 = trunk.new_empty(b, 2 * h, 2 * w, nf)
        ops.conv3x3_dense(trunk, self.conv_up1, up1, lrelu=LRELU, up2=True)
        del trunk
        up2 = up1.new_empty(b, 4 * h, 4 * w, nf)
        ops.conv3x3_dense(up1, self.conv_up2, up2, lrelu=LRELU, up2=True)
        del up1
        hr = torch.empty_like(up2)
        ops.conv3x3_dense(up2, self.conv_hr, hr, lrelu=LRELU)
        del up2
        # out_ch = 3 at a pixel pitch of 8 elements (the kernel's alignment)
        pitch = (cfg.out_ch + 7) // 8 * 8
        last = hr.new_empty(b, 4 * h, 4 * w, pitch)[..., :cfg.out_ch]
        ops.conv3x3_dense(hr, self.conv_last, last)
        return last

    # -- public ------------------------------------------------------------

    def forward(self, x_nhwc: torch.Tensor, route: str | None = None
                ) -> torch.Tensor:
        """[B, H, W, in_ch] -> [B, 4H, 4W, out_ch] in the parameters' dtype.
        ``route``: "dense" / "cat" force a forward; None takes the dense
        route for bf16 on the GPU (unless ``DISTGPU_RRDB_HIP=0``) and the
        textbook one elsewhere."""
        p = self.conv_first.weight
        x = x_nhwc.to(p.device, p.dtype)
        if route is None:
            route = ("dense" if x.is_cuda and ops._RRDB_HIP
                     and p.dtype == torch.bfloat16 and self.dense_supported()
                     else "cat")
        if route == "dense":
            return self.forward_dense(x)
        if route != "cat":
            raise ValueError(f"route {route!r} is not 'dense' or 'cat'")
        return self.forward_cat(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)

    @torch.no_grad()
    def upscale(self, images: torch.Tensor) -> torch.Tensor:
        """images [B, H, W, 3] in [0, 1] -> fp32 [B, 4H, 4W, 3] clamped to
        [0, 1], on the images' device. One image at a time, so the peak is
        one image's tail tensors (two ``[4H, 4W, nf]`` activations: 4 GiB in
        bf16 at a 1024 x 1024 input)."""
        outs = [self(images[i:i + 1]).float().clamp_(0, 1).to(images.device)
                for i in range(images.shape[0])]
        return torch.cat(outs, 0)


def create_upscale_model(name: str = "esrgan_x4", device="cpu",
                         dtype=torch.float32, seed: int = 0) -> RRDBNet:
    """A seeded random-init RRDBNet of a named config, in eval mode."""
    if name not in UPSCALE_CONFIGS:
        raise ValueError(f"unknown upscale model {name!r}; known: "
                         f"{sorted(UPSCALE_CONFIGS)}")
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        model = RRDBNet(UPSCALE_CONFIGS[name])
    return model.to(device=device, dtype=dtype).eval().requires_grad_(False)
