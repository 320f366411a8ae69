#!/usr/bin/env python3
"""Kernel microbenchmarks on MI355X: attention / groupnorm / tile ops.

Usage (on a GPU box):
    python tools/kernel_bench.py [--op attn|gn|glue|dit|conv256|fp8|norm_fp8|all] [--iters 50]

Prints per-shape timings + achieved TFLOP/s (attention) / GB/s (norms),
and an eager-torch comparison where applicable.
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from comfyui_distributed_amd.ops import dispatch  # noqa: E402


def timeit(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_attn(iters):
    print("== attention (bf16, fwd) ==")
    shapes = [
        # (name, BH, Nq, Nk, D, heads)  — SD1.5/SDXL/WAN hot shapes
        ("sd15 self 68x68 b16", 128, 4624, 4624, 40, 8),
        ("sd15 self 34x34 b16", 128, 1156, 1156, 80, 8),
        ("sd15 self 17x17 b16", 128, 289, 289, 160, 8),
        ("sd15 cross 68x68", 128, 4624, 77, 40, 8),
        ("sdxl self 64x64 b4", 80, 4096, 4096, 64, 20),
        ("wan self 32k d128", 16, 32760, 32760, 128, 16),
    ]
    for name, bh, nq, nk, d, heads in shapes:
        q = torch.randn(bh, nq, d, device="cuda", dtype=torch.bfloat16) / 2
        k = torch.randn(bh, nk, d, device="cuda", dtype=torch.bfloat16) / 2
        v = torch.randn(bh, nk, d, device="cuda", dtype=torch.bfloat16)

        t = timeit(lambda: dispatch.attention(q, k, v, heads=heads), iters)
        dp = dispatch._dpad_for(d)
        flops = 4 * bh * nq * nk * d  # 2 gemms, real D
        flops_pad = 4 * bh * nq * nk * dp
        print(f"{name:24s} D={d:3d}->{dp:3d}  {t*1e3:8.3f} ms  "
              f"{flops/t/1e12:7.1f} TF (real) {flops_pad/t/1e12:7.1f} TF (padded)")

    # the layouts the flagship runs: q/k/v read through strides out of the
    # fused projection outputs (one key's D values sit 3*H*D elements apart)
    print("== attention, fused-projection layouts (bf16, fwd) ==")
    fused = [
        # (name, B, Nq, Nk, heads, D); Nk == Nq -> attention_qkv
        ("sd15 qkv 68x68 b32", 32, 4624, 4624, 8, 40),
        ("sd15 qkv 34x34 b32", 32, 1156, 1156, 8, 80),
        ("sd15 q+kv 68x68 b32", 32, 4624, 77, 8, 40),
    ]
    for name, b, nq, nk, heads, d in fused:
        hd = heads * d
        if nk == nq:
            qkv = torch.randn(b, nq, 3 * hd, device="cuda",
                              dtype=torch.bfloat16) / 2
            fn = lambda: dispatch.attention_qkv(qkv, heads=heads)  # noqa: E731
        else:
            q = torch.randn(b, nq, hd, device="cuda", dtype=torch.bfloat16) / 2
            kv = torch.randn(b, nk, 2 * hd, device="cuda",
                             dtype=torch.bfloat16) / 2
            fn = lambda: dispatch.attention_q_kv(q, kv, heads=heads)  # noqa: E731
        t = timeit(fn, iters)
        flops = 4 * b * heads * nq * nk * d
        print(f"{name:24s} D={d:3d}->{dispatch._dpad_for(d):3d}  "
              f"{t*1e3:8.3f} ms  {flops/t/1e12:7.1f} TF (real)")


def bench_gn(iters):
    print("== fused GroupNorm+SiLU NCHW (bf16) ==")
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    for shape in [(16, 320, 68, 68), (16, 640, 34, 34), (16, 1280, 17, 17),
                  (8, 512, 136, 136), (1, 128, 1088, 1088)]:
        x = torch.randn(*shape, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(shape[1], device="cuda")
        b = torch.randn(shape[1], device="cuda")
        t = timeit(lambda: mod.group_norm_fused(x, 32, w, b, 1e-5, True), iters)
        gb = 2 * x.numel() * 2 / 1e9  # read + write bf16
        # eager comparison
        import torch.nn.functional as F

        xf = x
        te = timeit(lambda: F.silu(F.group_norm(xf.float(), 32, w, b, 1e-5)).to(torch.bfloat16), iters)
        print(f"{str(shape):24s} {t*1e3:7.3f} ms  {gb/t:7.0f} GB/s   "
              f"eager {te*1e3:7.3f} ms ({te/t:4.1f}x)")


def bench_gn_nhwc(iters):
    print("== fused GroupNorm+SiLU NHWC/channels-last (bf16) — the hot one ==")
    import torch.nn.functional as F

    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    # (B, H, W, C): UNet trunk levels at tile_batch=16, VAE decode stages
    for shape in [(16, 68, 68, 320), (16, 34, 34, 640), (16, 17, 17, 1280),
                  (16, 136, 136, 512), (16, 272, 272, 512),
                  (16, 544, 544, 128), (1, 1088, 1088, 128)]:
        x = torch.randn(*shape, device="cuda", dtype=torch.bfloat16)
        C = shape[3]
        w = torch.randn(C, device="cuda")
        b = torch.randn(C, device="cuda")
        y = mod.group_norm_nhwc(x, 32, w, b, 1e-5, True)
        # reference: fp32 NCHW group_norm on the same data
        xf = x.permute(0, 3, 1, 2).float()
        ref = F.silu(F.group_norm(xf, 32, w, b, 1e-5)).permute(0, 2, 3, 1)
        err = (y.float() - ref).abs().max().item()
        t = timeit(lambda: mod.group_norm_nhwc(x, 32, w, b, 1e-5, True), iters)
        gb = 3 * x.numel() * 2 / 1e9  # 2 reads + 1 write bf16
        print(f"{str(shape):24s} {t*1e3:7.3f} ms  {gb/t:7.0f} GB/s  "
              f"maxerr {err:.4f}")


# GroupNorm rows of the flagship (SD1.5 USDU 4x, tile batch 16 -> B = 32 with
# CFG): (name, B, H, W, C), G = 32. The decoder's concatenated inputs carry
# the widths 640/960/1920/2560; the VAE rows run at B = 16.
GN_UNET_ROWS = [
    ("unet 68 C320", 32, 68, 68, 320),
    ("unet 68 C640", 32, 68, 68, 640),
    ("unet 68 C960", 32, 68, 68, 960),
    ("unet 34 C320", 32, 34, 34, 320),
    ("unet 34 C640", 32, 34, 34, 640),
    ("unet 34 C960", 32, 34, 34, 960),
    ("unet 34 C1280", 32, 34, 34, 1280),
    ("unet 34 C1920", 32, 34, 34, 1920),
    ("unet 17 C640", 32, 17, 17, 640),
    ("unet 17 C1280", 32, 17, 17, 1280),
    ("unet 17 C1920", 32, 17, 17, 1920),
    ("unet 17 C2560", 32, 17, 17, 2560),
    ("unet 9 C1280", 32, 9, 9, 1280),
    ("unet 9 C2560", 32, 9, 9, 2560),
    ("vae 68 C512", 16, 68, 68, 512),
    ("vae 136 C512", 16, 136, 136, 512),
    ("vae 272 C512", 16, 272, 272, 512),
    ("vae 272 C256", 16, 272, 272, 256),
    ("vae 544 C256", 16, 544, 544, 256),
    ("vae 544 C128", 16, 544, 544, 128),
]
# GEGLU rows: (rows, I) of the proj_in output [rows, 2*I]
GEGLU_ROWS = [(32 * 4624, 1280), (32 * 1156, 2560), (32 * 289, 5120)]


def bench_gn_unet(iters, rounds=2):
    """group_norm_nhwc (+SiLU) at the flagship's own shapes. GB/s counts two
    reads and one write of the tensor; min..max over ``rounds`` timings."""
    print("== GroupNorm+SiLU NHWC, flagship shapes (bf16, G=32) ==")
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    for name, b, h, w, c in GN_UNET_ROWS:
        x = torch.randn(b, h, w, c, device="cuda", dtype=torch.bfloat16)
        wt = torch.randn(c, device="cuda")
        bs = torch.randn(c, device="cuda")
        fn = lambda: mod.group_norm_nhwc(x, 32, wt, bs, 1e-5, True)  # noqa: E731
        ts = [timeit(fn, iters) for _ in range(rounds)]
        nbytes = 3 * x.numel() * 2
        print(f"{name:16s} B{b:<3d} {nbytes/3e6:7.1f} MB  "
              f"{min(ts)*1e6:8.1f}..{max(ts)*1e6:8.1f} us  "
              f"{nbytes/min(ts)/1e9:7.0f} GB/s", flush=True)
        del x


def bench_geglu(iters, rounds=2):
    """act_mul (GELU) on the two chunk(2, -1) halves of a [rows, 2*I] buffer,
    read in place ("strided") against contiguous copies made beforehand
    ("copied", the copies not timed). GB/s counts two reads and one write of
    a half."""
    print("== GEGLU act_mul: strided halves vs contiguous copies (bf16) ==")
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    for rows, inner in GEGLU_ROWS:
        buf = torch.randn(rows, 2 * inner, device="cuda", dtype=torch.bfloat16)
        a, g = buf.chunk(2, dim=-1)
        ac, gc = a.contiguous(), g.contiguous()
        nbytes = 3 * ac.numel() * 2
        ts = [timeit(lambda: mod.act_mul(a, g, True), iters)
              for _ in range(rounds)]
        tc = [timeit(lambda: mod.act_mul(ac, gc, True), iters)
              for _ in range(rounds)]
        print(f"[{rows}, 2*{inner}]  strided {min(ts)*1e6:8.1f}..{max(ts)*1e6:8.1f} us "
              f"{nbytes/min(ts)/1e9:7.0f} GB/s | copied {min(tc)*1e6:8.1f}.."
              f"{max(tc)*1e6:8.1f} us {nbytes/min(tc)/1e9:7.0f} GB/s",
              flush=True)
        del buf, a, g, ac, gc


def bench_conv(iters):
    print("== conv3x3 bf16: ours (NHWC MFMA) vs MIOpen NCHW vs MIOpen CL ==")
    from comfyui_distributed_amd.ops import dispatch

    shapes = [
        # (B, C, H, W, K) — UNet/VAE hot shapes at tile batch 16
        (16, 320, 68, 68, 320),
        (16, 640, 34, 34, 640),
        (16, 1280, 17, 17, 1280),
        (1, 512, 136, 136, 512),
        (1, 256, 544, 544, 256),
        (1, 128, 1088, 1088, 128),
    ]
    for b, c, h, w, k in shapes:
        conv = torch.nn.Conv2d(c, k, 3, padding=1).cuda().to(torch.bfloat16)
        x = (torch.randn(b, c, h, w) / 4).cuda().to(torch.bfloat16)
        xcl = x.contiguous(memory_format=torch.channels_last)
        conv_cl = torch.nn.Conv2d(c, k, 3, padding=1).cuda().to(torch.bfloat16) \
            .to(memory_format=torch.channels_last)
        t_ours = timeit(lambda: dispatch.conv2d_mfma(xcl, conv), iters)
        t_nchw = timeit(lambda: conv(x), iters)
        t_cl = timeit(lambda: conv_cl(xcl), iters)
        flops = 2 * b * h * w * k * c * 9
        print(f"B{b} C{c} {h}x{w} K{k}: ours {t_ours*1e3:7.3f} ms "
              f"({flops/t_ours/1e12:6.1f} TF) | miopen-nchw {t_nchw*1e3:7.3f} "
              f"| miopen-cl {t_cl*1e3:7.3f}")


def bench_gemm(iters):
    print("== gemm256 bf16 (glds 256-tile) vs hipBLASLt ==")
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    shapes = [
        # (M, N, K) — UNet Linear hot shapes at tile_batch 16 (2x CFG batch)
        (32 * 4624, 320, 320),    # qkv proj level0 (N=960 fused)
        (32 * 4624, 960, 320),    # fused qkv
        (32 * 4624, 2560, 320),   # GEGLU in
        (32 * 4624, 320, 1280),   # GEGLU out
        (32 * 1156, 1920, 640),
        (32 * 289, 3840, 1280),
        (8192, 8192, 8192),       # reference square
    ]
    for (M, N, K) in shapes:
        x = (torch.randn(M, K, device="cuda") / 4).to(torch.bfloat16)
        w = (torch.randn(N, K, device="cuda") / 4).to(torch.bfloat16)
        b = torch.empty(0, device="cuda")
        t = timeit(lambda: mod.gemm256_bf16(x, w, b, False), iters)
        tl = timeit(lambda: torch.nn.functional.linear(x, w), iters)
        fl = 2.0 * M * N * K
        print(f"M{M} N{N} K{K}: ours {t*1e3:7.3f} ms ({fl/t/1e12:6.1f} TF) | "
              f"blaslt {tl*1e3:7.3f} ms ({fl/tl/1e12:6.1f} TF)")


# conv256 rows: (name, B, C, H, W, K, stride, up2). H, W are the INPUT size.
# The first six are the rows this bench has always had; the rest are the
# flagship UNet shapes they left out (9x9 and 17x17 levels, the decoder's
# concatenated inputs, the stride-2 downsample, the fused 2x upsample).
CONV256_ROWS = [
    ("unet 68 320->320", 32, 320, 68, 68, 320, 1, False),
    ("unet 34 640->640", 32, 640, 34, 34, 640, 1, False),
    ("unet 17 1280->1280", 32, 1280, 17, 17, 1280, 1, False),
    ("vae 136 512->512", 16, 512, 136, 136, 512, 1, False),
    ("vae 272 256->256", 16, 256, 272, 272, 256, 1, False),
    ("vae 544 128->128", 16, 128, 544, 544, 128, 1, False),
    ("unet 9 1280->1280", 32, 1280, 9, 9, 1280, 1, False),
    ("unet 9 2560->1280", 32, 2560, 9, 9, 1280, 1, False),
    ("unet 17 2560->1280", 32, 2560, 17, 17, 1280, 1, False),
    ("unet 68 960->320", 32, 960, 68, 68, 320, 1, False),
    ("unet 68 640->320", 32, 640, 68, 68, 320, 1, False),
    ("unet 34->17 s2 640->640", 32, 640, 34, 34, 640, 2, False),
    ("unet 34->68 up2 640->640", 32, 640, 34, 34, 640, 1, True),
    ("unet 17->34 up2 1280->1280", 32, 1280, 17, 17, 1280, 1, True),
    ("unet 68 320->4 out", 32, 320, 68, 68, 4, 1, False),
    # 1x1 skip convs of the decoder (rs = 1: 40 and 30 K-tiles)
    ("unet 9 1x1 2560->1280", 32, 2560, 9, 9, 1280, 1, False, 1),
    ("unet 17 1x1 1920->1280", 32, 1920, 17, 17, 1280, 1, False, 1),
]
# same M and K_out, C = 64 / 128 / 320: time against K-tile count, whose
# intercept is the prologue + epilogue cost of a workgroup
CONV256_INTERCEPT = [("68 C%d->320" % c, 32, c, 68, 68, 320, 1, False)
                     for c in (64, 128, 320)]


def _conv256_inputs(b, c, h, w, k, rs=9):
    x = (torch.randn(b, h, w, c, device="cuda") / 4).to(torch.bfloat16)
    wt = (torch.randn(k, rs * c, device="cuda") / 8).to(torch.bfloat16)
    bias = torch.randn(k, device="cuda")
    nores = torch.empty(0, device="cuda", dtype=torch.bfloat16)
    return x, wt, bias, nores


def bench_conv256(iters, sweep=False, rounds=2):
    """The 256-tile conv at every flagship shape, through the extension
    entry the models use. ``rounds`` timings per row (min and max printed:
    the row's spread) and the schedule conv256_sched gives it. With
    ``sweep``, also every pinned (bn, split_k) the chooser could take and the
    pinned stream-K tail at each width, so its thresholds and cost constants
    can be read off the table."""
    print("== conv256 (glds template), 3x3 unless named 1x1 ==")
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    has_ex = hasattr(mod, "conv256_nhwc_ex")
    for name, b, c, h, w, k, stride, up2, *rest in (CONV256_ROWS
                                                    + CONV256_INTERCEPT):
        rs = rest[0] if rest else 9
        x, wt, bias, nores = _conv256_inputs(b, c, h, w, k, rs)
        ho = 2 * h if up2 else (h - 1) // stride + 1
        wo = 2 * w if up2 else (w - 1) // stride + 1
        m, kdim = b * ho * wo, rs * c
        flops = 2.0 * m * k * kdim
        plan = tuple(mod.conv256_plan(m, k, kdim)) if has_ex else (256, 1)
        has_sk = hasattr(mod, "conv256_nhwc_sk")
        sched = tuple(mod.conv256_sched(m, k, kdim)) if has_sk else None

        def run(bn, split):
            if bn is None:
                fn = lambda: mod.conv256_nhwc(  # noqa: E731
                    x, wt, bias, nores, b, h, w, c, k, rs, stride, up2, False)
            else:
                fn = lambda: mod.conv256_nhwc_ex(  # noqa: E731
                    x, wt, bias, nores, b, h, w, c, k, rs, stride, up2, False,
                    bn, split)
            ts = [timeit(fn, iters) for _ in range(rounds)]
            return min(ts), max(ts)

        def run_sk(bn, dp, wgs):
            fn = lambda: mod.conv256_nhwc_sk(  # noqa: E731
                x, wt, bias, nores, b, h, w, c, k, rs, stride, up2, False,
                bn, dp, wgs)
            ts = [timeit(fn, iters) for _ in range(rounds)]
            return min(ts), max(ts)

        lo, hi = run(None, 0)
        tail = ""
        if sched and sched[3]:
            tail = (f" -> sched bn{sched[0]} dp{sched[2]} + {sched[3]} ranges"
                    f" over {-(-m // 256) * -(-k // sched[0]) - sched[2]}"
                    " tiles")
        elif sched:
            tail = " (no tail)"
        print(f"{name:26s} M{m} K{k} kt{kdim // 64}: plan bn{plan[0]} "
              f"split{plan[1]}{tail}  {lo*1e3:7.3f}..{hi*1e3:7.3f} ms "
              f"({flops/lo/1e12:6.1f} TF)", flush=True)
        if not (sweep and has_ex):
            continue
        for bn in (128, 256, 320):
            if bn == 128 and k > 256:
                continue
            tiles = -(-m // 256) * -(-k // bn)
            splits = [1]
            if tiles < 256:
                splits += [s for s in (2, 3, 4, 5, 6, 8) if tiles * s <= 288]
            for split in splits:
                lo, hi = run(bn, split)
                print(f"    bn{bn} split{split} ({tiles * split:5d} wg): "
                      f"{lo*1e3:7.3f}..{hi*1e3:7.3f} ms "
                      f"({flops/lo/1e12:6.1f} TF)", flush=True)
            # the stream-K tail at this width: whole rounds data-parallel,
            # the remainder in one round of ranges (L K-tile steps each)
            rem = tiles % 256
            if has_sk and rem and rem * (kdim // 64) >= 256:
                lo, hi = run_sk(bn, tiles - rem, 256)
                print(f"    bn{bn} tail dp{tiles - rem} + 256 ranges over "
                      f"{rem} tiles (L {-(-rem * (kdim // 64) // 256)}): "
                      f"{lo*1e3:7.3f}..{hi*1e3:7.3f} ms "
                      f"({flops/lo/1e12:6.1f} TF)", flush=True)


def bench_conv256_vs(iters):
    print("== conv256 (glds template) vs conv v2 vs MIOpen-CL ==")
    from comfyui_distributed_amd.ops import dispatch

    for name, b, c, h, w, k, stride, up2, *_ in CONV256_ROWS[:6]:
        conv = torch.nn.Conv2d(c, k, 3, padding=1).cuda().to(torch.bfloat16)
        x = (torch.randn(b, c, h, w) / 4).cuda().to(torch.bfloat16)
        xcl = x.contiguous(memory_format=torch.channels_last)
        conv_cl = torch.nn.Conv2d(c, k, 3, padding=1).cuda().to(torch.bfloat16) \
            .to(memory_format=torch.channels_last)
        dispatch._CONV256 = True
        t256 = timeit(lambda: dispatch.conv2d_mfma(xcl, conv), iters)
        dispatch._CONV256 = False
        tv2 = timeit(lambda: dispatch.conv2d_mfma(xcl, conv), iters)
        dispatch._CONV256 = True
        tmi = timeit(lambda: conv_cl(xcl), iters)
        flops = 2.0 * b * h * w * k * c * 9
        print(f"B{b} C{c} {h}x{w} K{k}: 256 {t256*1e3:7.3f} ms "
              f"({flops/t256/1e12:6.1f} TF) | v2 {tv2*1e3:7.3f} "
              f"({flops/tv2/1e12:6.1f} TF) | miopen-cl {tmi*1e3:7.3f} "
              f"({flops/tmi/1e12:6.1f} TF)")


def bench_tiles(iters):
    print("== tile ops (f32) ==")
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    src = torch.rand(1, 4096, 4096, 3, device="cuda")
    t = timeit(lambda: mod.extract_resize(src, 512, 512, 1056, 1056, 544, 544), iters)
    print(f"extract 544 from 4K     {t*1e3:7.3f} ms")
    canvas = torch.rand(1, 4096, 4096, 3, device="cuda").contiguous()
    tile = torch.rand(1, 544, 544, 3, device="cuda")
    t = timeit(lambda: mod.blend_tile(canvas, tile, 512, 512, 1056, 1056,
                                      544, 544, 1024, 1024, 8.0), iters)
    print(f"blend 544 into 4K       {t*1e3:7.3f} ms")


def bench_dit(iters):
    """Fused dit_ops.hip kernels vs the eager torch chains (_DIT_FUSED off)
    at the WAN-14B and Flux-12B block shapes. GB/s is over the minimum
    traffic: every input read once, every output written once."""
    print("== DiT glue ops: fused HIP vs eager chain (bf16) ==")
    bf = torch.bfloat16

    def ab(name, fn, nbytes):
        # alternate the two paths, keep the best round of each
        tf = te = float("inf")
        for _ in range(3):
            dispatch._DIT_FUSED = True
            tf = min(tf, timeit(fn, iters))
            dispatch._DIT_FUSED = False
            te = min(te, timeit(fn, iters))
        dispatch._DIT_FUSED = True
        print(f"{name:34s} fused {tf*1e6:8.1f} us {nbytes/tf/1e9:7.0f} GB/s | "
              f"eager {te*1e6:8.1f} us {nbytes/te/1e9:7.0f} GB/s | "
              f"{te/tf:5.2f}x")

    for fam, b, n, c, h, mode in [("wan14b", 2, 4500, 5120, 40, "rms"),
                                  ("flux12b", 1, 4608, 3072, 24, "layer")]:
        d = c // h
        act = b * n * c * 2  # one bf16 activation tensor, bytes
        x = torch.randn(b, n, c, device="cuda", dtype=bf)
        y = torch.randn(b, n, c, device="cuda", dtype=bf)
        w = torch.randn(c, device="cuda") if mode == "rms" else None
        wq = torch.randn(d, device="cuda")
        wk = torch.randn(d, device="cuda")
        ang = torch.rand(n, d // 2, device="cuda") * 6.28
        cos, sin = ang.cos(), ang.sin()
        if fam == "wan14b":
            # separate q / k Linears; modulation rows of the [B, 6, C] table
            q = torch.randn(b, n, c, device="cuda", dtype=bf)
            k = torch.randn(b, n, c, device="cuda", dtype=bf)
            shift, scale, gate = torch.randn(
                b, 6, c, device="cuda", dtype=bf).unbind(1)[:3]
        else:
            # q / k read in place from the single-stream linear1 output
            proj = torch.randn(b, n, 7 * c, device="cuda", dtype=bf)
            q, k = torch.split(proj, [c, c, c, 4 * c], dim=-1)[:2]
            shift, scale, gate = torch.randn(
                b, 3 * c, device="cuda", dtype=bf).chunk(3, dim=-1)
        tag = f"{fam} [{b},{n},{c}]"
        ab(f"{tag} qk_norm_rope",
           lambda: dispatch.qk_norm_rope(q, k, wq, wk, cos, sin, h),
           4 * act + 2 * cos.numel() * 4)
        ab(f"{tag} norm_modulate/{mode}",
           lambda: dispatch.norm_modulate(x, mode, w, scale, shift),
           2 * act)
        if mode == "rms":
            ab(f"{tag} rms_norm",
               lambda: dispatch.rms_norm(x, w), 2 * act)
        ab(f"{tag} gated_residual",
           lambda: dispatch.gated_residual(x, gate, y), 3 * act)


# FP8 Linear rows: (name, M, N, K), the projection and FFN shapes of a WAN
# step at [2, 4500, 5120] and of a Flux step at 4608 tokens
FP8_ROWS = [
    ("wan qkvo", 9000, 5120, 5120),
    ("wan ffn1", 9000, 13824, 5120),
    ("wan ffn2", 9000, 5120, 13824),
    ("wan ck/cv", 1024, 5120, 4096),
    ("flux qkv", 4608, 9216, 3072),
    ("flux mlp.0", 4608, 12288, 3072),
    ("flux mlp.2", 4608, 3072, 12288),
    ("flux linear1", 4608, 21504, 3072),
    ("flux linear2", 4608, 3072, 15360),
]


def bench_fp8(iters, rounds=3):
    """Per shape: (a) F.linear bf16 (hipBLASLt), (b) quant_rows_fp8,
    (c) gemm_fp8, (d) b + c as dispatch.linear_fp8 runs them, (e)
    torch._scaled_mm with row-wise scales where this torch has it. Random
    operands; the candidates alternate inside each round and the minimum
    over the rounds is reported."""
    print("== fp8 linear (quant_rows_fp8 + gemm_fp8) vs bf16 F.linear ==")
    F = torch.nn.functional
    print(f"{'shape':>14} {'M':>5} {'N':>6} {'K':>6} | {'a bf16':>8} "
          f"{'b quant':>8} {'c gemm':>8} {'d b+c':>8} {'e smm':>8} ms | "
          f"{'a TF':>6} {'c TF':>6} {'d TF':>6} | d/a")
    for name, M, N, K in FP8_ROWS:
        x = (torch.randn(M, K, device="cuda") / 4).to(torch.bfloat16)
        w = (torch.randn(N, K, device="cuda") / 4).to(torch.bfloat16)
        bias = torch.randn(N, device="cuda")
        bias16 = bias.to(torch.bfloat16)
        qw, sw = dispatch.quantize_weight_fp8(w)
        qa, sa = dispatch.quant_rows_fp8(x)
        cands = {
            "a": lambda: F.linear(x, w, bias16),
            "b": lambda: dispatch.quant_rows_fp8(x),
            "c": lambda: dispatch.gemm_fp8(qa, sa, qw, sw, bias, None),
            "d": lambda: dispatch.linear_fp8(x, qw, sw, bias, None),
        }
        if hasattr(torch, "_scaled_mm"):
            wt, sa2, sw2 = qw.t(), sa[:, None].contiguous(), sw[None].contiguous()

            def smm():
                return torch._scaled_mm(qa, wt, scale_a=sa2, scale_b=sw2,
                                        bias=bias16, out_dtype=torch.bfloat16)
            try:
                smm()
                torch.cuda.synchronize()
                cands["e"] = smm
            except Exception as exc:  # noqa: BLE001: this build lacks it
                print(f"  (torch._scaled_mm row-wise unavailable: "
                      f"{str(exc).splitlines()[0][:80]})")
        best = {k: float("inf") for k in cands}
        for _ in range(rounds):
            for k, fn in cands.items():
                best[k] = min(best[k], timeit(fn, iters))
        fl = 2.0 * M * N * K
        e = f"{best['e']*1e3:8.3f}" if "e" in best else f"{'-':>8}"
        print(f"{name:>14} {M:5d} {N:6d} {K:6d} | {best['a']*1e3:8.3f} "
              f"{best['b']*1e3:8.3f} {best['c']*1e3:8.3f} {best['d']*1e3:8.3f} "
              f"{e}    | {fl/best['a']/1e12:6.0f} {fl/best['c']/1e12:6.0f} "
              f"{fl/best['d']/1e12:6.0f} | {best['d']/best['a']:.2f}")


def bench_norm_fp8(iters, rounds=3):
    """Norm -> FP8 rows at the WAN and Flux block shapes: (p) norm_modulate,
    (b) quant_rows_fp8 of its output, (f) norm_modulate_fp8, which replaces
    p + b. The candidates alternate inside each round; the minimum over the
    rounds is reported. GB/s of f is over its 3 bytes per element."""
    print("== norm_modulate_fp8 (f) vs norm_modulate (p) + quant_rows_fp8 (b) ==")
    bf = torch.bfloat16
    for fam, b, n, c, mode in [("wan14b", 2, 4500, 5120, "rms"),
                               ("flux12b", 1, 4608, 3072, "layer")]:
        x = torch.randn(b, n, c, device="cuda", dtype=bf)
        w = torch.randn(c, device="cuda") if mode == "rms" else None
        shift, scale = torch.randn(
            b, 6, c, device="cuda", dtype=bf).unbind(1)[:2]
        y2 = dispatch.norm_modulate(x, mode, w, scale, shift).reshape(-1, c)
        cands = {
            "p": lambda: dispatch.norm_modulate(x, mode, w, scale, shift),
            "b": lambda: dispatch.quant_rows_fp8(y2),
            "f": lambda: dispatch.norm_modulate_fp8(x, mode, w, scale, shift),
        }
        best = {k: float("inf") for k in cands}
        for _ in range(rounds):
            for k, fn in cands.items():
                best[k] = min(best[k], timeit(fn, iters))
        p, q, f = (best[k] for k in "pbf")
        print(f"{fam} [{b},{n},{c}] {mode}+mod | p {p*1e6:7.1f} us  "
              f"b {q*1e6:7.1f} us  f {f*1e6:7.1f} us "
              f"({3 * b * n * c / f / 1e9:5.0f} GB/s) | f/p {f/p:.3f}  "
              f"f/(p+b) {f/(p+q):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", default="all")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sweep", action="store_true",
                    help="conv256: also time every pinned (bn, split_k)")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    if args.op in ("attn", "all"):
        bench_attn(args.iters)
    if args.op in ("gn", "all"):
        bench_gn(args.iters)
    if args.op in ("gn_nhwc", "gn", "all"):
        bench_gn_nhwc(args.iters)
    if args.op in ("gn_unet", "glue", "all"):
        bench_gn_unet(args.iters)
    if args.op in ("geglu", "glue", "all"):
        bench_geglu(args.iters)
    if args.op in ("conv", "all"):
        bench_conv(args.iters)
    if args.op in ("gemm", "all"):
        bench_gemm(args.iters)
    if args.op in ("conv256", "all"):
        bench_conv256(args.iters, sweep=args.sweep)
    if args.op in ("conv256_vs", "all"):
        bench_conv256_vs(args.iters)
    if args.op in ("tiles", "all"):
        bench_tiles(args.iters)
    if args.op in ("dit", "all"):
        bench_dit(args.iters)
    if args.op in ("fp8", "all"):
        bench_fp8(args.iters)
    if args.op in ("norm_fp8", "fp8", "all"):
        bench_norm_fp8(args.iters)


if __name__ == "__main__":
    main()
