#!/usr/bin/env python3
"""Kernel microbenchmarks on MI355X: attention / groupnorm / tile ops.

Usage (on a GPU box):
    python tools/kernel_bench.py [--op attn|gn|glue|dit|conv256|linear_route|fp8|norm_fp8|mxfp8|attn_fp8|attn_fp8_sparse|unet_fp8|conv_fp8|rrdb|rrdb_model|all] [--iters 50]

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

    # the VAE mid-block attention as the autoencoder-KL checkpoints have it:
    # one head over all 512 channels (attn_wide_kernel<512>). Yardsticks on
    # the same tensor, same FLOPs: the 8 x 64 split the VAE used before
    # (attn_fwd_kernel<64>) and torch SDPA on strided views, the three
    # alternated within each round.
    print("== attention, single-head VAE mid block (bf16, fwd) ==")
    import torch.nn.functional as F

    for name, b, n in [("vae 68x68 tile b32", 32, 4624),
                       ("vae 136x136 b4", 4, 18496)]:
        c = 512
        qkv = torch.randn(b, n, 3 * c, device="cuda", dtype=torch.bfloat16) / 2
        q4, k4, v4 = (u.unsqueeze(1) for u in qkv.split(c, dim=-1))
        fns = {
            "wide H=1 D=512": lambda: dispatch.attention_qkv(qkv, heads=1),
            "8 x 64 (parent)": lambda: dispatch.attention_qkv(qkv, heads=8),
            "torch SDPA H=1": lambda: F.scaled_dot_product_attention(q4, k4, v4),
        }
        rounds = 5
        per = max(iters // rounds, 1)
        best = {key: float("inf") for key in fns}
        for _ in range(rounds):
            for key, fn in fns.items():
                best[key] = min(best[key], timeit(fn, per, warmup=2))
        flops = 4 * b * n * n * c
        for key, t in best.items():
            print(f"{name:20s} {key:16s} {t*1e3:9.3f} ms  "
                  f"{flops/t/1e12:7.1f} TF   "
                  f"{t/best['8 x 64 (parent)']:5.2f}x the 8-head time")


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


# fused GEGLU Linear rows: (M, K, inner) of the three UNet levels, tile batch 32
GEGLU_GEMM_ROWS = [(32 * 4624, 320, 1280), (32 * 1156, 640, 2560),
                   (32 * 289, 1280, 5120)]


def bench_geglu_gemm(iters, rounds=3):
    """gemm_geglu (f: chooser's width, f128 / f256: pinned) against the pair
    it replaces (p: F.linear on hipBLASLt + act_mul on the two halves in
    place; l: that F.linear alone), same session, candidates alternating
    inside each round; min..max over the rounds. TF counts the projection's
    2*M*K*2*inner operations."""
    print("== GEGLU Linear: gemm_geglu (f) vs F.linear + act_mul (p) ==")
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    F = torch.nn.functional
    for M, K, inner in GEGLU_GEMM_ROWS:
        x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
        w = (torch.randn(2 * inner, K, device="cuda") / K ** 0.5).to(
            torch.bfloat16)
        b = torch.randn(2 * inner, device="cuda", dtype=torch.bfloat16)
        wp, bp = dispatch.pack_geglu_weight(w, b)

        def pair():
            a, g = F.linear(x, w, b).chunk(2, dim=-1)
            return mod.act_mul(a, g, True)

        cands = {
            "p": pair,
            "l": lambda: F.linear(x, w, b),
            "f": lambda: mod.gemm_geglu(x, wp, bp),
            "f128": lambda: mod.gemm_geglu_ex(x, wp, bp, 128),
            "f256": lambda: mod.gemm_geglu_ex(x, wp, bp, 256),
        }
        ts = {k: [] for k in cands}
        for _ in range(rounds):
            for k, fn in cands.items():
                ts[k].append(timeit(fn, iters))
        fl = 4.0 * M * K * inner
        cols = "  ".join(
            f"{k} {min(v)*1e6:7.1f}..{max(v)*1e6:7.1f} us" for k, v in ts.items())
        print(f"[{M}, {K}] x [2*{inner}, {K}] | {cols} | "
              f"p {fl/min(ts['p'])/1e12:5.0f} TF  f {fl/min(ts['f'])/1e12:5.0f} TF"
              f" | f/p {max(ts['f'])/min(ts['p']):.3f} (slowest f / fastest p)",
              flush=True)
        del x, w, b, wp, bp


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


# linear_route rows: (name, M, N, K). The SD1.5 UNet Linears at tile batch 32
# (68x68, 34x34, 17x17 tokens at C = 320, 640, 1280): N in {C, 3C}, K in
# {C, 4C}; the cross-attention KV projection of 32 x 77 context tokens; the
# SDXL pair.
def _linear_route_rows():
    rows = []
    for lvl, m, c in (("68", 147968, 320), ("34", 36992, 640),
                      ("17", 9248, 1280), ("xl64", 32768, 640),
                      ("xl32", 8192, 1280)):
        for n in (c, 3 * c):
            for k in (c, 4 * c):
                if n == 3 * c and k == 4 * c:
                    continue  # no such Linear
                rows.append((f"{lvl} {k}->{n}", m, n, k))
    for c in (320, 640, 1280):
        rows.append((f"kv 768->{2 * c}", 2464, 2 * c, 768))
    # the routed SD1.5 shapes at tile batch 16 and 24, for the M ranges of
    # dispatch._LINEAR_ROUTES
    for tb in (16, 24):
        for n, k in ((320, 320), (960, 320)):
            rows.append((f"68/tb{tb} {k}->{n}", 4624 * tb, n, k))
        for n, k in ((640, 640), (640, 2560)):
            rows.append((f"34/tb{tb} {k}->{n}", 1156 * tb, n, k))
    return rows


def bench_linear_route(rounds=3):
    """gemm256_linear against F.linear (hipBLASLt) at every UNet Linear shape,
    without and with the residual operand (the library side then runs its
    product and the eager add). Per row: l = F.linear, g = gemm256_linear by
    its chooser, b128 / b256 / b320 = the width pinned (plain: conv256_split
    gives no split at any of these rows), s2 / s3 (b128s2 / b128s3) = the K
    split pinned at 256 (128) wide where the grid is under one round, sk = the
    stream-K tail pinned at the chooser's width where the grid has a partial
    round; then l+ = F.linear +
    add and g+ = gemm256_linear with res. Candidates alternate inside each
    round; min..max over the rounds in ms."""
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    print("== linear_route: gemm256_linear (g) vs F.linear (l); + = with "
          "residual ==")
    for name, M, N, K in _linear_route_rows():
        x = (torch.randn(M, K, device="cuda") / 4).to(torch.bfloat16)
        w = (torch.randn(N, K, device="cuda") / 4).to(torch.bfloat16)
        bias = torch.randn(N, device="cuda")
        bias16 = bias.to(torch.bfloat16)
        res = torch.randn(M, N, device="cuda").to(torch.bfloat16)
        nores = torch.empty(0, device="cuda", dtype=torch.bfloat16)
        bn, split, dp, skw = mod.gemm256_linear_plan(M, N, K)
        cands = {
            "l": lambda: torch.nn.functional.linear(x, w, bias16),
            "g": lambda: mod.gemm256_linear(x, w, bias, nores, False),
        }
        for b in (128, 256, 320):
            if b == 128 and N > 640:
                continue
            cands[f"b{b}"] = (lambda b=b: mod.gemm256_linear_ex(
                x, w, bias, nores, False, b, 0, 0, 0))
        # under one round of the 256 CUs: the K split pinned, 2 and 3 slices
        # at 256 wide, and at 128 wide on the context KV rows
        if -(-M // 256) * -(-N // 256) < 256:
            for sp in (2, 3):
                cands[f"s{sp}"] = (lambda sp=sp: mod.gemm256_linear_ex(
                    x, w, bias, nores, False, 256, sp, 0, 0))
                if M < 4096 and N <= 640:
                    cands[f"b128s{sp}"] = (lambda sp=sp: mod.gemm256_linear_ex(
                        x, w, bias, nores, False, 128, sp, 0, 0))
        tiles = -(-M // 256) * -(-N // bn)
        if tiles % 256 and tiles > 256 and not skw:
            cands["sk"] = lambda: mod.gemm256_linear_ex(
                x, w, bias, nores, False, bn, 1, tiles - tiles % 256, 256)
        cands["l+"] = lambda: torch.nn.functional.linear(x, w, bias16) + res
        cands["g+"] = lambda: mod.gemm256_linear(x, w, bias, res, False)
        t = _timed_rounds(cands, rounds)
        cells = "  ".join(f"{k} {v[0]*1e3:.3f}..{v[1]*1e3:.3f}"
                          for k, v in t.items())
        print(f"{name:>16} M{M} N{N} K{K} plan({bn},{split},{dp},{skw}) | "
              f"{cells} | g/l {t['g'][0]/t['l'][0]:.3f} g+/l+ "
              f"{t['g+'][0]/t['l+'][0]:.3f} g+/(g&add) "
              f"{t['g+'][0]/(t['g'][0]+t['l+'][0]-t['l'][0]):.3f}",
              flush=True)


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


# (tokens, width) of the transformer levels at tile batch 32: SD1.5's 544-px
# tiles (68^2, 34^2, 17^2 tokens) and SDXL's 1024-px (32^2, 16^2 at the two
# transformer levels)
UNET_FP8_LEVELS = [(147968, 320), (36992, 640), (9248, 1280),
                   (32768, 640), (8192, 1280)]


def bench_unet_fp8(iters, rounds=3):
    """Each UNet Linear class on the FP8 path (f) against what it replaces
    (p), same process, candidates alternating inside each round, min..max
    over the rounds:
      ln    layer_norm_fp8 + gemm_fp8        vs layer_norm + F.linear
            (N = 3C: the fused QKV; C: to_q)
      own   padded quantiser + gemm_fp8      vs F.linear
            (K = C, N = C: to_out / ST proj; K = 4C, N = C: proj_out)
      geglu layer_norm_fp8 + gemm_geglu_fp8  vs layer_norm + F.linear +
            act_mul; gg: linear_geglu_fp8 on given rows vs F.linear + act_mul
    """
    print("== UNet FP8 Linears (f) vs bf16 hipBLASLt (p) ==")
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    F = torch.nn.functional
    bf = torch.bfloat16
    for M, C in UNET_FP8_LEVELS:
        x = torch.randn(M, C, device="cuda", dtype=bf)
        h = torch.randn(M, 4 * C, device="cuda", dtype=bf)
        lw, lb = torch.randn(2, C, device="cuda").unbind(0)

        def weights(n, k):
            w = (torch.randn(n, k, device="cuda") / k ** 0.5).to(bf)
            return (w,) + dispatch.quantize_weight_fp8(w, pad_k=True)

        b_c = torch.randn(C, device="cuda")
        b_g = torch.randn(8 * C, device="cuda")
        w3, q3, s3 = weights(3 * C, C)
        w1, q1, s1 = weights(C, C)
        w4, q4, s4 = weights(C, 4 * C)
        wg = (torch.randn(8 * C, C, device="cuda") / C ** 0.5).to(bf)
        qg, sg, bg = dispatch.pack_geglu_weight_fp8(wg, b_g, pad_k=True)
        b_cb, b_gb = b_c.to(bf), b_g.to(bf)
        rows = dispatch.layer_norm_fp8(x, lw, lb)

        def ln(t):
            return dispatch.layer_norm(t, lw, lb)

        def pair_geglu(t):
            a, g = F.linear(t, wg, b_gb).chunk(2, dim=-1)
            return mod.act_mul(a, g, True)

        def own(t, q, s):
            return dispatch.linear_fp8(
                dispatch.quantize_rows(t, pad_k=t.shape[-1] % 128 != 0), q, s,
                b_c)

        cands = {
            "ln_qkv": (lambda: F.linear(ln(x), w3),
                       lambda: dispatch.linear_fp8(
                           dispatch.layer_norm_fp8(x, lw, lb), q3, s3)),
            "ln_q": (lambda: F.linear(ln(x), w1),
                     lambda: dispatch.linear_fp8(
                         dispatch.layer_norm_fp8(x, lw, lb), q1, s1)),
            "own_c": (lambda: F.linear(x, w1, b_cb), lambda: own(x, q1, s1)),
            "own_4c": (lambda: F.linear(h, w4, b_cb), lambda: own(h, q4, s4)),
            "ln_geglu": (lambda: pair_geglu(ln(x)),
                         lambda: dispatch.linear_geglu_fp8(
                             dispatch.layer_norm_fp8(x, lw, lb), qg, sg, bg)),
            "gg": (lambda: pair_geglu(x),
                   lambda: dispatch.linear_geglu_fp8(rows, qg, sg, bg)),
        }
        for name, (p, f) in cands.items():
            tp, tf = [], []
            for _ in range(rounds):
                tp.append(timeit(p, iters))
                tf.append(timeit(f, iters))
            print(f"[{M}, {C}] {name:9s} | p {min(tp)*1e6:7.1f}..{max(tp)*1e6:7.1f} us"
                  f"  f {min(tf)*1e6:7.1f}..{max(tf)*1e6:7.1f} us | f/p "
                  f"{min(tf)/min(tp):.3f} (min/min) {max(tf)/min(tp):.3f} "
                  f"(slowest f / fastest p)", flush=True)
        del x, h, rows


# (name, C_in, K_out, source H = W, up2, epilogue) of the RRDBNet convs at a
# 1024 x 1024 input: the five dense-block shapes, then the 4x tail
RRDB_SHAPES = [
    ("conv1", 64, 32, 1024, False, "lrelu"),
    ("conv2", 96, 32, 1024, False, "lrelu"),
    ("conv3", 128, 32, 1024, False, "lrelu"),
    ("conv4", 160, 32, 1024, False, "lrelu"),
    ("conv5", 192, 64, 1024, False, "res"),
    ("up1", 64, 64, 1024, True, "lrelu"),
    ("up2", 64, 64, 2048, True, "lrelu"),
    ("hr", 64, 64, 4096, False, "lrelu"),
    ("last", 64, 3, 4096, False, None),
]


def _timed_rounds(cands, rounds=3, window=0.03):
    """{name: (min, max) seconds per call}: the candidates alternate inside
    each round, each timed over enough calls for a window of tens of ms."""
    iters = {}
    for k, fn in cands.items():
        one = timeit(fn, iters=2, warmup=2)
        iters[k] = max(3, min(200, int(window / max(one, 1e-6))))
    times = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(timeit(fn, iters[k], warmup=1))
    return {k: (min(v), max(v)) for k, v in times.items()}


def bench_mxfp8(rounds=3):
    """MXFP8 rows. Per shape of FP8_ROWS: gemm_fp8 (c) against gemm_mxfp8 (m)
    on the same codes. Per feed-forward pair: gemm_fp8(act) -> quant_rows_fp8
    -> gemm_fp8 (row) against gemm_mxfp8(act, emit) -> gemm_mxfp8 (mx), both
    from rows that are quantised already. Candidates alternate inside each
    round; min and max over the rounds are printed."""
    print("== gemm_mxfp8 (m) vs gemm_fp8 (c), same codes ==")
    ops = {}
    for name, M, N, K in FP8_ROWS:
        x = (torch.randn(M, K, device="cuda") / 4).to(torch.bfloat16)
        w = (torch.randn(N, K, device="cuda") / 4).to(torch.bfloat16)
        bias = torch.randn(N, device="cuda")
        qw, sw = dispatch.quantize_weight_fp8(w)
        qa, sa = dispatch.quant_rows_fp8(x)
        qm, em = dispatch.quant_rows_mxfp8(x)
        ops[name] = (qa, sa, qm, em, qw, sw, bias)
        t = _timed_rounds({
            "c": lambda: dispatch.gemm_fp8(qa, sa, qw, sw, bias, None),
            "m": lambda: dispatch.gemm_mxfp8(qm, em, qw, sw, bias, None),
        }, rounds)
        print(f"{name:>14} {M:5d} {N:6d} {K:6d} | c {t['c'][0]*1e3:7.3f}"
              f"..{t['c'][1]*1e3:7.3f}  m {t['m'][0]*1e3:7.3f}.."
              f"{t['m'][1]*1e3:7.3f} ms | m/c {t['m'][0]/t['c'][0]:.3f}")
    print("== feed-forward pair: row = gemm_fp8(act) + quant_rows_fp8 + "
          "gemm_fp8, mx = gemm_mxfp8(act, emit) + gemm_mxfp8 ==")
    for first, second, act in (("wan ffn1", "wan ffn2", "silu"),
                               ("flux mlp.0", "flux mlp.2", "gelu_tanh")):
        qa, sa, qm, em, qw1, sw1, b1 = ops[first]
        qw2, sw2, b2 = ops[second][4:]

        def row():
            h = dispatch.gemm_fp8(qa, sa, qw1, sw1, b1, act)
            return dispatch.gemm_fp8(*dispatch.quant_rows_fp8(h), qw2, sw2, b2)

        def mx():
            q, e = dispatch.gemm_mxfp8(qm, em, qw1, sw1, b1, act, emit=True)
            return dispatch.gemm_mxfp8(q, e, qw2, sw2, b2)

        t = _timed_rounds({"row": row, "mx": mx}, rounds)
        print(f"{first:>14} -> {second:<12} | row {t['row'][0]*1e3:7.3f}.."
              f"{t['row'][1]*1e3:7.3f}  mx {t['mx'][0]*1e3:7.3f}.."
              f"{t['mx'][1]*1e3:7.3f} ms | mx/row "
              f"{t['mx'][0]/t['row'][0]:.3f}")


# conv_fp8 rows: (name, C, H, W, K_out, stride), every 3x3 conv shape of the
# SD1.5 UNet at tile batch 32 that the FP8 route covers (H, W: INPUT size)
CONV_FP8_B = 32
CONV_FP8_ROWS = [
    ("68 320->320", 320, 68, 68, 320, 1),
    ("68 960->320", 960, 68, 68, 320, 1),
    ("68 640->320", 640, 68, 68, 320, 1),
    ("68 320->4 out", 320, 68, 68, 4, 1),
    ("34 320->640", 320, 34, 34, 640, 1),
    ("34 640->640", 640, 34, 34, 640, 1),
    ("34 1920->640", 1920, 34, 34, 640, 1),
    ("34 1280->640", 1280, 34, 34, 640, 1),
    ("34 960->640", 960, 34, 34, 640, 1),
    ("17 640->1280", 640, 17, 17, 1280, 1),
    ("17 1280->1280", 1280, 17, 17, 1280, 1),
    ("17 2560->1280", 2560, 17, 17, 1280, 1),
    ("17 1920->1280", 1920, 17, 17, 1280, 1),
    ("9 1280->1280", 1280, 9, 9, 1280, 1),
    ("9 2560->1280", 2560, 9, 9, 1280, 1),
    ("68->34 s2 320->320", 320, 68, 68, 320, 2),
    ("34->17 s2 640->640", 640, 34, 34, 640, 2),
    ("17->9 s2 1280->1280", 1280, 17, 17, 1280, 2),
]


def bench_conv_fp8(rounds=3):
    """conv_fp8 against conv256_nhwc on the same tensors, alternating in one
    process: b = the bf16 conv, c = conv_fp8 alone on codes made beforehand
    (the entry's width), c256 / c320 = the same pinned to each width where
    K_out % 320 == 0, qc = quantiser + conv_fp8, what the route runs. The
    activations are SiLU outputs, as the convs see them. Rows whose qc / b is
    not below 1 belong in dispatch._CONV_FP8_LOSSES. The last lines are the
    relative rms error of both kernels against the fp64 conv of the
    unquantised operands at 68x68 C320 (batch 2)."""
    from comfyui_distributed_amd.ops import ext

    mod = ext.get_ext(True)
    b = CONV_FP8_B
    print("== conv_fp8 (c, qc = with quantiser) vs conv256_nhwc (b), 3x3, "
          f"batch {b}: min..max ms over {rounds} rounds ==")
    nores = torch.empty(0, device="cuda", dtype=torch.bfloat16)

    def operands(bb, c, h, w, k):
        x = torch.nn.functional.silu(
            torch.randn(bb, h, w, c, device="cuda")).to(torch.bfloat16)
        wt = (torch.randn(k, 9 * c, device="cuda") / (9 * c) ** 0.5).to(
            torch.bfloat16)
        return x, wt, torch.randn(k, device="cuda")

    for name, c, h, w, k, stride in CONV_FP8_ROWS:
        x, wt, bias = operands(b, c, h, w, k)
        qw, sw = dispatch.quantize_weight_fp8(wt, pad_k=True)
        q, sa = dispatch.quant_nhwc_fp8(x)
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        flops = 2.0 * b * ho * wo * k * 9 * c

        def conv(bn=0):
            return dispatch.conv_fp8(q, sa, qw, sw, bias, stride=stride, bn=bn)

        cands = {
            "b": lambda: mod.conv256_nhwc(x, wt, bias, nores, b, h, w, c, k,
                                          9, stride, False, False),
            "c": conv,
            "qc": lambda: dispatch.conv_fp8(*dispatch.quant_nhwc_fp8(x), qw,
                                            sw, bias, stride=stride),
        }
        if k % 320 == 0:
            cands["c256"] = lambda: conv(256)
            cands["c320"] = lambda: conv(320)
        t = _timed_rounds(cands, rounds)
        cells = "  ".join(
            f"{n} {t[n][0]*1e3:6.3f}..{t[n][1]*1e3:6.3f}" for n in cands)
        print(f"{name:>20} | {cells} ms | TF b {flops/t['b'][0]/1e12:5.0f} "
              f"c {flops/t['c'][0]/1e12:5.0f} | c/b {t['c'][0]/t['b'][0]:.3f} "
              f"qc/b {t['qc'][0]/t['b'][0]:.3f}", flush=True)

    c, h, w, k = 320, 68, 68, 320
    x, wt, bias = operands(2, c, h, w, k)
    qw, sw = dispatch.quantize_weight_fp8(wt, pad_k=True)
    y_q = dispatch.conv_fp8(*dispatch.quant_nhwc_fp8(x), qw, sw, bias)
    y_b = mod.conv256_nhwc(x, wt, bias, nores, 2, h, w, c, k, 9, 1, False,
                           False)
    ref = torch.nn.functional.conv2d(
        x.cpu().double().permute(0, 3, 1, 2),
        wt.cpu().double().reshape(k, 3, 3, c).permute(0, 3, 1, 2),
        bias.cpu().double(), padding=1).permute(0, 2, 3, 1)
    for tag, y in (("fp8", y_q), ("bf16", y_b)):
        err = (y.cpu().double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()
        print(f"rel rms error vs fp64 conv, 68x68 C320: {tag} {err.item():.3e}")


# the 16-head row is bench_attn's "wan self 32k d128" (profiles/r03)
ATTN_FP8_SHAPES = [("wan self 32k", 1, 32760, 40), ("wan 32k 16h", 1, 32760, 16),
                   ("wan 4.5k", 2, 4500, 40), ("flux joint", 1, 5120, 24)]


def bench_attn_fp8(rounds=3):
    """attention_fp8 against attention_packed on the same bf16 tensors, head
    dim 128: bf = attn_fwd_kernel<128>, k8 = attn_fp8_kernel on operands
    quantised beforehand, q8 = the quantiser launches + attn_fp8_kernel. TF
    counts 4 * B * H * N^2 * 128 flops. Candidates alternate inside each
    round; min..max over the rounds."""
    print("== attention_fp8 (k8 kernel, q8 quantiser + kernel) vs "
          "attention_packed (bf) ==")
    for name, b, n, h in ATTN_FP8_SHAPES:
        q, k, v = (torch.randn(b, n, h * 128, device="cuda").to(torch.bfloat16)
                   for _ in range(3))
        a = dispatch.quantize_attn_qkv(q, k, v, h)
        t = _timed_rounds({
            "bf": lambda: dispatch.attention_packed(q, k, v, heads=h),
            "k8": lambda: dispatch.attention_fp8(a),
            "q8": lambda: dispatch.attention_fp8(q, k, v, h),
        }, rounds, window=0.1)
        flop = 4.0 * b * h * n * n * 128
        print(f"{name:>13} [{b}, {n}, {h}*128] | " + "  ".join(
            f"{c} {t[c][0]*1e3:7.3f}..{t[c][1]*1e3:7.3f} ms "
            f"{flop / t[c][0] / 1e12:6.0f} TF" for c in ("bf", "k8", "q8"))
            + f" | k8/bf {t['k8'][0]/t['bf'][0]:.3f} "
            f"q8/bf {t['q8'][0]/t['bf'][0]:.3f}")


def bench_attn_fp8_sparse(rounds=3):
    """attn_fp8_sparse_kernel (s) against attn_fp8_kernel (d) on the same
    quantised operands at the WAN self-attention shape, token grid (21, 30,
    52), per window; candidates alternate inside each round, min..max over
    the rounds. Then a 2-layer WAN forward at the 14B widths (bf16 Linears,
    FP8 attention) with and without the window, alternating."""
    from comfyui_distributed_amd.models import quant
    from comfyui_distributed_amd.models.wan import WanConfig, WanModel

    grid, b, h = (21, 30, 52), 1, 40
    n = grid[0] * grid[1] * grid[2]
    windows = [("tile 3,5,13 r 1,1,1", (3, 5, 13), (1, 1, 1)),
               ("tile 3,6,13 r 1,1,1", (3, 6, 13), (1, 1, 1)),
               ("full window", (3, 6, 13), (9, 9, 9))]
    print(f"== attention_fp8(blocks=) (s) vs attention_fp8 (d), "
          f"[{b}, {n}, {h}*128], grid {grid} ==", flush=True)
    q, k, v = (torch.randn(b, n, h * 128, device="cuda").to(torch.bfloat16)
               for _ in range(3))
    a = dispatch.quantize_attn_qkv(q, k, v, h)
    for name, tile, radius in windows:
        _, _, blocks = dispatch.attn_window(grid, tile, radius, "cuda")
        cnt = blocks.cnt.cpu()
        t = _timed_rounds({
            "d": lambda: dispatch.attention_fp8(a),
            "s": lambda: dispatch.attention_fp8(a, blocks=blocks),
        }, rounds, window=0.1)
        line = (f"{name:>20} density {blocks.density:.3f} tiles/q-block "
                f"{int(cnt.min())}..{int(cnt.max())} | d {t['d'][0]*1e3:7.3f}.."
                f"{t['d'][1]*1e3:7.3f}  s {t['s'][0]*1e3:7.3f}.."
                f"{t['s'][1]*1e3:7.3f} ms | s/d {t['s'][0]/t['d'][0]:.3f} "
                f"(s/d)/density {t['s'][0]/t['d'][0]/blocks.density:.3f}")
        if blocks.density == 1.0:
            same = torch.equal(dispatch.attention_fp8(a, blocks=blocks),
                               dispatch.attention_fp8(a))
            line += f" | equal to dense: {same}"
        print(line, flush=True)
    del q, k, v, a
    torch.cuda.empty_cache()

    print("== WAN, 2 layers at the 14B widths, 32760 tokens, 512 text tokens: "
          "attn fp8 with (w) and without (n) the window ==", flush=True)
    torch.manual_seed(0)
    model = WanModel(WanConfig(num_layers=2)).to("cuda", torch.bfloat16).eval()
    quant.set_attn_dtype(model, "fp8")
    x = torch.randn(1, 16, 21, 60, 104, device="cuda", dtype=torch.bfloat16)
    ts = torch.tensor([500.0], device="cuda")
    ctx = torch.randn(1, 512, 4096, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        y0 = model(x, ts, ctx)
        for name, tile, radius in windows:
            def run(window):
                quant.set_attn_window(model, *(window or (None, None)))
                return model(x, ts, ctx)
            t = _timed_rounds({"n": lambda: run(None),
                               "w": lambda: run((tile, radius))},
                              rounds, window=0.3)
            dist = ((run((tile, radius)).float() - y0.float()).norm()
                    / y0.float().norm()).item()
            print(f"{name:>20} | n {t['n'][0]*1e3:7.1f}..{t['n'][1]*1e3:7.1f}  "
                  f"w {t['w'][0]*1e3:7.1f}..{t['w'][1]*1e3:7.1f} ms | w/n "
                  f"{t['w'][0]/t['n'][0]:.3f} | output distance {dist:.4f}",
                  flush=True)


def bench_rrdb(iters):
    """conv_dense (d) per RRDBNet shape against what the shape costs without
    it, same process, alternating: (e) the eager pieces, torch.cat of the
    dense inputs + F.conv2d on channels_last (MIOpen) + LeakyReLU or
    ``0.2 * y + x`` (+ F.interpolate in front for the up2 convs); (m)
    conv2d_mfma + the same eager pieces where that path takes the shape and
    its 32-bit offsets reach."""
    print("== conv_dense (d) vs eager cat + MIOpen conv + epilogue (e) / "
          "conv2d_mfma (m) ==", flush=True)
    F = torch.nn.functional
    bf = torch.bfloat16
    for name, c, k, hs, up2, epi in RRDB_SHAPES:
        ho = 2 * hs if up2 else hs
        conv = torch.nn.Conv2d(c, k, 3, 1, 1).cuda().to(bf)
        conv_cl = torch.nn.Conv2d(c, k, 3, 1, 1).cuda().to(bf).to(
            memory_format=torch.channels_last)
        if up2 or c + k > 192 or k < 8:
            x = torch.randn(1, hs, hs, c, device="cuda", dtype=bf) / 4
            out = torch.empty(1, ho, ho, max(k, 8), device="cuda",
                              dtype=bf)[..., :k]
        else:   # slices of one dense-block buffer, as the model runs them
            buf = torch.randn(1, hs, hs, 192, device="cuda", dtype=bf) / 4
            x, out = buf[..., :c], buf[..., c:c + k]
        res = (torch.randn(1, ho, ho, k, device="cuda", dtype=bf)
               if epi == "res" else None)
        kw = dict(lrelu=0.2) if epi == "lrelu" else (
            dict(alpha=0.2, res2=res) if epi == "res" else {})
        # the eager side's operands: the channel groups a dense block holds
        # as separate NCHW channels_last tensors
        widths = [64] + [32] * ((c - 64) // 32)
        parts = [torch.randn(1, wd, hs, hs, device="cuda", dtype=bf)
                 .contiguous(memory_format=torch.channels_last) / 4
                 for wd in widths]
        res_cl = None if res is None else res.permute(0, 3, 1, 2)

        def tail_ops(y):
            if epi == "lrelu":
                return F.leaky_relu(y, 0.2)
            if epi == "res":
                return y * 0.2 + res_cl
            return y

        def gather():
            t = parts[0] if len(parts) == 1 else torch.cat(parts, 1)
            return F.interpolate(t, scale_factor=2, mode="nearest") if up2 else t

        def eager():
            return tail_ops(conv_cl(gather()))

        def mfma():
            t = parts[0] if len(parts) == 1 else torch.cat(parts, 1)
            return tail_ops(dispatch.conv2d_mfma(t, conv, up2=up2))

        cands = {"d": lambda: dispatch.conv3x3_dense(x, conv, out, up2=up2,
                                                     **kw)}
        try:
            eager()
            torch.cuda.synchronize()
            cands["e"] = eager
        except Exception as exc:  # noqa: BLE001: MIOpen refuses the size
            print(f"  ({name}: eager baseline failed: "
                  f"{str(exc).splitlines()[0][:90]})", flush=True)
        big = max(hs * hs * c, ho * ho * max(k, 64)) * 2 >= 2 ** 31
        if dispatch.conv_supported(conv) and not big and (
                c % 64 == 0 or not up2):
            cands["m"] = mfma
        t = _timed_rounds(cands)
        fl = 2.0 * 9 * c * k * ho * ho
        line = (f"{name:>6} C{c:3d}->K{k:2d} {ho}x{ho}{' up2' if up2 else ''} | "
                f"d {t['d'][0]*1e3:7.3f}..{t['d'][1]*1e3:7.3f} ms "
                f"{fl/t['d'][0]/1e12:6.1f} TF")
        for key in ("e", "m"):
            if key in t:
                line += (f" | {key} {t[key][0]*1e3:7.3f}..{t[key][1]*1e3:7.3f}"
                         f" ms d/{key} {t['d'][0]/t[key][0]:.3f}")
        print(line, flush=True)
        del x, out, parts, res, res_cl, conv, conv_cl
        torch.cuda.empty_cache()


def bench_rrdb_model(iters, rounds=3):
    """Whole esrgan_x4 on one 1024 x 1024 image: the dense route against the
    DISTGPU_RRDB_HIP=0 (textbook, eager) route, alternating."""
    from comfyui_distributed_amd.models.upscaler import create_upscale_model

    print("== esrgan_x4, one 1024x1024 image: dense route vs DISTGPU_RRDB_HIP=0 ==",
          flush=True)
    model = create_upscale_model("esrgan_x4", device="cuda",
                                 dtype=torch.bfloat16)
    x = torch.rand(1, 1024, 1024, 3, device="cuda")
    times = {True: [], False: []}
    with torch.no_grad():
        for r in range(rounds + 1):   # round 0 is the warm-up
            for hip in (True, False):
                dispatch._RRDB_HIP = hip
                t = timeit(lambda: model(x), iters=1, warmup=0)
                if r:
                    times[hip].append(t)
                print(f"  round {r} hip={hip}: {t*1e3:.1f} ms", flush=True)
    dispatch._RRDB_HIP = True
    d, e = times[True], times[False]
    print(f"dense {min(d)*1e3:.1f}..{max(d)*1e3:.1f} ms | eager "
          f"{min(e)*1e3:.1f}..{max(e)*1e3:.1f} ms | dense/eager "
          f"{min(d)/min(e):.3f}", flush=True)


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
        bench_geglu_gemm(args.iters)
    if args.op in ("conv", "all"):
        bench_conv(args.iters)
    if args.op in ("gemm", "all"):
        bench_gemm(args.iters)
    if args.op in ("linear_route", "all"):
        bench_linear_route()
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
    if args.op in ("mxfp8", "all"):
        bench_mxfp8()
    if args.op in ("attn_fp8", "all"):
        bench_attn_fp8()
    if args.op in ("attn_fp8_sparse", "all"):
        bench_attn_fp8_sparse()
    if args.op in ("unet_fp8", "all"):
        bench_unet_fp8(args.iters)
    if args.op in ("conv_fp8", "all"):
        bench_conv_fp8()
    if args.op in ("rrdb", "all"):
        bench_rrdb(args.iters)
    if args.op in ("rrdb_model", "all"):
        bench_rrdb_model(args.iters)


if __name__ == "__main__":
    main()
