// 256x256x64 MFMA GEMM / implicit-GEMM conv for the UNet trunk, on the
// 256-row tile skeleton of gemm_tile.h (thread constants, glds stages and the
// K-tile interleave are there, shared with gemm_fp8.hip). This file has the
// bf16 `cluster` (MFMA 16x16x32 under s_setprio), the conv address mode, the
// epilogue, the split-K reduce, the chooser and the launchers. It is the
// CDNA4 guide's "glds + 2 LDS buffers + BK=64" tier (§5), which ties the best
// register pipeline (~1100-1200 TF on random data) at 32 fewer VGPRs.
//
// The conv entry picks the decomposition per call (conv256_choose): N-tile
// width BN = 128 / 256 / 320 so the UNet's 320-multiples and the VAE's
// 128-wide level do not pad to 256, and a K split (third grid dimension,
// fp32 slabs, splitk_reduce_kernel) where the plain grid would leave most
// of the 256 CUs idle. Where the grid is not a whole number of rounds,
// conv256_sched gives the tiles of the last partial round to all CUs in equal
// shares of K-tile steps (stream-K tail, streamk_reduce_kernel).
//
// Two A-operand address modes share the kernel:
//   GEMM:  A[m][k]        (tokens x features; torch Linear with W[N][K])
//   CONV:  A = NHWC activations addressed per (pixel, tap) — the implicit
//          im2col: k = tap*C + c, tap shifts the source pixel, out-of-
//          bounds taps are redirected to a zero page (glds cannot
//          conditionally zero, but its per-lane SOURCE address is free).
//
// Replaces: hipBLASLt Linears (~9% of round-1 kernel time) and MIOpen
// igemm convs (~33%) — profiles/r01_prof_final_summary.csv. Reference
// counterpart: the ComfyUI conv/linear substrate of upscale/tile_ops.py
// (SURVEY.md §2.8 K6).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "gemm_tile.h"

#define GBM TILE_BM
#define GBN 256   // the GEMM entry's N-tile; the conv picks BN per call
#define GBK 64    // bf16 elements per 128-byte tile row

struct ConvGeo {
  int H, W, C;     // INPUT spatial + channels
  int Ho, Wo;      // output spatial (Ho = H/stride for 3x3 pad1)
  int stride;      // 1 or 2 (the UNet/VAE Downsample convs)
  int up2;         // 1: conv consumes a VIRTUAL nearest-2x upsample of x
                   // (Ho = 2H) — the upsampled tensor never exists, the
                   // tap address just halves: the VAE decoder's biggest
                   // intermediates (F.interpolate output + its re-read)
                   // disappear entirely
  int RS;          // 9 for 3x3 (pad 1), 1 for 1x1
  int tile2d;      // 1: blocks cover 16x16 pixel tiles (H,W % 16 == 0) —
                   // a 3x3 tap re-reads an 18x18 halo (1.27x) instead of
                   // the scanline tile's 9x; the VAE-decode C=128/256
                   // shapes are HBM-bound on exactly that re-read
  int xcd_swz;     // 1: bijective blockIdx.x -> XCD-major remap (T1)
};

// bijective XCD-aware remap (guide §5 "XCD swizzle must be bijective"):
// consecutive original ids spread across the 8 XCDs' L2s
__device__ __forceinline__ unsigned xcd_remap(unsigned id, unsigned nwg) {
  const unsigned q = nwg / 8u, r = nwg % 8u;
  const unsigned xcd = id % 8u, pos = id / 8u;
  return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + pos;
}

// ---- stream-K tail schedule (MODE_STREAMK) -------------------------------
// Tiles are numbered in launch order (tile = n_block * gx + m_block). The
// first dp_tiles tiles have one workgroup each; the rest, R tiles of kt
// K-tiles, are R * kt units in (tile, K-tile) order, cut into sk_wgs
// contiguous ranges whose lengths differ by at most one. A workgroup walks
// its range as segments (one tile, one K-tile interval). A segment covering
// a whole tile runs the epilogue; any other stores its fp32 accumulators to
// slot (range index + tile index within the tail) of the workspace: along
// the unit order every new segment advances the range, the tile or both, so
// the sum is distinct per segment and below sk_wgs + R - 1. The host
// (launcher, chooser, conv256_sk_segments) and both kernels use these
// functions, so there is one definition of the arithmetic.
struct SkSched {
  int gx;        // M-blocks per N-block row (tile -> (bx, by))
  int kt;        // K-tiles per tile
  int dp_tiles;  // tiles with one owner; workgroups [0, dp_tiles)
  int sk_wgs;    // ranges over the tail; workgroups [dp_tiles, +sk_wgs)
  int units;     // (tiles - dp_tiles) * kt
  int silu;      // the epilogue's SiLU, a runtime flag in this mode
};

struct SkSeg {
  int tile, kt0, kt1;
  int slot;      // -1: whole tile, direct epilogue
};

// units [b, e) of range j, tail-relative
__host__ __device__ inline void sk_range(const SkSched& s, int j, int& b,
                                         int& e) {
  const int q = s.units / s.sk_wgs, r = s.units % s.sk_wgs;
  b = j * q + (j < r ? j : r);
  e = b + q + (j < r ? 1 : 0);
}

// the range that holds tail-relative unit u
__host__ __device__ inline int sk_range_of(const SkSched& s, int u) {
  const int q = s.units / s.sk_wgs, r = s.units % s.sk_wgs;
  const int head = r * (q + 1);
  return u < head ? u / (q + 1) : r + (u - head) / q;
}

// first segment of tail-relative units [u, u_end) of range j
__host__ __device__ inline SkSeg sk_segment(const SkSched& s, int j, int u,
                                            int u_end) {
  SkSeg g;
  const int t_rel = u / s.kt;
  g.tile = s.dp_tiles + t_rel;
  g.kt0 = u - t_rel * s.kt;
  const int left = u_end - u;
  g.kt1 = g.kt0 + left < s.kt ? g.kt0 + left : s.kt;
  g.slot = (g.kt0 == 0 && g.kt1 == s.kt) ? -1 : j + t_rel;
  return g;
}

// Per-thread precomputed source descriptor of one A glds chunk slot
// (2 instrs x 2 pieces); the B image needs one offset for all its slots.
template <bool IS_CONV>
struct AChunk {
  // element offset from A. gemm: m*K + c. conv: image base + c, plus the
  // centre pixel (y*stride, x*stride) unless up2, so a tap is a uniform
  // offset from it; 32 bits there (the launcher checks numel < 2^32)
  typename std::conditional<IS_CONV, unsigned, long long>::type off;
  int yx;  // conv: centre pixel ((y*stride + 1) << 16) | (x*stride + 1);
           // the +1 keeps both fields >= 0 under a tap of -1, so one add
           // of (dy << 16) + dx moves both. Rows with m >= M hold
           // A_ROW_DEAD, whose y fails every bounds test. gemm: 0 = live
};
#define A_ROW_DEAD 0x7fff0001  // y field 32767: dims are checked < 16384

// How a workgroup gets its work and where the accumulators go:
//   MODE_PLAIN    one tile per workgroup, whole K, epilogue
//   MODE_SPLITK   blockIdx.z is a K-slice; raw fp32 accumulators go to slab
//                 blockIdx.z of ws (splitk_reduce_kernel runs the epilogue)
//   MODE_STREAMK  1-D grid, work from SkSched: a tile, or a range of the
//                 tail's (tile, K-tile) units walked as segments
#define MODE_PLAIN 0
#define MODE_SPLITK 1
#define MODE_STREAMK 2

// One tile (bx, by) over K-tiles [kt_begin, kt_end). BN: N-tile width, 128 /
// 256 / 320. The wave grid stays 2M x 4N, so a wave owns BN/64 16-column
// fragments (2 / 4 / 5) and the B image is BN/64 glds instructions of 8 KiB.
// dst_raw: where the raw fp32 accumulators go instead of the epilogue
// (MODE_SPLITK: the slice's [M][N] slab; MODE_STREAMK: the segment's
// [256][BN] slot, or nullptr for a whole tile).
template <bool IS_CONV, bool FUSE_SILU, int BN, int MODE>
__device__ __forceinline__ void gemm256_tile(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ Bw,
    const float* __restrict__ bias,
    const uint16_t* __restrict__ zero_page,
    const uint16_t* __restrict__ residual, uint16_t* __restrict__ Y,
    float* __restrict__ dst_raw, long long M, int N, int Kdim,
    const ConvGeo& geo, unsigned bx, unsigned gx, unsigned by, int kt_begin,
    int kt_end, bool silu_rt) {
  static_assert(BN == 128 || BN == 256 || BN == 320, "unsupported N-tile");
  constexpr int NF = BN / 64;        // 16-column fragments per wave
  constexpr int NB = BN / 64;        // B glds instructions per K-tile
  constexpr unsigned B_TILE = BN * 128u;  // one BN x 64 bf16 B image
  // Stream-K runs this body in a loop over segments: the thread id is opaque
  // there, so what derives from it is computed per segment as in the other
  // modes, not hoisted out of that loop to live through the K loop, where
  // the registers are not there (116-128 bytes/lane of scratch when tried)
  int tid = threadIdx.x;
  if constexpr (MODE == MODE_STREAMK) asm volatile("" : "+v"(tid));
  const TileThread t = tile_thread(tid);
  // scalar copies for the lambdas to capture: through the struct the code is
  // the same but every register is numbered differently (r11_gemm_tile.md)
  const int wave = t.wave, wm = t.wm, wn = t.wn, fr = t.fr, kgrp = t.kgrp,
            r0 = t.r0;

  // A images then B images, byte offsets per gemm_tile.h. One object per
  // kernel: the function is inlined once into each
  __shared__ __align__(16) uint16_t lds[32768 + BN * 128];
  uint8_t* const lds8 = reinterpret_cast<uint8_t*>(lds);

  if (IS_CONV && geo.xcd_swz) bx = xcd_remap(bx, gx);
  // output size for the tile -> pixel maps below. Opaque per segment in
  // stream-K, like tid: what derives from it (the constants of the divisions)
  // is otherwise kept in scalar registers through the K loop, and BN = 320
  // has none left (16 bytes/lane of scratch when tried)
  int out_h = geo.Ho, out_w = geo.Wo;
  if constexpr (MODE == MODE_STREAMK)
    asm volatile("" : "+s"(out_h), "+s"(out_w));
  long long m_blk = 0;
  int t_b = 0, t_py0 = 0, t_px0 = 0;
  if (IS_CONV && geo.tile2d) {
    const int tx_n = out_w >> 4;
    const int per_img = tx_n * (out_h >> 4);
    t_b = (int)(bx / per_img);
    const int rem = (int)(bx % per_img);
    t_py0 = (rem / tx_n) << 4;
    t_px0 = (rem % tx_n) << 4;
  } else {
    m_blk = (long long)bx * GBM;
  }
  const int n_blk = by * BN;

  // ---- per-thread glds chunk descriptors (chunk map: gemm_tile.h) --------
  const int c_loc = (int)(t.c_byte >> 1);  // channel offset within the row
  // B instr j reads row bn0 + 64*j: one pointer, a uniform stride per j
  const int bn0 = n_blk + r0;
  const long long b_off = (long long)bn0 * Kdim + c_loc;
  AChunk<IS_CONV> a_desc[2][2];   // [a_piece][instr]
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      // ---- A piece pc: image rows pc*128..+128 (quarter-permuted):
      // img_row = pc*128 + i*64 + r0, quarter qq = pc*2 + i
      const int m_local = t.a_row(0, pc, i);
      AChunk<IS_CONV> d;
      if (IS_CONV) {
        long long img;
        int py, px;
        bool ok = true;
        if (geo.tile2d) {
          py = t_py0 + (m_local >> 4);
          px = t_px0 + (m_local & 15);
          img = (long long)t_b * geo.H * geo.W * geo.C;
        } else {
          const long long m = m_blk + m_local;
          ok = m < M;
          const long long HWo = (long long)out_h * out_w;
          const long long mm = ok ? m : 0;
          const int pb = (int)(mm / HWo);
          const int rem = (int)(mm - (long long)pb * HWo);
          py = rem / out_w;   // OUTPUT pixel coords
          px = rem % out_w;
          img = (long long)pb * geo.H * geo.W * geo.C;
        }
        // up2 halves the tap coordinate, so only the plain modes can fold
        // the centre pixel into the pointer
        const long long pix =
            geo.up2 ? 0
                    : ((long long)py * geo.stride * geo.W +
                       (long long)px * geo.stride) * geo.C;
        d.off = img + pix + c_loc;
        d.yx = ok ? ((py * geo.stride + 1) << 16) | (px * geo.stride + 1)
                  : A_ROW_DEAD;
      } else {
        const long long m = m_blk + m_local;
        const bool ok = m < M;
        d.off = (ok ? m * (long long)Kdim : 0) + c_loc;
        d.yx = ok ? 0 : A_ROW_DEAD;
      }
      a_desc[pc][i] = d;
    }
  }

  // ---- accumulators -----------------------------------------------------
  f32x4_t acc[8][NF];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // ---- glds stage of B instrs [J0, J0+JN) into buffer p (fenced at 320) --
  auto stage_b = [&](int kt, int p, auto J0, auto JN) {
    tile_stage_b<BN == 320, decltype(J0)::value, decltype(JN)::value>(
        Bw, zero_page, b_off, bn0, N, Kdim, kt * GBK,
        lds8 + (unsigned)TILE_BBUF + p * B_TILE, wave);
  };

  // ---- glds stage of one 16 KiB A piece (2 instrs) into buffer p -------
  // pc 0 = A quarters 0-1 (mq=0 rows of both wave halves), 1 = quarters
  // 2-3 (mq=1 rows)
  auto stage_a = [&](int kt, int p, int pc) {
    const int kbase = kt * GBK;
    uint8_t* const piece =
        lds8 + ((unsigned)TILE_ABUF + p * TILE_IMG + pc * 16384u);
    if constexpr (!IS_CONV) {
      tile_stage_a(A, zero_page,
                   [&](int i, long long& off) {
                     off = a_desc[pc][i].off;
                     return a_desc[pc][i].yx == 0;
                   },
                   kbase, piece, wave);
    } else {
      int tap_dy = 0, tap_dx = 0, cbase = kbase;
      if (geo.RS == 9) {
        const int tap = kbase / geo.C;
        cbase = kbase - tap * geo.C;
        tap_dy = tap / 3 - 1;
        tap_dx = tap % 3 - 1;
      }
      // the tap's offset from the centre pixel is the same for every lane
      const long long tap_off =
          ((long long)tap_dy * geo.W + tap_dx) * geo.C + cbase;
      const int tap_dq = tap_dy * 65536 + tap_dx;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        AChunk<IS_CONV> d = a_desc[pc][i];
        if constexpr (BN == 320) {
          // opaque to the optimiser: otherwise it hoists the 64-bit
          // address parts of all four slots out of the K loop, and with
          // 160 accumulators those registers are not there (32 bytes/lane
          // of scratch, reloaded inside the loop)
          asm volatile("" : "+v"(d.off), "+v"(d.yx));
        }
        // tap coordinate + 1 in both fields; (unsigned)(v - 1) < dim
        // is the two-sided bounds test
        const int q = d.yx + tap_dq;
        const unsigned ty = (unsigned)(q >> 16) - 1u;
        const unsigned tx = (unsigned)(q & 0xffff) - 1u;
        const uint16_t* src;
        if (geo.up2) {
          // pad is applied on the VIRTUAL upsampled canvas [2H, 2W]
          const bool ok = ty < 2u * geo.H && tx < 2u * geo.W;
          src = ok ? A + d.off +
                         ((long long)(ty >> 1) * geo.W + (tx >> 1)) * geo.C +
                         cbase
                   : zero_page;
        } else {
          const bool ok = ty < (unsigned)geo.H && tx < (unsigned)geo.W;
          src = ok ? A + d.off + tap_off : zero_page;
        }
        // wave-uniform LDS base; hardware adds lane*16
        glds16(src, piece + (wave * 64u + i * 512u) * 16u);
      }
    }
  };

  // ---- one cluster: A rows of half mq x fragments [nf0, nf0+nfn) over the
  // K-tile's 64-deep K (8*nfn MFMA; a quadrant of 16 at BN = 256) ---------
  auto compute_cluster = [&](int p, auto MQ, auto NF0, auto NFN, auto KS0,
                             auto KSN) {
    constexpr int mq = decltype(MQ)::value;
    constexpr int nf0 = decltype(NF0)::value;
    constexpr int nfn = decltype(NFN)::value;
    constexpr int ks0 = decltype(KS0)::value;  // 32-deep k-steps [ks0,
    constexpr int ksn = decltype(KSN)::value;  // ks0 + ksn) of the tile's 2
    const unsigned a_base = (unsigned)TILE_ABUF + p * TILE_IMG;
    const unsigned b_base = (unsigned)TILE_BBUF + p * B_TILE;
    const int qq = mq * 2 + wm;  // A image quarter for this wave
    s16x8_t af[4][ksn], bfr[nfn][ksn];
#pragma unroll
    for (int mf = 0; mf < 4; ++mf)
#pragma unroll
      for (int ks = 0; ks < ksn; ++ks) {
        const unsigned lo =
            (qq * 64 + mf * 16 + fr) * 128u + (ks0 + ks) * 64u +
            kgrp * 16u;
        af[mf][ks] = *reinterpret_cast<const s16x8_t*>(
            lds + ((a_base + swz(lo)) >> 1));
      }
#pragma unroll
    for (int nf = 0; nf < nfn; ++nf)
#pragma unroll
      for (int ks = 0; ks < ksn; ++ks) {
        const int brow = wn * (BN / 4) + (nf0 + nf) * 16 + fr;
        const unsigned lo = brow * 128u + (ks0 + ks) * 64u + kgrp * 16u;
        bfr[nf][ks] = *reinterpret_cast<const s16x8_t*>(
            lds + ((b_base + swz(lo)) >> 1));
      }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mf = 0; mf < 4; ++mf)
#pragma unroll
      for (int nf = 0; nf < nfn; ++nf)
#pragma unroll
        for (int ks = 0; ks < ksn; ++ks)
          // operands swapped: the 16x16 result is the transposed tile, so
          // a lane holds 4 adjacent COLUMNS (n = kgrp*4 + reg) of one row
          // (m = fr) and the epilogue stores 8 bytes per fragment, not four
          // 2-byte pieces (the A and B fragment maps are the same form, so
          // the swap needs no other change)
          acc[mq * 4 + mf][nf0 + nf] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  bfr[nf][ks], af[mf][ks], acc[mq * 4 + mf][nf0 + nf],
                  0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  // one (mq, fragment range) cluster over the whole 64-deep K-tile. At
  // BN = 320 the 160 accumulators leave no room for both k-steps' fragments
  // at once (136 bytes/lane of scratch when tried), so it runs them in turn.
  auto cluster = [&](int p, auto MQ, auto NF0, auto NFN) {
    if constexpr (BN == 320) {
      compute_cluster(p, MQ, NF0, NFN, ic<0>{}, ic<1>{});
      compute_cluster(p, MQ, NF0, NFN, ic<1>{}, ic<1>{});
    } else {
      compute_cluster(p, MQ, NF0, NFN, ic<0>{}, ic<2>{});
    }
  };

  // ---- main loop: prologue stage, then one tile_ktile per K-tile ----------
  stage_b(kt_begin, 0, ic<0>{}, ic<NB>{});
  stage_a(kt_begin, 0, 0);
  stage_a(kt_begin, 0, 1);
  for (int kt = kt_begin; kt < kt_end; ++kt) {
    const int p = (kt - kt_begin) & 1;
    const bool more = kt + 1 < kt_end;
    tile_ktile<BN>(p, kt + 1, more, stage_b, stage_a, cluster);
  }

  // the lane's place in the tile, for the stores
  const int e_row = wm * 128 + fr, e_col = wn * (BN / 4) + kgrp * 4;

  // A lane holds, per fragment, columns n0..n0+3 (n0 = 16*nf + 4*kgrp) of
  // row m = 16*mf + fr. With N % 4 == 0 those 4 values are one aligned
  // vector in a row-major [M][N] array and a live n0 means 4 live columns;
  // any other N takes them one by one.
  const bool vec4 = (N & 3) == 0;

  if constexpr (MODE == MODE_STREAMK) {
    // ---- partial segment: the whole 256 x BN accumulator image to its
    // slot, tile-local and unmasked (rows past M and columns past N hold
    // what the zero page gave them; the reduce pass reads live ones only)
    if (dst_raw) {
#pragma unroll
      for (int mf = 0; mf < 8; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
          *reinterpret_cast<f32x4_t*>(
              dst_raw + (e_row + mf * 16) * BN + e_col + nf * 16) =
              acc[mf][nf];
      return;
    }
  }
  const bool silu = FUSE_SILU || (MODE == MODE_STREAMK && silu_rt);

#pragma unroll
  for (int mf = 0; mf < 8; ++mf) {
    long long m;
    if (IS_CONV && geo.tile2d) {
      const int idx = e_row + mf * 16;
      m = ((long long)t_b * out_h + t_py0 + (idx >> 4)) * out_w + t_px0 +
          (idx & 15);
    } else {
      m = m_blk + e_row + mf * 16;
      if (m >= M) continue;
    }
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const int n0 = n_blk + e_col + nf * 16;
      if (n0 >= N) continue;
      if constexpr (MODE == MODE_SPLITK) {
        // ---- split-K: raw fp32 accumulators to this slice's slab -------
        float* dst = dst_raw + m * N + n0;
        if (vec4) {
          *reinterpret_cast<f32x4_t*>(dst) = acc[mf][nf];
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (n0 + c < N) dst[c] = acc[mf][nf][c];
        }
      } else {
        // ---- epilogue: bias + optional SiLU (+ residual), bf16 store ---
        if (vec4) {
          f32x4_t v = acc[mf][nf];
          if (bias) v += *reinterpret_cast<const f32x4_t*>(bias + n0);
          if (silu) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = silu_f(v[c]);
          }
          if (residual) {
            const u16x4_t r =
                *reinterpret_cast<const u16x4_t*>(residual + m * N + n0);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] += bf16_bits_to_f32(r[c]);
          }
          u16x4_t o;
#pragma unroll
          for (int c = 0; c < 4; ++c) o[c] = f32_to_bf16_bits(v[c]);
          *reinterpret_cast<u16x4_t*>(Y + m * N + n0) = o;
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (n0 + c >= N) break;
            float v = acc[mf][nf][c] + (bias ? bias[n0 + c] : 0.f);
            if (silu) v = silu_f(v);
            if (residual) v += bf16_bits_to_f32(residual[m * N + n0 + c]);
            Y[m * N + n0 + c] = f32_to_bf16_bits(v);
          }
        }
      }
    }
  }
}

template <bool IS_CONV, bool FUSE_SILU, int BN, int MODE>
__global__ __launch_bounds__(512, 1) void gemm256_kernel(
    const uint16_t* __restrict__ A,   // gemm: [M,K]; conv: NHWC activations
    const uint16_t* __restrict__ Bw,  // [N, K] (conv: repacked [K_out][RS*C])
    const float* __restrict__ bias,   // [N] or nullptr
    const uint16_t* __restrict__ zero_page,  // >=16B of zeros
    const uint16_t* __restrict__ residual,   // [M, N] bf16 or nullptr:
                                             // fused skip-connection add
    uint16_t* __restrict__ Y,         // [M, N] bf16
    float* __restrict__ ws,           // MODE_SPLITK: fp32 slabs [gridDim.z]
                                      // [M][N]; MODE_STREAMK: slots [256][BN]
    long long M, int N, int Kdim, ConvGeo geo, SkSched sk) {
  auto tile = [&](unsigned bx, unsigned gx, unsigned by, int kt_begin,
                  int kt_end, float* dst_raw) {
    gemm256_tile<IS_CONV, FUSE_SILU, BN, MODE>(
        A, Bw, bias, zero_page, residual, Y, dst_raw, M, N, Kdim, geo, bx, gx,
        by, kt_begin, kt_end, sk.silu != 0);
  };
  if constexpr (MODE == MODE_PLAIN) {
    tile(blockIdx.x, gridDim.x, blockIdx.y, 0, Kdim / GBK, nullptr);
  } else if constexpr (MODE == MODE_SPLITK) {
    // slice blockIdx.z of gridDim.z contiguous K-tile ranges whose lengths
    // differ by at most one
    const int nkt = Kdim / GBK, ns = (int)gridDim.z, s = (int)blockIdx.z;
    const int q = nkt / ns, r = nkt % ns;
    const int kt_begin = s * q + (s < r ? s : r);
    tile(blockIdx.x, gridDim.x, blockIdx.y, kt_begin,
         kt_begin + q + (s < r ? 1 : 0), ws + (long long)s * M * N);
  } else {
    const int w = (int)blockIdx.x;
    // a data-parallel workgroup is one whole-tile segment of the same loop
    // (one inlined copy of the tile body)
    const bool dp = w < sk.dp_tiles;
    // consecutive ranges share a tile's pixels and weights: with the XCD
    // renumbering they go to one XCD's L2. That holds where dp_tiles is a
    // multiple of 8, so that workgroup w runs on XCD (w - dp_tiles) % 8: the
    // chooser's dp_tiles (whole rounds) always is, a pinned one need not be.
    // Speed only: any bijection of the range index gives the same result.
    int j = w - sk.dp_tiles;
    if (!dp && IS_CONV && geo.xcd_swz)
      j = (int)xcd_remap((unsigned)j, (unsigned)sk.sk_wgs);
    int u = 0, u_end = sk.kt;
    if (!dp) sk_range(sk, j, u, u_end);
    while (u < u_end) {
      const SkSeg g =
          dp ? SkSeg{w, 0, sk.kt, -1} : sk_segment(sk, j, u, u_end);
      tile((unsigned)(g.tile % sk.gx), (unsigned)sk.gx,
           (unsigned)(g.tile / sk.gx), g.kt0, g.kt1,
           g.slot < 0 ? nullptr : ws + (long long)g.slot * (GBM * BN));
      u += g.kt1 - g.kt0;
      if (u < u_end) {
        // the next prologue stages into the LDS images this segment's last
        // K-tile was read from: every wave's fragment reads first
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
    }
  }
}

// Second pass of a stream-K tail: a thread owns 4 adjacent columns of one row
// of one tail tile. A tile cut between ranges j0..j1 has one slot per range,
// j + (tile index in the tail) (SkSched); they are added in range order,
// which is K order, then bias, SiLU and residual once and one bf16 rounding.
// A tile inside one range was finished by its workgroup. No slot is read
// that was not written by this call, and the order is fixed, so results
// repeat bit for bit.
template <int BN>
__global__ __launch_bounds__(256) void streamk_reduce_kernel(
    const float* __restrict__ ws, const float* __restrict__ bias,
    const uint16_t* __restrict__ residual, uint16_t* __restrict__ Y,
    long long M, int N, ConvGeo geo, SkSched sk) {
  constexpr int NG = BN / 4;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(t % NG);
  const int idx = (int)((t / NG) % GBM);
  const int t_rel = (int)(t / ((long long)NG * GBM));
  if (t_rel * sk.kt >= sk.units) return;
  const int j0 = sk_range_of(sk, t_rel * sk.kt);
  const int j1 = sk_range_of(sk, (t_rel + 1) * sk.kt - 1);
  if (j0 == j1) return;
  const int tile = sk.dp_tiles + t_rel;
  unsigned bx = (unsigned)(tile % sk.gx);
  if (geo.xcd_swz) bx = xcd_remap(bx, (unsigned)sk.gx);
  long long m;
  if (geo.tile2d) {
    const int tx_n = geo.Wo >> 4;
    const int per_img = tx_n * (geo.Ho >> 4);
    const int rem = (int)(bx % per_img);
    m = ((long long)(bx / per_img) * geo.Ho + ((rem / tx_n) << 4) +
         (idx >> 4)) * geo.Wo + ((rem % tx_n) << 4) + (idx & 15);
  } else {
    m = (long long)bx * GBM + idx;
  }
  const int n0 = (tile / sk.gx) * BN + cg * 4;
  if (m >= M || n0 >= N) return;
  const float* src =
      ws + (long long)(j0 + t_rel) * (GBM * BN) + idx * BN + cg * 4;
  f32x4_t v = *reinterpret_cast<const f32x4_t*>(src);
  for (int j = j0 + 1; j <= j1; ++j)
    v += *reinterpret_cast<const f32x4_t*>(src + (long long)(j - j0) *
                                                     (GBM * BN));
  if ((N & 3) == 0) {
    if (bias) v += *reinterpret_cast<const f32x4_t*>(bias + n0);
    if (sk.silu) {
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = silu_f(v[c]);
    }
    if (residual) {
      const u16x4_t r =
          *reinterpret_cast<const u16x4_t*>(residual + m * N + n0);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] += bf16_bits_to_f32(r[c]);
    }
    u16x4_t o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = f32_to_bf16_bits(v[c]);
    *reinterpret_cast<u16x4_t*>(Y + m * N + n0) = o;
  } else {
    for (int c = 0; c < 4 && n0 + c < N; ++c) {
      float x = v[c];
      if (bias) x += bias[n0 + c];
      if (sk.silu) x = silu_f(x);
      if (residual) x += bf16_bits_to_f32(residual[m * N + n0 + c]);
      Y[m * N + n0 + c] = f32_to_bf16_bits(x);
    }
  }
}

// Second pass of a split-K conv: sum the slices' slabs in slice order in
// fp32, then bias, SiLU and residual once, one bf16 rounding. A thread owns
// 4 adjacent columns of one row: one 16-byte slab load per slice and one
// 8-byte store when N % 4 == 0. The order of additions is fixed, so results
// repeat bit for bit.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(
    const float* __restrict__ ws,     // [S][M][N]
    const float* __restrict__ bias,   // [N] or nullptr
    const uint16_t* __restrict__ residual,  // [M, N] bf16 or nullptr
    uint16_t* __restrict__ Y,         // [M, N] bf16
    long long M, int N, int S, int fuse_silu) {
  const int ng = (N + 3) >> 2;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M * ng) return;
  const long long m = t / ng;
  const int n0 = (int)(t - m * ng) * 4;
  const long long slab = M * N;
  const float* src = ws + m * N + n0;
  if ((N & 3) == 0) {
    f32x4_t v = *reinterpret_cast<const f32x4_t*>(src);
    for (int s = 1; s < S; ++s)
      v += *reinterpret_cast<const f32x4_t*>(src + s * slab);
    if (bias) v += *reinterpret_cast<const f32x4_t*>(bias + n0);
    if (fuse_silu) {
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = silu_f(v[c]);
    }
    if (residual) {
      const u16x4_t r =
          *reinterpret_cast<const u16x4_t*>(residual + m * N + n0);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] += bf16_bits_to_f32(r[c]);
    }
    u16x4_t o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = f32_to_bf16_bits(v[c]);
    *reinterpret_cast<u16x4_t*>(Y + m * N + n0) = o;
  } else {
    for (int c = 0; c < 4 && n0 + c < N; ++c) {
      float v = src[c];
      for (int s = 1; s < S; ++s) v += src[c + s * slab];
      if (bias) v += bias[n0 + c];
      if (fuse_silu) v = silu_f(v);
      if (residual) v += bf16_bits_to_f32(residual[m * N + n0 + c]);
      Y[m * N + n0 + c] = f32_to_bf16_bits(v);
    }
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

// One launch for every instantiation: the runtime flags pick the bool template
// arguments. A split conv (grid.z > 1) leaves SiLU to splitk_reduce_kernel;
// a stream-K conv (sk non-null, 1-D grid) takes it from sk->silu.
template <bool IS_CONV, int BN>
static void gemm256_launch(dim3 grid, hipStream_t stream, bool fuse_silu,
                           const uint16_t* x, const uint16_t* w,
                           const float* bias, const uint16_t* zero,
                           const uint16_t* res, uint16_t* y, float* ws,
                           long long M, int N, int Kdim, ConvGeo geo,
                           const SkSched* sk = nullptr) {
  const SkSched sched = sk ? *sk : SkSched{0, 0, 0, 0, 0, 0};
  auto go = [&](auto SILU, auto MODE) {
    hipLaunchKernelGGL((gemm256_kernel<IS_CONV, decltype(SILU)::value, BN,
                                       decltype(MODE)::value>),
                       grid, dim3(512), 0, stream, x, w, bias, zero, res, y,
                       ws, M, N, Kdim, geo, sched);
  };
  if constexpr (IS_CONV) {
    if (sk) return go(std::false_type{}, ic<MODE_STREAMK>{});
    if (grid.z > 1) return go(std::false_type{}, ic<MODE_SPLITK>{});
  }
  if (fuse_silu) go(std::true_type{}, ic<MODE_PLAIN>{});
  else go(std::false_type{}, ic<MODE_PLAIN>{});
}

torch::Tensor gemm256_bf16(torch::Tensor x, torch::Tensor w,
                           torch::Tensor bias, bool fuse_silu) {
  // (plain-GEMM entry has no residual fusion)
  // x [M, K] bf16, w [N, K] bf16 (torch Linear layout) -> y [M, N] bf16
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
              x.is_contiguous());
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 &&
              w.is_contiguous());
  const long long M = x.size(0);
  const int K = (int)x.size(1), N = (int)w.size(0);
  TORCH_CHECK(w.size(1) == K && K % GBK == 0, "K must be a multiple of 64");
  auto y = torch::empty({M, (long long)N}, x.options());
  torch::Tensor bf32;
  const float* bptr = bias_f32_ptr(bias, bf32);
  dim3 grid((unsigned)((M + GBM - 1) / GBM), (unsigned)((N + GBN - 1) / GBN));
  auto stream = at::hip::getCurrentHIPStream();
  ConvGeo geo{0, 0, 0, 0, 0, 1, 0, 0, 0, 0};
  gemm256_launch<false, GBN>(
      grid, stream, fuse_silu, (const uint16_t*)x.data_ptr(),
      (const uint16_t*)w.data_ptr(), bptr,
      (const uint16_t*)device_zero_page(x), nullptr, (uint16_t*)y.data_ptr(),
      nullptr, M, N, K, geo);
  HIP_CHECK_LAUNCH();
  return y;
}

// ---------------------------------------------------------------------------
// conv: N-tile width and K split per call
// ---------------------------------------------------------------------------
// One workgroup per CU (LDS), 256 CUs: a launch takes rounds x per-tile time.
// The constants are measured on MI355X (profiles/r07_conv_tiles.md), not
// taken from MFMA counts:
//  - a K-tile step of the 320-wide tile costs 1.13x the 256-wide one (same
//    grid at both widths: 1.801 / 1.587 ms, 0.428 / 0.377 ms), of the
//    128-wide one 0.70x (2.414 / 3.440 ms, 0.196 / 0.284 ms);
//  - under one round the reduction is split until the grid fills the round;
//    slices down to kMinSliceKtiles K-tiles still paid for their slab
//    (40 K-tiles: split 4 0.045 ms, split 3 0.050, unsplit 0.092);
//  - with both widths split to the same ~220 workgroups the wider tile has
//    fewer K-tile steps per workgroup and wins by less than the step count
//    says (9x9: 0.111 against 0.115 ms, stride-2 17x17: 0.100 against
//    0.118), so it has to be 5 % ahead on paper.
static constexpr int kNumCU = 256;
static constexpr double kStepCost128 = 0.70;
static constexpr double kStepCost320 = 1.13;
static constexpr int kMinSliceKtiles = 10;

struct ConvPlan {
  int bn, split_k;
};

static long long conv256_tiles(long long M, int K_out, int bn) {
  return ((M + GBM - 1) / GBM) * (long long)((K_out + bn - 1) / bn);
}

// split for a given width: fill at most one round, never a slice under the
// floor, 1 wherever the plain grid already has a round's worth
static int conv256_split(long long tiles, int Kdim) {
  if (tiles >= kNumCU) return 1;
  const int nkt = Kdim / GBK;
  return (int)std::max<long long>(
      1, std::min<long long>(kNumCU / tiles, nkt / kMinSliceKtiles));
}

static ConvPlan conv256_choose(long long M, int K_out, int Kdim) {
  const long long t256 = conv256_tiles(M, K_out, 256);
  if (t256 < kNumCU) {
    const int nkt = Kdim / GBK;
    const int s256 = conv256_split(t256, Kdim);
    const int s320 = conv256_split(conv256_tiles(M, K_out, 320), Kdim);
    const double c256 = (nkt + s256 - 1) / s256;
    const double c320 = (nkt + s320 - 1) / s320 * kStepCost320;
    // measured only where the 256-wide tile splits too; elsewhere keep it
    if (s256 > 1 && c320 < 0.95 * c256) return {320, s320};
    return {256, s256};
  }
  auto rounds = [](long long tiles) {
    return (double)((tiles + kNumCU - 1) / kNumCU);
  };
  ConvPlan best{256, 1};
  double cost = rounds(t256);
  // a new width has to win by more than the microbench rows' spread
  const double c320 = rounds(conv256_tiles(M, K_out, 320)) * kStepCost320;
  if (c320 < 0.97 * cost) {
    best = {320, 1};
    cost = c320;
  }
  if (K_out <= 128) {
    const double c128 = rounds(conv256_tiles(M, K_out, 128)) * kStepCost128;
    if (c128 < 0.97 * cost) best = {128, 1};
  }
  return best;
}

std::tuple<int64_t, int64_t> conv256_plan(int64_t M, int64_t K_out,
                                          int64_t Kdim) {
  TORCH_CHECK(M > 0 && K_out > 0 && Kdim > 0 && Kdim % GBK == 0);
  const ConvPlan p = conv256_choose(M, (int)K_out, (int)Kdim);
  return {p.bn, p.split_k};
}

// ---------------------------------------------------------------------------
// conv: width and stream-K tail together, by predicted time
// ---------------------------------------------------------------------------
// conv256_choose counts whole rounds. Where the last round is partly filled
// its R tiles can instead be cut into kNumCU equal shares of K-tile steps
// (SkSched above), which costs L = ceil(R * KT / kNumCU) steps instead of KT,
// plus what the cut itself costs. Measured on MI355X with tools/kernel_bench.py
// --op conv256 --sweep (profiles/r15_conv_streamk.md, section 2), in units of
// one 256-wide K-tile step (2.08 us):
//  - a tail call ends 40-50 us (K_out 4 at BN 128: 21 us) after full rounds +
//    L steps would, with 95-130 MB (42 MB) of fp32 slots written and read
//    once more: kSkSegSteps for the second pipeline fill and the slot stores
//    of a workgroup, kSkReduceStepsPerMB per MB of slots for the reduce;
//  - with every CU busy a step is slower than in a partly filled round, and
//    at BN 320 that grows with L (17x17: 65 us over at L 105, 93 at L 209):
//    kSkTailStep on the tail's steps.
// The tail path is taken where it is predicted kSkMargin ahead of the
// round-counting plan (the rows it was taken on measured 8-25 % faster, the
// one row predicted 3 % ahead measured 2.5 %); not where R = 0, where the
// last round is nearly full (kSkMaxFill), where a share would be under
// kMinSliceKtiles K-tiles (shares of 3-5 K-tiles: four rows slower, one 4 %
// and one 0.5 % faster), or where the plan already splits K (9x9 rows: tail
// 0.115 / 0.193 ms against split 5's 0.111 / 0.192).
static constexpr double kSkSegSteps = 3.0;
static constexpr double kSkReduceStepsPerMB = 0.17;
static constexpr double kSkTailStep = 1.15;
static constexpr double kSkMargin = 0.96;
static constexpr double kSkMaxFill = 0.85;

struct ConvSched {
  int bn, split_k;
  long long dp_tiles;  // tiles with one owner (all of them when sk_wgs = 0)
  int sk_wgs;          // 0: no tail path
};

static bool conv256_streamk_enabled() {
  static const bool on = [] {
    const char* e = getenv("DISTGPU_CONV_STREAMK");
    return !e || e[0] == '1';
  }();
  return on;
}

static double conv256_step_cost(int bn) {
  return bn == 320 ? kStepCost320 : bn == 128 ? kStepCost128 : 1.0;
}

static ConvSched conv256_sched_choose(long long M, int K_out, int Kdim) {
  const ConvPlan base = conv256_choose(M, K_out, Kdim);
  const int nkt = Kdim / GBK;
  const long long t_base = conv256_tiles(M, K_out, base.bn);
  ConvSched best{base.bn, base.split_k, t_base, 0};
  if (!conv256_streamk_enabled() || base.split_k > 1) return best;
  const double base_cost = (double)((t_base + kNumCU - 1) / kNumCU) * nkt *
                           conv256_step_cost(base.bn);
  double cost = kSkMargin * base_cost;
  // widths: the plan's own and 320 (measured: 256 -> 320 on the 34x34, 17x17
  // and 17 -> 34 up2 rows); other changes of width are not measured
  const int widths[2] = {base.bn, 320};
  for (int i = 0; i < (base.bn == 320 || K_out <= 128 ? 1 : 2); ++i) {
    const int bn = widths[i];
    const long long tiles = conv256_tiles(M, K_out, bn);
    const long long R = tiles % kNumCU;
    if (R == 0 || R > kSkMaxFill * kNumCU) continue;
    if (tiles < kNumCU && conv256_split(tiles, Kdim) > 1) continue;
    // the floor is on the shortest range, floor(R * nkt / kNumCU); the
    // longest, L, is what the tail takes
    if (R * nkt / kNumCU < kMinSliceKtiles) continue;
    const long long L = (R * nkt + kNumCU - 1) / kNumCU;
    const double step = conv256_step_cost(bn);
    const double slot_mb = (double)(kNumCU + R - 1) * GBM * bn * 4 / 1e6;
    const double c = (double)(tiles / kNumCU) * nkt * step +
                     kSkTailStep * L * step + kSkSegSteps +
                     kSkReduceStepsPerMB * slot_mb;
    if (c < cost) {
      cost = c;
      best = {bn, 1, tiles - R, kNumCU};
    }
  }
  return best;
}

std::tuple<int64_t, int64_t, int64_t, int64_t> conv256_sched(int64_t M,
                                                             int64_t K_out,
                                                             int64_t Kdim) {
  TORCH_CHECK(M > 0 && K_out > 0 && Kdim > 0 && Kdim % GBK == 0);
  const ConvSched s = conv256_sched_choose(M, (int)K_out, (int)Kdim);
  return {s.bn, s.split_k, s.dp_tiles, s.sk_wgs};
}

// Every segment of a pinned tail schedule, as (range, tile, kt0, kt1, slot)
// rows with slot -1 for a whole tile: the kernel's walk, run on the host
// through the same functions (tests compare it with their own arithmetic).
std::vector<std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t>>
conv256_sk_segments(int64_t tiles, int64_t kt, int64_t dp_tiles,
                    int64_t sk_wgs) {
  TORCH_CHECK(tiles > 0 && kt > 0 && dp_tiles >= 0 && dp_tiles <= tiles &&
              sk_wgs >= 1 && (tiles - dp_tiles) * kt < (1LL << 31));
  const SkSched s{1, (int)kt, (int)dp_tiles, (int)sk_wgs,
                  (int)((tiles - dp_tiles) * kt), 0};
  std::vector<std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t>> out;
  for (int j = 0; j < s.sk_wgs; ++j) {
    int u, u_end;
    sk_range(s, j, u, u_end);
    while (u < u_end) {
      const SkSeg g = sk_segment(s, j, u, u_end);
      TORCH_CHECK(sk_range_of(s, u) == j && sk_range_of(s, u_end - 1) == j);
      out.emplace_back(j, g.tile, g.kt0, g.kt1, g.slot);
      u += g.kt1 - g.kt0;
    }
  }
  return out;
}

// x [B,H,W,C] bf16 NHWC, wt [K_out, rs*C] repacked -> y [B,Ho,Wo,K], by the
// schedule `pick` returns for (M, Kdim)
template <typename Pick>
static torch::Tensor conv256_run(torch::Tensor x, torch::Tensor wt,
                                 torch::Tensor bias, torch::Tensor residual,
                                 int64_t B, int64_t H, int64_t W, int64_t C,
                                 int64_t K, int64_t rs, int64_t stride,
                                 bool up2, bool fuse_silu, const Pick& pick) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
              x.is_contiguous());
  TORCH_CHECK(wt.is_cuda() && wt.is_contiguous());
  TORCH_CHECK(rs == 9 || rs == 1);
  TORCH_CHECK(stride == 1 || (stride == 2 && rs == 9));
  TORCH_CHECK(!up2 || (stride == 1 && rs == 9));
  TORCH_CHECK(C % GBK == 0, "C must be a multiple of 64");
  // 3x3 always pad 1: Ho = ceil(H/stride) (stride 2 needs even dims for
  // the torch formula (H+2-3)/2+1 = H/2 when H even); up2 doubles
  const int64_t Ho = up2 ? 2 * H : (stride == 1 ? H : (H + 2 - 3) / 2 + 1);
  const int64_t Wo = up2 ? 2 * W : (stride == 1 ? W : (W + 2 - 3) / 2 + 1);
  TORCH_CHECK(H < 16384 && W < 16384, "pixel coords are packed in 16 bits");
  TORCH_CHECK(x.numel() < (1LL << 32), "activation offsets are 32-bit");
  const long long M = B * Ho * Wo;
  const int Kdim = (int)(rs * C);
  TORCH_CHECK(wt.numel() == K * (int64_t)Kdim, "weight must be [K, rs*C]");
  const ConvSched plan = pick(M, Kdim);
  auto y = torch::empty({B, Ho, Wo, K}, x.options());
  torch::Tensor bf32;
  const float* bptr = bias_f32_ptr(bias, bf32);
  static const int xcd_swz = [] {
    const char* e = getenv("DISTGPU_CONV_XCDSWZ");
    return (!e || e[0] == '1') ? 1 : 0;
  }();
  const int tile2d = (Ho % 16 == 0 && Wo % 16 == 0) ? 1 : 0;
  const unsigned gx = tile2d
      ? (unsigned)(B * (Ho / 16) * (Wo / 16))
      : (unsigned)((M + GBM - 1) / GBM);
  dim3 grid(gx, (unsigned)((K + plan.bn - 1) / plan.bn),
            (unsigned)plan.split_k);
  auto stream = at::hip::getCurrentHIPStream();
  ConvGeo geo{(int)H, (int)W, (int)C, (int)Ho, (int)Wo, (int)stride,
              up2 ? 1 : 0, (int)rs, tile2d, xcd_swz};
  const uint16_t* resptr = nullptr;
  if (residual.defined() && residual.numel() > 0) {
    TORCH_CHECK(residual.is_cuda() && residual.is_contiguous() &&
                residual.scalar_type() == at::kBFloat16 &&
                residual.numel() == M * K,
                "residual must be a contiguous bf16 [B,Ho,Wo,K] tensor");
    resptr = (const uint16_t*)residual.data_ptr();
  }
  // split-K slabs: fp32 [split_k][M][K] from torch's caching allocator
  // (safe under graph capture); every slice writes every element, so no
  // memset
  torch::Tensor ws;
  float* wsptr = nullptr;
  if (plan.split_k > 1) {
    ws = torch::empty({(long long)plan.split_k * M * K},
                      x.options().dtype(at::kFloat));
    wsptr = ws.data_ptr<float>();
  }
  // stream-K tail: one 1-D grid, data-parallel tiles first, then the ranges;
  // slots [sk_wgs + R - 1][256][bn] fp32 from the same allocator, each one
  // that the reduce pass reads written whole by one segment, so no memset
  SkSched sk{(int)gx, Kdim / GBK, 0, 0, 0, fuse_silu ? 1 : 0};
  const bool tail = plan.sk_wgs > 0;
  if (tail) {
    const long long tiles = (long long)gx * grid.y;
    const long long R = tiles - plan.dp_tiles;
    TORCH_CHECK(plan.split_k == 1 && plan.dp_tiles >= 0 && R >= 0,
                "dp_tiles must be in [0, tiles]");
    TORCH_CHECK(tiles * sk.kt < (1LL << 31) &&
                plan.dp_tiles + plan.sk_wgs < (1LL << 31),
                "schedule units are 32-bit");
    sk.dp_tiles = (int)plan.dp_tiles;
    sk.sk_wgs = plan.sk_wgs;
    sk.units = (int)(R * sk.kt);
    grid = dim3((unsigned)(plan.dp_tiles + (R > 0 ? plan.sk_wgs : 0)));
    if (R > 0) {
      ws = torch::empty({(plan.sk_wgs + R - 1) * (long long)GBM * plan.bn},
                        x.options().dtype(at::kFloat));
      wsptr = ws.data_ptr<float>();
    }
  }
  const uint16_t* xp = (const uint16_t*)x.data_ptr();
  const uint16_t* wp = (const uint16_t*)wt.data_ptr();
  uint16_t* yp = (uint16_t*)y.data_ptr();
  const uint16_t* zp = (const uint16_t*)device_zero_page(x);
  auto launch = [&](auto BN) {
    constexpr int bn = decltype(BN)::value;
    gemm256_launch<true, bn>(grid, stream, fuse_silu, xp, wp, bptr, zp,
                             resptr, yp, wsptr, M, (int)K, Kdim, geo,
                             tail ? &sk : nullptr);
    HIP_CHECK_LAUNCH();
    if (tail && sk.units > 0) {
      const long long nthreads =
          (long long)(sk.units / sk.kt) * GBM * (bn / 4);
      hipLaunchKernelGGL(streamk_reduce_kernel<bn>,
                         dim3((unsigned)((nthreads + 255) / 256)), dim3(256),
                         0, stream, (const float*)wsptr, bptr, resptr, yp, M,
                         (int)K, geo, sk);
      HIP_CHECK_LAUNCH();
    }
  };
  if (plan.bn == 128) launch(ic<128>{});
  else if (plan.bn == 320) launch(ic<320>{});
  else launch(ic<256>{});
  if (plan.split_k > 1) {
    const long long nthreads = M * ((K + 3) / 4);
    hipLaunchKernelGGL(splitk_reduce_kernel,
                       dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0,
                       stream, (const float*)wsptr, bptr, resptr, yp, M,
                       (int)K, plan.split_k, fuse_silu ? 1 : 0);
    HIP_CHECK_LAUNCH();
  }
  return y;
}

torch::Tensor conv256_nhwc_ex(torch::Tensor x, torch::Tensor wt,
                              torch::Tensor bias, torch::Tensor residual,
                              int64_t B, int64_t H,
                              int64_t W, int64_t C, int64_t K, int64_t rs,
                              int64_t stride, bool up2, bool fuse_silu,
                              int64_t bn, int64_t split_k) {
  // bn (128/256/320) and split_k pin the variant; 0 leaves it to the
  // chooser. split_k above the K-tile count is clamped to it. With both 0
  // this is conv256_sched's answer, tail path included; a pinned call never
  // takes the tail path.
  TORCH_CHECK(bn == 0 || bn == 128 || bn == 256 || bn == 320,
              "bn must be 0, 128, 256 or 320");
  TORCH_CHECK(split_k >= 0, "split_k must be >= 0");
  return conv256_run(
      x, wt, bias, residual, B, H, W, C, K, rs, stride, up2, fuse_silu,
      [&](long long M, int Kdim) -> ConvSched {
        if (bn == 0 && split_k == 0)
          return conv256_sched_choose(M, (int)K, Kdim);
        ConvPlan plan = conv256_choose(M, (int)K, Kdim);
        if (bn != 0 && bn != plan.bn)
          plan = {(int)bn,
                  conv256_split(conv256_tiles(M, (int)K, (int)bn), Kdim)};
        if (split_k != 0)
          plan.split_k = (int)std::min<int64_t>(split_k, Kdim / GBK);
        return {plan.bn, plan.split_k, conv256_tiles(M, (int)K, plan.bn), 0};
      });
}

torch::Tensor conv256_nhwc_sk(torch::Tensor x, torch::Tensor wt,
                              torch::Tensor bias, torch::Tensor residual,
                              int64_t B, int64_t H,
                              int64_t W, int64_t C, int64_t K, int64_t rs,
                              int64_t stride, bool up2, bool fuse_silu,
                              int64_t bn, int64_t dp_tiles, int64_t sk_wgs) {
  // the whole schedule pinned: width bn, the first dp_tiles tiles one
  // workgroup each, the rest cut into sk_wgs >= 1 ranges. dp_tiles = tiles
  // runs every tile whole, through the stream-K kernel.
  TORCH_CHECK(bn == 128 || bn == 256 || bn == 320,
              "bn must be 128, 256 or 320");
  TORCH_CHECK(sk_wgs >= 1 && sk_wgs < (1LL << 30), "sk_wgs must be >= 1");
  return conv256_run(x, wt, bias, residual, B, H, W, C, K, rs, stride, up2,
                     fuse_silu, [&](long long, int) -> ConvSched {
                       return {(int)bn, 1, dp_tiles, (int)sk_wgs};
                     });
}

torch::Tensor conv256_nhwc(torch::Tensor x, torch::Tensor wt,
                           torch::Tensor bias, torch::Tensor residual,
                           int64_t B, int64_t H,
                           int64_t W, int64_t C, int64_t K, int64_t rs,
                           int64_t stride, bool up2, bool fuse_silu) {
  return conv256_nhwc_ex(x, wt, bias, residual, B, H, W, C, K, rs, stride,
                         up2, fuse_silu, 0, 0);
}
