// FP8 (OCP e4m3fn) implicit-GEMM convolution for the UNet's 3x3 / 1x1 convs:
// a per-image activation quantiser and a 256 x BN x 128 block-scaled-MFMA
// conv kernel.
//
//   quant_nhwc_fp8   x [B,H,W,C] bf16 -> q [B,H,W,C] e4m3, scale [B] fp32:
//                    common.h's row formula taken over the whole image,
//                    scale = max(amax, 2^-126 * 448) * (1/448),
//                    q = rne_e4m3(clamp(x * (1/scale), +-448)). One scalar per
//                    image factors out of an im2col row, which spans nine
//                    pixels; a scale per pixel would not.
//   conv_fp8_nhwc    y[m][n] = act(acc * sa[image of m] * sw[n] + bias[n])
//                    (+ res[m][n]), acc the e4m3 dot product over k = tap*C + c
//                    against qw [K_out, Kp], Kp = RS*C rounded up to 128 with
//                    zero bytes behind RS*C. fp32 throughout, one bf16 rounding.
//
// The conv runs on the 256-tile skeleton of gemm_tile.h with gemm_fp8.hip's
// work split: 8 waves (2M x 4N), both operands glds-staged into double-
// buffered swizzled LDS images, one drain + barrier per K-tile, unconditional
// staging, operands swapped so a lane holds 4 adjacent output channels. What is
// its own is the A address mode. A K-tile is 128 e4m3 of k, and the UNet's
// C = 320, 960, 1920 are multiples of 64 only, so a K-tile can straddle a tap
// boundary, but never inside one of its two 64-byte halves. A lane's chunk
// sits at a fixed byte c_byte of the 128-byte row, so it is in the same half
// for every K-tile: per K-tile the two halves' taps are scalar, and the lane
// picks one by a predicate computed once. The half at k >= RS*C (tap index
// RS) reads the zero page like an out-of-image tap; e4m3 byte 0 is +0.
//
// Scanline M mapping (a tile may straddle images), no up2, no 2-D pixel tiles,
// no K split: the launcher's cover is 3x3 pad 1 (stride 1 or 2) and 1x1,
// C % 64 == 0, any K_out.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "gemm_tile.h"
#include "fp8_act.h"

#define CQ_BK 128  // e4m3 elements = bytes per tile row

// ---------------------------------------------------------------------------
// quantiser: two launches over a (blocks, B) grid, block j of image b owning
// the contiguous 8-element chunks [j * per, (j + 1) * per) of the image. The
// first writes the block's absmax to part[b][j]; the second re-reduces its
// image's partials (every block the same values in the same order) and
// converts its chunks. 16-byte loads, 8-byte stores, no atomics and nothing
// to clear: capture-safe, and the same bits on every call.
// ---------------------------------------------------------------------------
#define CQ_QT 256  // threads; at most CQ_QT blocks per image

__global__ void __launch_bounds__(CQ_QT)
quant_nhwc_absmax_kernel(const uint16_t* __restrict__ x,
                         float* __restrict__ part, long long chunks, int per) {
  __shared__ float red[CQ_QT / 64];
  const uint16_t* xi = x + (long long)blockIdx.y * chunks * 8;
  const long long c0 = (long long)blockIdx.x * per;
  const long long c1 = c0 + per < chunks ? c0 + per : chunks;
  float amax = 0.f;
  for (long long c = c0 + threadIdx.x; c < c1; c += CQ_QT)
    amax = fp8_absmax8(*reinterpret_cast<const ushort8_t*>(xi + c * 8), amax);
  amax = block_reduce(amax, red, MaxOp{}, 0.f);
  if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = amax;
}

__global__ void __launch_bounds__(CQ_QT)
quant_nhwc_convert_kernel(const uint16_t* __restrict__ x,
                          const float* __restrict__ part,
                          uint8_t* __restrict__ q, float* __restrict__ scale,
                          long long chunks, int per) {
  __shared__ float red[CQ_QT / 64];
  const int nb = (int)gridDim.x;  // <= CQ_QT
  float amax = (int)threadIdx.x < nb ? part[blockIdx.y * nb + threadIdx.x] : 0.f;
  amax = block_reduce(amax, red, MaxOp{}, 0.f);
  const float s = fp8_row_scale(amax);
  const float inv = fp8_row_inv_scale(s);
  if (blockIdx.x == 0 && threadIdx.x == 0) scale[blockIdx.y] = s;
  const long long img = (long long)blockIdx.y * chunks * 8;
  const long long c0 = (long long)blockIdx.x * per;
  const long long c1 = c0 + per < chunks ? c0 + per : chunks;
  for (long long c = c0 + threadIdx.x; c < c1; c += CQ_QT)
    *reinterpret_cast<u32x2_t*>(q + img + c * 8) = fp8_quant8(
        *reinterpret_cast<const ushort8_t*>(x + img + c * 8), inv);
}

// ---------------------------------------------------------------------------
// conv
// ---------------------------------------------------------------------------
struct ConvFp8Geo {
  int H, W, C;  // input
  int Ho, Wo;   // output (3x3 pad 1: ceil(H / stride))
  int stride;   // 1 or 2
  int RS;       // 9 or 1
};

// Source descriptor of one A glds slot (2 pieces x 2 instrs), K-invariant, as
// gemm.hip's AChunk<true>: the byte (= element) offset of the centre pixel's
// channel (c_byte % 64), 32 bits (the launcher checks numel < 2^32), and the
// packed centre ((y*stride + 1) << 16) | (x*stride + 1). The +1 keeps both
// fields >= 0 under a tap of -1, so one add of (dy << 16) + dx moves both and
// (unsigned)(field - 1) < dim is the two-sided bounds test.
struct AChunkQ {
  unsigned off;
  unsigned yx;
};
// rows with m >= M: the y field fails every bounds test (dims < 16384)
#define CQ_ROW_DEAD 0x7fff0001u
// the tap "delta" of a half tile at k >= RS*C: y + 16384 fails them too, and
// 0x7fff + 0x4000 stays inside the 16-bit field
#define CQ_TAP_DEAD 0x40000000u

template <int BN, int ACT>
__global__ __launch_bounds__(512, 1) void conv_fp8_kernel(
    const uint8_t* __restrict__ A,    // [B, H, W, C] e4m3
    const uint8_t* __restrict__ Bw,   // [N, Kp] e4m3, zero bytes in [RS*C, Kp)
    const float* __restrict__ sa,     // [B] image scales
    const float* __restrict__ sw,     // [N] output-channel scales
    const float* __restrict__ bias,   // [N] or nullptr
    const uint8_t* __restrict__ zero_page,   // >= 16 B of zeros
    const uint16_t* __restrict__ residual,   // [M, N] bf16 or nullptr
    uint16_t* __restrict__ Y,         // [M, N] bf16
    int M, int N, int Kp, ConvFp8Geo geo) {
  static_assert(BN == 256 || BN == 320, "unsupported N-tile");
  static_assert(ACT == ACT_NONE || ACT == ACT_SILU, "none or SiLU");
  constexpr int NF = BN / 64;   // 16-column fragments per wave
  constexpr int NB = BN / 64;   // B glds instructions per K-tile
  constexpr unsigned B_TILE = BN * 128u;
  const TileThread t = tile_thread();
  // scalar copies for the lambdas to capture (profiles/r11_gemm_tile.md)
  const int wave = t.wave, wm = t.wm, wn = t.wn, fr = t.fr, kgrp = t.kgrp,
            r0 = t.r0;

  // A images then B images, one object (a second __shared__ de-pipelines
  // the glds)
  __shared__ __align__(16) uint8_t lds[65536 + 2 * BN * 128];

  const int m_blk = (int)blockIdx.x * TILE_BM;
  const int n_blk = (int)blockIdx.y * BN;

  // ---- per-thread glds chunk descriptors (chunk map: gemm_tile.h) --------
  const int bn0 = n_blk + r0;
  const long long b_off = (long long)bn0 * Kp + t.c_byte;
  // which 64-byte half of the tile row this lane stages, for every slot and
  // every K-tile
  const bool hi = t.c_byte >= 64;
  const int c_half = t.c_byte & 63;
  AChunkQ a_desc[2][2];   // [a_piece][instr]
  {
    const int HWo = geo.Ho * geo.Wo;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) {
        const int m = t.a_row(m_blk, pc, i);
        const bool ok = m < M;
        const int mm = ok ? m : 0;
        const int pb = mm / HWo;
        const int rem = mm - pb * HWo;
        const int py = rem / geo.Wo, px = rem - py * geo.Wo;  // OUTPUT pixel
        // below 2^32: the offset of a real element
        a_desc[pc][i].off =
            ((unsigned)(pb * geo.H + py * geo.stride) * (unsigned)geo.W +
             (unsigned)(px * geo.stride)) * (unsigned)geo.C + (unsigned)c_half;
        a_desc[pc][i].yx =
            ok ? ((unsigned)(py * geo.stride + 1) << 16) |
                     (unsigned)(px * geo.stride + 1)
               : CQ_ROW_DEAD;
      }
  }

  f32x4_t acc[8][NF];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int kt_end = Kp / CQ_BK;

  // fragment read addresses, as gemm_fp8_tile
  unsigned a_lane = swz((unsigned)((wm * 64 + fr) * 128 + kgrp * 16));
  unsigned b_lane =
      swz((unsigned)((wn * (BN / 4) + fr) * 128 + kgrp * 16));
  // opaque, so the reads stay one address register + immediate offsets
  asm volatile("" : "+v"(a_lane), "+v"(b_lane));
  const uint8_t* lds_a = lds + TILE_ABUF + a_lane;
  const uint8_t* lds_b = lds + TILE_BBUF + b_lane;

  auto stage_b = [&](int kt, int p, auto J0, auto JN) {
    tile_stage_b<BN == 320, decltype(J0)::value, decltype(JN)::value>(
        Bw, zero_page, b_off, bn0, N, Kp, kt * CQ_BK,
        lds + (unsigned)TILE_BBUF + p * B_TILE, wave);
  };

  // ---- glds stage of one 16 KiB A piece (2 instrs) into buffer p ---------
  // k = tap*C + c. Half h of K-tile kt starts at k_h = kt*128 + 64*h, inside
  // one tap because C % 64 == 0: tap_h = k_h / C, channel base c_h. Half 1 is
  // the same tap 64 channels on, or channel 0 of the next tap. Both are
  // uniform; the lane takes its half's tap offset and coordinate delta.
  auto stage_a = [&](int kt, int p, int pc) {
    const int k0 = kt * CQ_BK;
    const int tap0 = k0 / geo.C;
    const int c0 = k0 - tap0 * geo.C;
    // masks and bitwise tests, not branches, here and below: with control
    // flow in the K loop the compiler sinks the MFMAs below it, behind the
    // fragment reads of all four clusters, and the accumulators spill
    const int next = -(int)(c0 + 64 >= geo.C);  // -1: half 1 is the next tap
    const int tap1 = tap0 - next;
    const int c1 = (c0 + 64) & ~next;
    const int rs9 = -(int)(geo.RS == 9);
    auto tap_terms = [&](int tap, int cbase, unsigned& off, unsigned& dq) {
      const int t3 = tap / 3;
      const int dy = (t3 - 1) & rs9, dx = (tap - t3 * 3 - 1) & rs9;
      // the tap's offset from the centre pixel, the same for every lane;
      // modulo 2^32 it adds to AChunkQ::off to a real element's offset
      off = (unsigned)((dy * geo.W + dx) * geo.C + cbase);
      const unsigned dead = 0u - (unsigned)(tap >= geo.RS);
      dq = ((unsigned)(dy * 65536 + dx) & ~dead) | (CQ_TAP_DEAD & dead);
    };
    unsigned off0, dq0, off1, dq1;
    tap_terms(tap0, c0, off0, dq0);
    tap_terms(tap1, c1, off1, dq1);
    const unsigned tap_off = hi ? off1 : off0;
    const unsigned tap_dq = hi ? dq1 : dq0;
    uint8_t* const piece =
        lds + ((unsigned)TILE_ABUF + p * TILE_IMG + pc * 16384u);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      AChunkQ d = a_desc[pc][i];
      if constexpr (BN == 320) {
        // opaque to the optimiser, as in gemm256_tile: it would otherwise
        // hoist the address parts of all four slots out of the K loop, and
        // with 160 accumulators those registers are not there
        asm volatile("" : "+v"(d.off), "+v"(d.yx));
      }
      const unsigned q = d.yx + tap_dq;
      const unsigned ty = (q >> 16) - 1u;
      const unsigned tx = (q & 0xffffu) - 1u;
      const bool ok = (ty < (unsigned)geo.H) & (tx < (unsigned)geo.W);
      const uint8_t* src = ok ? A + (unsigned)(d.off + tap_off) : zero_page;
      // wave-uniform LDS base; hardware adds lane*16
      glds16(src, piece + (wave * 64u + i * 512u) * 16u);
    }
  };

  // one cluster: A rows of half mq x fragments [nf0, nf0+nfn) over the
  // K-tile's 128-deep K: 4*nfn MFMAs. A lane's 32-byte operand is the two
  // 16-byte fragments at k-groups kgrp and kgrp + 4 of the row, for A and B
  // alike, and every block scale is 1, so whatever k permutation the
  // instruction applies inside the tile, the same products are summed.
  auto cluster = [&](int p, auto MQ, auto NF0, auto NFN) {
    constexpr int mq = decltype(MQ)::value;
    constexpr int nf0 = decltype(NF0)::value;
    constexpr int nfn = decltype(NFN)::value;
    // keep this cluster's reads behind the previous cluster's MFMAs: hoisted,
    // two clusters' fragments are live at once and the accumulators spill
    __builtin_amdgcn_sched_barrier(0);
    const uint8_t* ap = lds_a + p * TILE_IMG;
    const uint8_t* bp = lds_b + p * B_TILE;
    i32x8_t af[4], bfr[nfn];
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
      constexpr unsigned base = mq * 16384u;
      const i32x4_t h0 =
          *reinterpret_cast<const i32x4_t*>(ap + base + mf * 2048u);
      const i32x4_t h1 =
          *reinterpret_cast<const i32x4_t*>(ap + base + mf * 2048u + 64u);
      af[mf] = i32x8_t{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    }
#pragma unroll
    for (int nf = 0; nf < nfn; ++nf) {
      const i32x4_t h0 =
          *reinterpret_cast<const i32x4_t*>(bp + (nf0 + nf) * 2048u);
      const i32x4_t h1 =
          *reinterpret_cast<const i32x4_t*>(bp + (nf0 + nf) * 2048u + 64u);
      bfr[nf] = i32x8_t{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mf = 0; mf < 4; ++mf)
#pragma unroll
      for (int nf = 0; nf < nfn; ++nf)
        // operands swapped (W fragment first): the 16x16 result is the
        // transposed tile, a lane holds 4 adjacent COLUMNS n = kgrp*4 + reg
        // of row m = fr. cbsz = blgp = 0: e4m3 for both; E8M0 scale bytes
        // 0x7f = 1.0
        acc[mq * 4 + mf][nf0 + nf] =
            __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                bfr[nf], af[mf], acc[mq * 4 + mf][nf0 + nf], 0, 0, 0,
                0x7f7f7f7f, 0, 0x7f7f7f7f);
    __builtin_amdgcn_s_setprio(0);
  };

  // ---- main loop: prologue stage, then one tile_ktile per K-tile ---------
  stage_b(0, 0, ic<0>{}, ic<NB>{});
  stage_a(0, 0, 0);
  stage_a(0, 0, 1);
  // unconditional staging (gemm_fp8_tile has why): the last K-tile stages
  // itself once more into the idle buffer, in bounds and never read
  for (int kt = 0; kt < kt_end; ++kt) {
    const int ktn = kt + 1 < kt_end ? kt + 1 : kt;
    tile_ktile<BN>(kt & 1, ktn, std::true_type{}, stage_b, stage_a, cluster);
  }
  // the redundant stage must land before the LDS can be handed on
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue: image scale, channel scale, bias, act, residual ---------
  const int m_wave = m_blk + wm * 128;
  const int n_wave = n_blk + wn * (BN / 4);
  const bool vec4 = (N & 3) == 0;
  const int HWo = geo.Ho * geo.Wo;

#pragma unroll
  for (int mf = 0; mf < 8; ++mf) {
    const int m = m_wave + mf * 16 + fr;
    if (m >= M) continue;
    const float s_m = sa[m / HWo];
    const long long row = (long long)m * N;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const int n0 = n_wave + nf * 16 + kgrp * 4;
      if (n0 >= N) continue;
      if (vec4) {
        const f32x4_t s_n = *reinterpret_cast<const f32x4_t*>(sw + n0);
        f32x4_t v = acc[mf][nf] * s_m * s_n;
        if (bias) v += *reinterpret_cast<const f32x4_t*>(bias + n0);
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = act_q<ACT>(v[c]);
        if (residual) {
          const u16x4_t r =
              *reinterpret_cast<const u16x4_t*>(residual + row + n0);
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] += bf16_bits_to_f32(r[c]);
        }
        u16x4_t o;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = f32_to_bf16_bits(v[c]);
        *reinterpret_cast<u16x4_t*>(Y + row + n0) = o;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (n0 + c >= N) break;
          float v = acc[mf][nf][c] * s_m * sw[n0 + c];
          if (bias) v += bias[n0 + c];
          v = act_q<ACT>(v);
          if (residual) v += bf16_bits_to_f32(residual[row + n0 + c]);
          Y[row + n0 + c] = f32_to_bf16_bits(v);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

std::tuple<torch::Tensor, torch::Tensor> quant_nhwc_fp8(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.is_contiguous(),
              "x must be contiguous [B, H, W, C] on device");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "x must be bf16");
  const long long B = x.size(0);
  const long long n = x.size(1) * x.size(2) * x.size(3);
  TORCH_CHECK(x.size(3) % 8 == 0 && n > 0,
              "C must be a positive multiple of 8, got ", x.size(3));
  TORCH_CHECK(B < 65536, "B must be below 65536, got ", B);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0,
              "x must be 16-byte aligned");
  auto q = torch::empty_like(x, x.options().dtype(at::kFloat8_e4m3fn));
  auto scale = torch::empty({B}, x.options().dtype(at::kFloat));
  if (B == 0) return {q, scale};
  // 8 chunks per thread where the image is large enough for CQ_QT blocks
  const long long chunks = n / 8;
  const long long blocks = std::min<long long>(
      CQ_QT, (chunks + 8 * CQ_QT - 1) / (8 * CQ_QT));
  const long long per = (chunks + blocks - 1) / blocks;
  TORCH_CHECK(per < (1LL << 31), "quant_nhwc_fp8: image too large");
  auto part = torch::empty({B, blocks}, x.options().dtype(at::kFloat));
  const dim3 grid((unsigned)blocks, (unsigned)B);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(quant_nhwc_absmax_kernel, grid, dim3(CQ_QT), 0, stream,
                     (const uint16_t*)x.data_ptr(), part.data_ptr<float>(),
                     chunks, (int)per);
  HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(quant_nhwc_convert_kernel, grid, dim3(CQ_QT), 0, stream,
                     (const uint16_t*)x.data_ptr(),
                     (const float*)part.data_ptr<float>(),
                     (uint8_t*)q.data_ptr(), scale.data_ptr<float>(), chunks,
                     (int)per);
  HIP_CHECK_LAUNCH();
  return {q, scale};
}

// N-tile width: 320 only where it does not pad (K_out % 320 == 0), and there
// by rounds of the 256 CUs (one workgroup per CU) times the cost of a K-tile
// step. Measured with both widths on the same round counts, a 320-wide step
// costs 1.11-1.16 of a 256-wide one (profiles/r25_conv_fp8.md): 68x68
// K_out 320 takes 320 (3 rounds against 5), the 34x34 and 17x17 levels take
// 256 (equal rounds).
static int conv_fp8_choose_bn(long long M, long long K_out) {
  if (K_out % 320) return 256;
  const long long gx = (M + TILE_BM - 1) / TILE_BM;
  auto rounds = [&](int bn) {
    return (double)((gx * ((K_out + bn - 1) / bn) + 255) / 256);
  };
  return rounds(320) * 1.16 < rounds(256) ? 320 : 256;
}

// q [B,H,W,C] e4m3, sa [B], qw [K_out, Kp] e4m3, sw [K_out], bias [K_out] or
// empty, res [B,Ho,Wo,K_out] bf16 or empty -> y [B,Ho,Wo,K_out] bf16.
// bn (256 / 320) pins the N-tile width; 0 leaves it to conv_fp8_choose_bn.
torch::Tensor conv_fp8_nhwc_ex(torch::Tensor q, torch::Tensor sa,
                               torch::Tensor qw, torch::Tensor sw,
                               torch::Tensor bias, torch::Tensor res,
                               int64_t B, int64_t H, int64_t W, int64_t C,
                               int64_t K_out, int64_t RS, int64_t stride,
                               bool fuse_silu, int64_t bn) {
  TORCH_CHECK(q.is_cuda() && q.is_contiguous() &&
                  q.scalar_type() == at::kFloat8_e4m3fn,
              "q must be a contiguous float8_e4m3fn tensor on device");
  TORCH_CHECK(qw.is_cuda() && qw.is_contiguous() && qw.dim() == 2 &&
                  qw.scalar_type() == at::kFloat8_e4m3fn &&
                  qw.device() == q.device(),
              "qw must be a contiguous float8_e4m3fn [K_out, Kp] on q's device");
  TORCH_CHECK(RS == 9 || RS == 1, "RS must be 9 (3x3, pad 1) or 1");
  TORCH_CHECK(stride == 1 || (stride == 2 && RS == 9),
              "stride must be 1, or 2 for 3x3");
  TORCH_CHECK(B > 0 && H > 0 && W > 0 && K_out > 0 && K_out < (1LL << 31));
  TORCH_CHECK(C > 0 && C % 64 == 0, "C must be a multiple of 64, got ", C);
  TORCH_CHECK(H < 16384 && W < 16384, "pixel coords are packed in 16 bits");
  TORCH_CHECK(q.numel() == B * H * W * C, "q must hold B*H*W*C codes");
  TORCH_CHECK(q.numel() < (1LL << 32), "activation offsets are 32-bit");
  TORCH_CHECK(bn == 0 || bn == 256 || bn == 320, "bn must be 0, 256 or 320");
  const int64_t Kp = (RS * C + CQ_BK - 1) / CQ_BK * CQ_BK;
  TORCH_CHECK(qw.size(0) == K_out && qw.size(1) == Kp,
              "qw must be [K_out, RS*C rounded up to 128] = [", K_out, ", ",
              Kp, "]");
  const int64_t Ho = stride == 1 ? H : (H + 2 - 3) / 2 + 1;
  const int64_t Wo = stride == 1 ? W : (W + 2 - 3) / 2 + 1;
  const long long M = B * Ho * Wo;  // < 2^26: numel < 2^32 and C >= 64
  auto on_dev_f32 = [&](const torch::Tensor& s, int64_t n) {
    return s.is_cuda() && s.device() == q.device() &&
           s.scalar_type() == at::kFloat && s.is_contiguous() &&
           s.numel() == n;
  };
  TORCH_CHECK(on_dev_f32(sa, B), "sa must be contiguous fp32 [B]");
  TORCH_CHECK(on_dev_f32(sw, K_out), "sw must be contiguous fp32 [K_out]");
  const bool has_bias = bias.defined() && bias.numel() > 0;
  TORCH_CHECK(!has_bias || (bias.is_cuda() && bias.device() == q.device() &&
                            bias.numel() == K_out),
              "bias must hold K_out values on q's device");
  const uint16_t* resptr = nullptr;
  if (res.defined() && res.numel() > 0) {
    TORCH_CHECK(res.is_cuda() && res.device() == q.device() &&
                    res.is_contiguous() &&
                    res.scalar_type() == at::kBFloat16 &&
                    res.numel() == M * K_out,
                "res must be a contiguous bf16 [B,Ho,Wo,K_out] tensor");
    resptr = (const uint16_t*)res.data_ptr();
  }
  torch::Tensor bf32;
  const float* bptr = bias_f32_ptr(bias, bf32);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(q.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(qw.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(sw.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(bptr) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(resptr) & 7) == 0,
              "q, qw, sw and bias must be 16-byte aligned, res 8-byte");
  auto y = torch::empty({B, Ho, Wo, K_out}, q.options().dtype(at::kBFloat16));
  const int width = bn ? (int)bn : conv_fp8_choose_bn(M, K_out);
  const long long gx = (M + TILE_BM - 1) / TILE_BM;
  const long long gy = (K_out + width - 1) / width;
  TORCH_CHECK(gy < 65536, "conv_fp8: grid too large");
  const dim3 grid((unsigned)gx, (unsigned)gy);
  auto stream = at::hip::getCurrentHIPStream();
  const ConvFp8Geo geo{(int)H, (int)W, (int)C, (int)Ho, (int)Wo, (int)stride,
                       (int)RS};
  auto launch = [&](auto BN, auto ACT) {
    hipLaunchKernelGGL(
        (conv_fp8_kernel<decltype(BN)::value, decltype(ACT)::value>), grid,
        dim3(512), 0, stream, (const uint8_t*)q.data_ptr(),
        (const uint8_t*)qw.data_ptr(), sa.data_ptr<float>(),
        sw.data_ptr<float>(), bptr, (const uint8_t*)device_zero_page(q),
        resptr, (uint16_t*)y.data_ptr(), (int)M, (int)K_out, (int)Kp, geo);
  };
  if (width == 320) {
    if (fuse_silu) launch(ic<320>{}, ic<ACT_SILU>{});
    else launch(ic<320>{}, ic<ACT_NONE>{});
  } else {
    if (fuse_silu) launch(ic<256>{}, ic<ACT_SILU>{});
    else launch(ic<256>{}, ic<ACT_NONE>{});
  }
  HIP_CHECK_LAUNCH();
  return y;
}

torch::Tensor conv_fp8_nhwc(torch::Tensor q, torch::Tensor sa, torch::Tensor qw,
                            torch::Tensor sw, torch::Tensor bias,
                            torch::Tensor res, int64_t B, int64_t H, int64_t W,
                            int64_t C, int64_t K_out, int64_t RS,
                            int64_t stride, bool fuse_silu) {
  return conv_fp8_nhwc_ex(q, sa, qw, sw, bias, res, B, H, W, C, K_out, RS,
                          stride, fuse_silu, 0);
}
