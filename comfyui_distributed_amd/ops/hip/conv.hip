// Hand-written CDNA4 convolution kernels for the shapes the 256-tile
// implicit-GEMM conv (gemm.hip) does not take.
//
// conv_nhwc: direct implicit-GEMM convolution on MFMA 16x16x32 bf16. Output
// pixels are GEMM rows (M = B*H*W), output channels are GEMM columns (N = K),
// the reduction runs over (r, s, c) with the channel dim innermost (NHWC
// activations, so every A fragment is a contiguous 16-byte load; no im2col
// materialization, no NCHW<->NHWC transposes). Weights are host-repacked once
// per module to W_t[k_out][(r*3+s)*C + c] so B fragments are contiguous too.
// Covers 3x3 stride-1 pad-1 and 1x1 convs with C % 32 == 0, K % 16 == 0.
// dispatch.conv2d_mfma sends here every such conv with C % 64 != 0, or with
// M < 256 and no fused upsample: the 9x9 level of the SD1.5 UNet at tile
// batch 1-3 and the tiny-config models of the test suite.
//
// conv_smallc: the C_in <= 8 stems (4 latents -> 320, RGB -> 128).
//
// Reference counterpart: the VAEDecode / KSampler ComfyUI ops the reference
// calls per tile.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define ZERO8_C short8{0, 0, 0, 0, 0, 0, 0, 0}
#define W_PITCH 40  // elements per LDS weight row (32 + 8 pad = 80 B)

// ---------------------------------------------------------------------------
// Direct conv, one template for both tiles. Waves form a 2 x WN grid; a wave
// owns MI x 2 MFMA fragments (MI*16 pixels x 32 channels), so the workgroup
// tile is BM = 2*MI*16 pixels x BN = WN*32 channels on 2*WN*64 threads.
// A fragments stream from global (L1/L2-cached: consecutive k-steps walk a
// pixel row sequentially). B fragments come
//  - STAGE_B = false: straight from global, no LDS, no barrier;
//  - STAGE_B = true: from a BN x 32 weight chunk staged per 32-deep k-step in
//    a conflict-free 80-byte-pitch LDS image shared by all waves, one 16-byte
//    piece per thread (BN * 4 pieces == block size), two barriers per k-step.
// Instances: <RS, 2, 2, false> (64x64 tile, 4 waves) and <RS, 4, 4, true>
// (128x128 tile, 8 waves), RS = 9 (3x3) or 1 (1x1).
// ---------------------------------------------------------------------------

template <int RS, int MI, int WN, bool STAGE_B>
__global__ __launch_bounds__(2 * WN * 64) void conv_direct_kernel(
    const uint16_t* __restrict__ x,   // [B, H, W, C]
    const uint16_t* __restrict__ wt,  // [K, RS*C] repacked
    const float* __restrict__ bias,   // [K] or nullptr
    uint16_t* __restrict__ y,         // [B, H, W, K]
    int B, int H, int W, int C, int K, int fuse_silu) {
  constexpr int BM = 2 * MI * 16;
  constexpr int BN = WN * 32;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave / WN;          // wave row (0..1)
  const int wn = wave % WN;          // wave col (0..WN-1)
  const long long HW = (long long)H * W;
  const long long M = (long long)B * HW;

  const long long m_base = (long long)blockIdx.x * BM + wm * (MI * 16);
  const int n_base = blockIdx.y * BN + wn * 32;

  // only the staged variant touches it; unused, it takes no LDS
  __shared__ __align__(16) uint16_t w_lds[STAGE_B ? BN : 1][W_PITCH];

  // accumulators: MI x 2 fragments of 16x16
  f32x4 acc[MI][2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15;          // fragment row/col index
  const int kgrp = lane >> 4;        // k-group: elements kgrp*8..+8

  // decompose the MI pixel rows this lane loads for A
  int px_y[MI], px_x[MI], px_b[MI];
  bool m_ok[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const long long m_row = m_base + i * 16 + fr;
    m_ok[i] = m_row < M;
    long long mm = m_ok[i] ? m_row : 0;
    px_b[i] = (int)(mm / HW);
    int rem = (int)(mm - (long long)px_b[i] * HW);
    px_y[i] = rem / W;
    px_x[i] = rem % W;
  }

  const int csteps = C / 32;
  for (int rs = 0; rs < RS; ++rs) {
    const int r = RS == 1 ? 0 : rs / 3;
    const int s = RS == 1 ? 0 : rs % 3;
    // source pixel of this tap (pad 1 for 3x3) and whether it exists
    int sy[MI], sx[MI];
    bool tap_ok[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      sy[i] = px_y[i] + (RS == 1 ? 0 : r - 1);
      sx[i] = px_x[i] + (RS == 1 ? 0 : s - 1);
      tap_ok[i] = m_ok[i] && sy[i] >= 0 && sy[i] < H && sx[i] >= 0 && sx[i] < W;
    }
    for (int cs = 0; cs < csteps; ++cs) {
      const int kdim = rs * C + cs * 32;
      if (STAGE_B) {
        // ---- stage the BN x 32 weight chunk (one 16B piece per thread) ----
        __syncthreads();
        const int row = threadIdx.x >> 2;            // BN rows
        const int koff = (threadIdx.x & 3) * 8;      // 4 pieces
        const int n = blockIdx.y * BN + row;
        short8 wv = (n < K)
            ? *reinterpret_cast<const short8*>(wt + (long long)n * (RS * C) + kdim + koff)
            : ZERO8_C;
        *reinterpret_cast<short8*>(&w_lds[row][koff]) = wv;
        __syncthreads();
      }

      // A fragments (MI pixel rows x 8 contiguous channels), zero outside
      const int c0 = cs * 32 + kgrp * 8;
      short8 a[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        if (tap_ok[i]) {
          const uint16_t* p =
              x + (((long long)px_b[i] * H + sy[i]) * W + sx[i]) * C + c0;
          a[i] = *reinterpret_cast<const short8*>(p);
        } else {
          a[i] = ZERO8_C;
        }
      }
      // B fragments (2 output channels x 8 contiguous k-elements)
      short8 bfr[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (STAGE_B) {
          bfr[j] = *reinterpret_cast<const short8*>(
              &w_lds[wn * 32 + j * 16 + fr][kgrp * 8]);
        } else {
          const int n = n_base + j * 16 + fr;
          bfr[j] = (n < K)
              ? *reinterpret_cast<const short8*>(
                    wt + (long long)n * (RS * C) + (kdim + kgrp * 8))
              : ZERO8_C;
        }
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bfr[j],
                                                              acc[i][j], 0, 0, 0);
    }
  }

  // epilogue: bias + optional SiLU, store NHWC
  const int out_col = lane & 15;
  const int rgrp = lane >> 4;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n_base + j * 16 + out_col;
      if (n >= K) continue;
      const float bval = bias ? bias[n] : 0.f;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const long long m = m_base + i * 16 + rgrp * 4 + rr;
        if (m >= M) continue;
        float v = acc[i][j][rr] + bval;
        if (fuse_silu) v = silu_f(v);
        y[m * K + n] = f32_to_bf16_bits(v);
      }
    }
  }
}

template <int RS, int MI, int WN, bool STAGE_B>
static void conv_direct_launch(const torch::Tensor& x, const torch::Tensor& wt,
                               const float* bias, torch::Tensor& y, int B,
                               int H, int W, int C, int K, bool fuse_silu) {
  constexpr int BM = 2 * MI * 16, BN = WN * 32;
  const long long M = (long long)B * H * W;
  dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((K + BN - 1) / BN));
  hipLaunchKernelGGL((conv_direct_kernel<RS, MI, WN, STAGE_B>), grid,
                     dim3(2 * WN * 64), 0, at::hip::getCurrentHIPStream(),
                     (const uint16_t*)x.data_ptr(), (const uint16_t*)wt.data_ptr(),
                     bias, (uint16_t*)y.data_ptr(), B, H, W, C, K,
                     fuse_silu ? 1 : 0);
}

torch::Tensor conv_nhwc(torch::Tensor x, torch::Tensor wt, torch::Tensor bias,
                        int64_t B, int64_t H, int64_t W, int64_t C, int64_t K,
                        int64_t rs, bool fuse_silu) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous());
  TORCH_CHECK(wt.is_cuda() && wt.scalar_type() == at::kBFloat16 && wt.is_contiguous());
  TORCH_CHECK(C % 32 == 0, "C must be a multiple of 32");
  TORCH_CHECK(rs == 9 || rs == 1, "only 3x3 and 1x1");
  auto y = torch::empty({B, H, W, K}, x.options());
  const long long M = B * H * W;
  torch::Tensor bf;
  const float* bptr = bias_f32_ptr(bias, bf);
  // the 128x128 tile with LDS-staged weights when the N dim fills it, the
  // 64x64 tile otherwise; M and K tails are handled by in-kernel bounds
  const bool staged = (K % 128 == 0) && (M >= 128);
  auto launch = [&](auto taps) {
    constexpr int RS = decltype(taps)::value;
    if (staged)
      conv_direct_launch<RS, 4, 4, true>(x, wt, bptr, y, (int)B, (int)H, (int)W,
                                         (int)C, (int)K, fuse_silu);
    else
      conv_direct_launch<RS, 2, 2, false>(x, wt, bptr, y, (int)B, (int)H, (int)W,
                                          (int)C, (int)K, fuse_silu);
  };
  if (rs == 9) launch(std::integral_constant<int, 9>{});
  else launch(std::integral_constant<int, 1>{});
  HIP_CHECK_LAUNCH();
  return y;
}

// ---------------------------------------------------------------------------
// Small-C conv (the UNet/VAE stem: C_in <= 8, e.g. 4 latents -> 320).
// MIOpen/CK fall back to very slow paths for NHWC C=4; this is a simple
// HBM-bound kernel: 32 pixels x 8 k-slots per 256-thread block, weights
// staged in LDS, per-pixel taps read once and reused across the k-slots
// via L1.
// ---------------------------------------------------------------------------

#define SC_KSLOTS 8

template <int RS, int C>
__global__ __launch_bounds__(256) void conv_smallc_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ wt,
    const float* __restrict__ bias, uint16_t* __restrict__ y, int B, int H,
    int W, int K, int fuse_silu) {
  constexpr int KD = RS * C;
  extern __shared__ __align__(16) uint16_t w_sm[];  // [K][KD]
  for (int i = threadIdx.x; i < K * KD; i += blockDim.x) w_sm[i] = wt[i];
  __syncthreads();

  const long long HW = (long long)H * W;
  const long long M = (long long)B * HW;
  const int kper = (K + SC_KSLOTS - 1) / SC_KSLOTS;
  const int pix_local = threadIdx.x / SC_KSLOTS;   // 0..31
  const int kslot = threadIdx.x % SC_KSLOTS;
  const long long p = (long long)blockIdx.x * 32 + pix_local;
  if (p >= M) return;
  const int b = (int)(p / HW);
  const int rem = (int)(p - (long long)b * HW);
  const int py = rem / W, px = rem % W;

  // taps fully unrolled -> registers (a runtime-indexed array would live
  // in scratch: 5x slowdown)
  float taps[KD];
#pragma unroll
  for (int rs = 0; rs < RS; ++rs) {
    const int r = RS == 1 ? 0 : rs / 3;
    const int s = RS == 1 ? 0 : rs % 3;
    const int sy = py + (RS == 1 ? 0 : r - 1);
    const int sx = px + (RS == 1 ? 0 : s - 1);
    const bool ok = sy >= 0 && sy < H && sx >= 0 && sx < W;
    const uint16_t* src =
        x + (((long long)b * H + sy) * W + sx) * C;
#pragma unroll
    for (int c = 0; c < C; ++c)
      taps[rs * C + c] = ok ? bf16_bits_to_f32(src[c]) : 0.f;
  }

  const int k0 = kslot * kper;
  const int k1 = min(k0 + kper, K);
  uint16_t* dst = y + p * K;
  for (int k = k0; k < k1; ++k) {
    const uint16_t* wrow = &w_sm[k * KD];
    float acc = bias ? bias[k] : 0.f;
#pragma unroll
    for (int i = 0; i < KD; ++i)
      acc += taps[i] * bf16_bits_to_f32(wrow[i]);
    if (fuse_silu) acc = silu_f(acc);
    dst[k] = f32_to_bf16_bits(acc);
  }
}

torch::Tensor conv_smallc(torch::Tensor x, torch::Tensor wt, torch::Tensor bias,
                          int64_t B, int64_t H, int64_t W, int64_t C,
                          int64_t K, int64_t rs, bool fuse_silu) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous());
  TORCH_CHECK(C <= 8, "conv_smallc is for C <= 8");
  TORCH_CHECK(rs == 9 || rs == 1);
  auto y = torch::empty({B, H, W, K}, x.options());
  const long long M = B * H * W;
  dim3 grid((unsigned)((M + 31) / 32));
  dim3 block(256);
  const size_t smem = (size_t)K * rs * C * sizeof(uint16_t);
  TORCH_CHECK(smem <= 64 * 1024, "weights exceed LDS budget");
  auto stream = at::hip::getCurrentHIPStream();
  torch::Tensor bf;
  const float* bptr = bias_f32_ptr(bias, bf);
#define SC_LAUNCH(RS_, C_)                                                     \
  hipLaunchKernelGGL((conv_smallc_kernel<RS_, C_>), grid, block, smem, stream,\
                     (const uint16_t*)x.data_ptr(),                           \
                     (const uint16_t*)wt.data_ptr(), bptr,                    \
                     (uint16_t*)y.data_ptr(), (int)B, (int)H, (int)W, (int)K, \
                     fuse_silu ? 1 : 0)
  TORCH_CHECK(C == 3 || C == 4 || C == 8, "conv_smallc supports C in {3,4,8}");
  if (rs == 9) {
    if (C == 3) SC_LAUNCH(9, 3);
    else if (C == 4) SC_LAUNCH(9, 4);
    else SC_LAUNCH(9, 8);
  } else {
    if (C == 3) SC_LAUNCH(1, 3);
    else if (C == 4) SC_LAUNCH(1, 4);
    else SC_LAUNCH(1, 8);
  }
#undef SC_LAUNCH
  HIP_CHECK_LAUNCH();
  return y;
}
